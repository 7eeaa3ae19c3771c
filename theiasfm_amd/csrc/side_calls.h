// Host side of the one-shot calls and the batched small-problem solvers (small_lm.h): the C entry points beside the LM
// driver, written on one_shot.h.  Included by engine.hip after the driver: tmi_ba_solver, prepare_cameras,
// launch_track_lm and TMI_HIP are the driver's.  The five global pose estimators (robust, nonlinear and linear
// rotations, LUD and nonlinear positions) are in pose_graph_calls.h.
#pragma once

namespace {
// A per-view index of the handle's observation slots: fill_keys(keys) queues the kernel that writes one
// (view << 32 | x) key per slot, the keys are radix-sorted into keys_sorted [No_pad] and view_ptr [Nc + 1] is derived
// from them.  The temporaries are freed on every way out; the stream is synchronised if there was anything to sort.
template <class FillKeys>
int build_view_index(tmi_ba_solver* s, FillKeys fill_keys, unsigned long long* keys_sorted, long long* view_ptr) {
  const Structure& st = s->st;
  hipStream_t stream = s->stream;
  if (st.No_pad > 0) {
    OneShot tmp_mem(stream);
    unsigned long long* keys_in = nullptr;
    TMI_HIP(tmp_mem.alloc(&keys_in, (size_t)st.No_pad));
    fill_keys(keys_in);
    size_t tmp_bytes = 0;
    TMI_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, keys_in, keys_sorted, (int)st.No_pad, 0, 64, stream));
    unsigned char* tmp = nullptr;
    TMI_HIP(tmp_mem.alloc(&tmp, std::max<size_t>(tmp_bytes, 16)));
    TMI_HIP(hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, keys_in, keys_sorted, (int)st.No_pad, 0, 64, stream));
    TMI_HIP(hipStreamSynchronize(stream));
  }
  hipLaunchKernelGGL(select_view_ptr_kernel, dim3((st.Nc + 1 + 255) / 256), dim3(256), 0, stream, keys_sorted,
                     (long long)st.No_pad, st.Nc, view_ptr);
  return TMI_BA_OK;
}
}  // namespace
extern "C" {

// ---- per-track side kernels ----------------------------------
static int ensure_track_outputs(tmi_ba_solver* s) {
  if (s->d_trk_flag) return TMI_BA_OK;
  const size_t n = (size_t)std::max(s->st.Np_pad, 1);
  int rc;
  if ((rc = dev_alloc(s, &s->d_trk_flag, n))) return rc;
  if ((rc = dev_alloc(s, &s->d_trk_mean, n))) return rc;
  if ((rc = dev_alloc(s, &s->d_trk_term, n))) return rc;
  if ((rc = dev_alloc(s, &s->d_trk_iter, n))) return rc;
  if ((rc = dev_alloc(s, &s->d_trk_c0, n))) return rc;
  if ((rc = dev_alloc(s, &s->d_trk_c1, n))) return rc;
  const size_t nt = (size_t)std::max(s->st.Np_total, 1);
  if ((rc = dev_alloc(s, &s->d_out_u8, nt))) return rc;
  if ((rc = dev_alloc(s, &s->d_out_f64, nt))) return rc;
  if ((rc = dev_alloc(s, &s->d_out_i32, nt))) return rc;
  if ((rc = dev_alloc(s, &s->d_counters, 4))) return rc;
  TMI_HIP(hipHostMalloc((void**)&s->h_counters, 4 * sizeof(int), hipHostMallocDefault));
  TMI_HIP(hipHostMalloc((void**)&s->h_cell_total, sizeof(long long), hipHostMallocDefault));
  TMI_HIP(hipHostMalloc((void**)&s->h_stage, nt * 16, hipHostMallocDefault));
  return TMI_BA_OK;
}

int32_t tmi_ba_solver_filter_outlier_tracks(tmi_ba_solver* s, double max_inlier_reprojection_error,
                                            double min_triangulation_angle_degrees,
                                            uint8_t* track_flag, double* track_mean_sq_error,
                                            tmi_ba_filter_summary* sum) {
  if (!s || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  TMI_HIP(hipSetDevice(s->device));
  int rc = ensure_track_outputs(s);
  if (rc) return rc;
  const Structure& st = s->st;
  const double max_sq = max_inlier_reprojection_error * max_inlier_reprojection_error;
  const double cos_min = std::cos(min_triangulation_angle_degrees * (M_PI / 180.0));
  StreamTimer timer(s->stream);
  TMI_HIP(timer.status);
  TMI_HIP(timer.mark());
  if (st.nslices > 0)
    hipLaunchKernelGGL(outlier_filter_kernel, dim3(s->nblocks_tracks), dim3(256), 0, s->stream, s->v, max_sq,
                       cos_min, s->d_trk_flag, s->d_trk_mean);
  TMI_HIP(timer.mark());
  if (st.world == 1) {
    // counts and the permutation to the caller's track order happen on the device; one copy per
    // requested output (round 1: flags + means of every slot copied out and walked on the host)
    TMI_HIP(hipMemsetAsync(s->d_counters, 0, 4 * sizeof(int), s->stream));
    if (st.Np_pad > 0)
      hipLaunchKernelGGL(filter_finish_kernel, dim3((st.Np_pad + 255) / 256), dim3(256), 0, s->stream, s->d_pt_orig,
                         st.Np_pad, s->d_trk_flag, s->d_trk_mean, track_flag ? s->d_out_u8 : nullptr,
                         track_mean_sq_error ? s->d_out_f64 : nullptr, s->d_counters);
    TMI_HIP(download(s->stream, s->h_counters, s->d_counters, 4));
    const size_t ntot = (size_t)st.Np_total;
    unsigned char* stage_u8 = s->h_stage;
    double* stage_f64 = reinterpret_cast<double*>(s->h_stage + 8 * ntot);
    if (track_flag) TMI_HIP(download(s->stream, stage_u8, s->d_out_u8, ntot));
    if (track_mean_sq_error) TMI_HIP(download(s->stream, stage_f64, s->d_out_f64, ntot));
    TMI_HIP(hipStreamSynchronize(s->stream));
    if (track_flag && ntot > 0) memcpy(track_flag, stage_u8, ntot);
    if (track_mean_sq_error && ntot > 0) memcpy(track_mean_sq_error, stage_f64, ntot * sizeof(double));
    sum->num_estimated_tracks = s->h_counters[0];
    sum->num_bad_reprojections = s->h_counters[1];
    sum->num_insufficient_viewing_angles = s->h_counters[2];
  } else {
    std::vector<unsigned char> flag((size_t)st.Np_pad);
    std::vector<double> mean(track_mean_sq_error ? (size_t)st.Np_pad : 0);
    TMI_HIP(download(s->stream, flag.data(), s->d_trk_flag, flag.size()));
    TMI_HIP(download(s->stream, mean.data(), s->d_trk_mean, mean.size()));
    TMI_HIP(hipStreamSynchronize(s->stream));
    for (int lp = 0; lp < st.Np_pad; ++lp) {
      const int p = st.pt_orig[lp];
      if (p < 0) continue;
      const unsigned char f = flag[lp];
      sum->num_estimated_tracks++;
      if (f == 1) sum->num_bad_reprojections++;
      if (f == 2) sum->num_insufficient_viewing_angles++;
      if (track_flag) track_flag[p] = f;
      if (track_mean_sq_error) track_mean_sq_error[p] = mean[lp];
    }
  }
  // a track nobody observes: mean = 0 / 0, no ray pair -> insufficient viewing angle
  // (set_outlier_tracks_to_unestimated.cc:108,120-125 with empty lists)
  for (const int p : st.unobserved) {
    sum->num_estimated_tracks++;
    sum->num_insufficient_viewing_angles++;
    if (track_flag) track_flag[p] = 2;
    if (track_mean_sq_error) track_mean_sq_error[p] = std::nan("");
  }
  sum->kernel_seconds = timer.seconds();  // (both branches synchronised the stream)
  sum->seconds = now_s() - t0;
  return TMI_BA_OK;
}

int32_t tmi_ba_filter_outlier_tracks(const tmi_ba_problem* P, int32_t device,
                                     double max_inlier_reprojection_error,
                                     double min_triangulation_angle_degrees, uint8_t* track_flag,
                                     double* track_mean_sq_error, tmi_ba_filter_summary* sum) {
  if (!P || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  tmi_ba_options O;
  tmi_ba_options_init(&O);
  O.device = device;
  const int rc = with_light_handle(P, &O, nullptr, [&](tmi_ba_solver* s) {
    return tmi_ba_solver_filter_outlier_tracks(s, max_inlier_reprojection_error, min_triangulation_angle_degrees,
                                               track_flag, track_mean_sq_error, sum);
  });
  sum->seconds = now_s() - t0;
  return rc;
}

int32_t tmi_ba_solver_adjust_tracks(tmi_ba_solver* s, const tmi_ba_options* O, int8_t* track_termination,
                                    int32_t* track_iterations, double* track_initial_cost,
                                    double* track_final_cost, tmi_ba_track_batch_summary* sum) {
  if (!s || !O || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  if (O->point_dof != s->DP) return TMI_BA_ERR_INVALID_ARGUMENT;
  const double t0 = now_s();
  TMI_HIP(hipSetDevice(s->device));
  int rc = ensure_track_outputs(s);
  if (rc) return rc;
  const Structure& st = s->st;
  const SmallLmArgs A = small_lm_args(O);
  const SmallLmOut d{s->d_trk_term, s->d_trk_iter, s->d_trk_c0, s->d_trk_c1};
  const ItemArrays out{track_termination, track_iterations, track_initial_cost, track_final_cost};
  rc = run_small_lm(s, s->stream, d, (size_t)st.Np_pad, st.pt_orig.data(), [&] {
    prepare_cameras(s, s->v.ext, s->v.intr, s->v.prep);  // (inside the timed region: part of the call's device work)
    if (st.nslices > 0) launch_track_lm(s, s->v, s->v.prep, A);
  }, out, sum, &sum->num_tracks);
  if (rc) return rc;
  for (const int p : st.unobserved) {
    if (track_termination) track_termination[p] = -1;
    if (track_iterations) track_iterations[p] = 0;
    if (track_initial_cost) track_initial_cost[p] = 0.0;
    if (track_final_cost) track_final_cost[p] = 0.0;
  }
  sum->seconds = now_s() - t0;
  return TMI_BA_OK;
}

int32_t tmi_ba_adjust_tracks(tmi_ba_problem* P, const tmi_ba_options* O, int8_t* track_termination,
                             int32_t* track_iterations, double* track_initial_cost,
                             double* track_final_cost, tmi_ba_track_batch_summary* sum) {
  if (!P || !O || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  const int rc = with_light_handle(P, O, P, [&](tmi_ba_solver* s) {
    return tmi_ba_solver_adjust_tracks(s, O, track_termination, track_iterations, track_initial_cost,
                                       track_final_cost, sum);
  });
  sum->seconds = now_s() - t0;
  return rc;
}

// ---- batched BundleAdjustView (view_kernels.h) ---------------------------------------------
}  // extern "C"
namespace {
// Chains of the views to adjust (selected, observed, something free): the selected views of a group with free
// entries form one chain in ascending index order, every other view is a chain of its own; longest first.
void build_view_chains(int Nc, const std::vector<int4>& cam, const int* cam_group, int G,
                       const std::vector<long long>& vptr, const uint8_t* view_mask, std::vector<int>* chain_ptr,
                       std::vector<int>* chain_views) {
  std::vector<std::vector<int> > chains;
  std::vector<int> group_chain(std::max(G, 0), -1);
  for (int c = 0; c < Nc; ++c) {
    if (view_mask && !view_mask[c]) continue;
    if (cam[c].w == 0 || vptr[c + 1] == vptr[c]) continue;
    const int g = cam_group[c];
    if (((unsigned)cam[c].w >> 6) != 0) {
      if (group_chain[g] < 0) {
        group_chain[g] = (int)chains.size();
        chains.emplace_back();
      }
      chains[group_chain[g]].push_back(c);
    } else {
      chains.push_back({c});
    }
  }
  std::stable_sort(chains.begin(), chains.end(),
                   [](const std::vector<int>& a, const std::vector<int>& b) { return a.size() > b.size(); });
  chain_ptr->assign(1, 0);
  chain_views->clear();
  for (const auto& ch : chains) {
    chain_views->insert(chain_views->end(), ch.begin(), ch.end());
    chain_ptr->push_back((int)chain_views->size());
  }
}

// (model, intrinsics offset, intrinsics size, free mask over [extrinsics(6) | intrinsics(10)]) per camera
int4 view_cam_record(int flags, int model, int offset, int nk, uint32_t free_intr) {
  uint32_t m = 0;
  if (!(flags & TMI_BA_CAMERA_POSITION_CONSTANT)) m |= 0x07;
  if (!(flags & TMI_BA_CAMERA_ORIENTATION_CONSTANT)) m |= 0x38;
  m |= (free_intr & 0x3ffu) << 6;
  return make_int4(model, offset, nk, (int)m);
}

// Launches the chains on s->stream (B holds the parameter / observation pointers) and fills the per-view outputs.
int run_view_batch(OneShot* s, ViewBatch B, const tmi_ba_options* O, int Nc, const std::vector<int4>& cam,
                   const std::vector<int>& chain_ptr, const std::vector<int>& chain_views, const ItemArrays& out,
                   tmi_ba_view_batch_summary* sum) {
  const int n_chains = (int)chain_ptr.size() - 1;
  int* d_cptr;
  int* d_cviews;
  TMI_HIP(s->upload(&d_cptr, chain_ptr.data(), chain_ptr.size()));
  TMI_HIP(s->upload(&d_cviews, chain_views.data(), chain_views.size()));
  int rc = s->alloc_outputs(&B.out, (size_t)Nc);  // -1: not adjusted
  if (rc) return rc;
  B.chain_ptr = d_cptr;
  B.chain_views = d_cviews;
  bool pinhole = true;
  for (const int c : chain_views) pinhole = pinhole && cam[c].x == TMI_BA_PINHOLE;
  const SmallLmArgs A = small_lm_args(O);
  rc = run_small_lm(s, s->stream, B.out, (size_t)Nc, nullptr, [&] {
    if (n_chains == 0) return;
    if (pinhole)
      hipLaunchKernelGGL((view_lm_kernel<0>), dim3(n_chains), dim3(256), 0, s->stream, B, A);
    else
      hipLaunchKernelGGL(view_lm_kernel<-1>, dim3(n_chains), dim3(256), 0, s->stream, B, A);
  }, out, sum, &sum->num_views);
  sum->num_chains = n_chains;
  return rc;
}
}  // namespace
extern "C" {

int32_t tmi_ba_solver_adjust_views(tmi_ba_solver* s, const tmi_ba_options* O, const uint8_t* view_mask,
                                   int8_t* view_termination, int32_t* view_iterations, double* view_initial_cost,
                                   double* view_final_cost, tmi_ba_view_batch_summary* sum) {
  if (!s || !O || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const Structure& st = s->st;
  if (st.world > 1) {
    g_last_error = s->error = "view adjustment needs every observation of a view: run it on an unsharded handle";
    return TMI_BA_ERR_INVALID_ARGUMENT;
  }
  const double t0 = now_s();
  TMI_HIP(hipSetDevice(s->device));
  const int Nc = st.Nc;
  hipStream_t stream = s->stream;
  int rc;
  // static per handle: the view-major index of the handle's observations ((view, slot) keys).  Marked ready only
  // once every part of it exists: a build that fails part-way is redone by the next call (the handle's own arrays
  // are freed at destroy).
  if (!s->view_index_ready) {
    if (st.No_pad >= (int64_t)0xffffffffLL) {
      g_last_error = s->error = "view adjustment: more than 2^32 observation slots";
      return TMI_BA_ERR_UNSUPPORTED;
    }
    if ((rc = dev_alloc(s, &s->d_view_ptr, (size_t)Nc + 2))) return rc;
    if ((rc = dev_alloc(s, &s->d_view_keys, (size_t)std::max<int64_t>(st.No_pad, 1)))) return rc;
    if ((rc = dev_alloc(s, &s->d_view_slot_pt, (size_t)std::max<int64_t>(st.No_pad, 1)))) return rc;
    rc = build_view_index(s, [&](unsigned long long* keys) {
      hipLaunchKernelGGL(view_keys_kernel, dim3(s->nblocks_slices), dim3(256), 0, stream, s->v, keys, s->d_view_slot_pt);
    }, s->d_view_keys, s->d_view_ptr);
    if (rc) return rc;
    std::vector<long long> vptr_h((size_t)Nc + 1, 0);
    TMI_HIP(download(stream, vptr_h.data(), s->d_view_ptr, vptr_h.size()));
    TMI_HIP(hipStreamSynchronize(stream));
    std::vector<int4> cam_h((size_t)Nc);
    for (int c = 0; c < Nc; ++c) {
      const int g = st.cam_group[c];
      const int o = st.group_offset[g];
      cam_h[c] = view_cam_record(s->cam_flags_h.empty() ? 0 : s->cam_flags_h[c], s->grp_model_h[g], o,
                                 st.group_offset[g + 1] - o, st.grp_free[g]);
    }
    if ((rc = dev_upload(s, &s->d_view_cam, cam_h))) return rc;
    s->view_ptr_h.swap(vptr_h);
    s->view_cam_h.swap(cam_h);
    s->view_index_ready = true;
  }
  std::vector<int> chain_ptr, chain_views;
  build_view_chains(Nc, s->view_cam_h, st.cam_group.data(), st.G, s->view_ptr_h, view_mask, &chain_ptr, &chain_views);
  ViewBatch B;
  memset(&B, 0, sizeof(B));
  B.ext = s->v.ext;
  B.intr = s->v.intr;
  B.cam = s->d_view_cam;
  B.keys = s->d_view_keys;
  B.vptr = s->d_view_ptr;
  B.slot_pt = s->d_view_slot_pt;
  B.obs_xy = s->v.obs_xy;
  B.pts = s->v.pts;
  OneShot scratch(stream);
  rc = run_view_batch(&scratch, B, O, Nc, s->view_cam_h, chain_ptr, chain_views,
                      {view_termination, view_iterations, view_initial_cost, view_final_cost}, sum);
  if (rc) {
    g_last_error = s->error = scratch.error;
    return rc;
  }
  // the cameras moved: every camera-derived cache of the handle is stale
  prepare_cameras(s, s->v.ext, s->v.intr, s->v.prep);
  s->v.compact = 0;
  s->v.sums_ready = 0;
  TMI_HIP(hipStreamSynchronize(stream));
  sum->seconds = now_s() - t0;
  return TMI_BA_OK;
}

int32_t tmi_ba_adjust_views(tmi_ba_problem* P, const tmi_ba_options* O, const uint8_t* view_mask,
                            int8_t* view_termination, int32_t* view_iterations, double* view_initial_cost,
                            double* view_final_cost, tmi_ba_view_batch_summary* sum) {
  if (!P || !O || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  OneShot sc;
  OneShot* s = &sc;  // (TMI_HIP reports into s->error)
  const int Nc = P->num_cameras, G = P->num_groups, Np = P->num_points;
  const int64_t No = P->num_observations;
  if (Nc < 0 || G < 0 || Np < 0 || No < 0) return bad_argument("negative size");
  if ((Nc && (!P->extrinsics || !P->camera_group)) || (G && (!P->group_model || !P->group_offset)) ||
      (Np && !P->points) || (No && (!P->obs_camera || !P->obs_point || !P->obs_xy)))
    return bad_argument("missing array");
  if (No >= (int64_t)0xffffffffLL) return bad_argument("more than 2^32 observations");
  const int n_intr = G ? P->group_offset[G] : 0;
  if (n_intr && !P->intrinsics) return bad_argument("missing intrinsics");
  std::vector<uint32_t> grp_free((size_t)G, 0);
  for (int g = 0; g < G; ++g) {
    const int o = P->group_offset[g], nk = P->group_offset[g + 1] - o;
    if (P->group_model[g] < 0 || P->group_model[g] > 4 || nk != tmi_ba_intrinsics_size(P->group_model[g]) || o < 0)
      return bad_argument("bad intrinsics group");
    for (int j = 0; j < nk; ++j)
      if (!P->intrinsics_constant || !P->intrinsics_constant[o + j]) grp_free[g] |= 1u << j;
  }
  std::vector<int4> cam((size_t)Nc);
  for (int c = 0; c < Nc; ++c) {
    const int g = P->camera_group[c];
    if (g < 0 || g >= G) return bad_argument("bad camera group");
    const int o = P->group_offset[g];
    cam[c] = view_cam_record(P->camera_flags ? P->camera_flags[c] : 0, P->group_model[g], o,
                             P->group_offset[g + 1] - o, grp_free[g]);
  }
  // host work that does not shrink with the batch: one pass over all observations (check + count) and one over their
  // cameras (the gather below); summary.seconds - kernel_seconds is this plus the uploads
  std::vector<long long> optr((size_t)Nc + 1, 0);  // observations per view as ranges of the view-major order
  for (int64_t i = 0; i < No; ++i) {
    const int c = P->obs_camera[i], p = P->obs_point[i];
    if (c < 0 || c >= Nc || p < 0 || p >= Np) return bad_argument("bad observation index");
    optr[(size_t)c + 1]++;
  }
  for (int c = 0; c < Nc; ++c) optr[(size_t)c + 1] += optr[c];
  std::vector<int> chain_ptr, chain_views;
  build_view_chains(Nc, cam, P->camera_group, G, optr, view_mask, &chain_ptr, &chain_views);
  // Of the observations only the chains' views' go up, gathered in view-major order (ascending observation index
  // inside a view); the points go up whole (one sequential copy: renumbering the observed ones costs a random access
  // per observation on the host, more than the copy).
  std::vector<uint8_t> in_chain((size_t)Nc, 0);
  for (const int c : chain_views) in_chain[c] = 1;
  std::vector<long long> vptr((size_t)Nc + 1, 0);
  for (int c = 0; c < Nc; ++c) vptr[(size_t)c + 1] = vptr[c] + (in_chain[c] ? optr[(size_t)c + 1] - optr[c] : 0);
  const size_t M = (size_t)vptr[Nc];
  std::vector<unsigned long long> keys(M);
  std::vector<int> slot_pt(M);
  std::vector<double> xy(2 * M);
  if (M) {
    std::vector<long long> fill(vptr.begin(), vptr.end() - 1);
    for (int64_t i = 0; i < No; ++i) {
      const int c = P->obs_camera[i];
      if (!in_chain[c]) continue;
      const size_t o = (size_t)fill[c]++;
      keys[o] = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)o;
      slot_pt[o] = P->obs_point[i];
      xy[2 * o] = P->obs_xy[2 * i];
      xy[2 * o + 1] = P->obs_xy[2 * i + 1];
    }
  }
  int rc = s->open(O->device);
  if (rc) {
    g_last_error = s->error;
    return rc;
  }
  const hipStream_t stream = s->stream;
  ViewBatch B;
  memset(&B, 0, sizeof(B));
  int4* d_cam;
  long long* d_vptr;
  unsigned long long* d_keys;
  int* d_slot_pt;
  double *d_xy, *d_pts;
  TMI_HIP(s->upload(&B.ext, P->extrinsics, (size_t)6 * Nc));
  TMI_HIP(s->upload(&B.intr, P->intrinsics, (size_t)n_intr));
  TMI_HIP(s->upload(&d_cam, cam.data(), cam.size()));
  TMI_HIP(s->upload(&d_vptr, vptr.data(), vptr.size()));
  TMI_HIP(s->upload(&d_keys, keys.data(), keys.size()));
  TMI_HIP(s->upload(&d_slot_pt, slot_pt.data(), slot_pt.size()));
  TMI_HIP(s->upload(&d_xy, xy.data(), xy.size()));
  TMI_HIP(s->upload(&d_pts, M ? P->points : nullptr, M ? (size_t)4 * Np : 0));
  B.cam = d_cam;
  B.vptr = d_vptr;
  B.keys = d_keys;
  B.slot_pt = d_slot_pt;
  B.obs_xy = d_xy;
  B.pts = d_pts;
  rc = run_view_batch(s, B, O, Nc, cam, chain_ptr, chain_views,
                      {view_termination, view_iterations, view_initial_cost, view_final_cost}, sum);
  if (rc == TMI_BA_OK && Nc) {
    // the kernel wrote back exactly the usable views' cameras and their groups' free intrinsics
    TMI_HIP(s->download(P->extrinsics, B.ext, (size_t)6 * Nc));
    TMI_HIP(s->download(P->intrinsics, B.intr, (size_t)n_intr));
    TMI_HIP(hipStreamSynchronize(stream));
  }
  if (rc) g_last_error = s->error;
  sum->seconds = now_s() - t0;
  return rc;
}

// ---- batched TrackEstimator (track_estimate_kernels.h) ------------------------------------
void tmi_ba_track_estimator_options_init(tmi_ba_track_estimator_options* o) {
  if (!o) return;
  o->max_acceptable_reprojection_error_pixels = 5.0;  // estimate_track.h:63-70
  o->min_triangulation_angle_degrees = 3.0;
  o->bundle_adjustment = 1;
}

int32_t tmi_ba_solver_estimate_tracks(tmi_ba_solver* s, const tmi_ba_track_estimator_options* eo,
                                      const tmi_ba_options* O, const uint8_t* track_mask, int8_t* track_status,
                                      tmi_ba_track_estimate_summary* sum) {
  if (!s || !eo || !O || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const Structure& st = s->st;
  if (st.world > 1) {
    g_last_error = s->error = "track estimation needs every observation of a track: run it on an unsharded handle";
    return TMI_BA_ERR_INVALID_ARGUMENT;
  }
  if (O->point_dof != s->DP) {
    g_last_error = s->error = "track estimation: options->point_dof differs from the handle's";
    return TMI_BA_ERR_INVALID_ARGUMENT;
  }
  const double t0 = now_s();
  TMI_HIP(hipSetDevice(s->device));
  hipStream_t stream = s->stream;
  int rc = ensure_track_outputs(s);
  if (rc) return rc;
  const size_t npad = (size_t)st.Np_pad;
  // the caller's mask on the padded track order
  std::vector<unsigned char> attempt_h(npad, 0);
  for (size_t lp = 0; lp < npad; ++lp) {
    const int p = st.pt_orig[lp];
    if (p >= 0 && (!track_mask || track_mask[p])) attempt_h[lp] = 1;
  }
  OneShot scratch(stream);
  unsigned char* d_attempt = nullptr;
  signed char* d_status = nullptr;
  double* d_ray = nullptr;
  TMI_HIP(scratch.upload(&d_attempt, attempt_h.data(), npad));
  TMI_HIP(scratch.alloc(&d_status, npad));
  TMI_HIP(scratch.alloc(&d_ray, (size_t)3 * (size_t)std::max<int64_t>(st.No_pad, 1)));
  const double cos_min = std::cos(eo->min_triangulation_angle_degrees * (M_PI / 180.0));
  const double max_err = eo->max_acceptable_reprojection_error_pixels;
  StreamTimer timer(stream);
  TMI_HIP(timer.status);
  timer.mark();
  if (st.nslices > 0) {
    hipLaunchKernelGGL(track_rays_kernel, dim3(s->nblocks_tracks), dim3(256), 0, stream, s->v, d_attempt, d_ray);
    hipLaunchKernelGGL(track_triangulate_kernel, dim3(s->nblocks_tracks), dim3(256), 0, stream, s->v, d_attempt,
                       d_ray, cos_min, d_status);
    const signed char* term = nullptr;
    if (eo->bundle_adjustment) {
      // BundleAdjustTrack with the caller's options (DENSE_QR and no inner iterations change nothing for a
      // single track) on the tracks the triangulation accepted; the others are skipped like constant tracks
      prepare_cameras(s, s->v.ext, s->v.intr, s->v.prep);
      launch_track_lm(s, s->v, s->v.prep, small_lm_args(O), d_status);
      term = s->d_trk_term;
    }
    hipLaunchKernelGGL(track_accept_kernel, dim3(s->nblocks_tracks), dim3(256), 0, stream, s->v, max_err * max_err,
                       term, d_status);
  }
  timer.mark();
  ReadBack rb(stream);
  std::vector<signed char> status_h(npad);
  TMI_HIP(download(stream, status_h.data(), d_status, npad));
  TMI_HIP(rb.finish());
  auto count = [sum](int code) {
    if (code < 0) return;
    sum->num_attempts++;
    switch (code) {
      case 0: sum->num_estimated++; break;
      case 1: sum->num_bad_angle++; break;
      case 2: sum->num_failed_triangulation++; break;
      case 3: sum->num_failed_ba++; break;
      default: sum->num_bad_reprojection++; break;
    }
  };
  for (size_t lp = 0; lp < npad; ++lp) {
    const int p = st.pt_orig[lp];
    if (p < 0) continue;
    count(status_h[lp]);
    if (track_status) track_status[p] = (int8_t)status_h[lp];
  }
  // a track without observations has fewer than two views (estimate_track.cc:224-230)
  for (const int p : st.unobserved) {
    const int code = (!track_mask || track_mask[p]) ? 1 : -1;
    count(code);
    if (track_status) track_status[p] = (int8_t)code;
  }
  sum->kernel_seconds = timer.seconds();
  sum->seconds = now_s() - t0;
  return TMI_BA_OK;
}

int32_t tmi_ba_estimate_tracks(tmi_ba_problem* P, const tmi_ba_track_estimator_options* eo,
                               const tmi_ba_options* O, const uint8_t* track_mask, int8_t* track_status,
                               tmi_ba_track_estimate_summary* sum) {
  if (!P || !eo || !O || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is touched
  const int Nc = P->num_cameras, Np = P->num_points;
  const int64_t No = P->num_observations;
  if (Nc < 0 || P->num_groups < 0 || Np < 0 || No < 0) return bad_argument("negative size");
  if ((Nc && (!P->extrinsics || !P->camera_group)) || (Np && !P->points) ||
      (No && (!P->obs_camera || !P->obs_point || !P->obs_xy)))
    return bad_argument("missing array");
  if (O->point_dof != 3 && O->point_dof != 4) return bad_argument("point_dof must be 3 or 4");
  for (int64_t i = 0; i < No; ++i)
    if (P->obs_camera[i] < 0 || P->obs_camera[i] >= Nc || P->obs_point[i] < 0 || P->obs_point[i] >= Np)
      return bad_argument("observation index out of range");
  // constant points are never attempted, observed or not
  std::vector<uint8_t> mask;
  if (P->point_constant && P->num_points > 0) {
    mask.assign((size_t)P->num_points, 1);
    for (int p = 0; p < P->num_points; ++p)
      mask[p] = (uint8_t)((!track_mask || track_mask[p]) && !P->point_constant[p]);
  }
  const int rc = with_light_handle(P, O, P, [&](tmi_ba_solver* s) {
    return tmi_ba_solver_estimate_tracks(s, eo, O, mask.empty() ? track_mask : mask.data(), track_status, sum);
  });
  sum->seconds = now_s() - t0;
  return rc;
}

// BundleAdjustTwoViewsAngular for a batch of view pairs (two_view_kernels.h)
int32_t tmi_ba_adjust_two_views_angular(tmi_ba_two_view_angular_batch* Bh, int32_t max_num_iterations, int32_t device,
                                        int8_t* pair_termination, int32_t* pair_iterations,
                                        double* pair_initial_cost, double* pair_final_cost,
                                        tmi_ba_track_batch_summary* sum) {
  if (!Bh || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  if (Bh->num_pairs < 0 || max_num_iterations < 0) return TMI_BA_ERR_INVALID_ARGUMENT;
  const int P = Bh->num_pairs;
  if (P > 0 && (!Bh->rotation2 || !Bh->position2 || !Bh->correspondence_ptr)) return TMI_BA_ERR_INVALID_ARGUMENT;
  const int64_t N = P ? Bh->correspondence_ptr[P] : 0;
  for (int p = 0; p < P; ++p)
    if (Bh->correspondence_ptr[p + 1] < Bh->correspondence_ptr[p]) return TMI_BA_ERR_INVALID_ARGUMENT;
  if (N > 0 && (!Bh->features1 || !Bh->features2)) return TMI_BA_ERR_INVALID_ARGUMENT;
  return one_shot_batch(device, nullptr, P, t0, &sum->seconds, [&](OneShot* s) -> int {
    TwoViewAngularBatch B;
    memset(&B, 0, sizeof(B));
    B.num_pairs = P;
    double *d_f1, *d_f2;
    long long* d_cptr;
    TMI_HIP(s->upload(&B.rot2, Bh->rotation2, (size_t)3 * P));
    TMI_HIP(s->upload(&B.pos2, Bh->position2, (size_t)3 * P));
    TMI_HIP(s->upload(&d_f1, Bh->features1, (size_t)2 * N));
    TMI_HIP(s->upload(&d_f2, Bh->features2, (size_t)2 * N));
    TMI_HIP(s->upload(&d_cptr, (const long long*)Bh->correspondence_ptr, (size_t)P + 1));
    B.feat1 = d_f1;
    B.feat2 = d_f2;
    B.corr_ptr = d_cptr;
    SmallLmOut d;
    int rc = s->alloc_outputs(&d, (size_t)P);
    if (rc) return rc;
    const SmallLmArgs A = ceres_default_lm_args(max_num_iterations, TMI_BA_LOSS_TRIVIAL, 0.0);
    std::vector<signed char> term;
    rc = run_small_lm(s, s->stream, d, (size_t)P, nullptr, [&] {
      hipLaunchKernelGGL(two_view_angular_kernel, dim3((P + 3) / 4), dim3(256), 0, s->stream, B, A, d);
    }, ItemArrays{pair_termination, pair_iterations, pair_initial_cost, pair_final_cost}, sum, &sum->num_tracks, &term);
    if (rc) return rc;
    std::vector<double> rot((size_t)3 * P), pos((size_t)3 * P);
    TMI_HIP(s->download(rot.data(), B.rot2, rot.size()));
    TMI_HIP(s->download(pos.data(), B.pos2, pos.size()));
    TMI_HIP(hipStreamSynchronize(s->stream));
    for (int p = 0; p < P; ++p) {
      if (term[p] != 0 && term[p] != 1) continue;  // termination != FAILURE: write back
      for (int a = 0; a < 3; ++a) {
        Bh->rotation2[(size_t)3 * p + a] = rot[(size_t)3 * p + a];
        Bh->position2[(size_t)3 * p + a] = pos[(size_t)3 * p + a];
      }
    }
    return TMI_BA_OK;
  });
}

// OptimizeRelativePositionWithKnownRotation for a batch of view pairs (relative_position_kernels.h)
int32_t tmi_ba_optimize_relative_positions(tmi_ba_relative_position_batch* Bh, int32_t device, int8_t* pair_status,
                                           int32_t* pair_iterations, double* pair_cost, int32_t* pair_num_in_front,
                                           tmi_ba_track_batch_summary* sum) {
  if (!Bh || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is touched
  const int V = Bh->num_views, P = Bh->num_pairs;
  if (V < 0 || P < 0) return bad_argument("relative positions: negative size");
  if ((V > 0 && !Bh->view_rotation) || (P > 0 && (!Bh->pair_view1 || !Bh->pair_view2 || !Bh->correspondence_ptr ||
                                                   !Bh->position2)))
    return bad_argument("relative positions: missing array");
  if ((Bh->view_model != nullptr) != (Bh->view_intrinsics != nullptr))
    return bad_argument("relative positions: view_model and view_intrinsics come together");
  const bool pixels = Bh->view_model != nullptr;
  if (pixels)
    for (int v = 0; v < V; ++v)
      if (Bh->view_model[v] < TMI_BA_PINHOLE || Bh->view_model[v] > TMI_BA_DIVISION_UNDISTORTION)
        return bad_argument("relative positions: unknown camera model");
  // pairs too long for the kernel's registers keep their columns in a scratch plane
  std::vector<long long> sptr((size_t)std::max(P, 0), -1);
  long long slen = 0;
  for (int p = 0; p < P; ++p) {
    if (Bh->correspondence_ptr[p + 1] < Bh->correspondence_ptr[p] || Bh->correspondence_ptr[p] < 0)
      return bad_argument("relative positions: correspondence_ptr decreases");
    if (Bh->pair_view1[p] < 0 || Bh->pair_view1[p] >= V || Bh->pair_view2[p] < 0 || Bh->pair_view2[p] >= V)
      return bad_argument("relative positions: view index out of range");
    const long long n = Bh->correspondence_ptr[p + 1] - Bh->correspondence_ptr[p];
    if (n > 64LL * kRelPosRegColumns) {
      sptr[p] = slen;
      slen += n;
    }
  }
  const int64_t N = P ? Bh->correspondence_ptr[P] : 0;
  if (N > 0 && (!Bh->features1 || !Bh->features2)) return bad_argument("relative positions: missing array");
  return one_shot_batch(device, "relative positions: no such device", P, t0, &sum->seconds, [&](OneShot* s) -> int {
    RelativePositionBatch B;
    memset(&B, 0, sizeof(B));
    B.num_pairs = P;
    double *d_rot, *d_intr = nullptr, *d_f1, *d_f2;
    int *d_model = nullptr, *d_v1, *d_v2;
    long long *d_cptr, *d_sptr;
    TMI_HIP(s->upload(&d_rot, Bh->view_rotation, (size_t)3 * V));
    TMI_HIP(s->upload(&d_v1, (const int*)Bh->pair_view1, (size_t)P));
    TMI_HIP(s->upload(&d_v2, (const int*)Bh->pair_view2, (size_t)P));
    TMI_HIP(s->upload(&d_cptr, (const long long*)Bh->correspondence_ptr, (size_t)P + 1));
    TMI_HIP(s->upload(&d_sptr, (const long long*)sptr.data(), (size_t)P));
    TMI_HIP(s->upload(&d_f1, Bh->features1, (size_t)2 * N));
    TMI_HIP(s->upload(&d_f2, Bh->features2, (size_t)2 * N));
    if (pixels) {
      TMI_HIP(s->upload(&d_model, (const int*)Bh->view_model, (size_t)V));
      TMI_HIP(s->upload(&d_intr, Bh->view_intrinsics, (size_t)10 * V));
    }
    B.view_rot = d_rot;
    B.view_model = d_model;
    B.view_intr = d_intr;
    B.pair_view1 = d_v1;
    B.pair_view2 = d_v2;
    B.corr_ptr = d_cptr;
    B.feat1 = d_f1;
    B.feat2 = d_f2;
    B.scratch_ptr = d_sptr;
    B.scratch_len = slen;
    TMI_HIP(s->alloc(&B.scratch, (size_t)3 * (size_t)slen));
    TMI_HIP(s->alloc(&B.pos2, (size_t)3 * P));
    TMI_HIP(s->alloc(&B.status, (size_t)P));
    TMI_HIP(s->alloc(&B.iters, (size_t)P));
    TMI_HIP(s->alloc(&B.cost, (size_t)P));
    TMI_HIP(s->alloc(&B.in_front, (size_t)P));
    double *d_n1 = nullptr, *d_n2 = nullptr;
    if (pixels) {
      TMI_HIP(s->alloc(&d_n1, (size_t)2 * N));
      TMI_HIP(s->alloc(&d_n2, (size_t)2 * N));
    }
    StreamTimer timer(s->stream);
    TMI_HIP(timer.status);
    timer.mark();
    if (pixels) {
      hipLaunchKernelGGL(relative_position_normalise_kernel, dim3((P + 3) / 4), dim3(256), 0, s->stream, B, d_n1, d_n2);
      B.feat1 = d_n1;
      B.feat2 = d_n2;
    }
    hipLaunchKernelGGL(relative_position_kernel, dim3((P + 3) / 4), dim3(256), 0, s->stream, B);
    timer.mark();
    ReadBack rb(s->stream);
    std::vector<double> pos((size_t)3 * P), cost((size_t)P);
    std::vector<signed char> status((size_t)P);
    std::vector<int> iters((size_t)P), front((size_t)P);
    rb.add(pos.data(), B.pos2, pos.size());
    rb.add(cost.data(), B.cost, cost.size());
    rb.add(status.data(), B.status, status.size());
    rb.add(iters.data(), B.iters, iters.size());
    rb.add(front.data(), B.in_front, front.size());
    TMI_HIP(rb.finish());
    for (int p = 0; p < P; ++p) {
      const int st = status[p];
      if (st >= 0) {
        sum->num_tracks++;
        sum->total_iterations += iters[p];
      }
      if (st == 0 || st == 1) {  // the reference returns the position for both
        sum->num_success++;
        for (int a = 0; a < 3; ++a) Bh->position2[(size_t)3 * p + a] = pos[(size_t)3 * p + a];
      }
      if (pair_status) pair_status[p] = (int8_t)st;
      if (pair_iterations) pair_iterations[p] = iters[p];
      if (pair_cost) pair_cost[p] = cost[p];
      if (pair_num_in_front) pair_num_in_front[p] = front[p];
    }
    sum->kernel_seconds = timer.seconds();
    return TMI_BA_OK;
  });
}

// SelectGoodTracksForBundleAdjustment (select_good_tracks_for_bundle_adjustment.cc:251-327):
// the projections (track statistics) run on the device, the per-view grid / ranking logic --
// integer compares over the view's feature list -- on the host.
int32_t tmi_ba_solver_select_good_tracks(tmi_ba_solver* s, int32_t long_track_length_threshold,
                                         int32_t image_grid_cell_size_pixels,
                                         int32_t min_num_optimized_tracks_per_view,
                                         const uint8_t* view_mask, uint8_t* selected,
                                         int32_t* stats_len, double* stats_err,
                                         tmi_ba_select_summary* sum) {
  if (!s || !sum || !selected || image_grid_cell_size_pixels <= 0) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const Structure& st = s->st;
  if (st.world > 1) {
    g_last_error = s->error = "track selection ranks every view's tracks: run it on an unsharded handle";
    return TMI_BA_ERR_UNSUPPORTED;
  }
  const double t0 = now_s();
  TMI_HIP(hipSetDevice(s->device));
  int rc = ensure_track_outputs(s);
  if (rc) return rc;
  StreamTimer timer(s->stream);
  TMI_HIP(timer.status);
  TMI_HIP(timer.mark());
  prepare_cameras(s, s->v.ext, s->v.intr, s->v.prep);
  if (st.nslices > 0)
    hipLaunchKernelGGL(track_stats_kernel, dim3(s->nblocks_tracks), dim3(256), 0, s->stream, s->v, s->v.prep,
                       s->d_trk_iter, s->d_trk_mean);
  TMI_HIP(timer.mark());
  const int Np = st.Np_total, Nc = st.Nc;
  hipStream_t stream = s->stream;
  // static per handle: every view's tracks sorted by track index ((view, track) keys), and the selection's arrays.
  // Marked ready only once every part exists, as the view-major index of tmi_ba_solver_adjust_views is.
  if (!s->select_index_ready) {
    if ((rc = dev_alloc(s, &s->d_vt_ptr, (size_t)Nc + 2))) return rc;
    if ((rc = dev_alloc(s, &s->d_vt_keys, (size_t)std::max<int64_t>(st.No_pad, 1)))) return rc;
    if ((rc = dev_alloc(s, &s->d_vbox, (size_t)std::max(Nc, 1) * 4))) return rc;
    if ((rc = dev_alloc(s, &s->d_cell_off, (size_t)Nc + 2))) return rc;
    if ((rc = dev_alloc(s, &s->d_sel, (size_t)std::max(Np, 1)))) return rc;
    if ((rc = dev_alloc(s, &s->d_view_mask, (size_t)std::max(Nc, 1)))) return rc;
    if ((rc = dev_alloc(s, &s->d_vcount, (size_t)2 * std::max(Nc, 1)))) return rc;
    rc = build_view_index(s, [&](unsigned long long* keys) {
      hipLaunchKernelGGL(select_keys_kernel, dim3(s->nblocks_slices), dim3(256), 0, stream, s->v, s->d_pt_orig, keys);
    }, s->d_vt_keys, s->d_vt_ptr);
    if (rc) return rc;
    s->select_index_ready = true;
  }
  SelectView S;
  memset(&S, 0, sizeof(S));
  S.Nc = Nc;
  S.Np_total = Np;
  S.view_mask = nullptr;
  if (view_mask && Nc > 0) {
    TMI_HIP(hipMemcpyAsync(s->d_view_mask, view_mask, (size_t)Nc, hipMemcpyHostToDevice, stream));
    S.view_mask = s->d_view_mask;
  }
  S.pt_orig = s->d_pt_orig;
  S.cnt = s->d_trk_iter;
  S.mean = s->d_trk_mean;
  S.long_thr = long_track_length_threshold;
  S.inv_cell = 1.0 / image_grid_cell_size_pixels;
  S.vbox = s->d_vbox;
  S.cell_off = s->d_cell_off;
  S.sel = s->d_sel;
  S.counters = s->d_counters;
  const int nb_init = (std::max(std::max(Nc, Np), 4) + 255) / 256;
  hipLaunchKernelGGL(select_init_kernel, dim3(nb_init), dim3(256), 0, stream, S);
  if (st.nslices > 0) hipLaunchKernelGGL(select_bounds_kernel, dim3(s->nblocks_tracks), dim3(256), 0, stream, s->v, S);
  hipLaunchKernelGGL(select_offsets_kernel, dim3(1), dim3(1024), 0, stream, S);
  TMI_HIP(download(stream, s->h_cell_total, s->d_cell_off + Nc, 1));
  TMI_HIP(hipStreamSynchronize(stream));
  const long long ncells = *s->h_cell_total;
  if (ncells > ((long long)1 << 31)) {
    g_last_error = s->error = "track selection: the image grids need more than 2^31 cells (cell size too small "
                              "for the pixel range of the features)";
    return TMI_BA_ERR_UNSUPPORTED;
  }
  if (ncells > s->cell_capacity) {
    for (void* p : s->cell_allocs) hipFree(p);
    s->cell_allocs.clear();
    s->cell_capacity = 0;
    const size_t cap = (size_t)(ncells + ncells / 4 + 1024);
    TMI_HIP(hipMalloc((void**)&s->d_cell_len, cap * sizeof(unsigned)));
    s->cell_allocs.push_back(s->d_cell_len);
    TMI_HIP(hipMalloc((void**)&s->d_cell_err, cap * sizeof(unsigned long long)));
    s->cell_allocs.push_back(s->d_cell_err);
    TMI_HIP(hipMalloc((void**)&s->d_cell_trk, cap * sizeof(unsigned)));
    s->cell_allocs.push_back(s->d_cell_trk);
    s->cell_capacity = (long long)cap;
  }
  S.cell_len = s->d_cell_len;
  S.cell_err = s->d_cell_err;
  S.cell_trk = s->d_cell_trk;
  if (ncells > 0) {
    const unsigned nbc = (unsigned)((ncells + 255) / 256);
    hipLaunchKernelGGL(select_fill_cells_kernel, dim3(nbc), dim3(256), 0, stream, S, ncells);
    hipLaunchKernelGGL(select_cells_kernel<1>, dim3(s->nblocks_tracks), dim3(256), 0, stream, s->v, S);
    hipLaunchKernelGGL(select_cells_kernel<2>, dim3(s->nblocks_tracks), dim3(256), 0, stream, s->v, S);
    hipLaunchKernelGGL(select_cells_kernel<3>, dim3(s->nblocks_tracks), dim3(256), 0, stream, s->v, S);
    hipLaunchKernelGGL(select_mark_kernel, dim3(nbc), dim3(256), 0, stream, S, ncells);
  }
  if (Nc > 0 && st.No_pad > 0) {
    hipLaunchKernelGGL(select_view_count_kernel, dim3(Nc), dim3(256), 0, stream, S, s->d_vt_keys, s->d_vt_ptr, s->d_vcount);
    // the flags of all tracks as a bit vector in LDS when they fit beside the kernel's static 4 KB
    const size_t bit_bytes = ((size_t)Np + 31) / 32 * 4;
    if (bit_bytes <= 152 * 1024) {
      static bool attr_set = false;
      if (!attr_set) {
        TMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&select_topup_kernel<true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
        attr_set = true;
      }
      hipLaunchKernelGGL(select_topup_kernel<true>, dim3(1), dim3(kTopupThreads), bit_bytes, stream, S, s->d_vt_keys,
                         s->d_vt_ptr, s->d_vcount, s->d_vcount + Nc, min_num_optimized_tracks_per_view);
    } else {
      hipLaunchKernelGGL(select_topup_kernel<false>, dim3(1), dim3(kTopupThreads), 0, stream, S, s->d_vt_keys, s->d_vt_ptr,
                         s->d_vcount, s->d_vcount + Nc, min_num_optimized_tracks_per_view);
    }
  }
  if (Np > 0) hipLaunchKernelGGL(select_finish_kernel, dim3((Np + 255) / 256), dim3(256), 0, stream, S, s->d_out_u8);
  if ((stats_len || stats_err) && st.Np_pad > 0) {
    // tracks without observations keep length 0 / NaN error
    if (stats_len) TMI_HIP(hipMemsetAsync(s->d_out_i32, 0, (size_t)Np * sizeof(int), stream));
    if (stats_err) TMI_HIP(hipMemsetAsync(s->d_out_f64, 0xff, (size_t)Np * sizeof(double), stream));
    hipLaunchKernelGGL(scatter_track_stats_kernel, dim3((st.Np_pad + 255) / 256), dim3(256), 0, stream, s->d_pt_orig,
                       st.Np_pad, s->d_trk_iter, s->d_trk_mean, long_track_length_threshold,
                       stats_len ? s->d_out_i32 : nullptr, stats_err ? s->d_out_f64 : nullptr);
  }
  TMI_HIP(download(stream, s->h_counters, s->d_counters, 4));
  unsigned char* stage_u8 = s->h_stage;
  int* stage_i32 = reinterpret_cast<int*>(s->h_stage + 4 * (size_t)std::max(Np, 1));
  double* stage_f64 = reinterpret_cast<double*>(s->h_stage + 8 * (size_t)std::max(Np, 1));
  TMI_HIP(download(stream, stage_u8, s->d_out_u8, (size_t)Np));
  if (stats_len) TMI_HIP(download(stream, stage_i32, s->d_out_i32, (size_t)Np));
  if (stats_err) TMI_HIP(download(stream, stage_f64, s->d_out_f64, (size_t)Np));
  TMI_HIP(hipStreamSynchronize(stream));
  if (Np > 0) memcpy(selected, stage_u8, (size_t)Np);
  if (stats_len && Np > 0) memcpy(stats_len, stage_i32, (size_t)Np * sizeof(int));
  if (stats_err && Np > 0) memcpy(stats_err, stage_f64, (size_t)Np * sizeof(double));
  sum->kernel_seconds = timer.seconds();
  if (stats_err)  // 0xff.. is a NaN pattern; make it the quiet NaN the host path produced
    for (const int p : st.unobserved) stats_err[p] = std::nan("");
  sum->num_tracks = Np;
  sum->num_selected_grid = s->h_counters[0];
  sum->num_selected = s->h_counters[1];
  sum->seconds = now_s() - t0;
  return TMI_BA_OK;
}

int32_t tmi_ba_select_good_tracks(const tmi_ba_problem* P, int32_t device,
                                  int32_t long_track_length_threshold,
                                  int32_t image_grid_cell_size_pixels,
                                  int32_t min_num_optimized_tracks_per_view,
                                  const uint8_t* view_mask, uint8_t* selected,
                                  int32_t* stats_len, double* stats_err, tmi_ba_select_summary* sum) {
  if (!P || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  tmi_ba_options O;
  tmi_ba_options_init(&O);
  O.device = device;
  const int rc = with_light_handle(P, &O, nullptr, [&](tmi_ba_solver* s) {
    return tmi_ba_solver_select_good_tracks(s, long_track_length_threshold, image_grid_cell_size_pixels,
                                            min_num_optimized_tracks_per_view, view_mask, selected, stats_len,
                                            stats_err, sum);
  });
  sum->seconds = now_s() - t0;
  return rc;
}

// ---- batched two-view bundle adjustment and verification ----------------
}  // extern "C"
namespace {
// Argument errors of a two-view batch and its solve options, before the device is touched.
int validate_two_view_batch(const tmi_ba_two_view_batch* Bh, int point_dof, int max_num_iterations) {
  if (point_dof != 3 && point_dof != 4) return bad_argument("two views: point_dof must be 3 or 4");
  if (Bh->num_pairs < 0 || max_num_iterations < 0) return bad_argument("two views: negative size or iteration limit");
  const int P = Bh->num_pairs;
  if (P > 0 && (!Bh->extrinsics1 || !Bh->extrinsics2 || !Bh->model1 || !Bh->model2 || !Bh->intrinsics1 ||
                !Bh->intrinsics2 || !Bh->correspondence_ptr))
    return bad_argument("two views: missing array");
  for (int p = 0; p < P; ++p) {
    if (Bh->correspondence_ptr[p + 1] < Bh->correspondence_ptr[p])
      return bad_argument("two views: correspondence_ptr decreases");
    if (Bh->model1[p] < 0 || Bh->model1[p] > 4 || Bh->model2[p] < 0 || Bh->model2[p] > 4)
      return bad_argument("two views: unknown camera model");
  }
  if (P > 0 && Bh->correspondence_ptr[P] > 0 && (!Bh->features1 || !Bh->features2 || !Bh->points))
    return bad_argument("two views: missing array");
  return TMI_BA_OK;
}

// A caller's pairs on the device, all but the points.  upload() only queues the copies: the defaults of absent
// constant_intrinsics ("constant") are read from const_h until the stream is next synchronised.
struct TwoViewUpload {
  TwoViewBatch B;
  size_t Nn;  // correspondences, at least 1: the size unit of the per-correspondence buffers
  std::vector<unsigned char> const_h[2];
  int upload(OneShot* s, const tmi_ba_two_view_batch* Bh) {
    const int P = Bh->num_pairs;
    const int64_t N = Bh->correspondence_ptr[P];
    Nn = (size_t)std::max<int64_t>(N, 1);
    const uint8_t* const given[2] = {Bh->constant_intrinsics1, Bh->constant_intrinsics2};
    for (int v = 0; v < 2; ++v) {
      const_h[v].assign((size_t)P, 1);
      if (given[v]) const_h[v].assign(given[v], given[v] + P);
    }
    memset(&B, 0, sizeof(B));
    B.num_pairs = P;
    double *d_e1, *d_f1, *d_f2;
    int *d_m1, *d_m2;
    unsigned char *d_c1, *d_c2;
    long long* d_cptr;
    TMI_HIP(s->upload(&d_e1, Bh->extrinsics1, (size_t)6 * P));
    TMI_HIP(s->upload(&B.ext2, (const double*)Bh->extrinsics2, (size_t)6 * P));
    TMI_HIP(s->upload(&d_m1, Bh->model1, (size_t)P));
    TMI_HIP(s->upload(&d_m2, Bh->model2, (size_t)P));
    TMI_HIP(s->upload(&B.intr1, (const double*)Bh->intrinsics1, (size_t)10 * P));
    TMI_HIP(s->upload(&B.intr2, (const double*)Bh->intrinsics2, (size_t)10 * P));
    TMI_HIP(s->upload(&d_c1, (const unsigned char*)const_h[0].data(), (size_t)P));
    TMI_HIP(s->upload(&d_c2, (const unsigned char*)const_h[1].data(), (size_t)P));
    TMI_HIP(s->upload(&d_cptr, (const long long*)Bh->correspondence_ptr, (size_t)P + 1));
    TMI_HIP(s->upload(&d_f1, Bh->features1, (size_t)2 * N));
    TMI_HIP(s->upload(&d_f2, Bh->features2, (size_t)2 * N));
    B.ext1 = d_e1; B.model1 = d_m1; B.model2 = d_m2; B.const1 = d_c1; B.const2 = d_c2; B.corr_ptr = d_cptr;
    B.feat1 = d_f1; B.feat2 = d_f2;
    return TMI_BA_OK;
  }
};

// (two_view_lm_kernel keeps its own argument layout: two_view_kernels.h)
TwoViewArgs two_view_args(const SmallLmArgs& L, int point_dof) {
  TwoViewArgs A;
  A.point_dof = point_dof;
  A.max_num_iterations = L.max_num_iterations;
  A.jacobi_scaling = L.jacobi_scaling;
  A.function_tolerance = L.function_tolerance;
  A.gradient_tolerance = L.gradient_tolerance;
  A.parameter_tolerance = L.parameter_tolerance;
  A.initial_radius = L.initial_radius;
  A.max_radius = L.max_radius;
  A.min_radius = L.min_radius;
  A.min_relative_decrease = L.min_relative_decrease;
  A.lm_lo = L.lm_lo;
  A.lm_hi = L.lm_hi;
  A.max_num_consecutive_invalid_steps = L.max_num_consecutive_invalid_steps;
  return A;
}

template <int DP>
void launch_two_view_lm(hipStream_t stream, const TwoViewBatch& B, const TwoViewArgs& A, const SmallLmOut& d,
                        const long long* corr_end) {
  hipLaunchKernelGGL(two_view_lm_kernel<DP>, dim3((B.num_pairs + 3) / 4), dim3(256), 0, stream, B, A, d.term, d.iters,
                     d.c0, d.c1, corr_end);
}

// What a solve may change of a pair's cameras: camera 2 and the two focal lengths.  download() queues the copies.
struct TwoViewCameras {
  std::vector<double> e2, k1, k2;
  int download(OneShot* s, const TwoViewBatch& B) {
    const size_t P = (size_t)B.num_pairs;
    e2.resize(6 * P);
    k1.resize(10 * P);
    k2.resize(10 * P);
    TMI_HIP(s->download(e2.data(), B.ext2, e2.size()));
    TMI_HIP(s->download(k1.data(), B.intr1, k1.size()));
    TMI_HIP(s->download(k2.data(), B.intr2, k2.size()));
    return TMI_BA_OK;
  }
  void write_back(tmi_ba_two_view_batch* Bh, int p) const {
    for (int a = 0; a < 6; ++a) Bh->extrinsics2[(size_t)6 * p + a] = e2[(size_t)6 * p + a];
    Bh->intrinsics1[(size_t)10 * p] = k1[(size_t)10 * p];
    Bh->intrinsics2[(size_t)10 * p] = k2[(size_t)10 * p];
  }
};
}  // namespace
extern "C" {

int32_t tmi_ba_adjust_two_views(tmi_ba_two_view_batch* Bh, int32_t point_dof, int32_t max_num_iterations,
                                int32_t device, int8_t* pair_termination, int32_t* pair_iterations,
                                double* pair_initial_cost, double* pair_final_cost,
                                tmi_ba_track_batch_summary* sum) {
  if (!Bh || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  if (const int bad = validate_two_view_batch(Bh, point_dof, max_num_iterations)) return bad;
  const int P = Bh->num_pairs;
  return one_shot_batch(device, nullptr, P, t0, &sum->seconds, [&](OneShot* s) -> int {
    const int64_t N = Bh->correspondence_ptr[P];
    TwoViewUpload up;
    int rc = up.upload(s, Bh);
    if (rc) return rc;
    TwoViewBatch& B = up.B;
    TMI_HIP(s->upload(&B.points, (const double*)Bh->points, (size_t)4 * N));
    TMI_HIP(s->alloc(&B.points_c, 4 * up.Nn));
    TMI_HIP(s->alloc(&B.scale_p, 4 * up.Nn));
    SmallLmOut d;
    if ((rc = s->alloc_outputs(&d, (size_t)P))) return rc;
    const TwoViewArgs A = two_view_args(ceres_default_lm_args(max_num_iterations, TMI_BA_LOSS_TRIVIAL, 0.0), point_dof);
    std::vector<signed char> term;
    rc = run_small_lm(s, s->stream, d, (size_t)P, nullptr, [&] {
      if (point_dof == 3)
        launch_two_view_lm<3>(s->stream, B, A, d, nullptr);
      else
        launch_two_view_lm<4>(s->stream, B, A, d, nullptr);
    }, ItemArrays{pair_termination, pair_iterations, pair_initial_cost, pair_final_cost}, sum, &sum->num_tracks, &term);
    if (rc) return rc;
    TwoViewCameras cams;
    std::vector<double> pts((size_t)4 * N);
    if ((rc = cams.download(s, B))) return rc;
    TMI_HIP(s->download(pts.data(), B.points, pts.size()));
    TMI_HIP(hipStreamSynchronize(s->stream));
    for (int p = 0; p < P; ++p) {
      if (term[p] != 0 && term[p] != 1) continue;  // IsSolutionUsable: write back
      cams.write_back(Bh, p);
      for (int64_t q = Bh->correspondence_ptr[p]; q < Bh->correspondence_ptr[p + 1]; ++q)
        for (int a = 0; a < 4; ++a) Bh->points[4 * q + a] = pts[4 * q + a];
    }
    return TMI_BA_OK;
  });
}

// ---- batched two-view verification BA: triangulate, adjust, filter (two_view_verify_kernels.h) ----
void tmi_ba_two_view_verification_options_init(tmi_ba_two_view_verification_options* o) {
  if (!o) return;
  o->min_num_inlier_matches = 30;
  o->triangulation_max_reprojection_error = 15.0;
  o->min_triangulation_angle_degrees = 4.0;
  o->final_max_reprojection_error = 5.0;
  o->bundle_adjustment = 1;
}

int32_t tmi_ba_verify_two_views(tmi_ba_two_view_batch* Bh, const tmi_ba_two_view_verification_options* vo,
                                int32_t point_dof, int32_t max_num_iterations, int32_t device,
                                int8_t* correspondence_status, int8_t* pair_status, int32_t* pair_num_verified,
                                int8_t* pair_termination, int32_t* pair_iterations, double* pair_initial_cost,
                                double* pair_final_cost, tmi_ba_two_view_verification_summary* sum) {
  if (!Bh || !vo || !sum) return TMI_BA_ERR_INVALID_ARGUMENT;
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  if (const int bad = validate_two_view_batch(Bh, point_dof, max_num_iterations)) return bad;
  if (vo->min_num_inlier_matches < 0) return bad_argument("two-view verification: negative min_num_inlier_matches");
  const int P = Bh->num_pairs;
  if (P > 0 && Bh->correspondence_ptr[0] < 0) return bad_argument("two-view verification: negative correspondence_ptr");
  return one_shot_batch(device, nullptr, P, t0, &sum->seconds, [&](OneShot* s) -> int {
    sum->num_pairs = P;
    const int64_t N = Bh->correspondence_ptr[P];
    TwoViewUpload up;  // the caller's correspondences: what the triangulation reads
    int rc = up.upload(s, Bh);
    if (rc) return rc;
    const TwoViewBatch& B = up.B;
    const size_t Nn = up.Nn;
    TwoViewVerifyBuffers O;
    TMI_HIP(s->alloc(&O.feat1_c, 2 * Nn));
    TMI_HIP(s->alloc(&O.feat2_c, 2 * Nn));
    TMI_HIP(s->alloc(&O.points_c, 4 * Nn));
    TMI_HIP(s->alloc(&O.orig, Nn));
    TMI_HIP(s->alloc(&O.corr_end, (size_t)P));
    TMI_HIP(s->alloc(&O.points_out, 4 * Nn));
    TMI_HIP(s->alloc_filled(&O.corr_status, Nn, 0xff));
    TMI_HIP(s->alloc(&O.pair_status, (size_t)P));
    TMI_HIP(s->alloc(&O.pair_count, (size_t)P));
    TwoViewBatch C = B;  // the compacted survivors: what the solve and the last filter read
    C.feat1 = O.feat1_c;
    C.feat2 = O.feat2_c;
    C.points = O.points_c;
    TMI_HIP(s->alloc(&C.points_c, 4 * Nn));
    TMI_HIP(s->alloc(&C.scale_p, 4 * Nn));
    SmallLmOut d;
    if ((rc = s->alloc_outputs(&d, (size_t)P))) return rc;
    const TwoViewArgs A = two_view_args(ceres_default_lm_args(max_num_iterations, TMI_BA_LOSS_TRIVIAL, 0.0), point_dof);
    TwoViewVerifyArgs V;
    V.min_matches = vo->min_num_inlier_matches;
    V.cos_min = std::cos(vo->min_triangulation_angle_degrees * (M_PI / 180.0));
    V.tri_max_sq = vo->triangulation_max_reprojection_error * vo->triangulation_max_reprojection_error;
    V.final_max_sq = vo->final_max_reprojection_error * vo->final_max_reprojection_error;
    const bool ba = vo->bundle_adjustment != 0;
    StreamTimer split(s->stream, 3);  // marks between the launches: the split of kernel_seconds
    TMI_HIP(split.status);
    tmi_ba_track_batch_summary lm_sum;
    memset(&lm_sum, 0, sizeof(lm_sum));
    int64_t num_solved = 0;
    const dim3 grid((P + 3) / 4), block(256);
    rc = run_small_lm(s, s->stream, d, (size_t)P, nullptr, [&] {
      split.mark();
      hipLaunchKernelGGL(two_view_triangulate_kernel, grid, block, 0, s->stream, B, V, O);
      split.mark();
      if (!ba) return;
      if (point_dof == 3)
        launch_two_view_lm<3>(s->stream, C, A, d, O.corr_end);
      else
        launch_two_view_lm<4>(s->stream, C, A, d, O.corr_end);
      split.mark();
      hipLaunchKernelGGL(two_view_accept_kernel, grid, block, 0, s->stream, C, V, O, (const signed char*)d.term);
    }, ItemArrays{pair_termination, pair_iterations, pair_initial_cost, pair_final_cost}, &lm_sum, &num_solved);
    if (rc) return rc;
    sum->kernel_seconds = lm_sum.kernel_seconds;
    sum->triangulate_kernel_seconds = split.seconds(0, 1);
    sum->solve_kernel_seconds = ba ? split.seconds(1, 2) : 0.0;
    sum->accept_kernel_seconds =
        ba ? std::max(0.0, sum->kernel_seconds - sum->triangulate_kernel_seconds - sum->solve_kernel_seconds) : 0.0;
    sum->total_iterations = lm_sum.total_iterations;
    TwoViewCameras cams;
    std::vector<double> pts((size_t)4 * N);
    std::vector<signed char> cst((size_t)N), pst((size_t)P);
    std::vector<int> cnt((size_t)P);
    if ((rc = cams.download(s, B))) return rc;
    TMI_HIP(s->download(pst.data(), O.pair_status, pst.size()));
    TMI_HIP(s->download(cnt.data(), O.pair_count, cnt.size()));
    TMI_HIP(s->download(pts.data(), O.points_out, pts.size()));
    TMI_HIP(s->download(cst.data(), O.corr_status, cst.size()));
    TMI_HIP(hipStreamSynchronize(s->stream));
    int64_t* const pair_counter[5] = {&sum->num_pairs_verified, &sum->num_pairs_too_few_matches,
                                      &sum->num_pairs_too_few_triangulated, &sum->num_pairs_failed_ba,
                                      &sum->num_pairs_too_few_verified};
    int64_t* const corr_counter[5] = {&sum->num_verified, &sum->num_bad_triangulation_angles,
                                      &sum->num_failed_triangulations, &sum->num_bad_reprojection_errors,
                                      &sum->num_bad_final_reprojection_errors};
    for (int p = 0; p < P; ++p) {
      const int st = pst[p];
      ++*pair_counter[st];
      if (pair_status) pair_status[p] = (int8_t)st;
      if (pair_num_verified) pair_num_verified[p] = cnt[p];
      if (ba && (st == 0 || st == 4)) cams.write_back(Bh, p);  // :316-321 run before the last test of VerifyMatches
    }
    for (int64_t q = 0; q < N; ++q) {
      const int st = cst[q];
      if (correspondence_status) correspondence_status[q] = (int8_t)st;
      if (st < 0) continue;
      ++sum->num_correspondences;
      ++*corr_counter[st];
      if (st == 0 || st == 4)
        for (int a = 0; a < 4; ++a) Bh->points[4 * q + a] = pts[4 * q + a];
    }
    return TMI_BA_OK;
  });
}

// ---- the view-pair filters (view_pair_filter_kernels.h) --------------------------------------
}  // extern "C"
namespace {
// The axis generator documented at tmi_ba_filter_view_pairs_from_relative_translation.
struct AxisDeviates {
  uint64_t state;
  double spare = 0.0;
  bool has_spare = false;
  explicit AxisDeviates(uint64_t seed) : state(seed) {}
  double uniform() {
    uint64_t z = (state += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  }
  double normal() {
    if (has_spare) {
      has_spare = false;
      return spare;
    }
    const double u1 = uniform(), u2 = uniform();
    const double r = std::sqrt(-2.0 * std::log(u1)), a = 2.0 * M_PI * u2;
    spare = r * std::sin(a);
    has_spare = true;
    return r * std::cos(a);
  }
};

// The view count up to which mfas_order_kernel keeps its state in LDS (TMI_BA_1DSFM_LDS_VIEWS lowers it: a
// diagnostic knob, so that a small graph reaches the global-memory path).
int mfas_lds_view_cap() {
  int cap = kMfasLdsViews;
  if (const char* e = getenv("TMI_BA_1DSFM_LDS_VIEWS")) cap = std::max(0, std::min(cap, atoi(e)));
  return cap;
}
}  // namespace
extern "C" {

void tmi_ba_translation_filter_options_init(tmi_ba_translation_filter_options* o) {
  if (!o) return;
  o->num_iterations = 48;  // filter_view_pairs_from_relative_translation.h:59-64
  o->translation_projection_tolerance = 0.08;
  o->seed = 0;
}

int32_t tmi_ba_filter_view_pairs_from_relative_translation(const tmi_ba_view_pair_batch* Bh,
                                                           const tmi_ba_translation_filter_options* opt, double* axes,
                                                           int32_t axes_given, int32_t device, uint8_t* pair_removed,
                                                           double* pair_bad_weight, double* rotated_translation,
                                                           int32_t* iteration_order,
                                                           tmi_ba_view_pair_filter_summary* sum) {
  if (!Bh || !opt || !sum) return bad_argument("translation filter: null batch, options or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is touched
  if (const char* why = check_view_pair_batch(Bh, false, Bh->pair_position2)) return bad_argument(why);
  const int V = Bh->num_views, E = Bh->num_pairs, K = opt->num_iterations;
  if (K < 1) return bad_argument("translation filter: num_iterations < 1");
  if (axes_given && !axes) return bad_argument("translation filter: axes_given without axes");
  if (axes_given && !all_finite(axes, (size_t)3 * K)) return bad_argument("translation filter: non-finite axis");
  if (!std::isfinite(opt->translation_projection_tolerance))
    return bad_argument("translation filter: non-finite tolerance");
  if (!axes_given && E == 1) return bad_argument("translation filter: the variance of one translation is undefined");
  if ((int64_t)K * V > INT32_MAX) return bad_argument("translation filter: num_iterations * num_views exceeds 2^31");
  // the CSR of the undirected graph: both rows of an edge in ascending edge index
  std::vector<int> row_ptr((size_t)V + 1, 0);
  std::vector<int2> row((size_t)2 * E);
  int ordered = 0;
  if (E > 0) {
    for (int e = 0; e < E; ++e) {
      row_ptr[(size_t)Bh->pair_view1[e] + 1]++;
      row_ptr[(size_t)Bh->pair_view2[e] + 1]++;
    }
    for (int v = 0; v < V; ++v) {
      ordered += row_ptr[(size_t)v + 1] > 0;
      row_ptr[(size_t)v + 1] += row_ptr[v];
    }
    std::vector<int> fill(row_ptr.begin(), row_ptr.end() - 1);
    for (int e = 0; e < E; ++e) {
      const int a = Bh->pair_view1[e], b = Bh->pair_view2[e];
      row[(size_t)fill[a]++] = make_int2(b, e << 1);
      row[(size_t)fill[b]++] = make_int2(a, (e << 1) | 1);
    }
  }
  return one_shot_batch(device, "translation filter: no such device", E, t0, &sum->seconds, [&](OneShot* s) -> int {
    ViewPairGraph G;
    memset(&G, 0, sizeof(G));
    G.num_views = V;
    G.num_pairs = E;
    int *d_v1, *d_v2, *d_ptr, *d_order, *d_counter;
    int2* d_row;
    double *d_pos, *d_t, *d_rot = nullptr, *d_axes, *d_contrib, *d_weight, *d_moments;
    unsigned char *d_flag, *d_state = nullptr;
    TMI_HIP(s->upload(&d_v1, (const int*)Bh->pair_view1, (size_t)E));
    TMI_HIP(s->upload(&d_v2, (const int*)Bh->pair_view2, (size_t)E));
    TMI_HIP(s->upload(&d_ptr, row_ptr.data(), row_ptr.size()));
    TMI_HIP(s->upload(&d_row, row.data(), row.size()));
    TMI_HIP(s->upload(&d_pos, Bh->pair_position2, (size_t)3 * E));
    d_t = d_pos;
    if (Bh->view_rotation) {
      TMI_HIP(s->upload(&d_rot, Bh->view_rotation, (size_t)3 * V));
      TMI_HIP(s->alloc(&d_t, (size_t)3 * E));
    }
    TMI_HIP(s->alloc(&d_axes, (size_t)3 * K));
    TMI_HIP(s->alloc(&d_contrib, (size_t)K * E));
    TMI_HIP(s->alloc(&d_order, (size_t)K * V));
    TMI_HIP(s->alloc(&d_weight, (size_t)E));
    TMI_HIP(s->alloc(&d_flag, (size_t)E));
    TMI_HIP(s->alloc(&d_moments, 6));
    TMI_HIP(s->alloc(&d_counter, 1));
    const bool lds = V <= mfas_lds_view_cap();
    const size_t state_stride = (((size_t)V + 1) & ~(size_t)1) * 20;
    if (!lds) TMI_HIP(s->alloc(&d_state, state_stride * K));
    Pinned<double> pinned;  // [0..6) the moments, then the count of removed pairs
    TMI_HIP(pinned.alloc(8));
    double* h_moments = pinned.get();
    int* h_counter = reinterpret_cast<int*>(h_moments + 6);
    G.pair_view1 = d_v1;
    G.pair_view2 = d_v2;
    G.translation = d_t;
    G.row_ptr = d_ptr;
    G.row = d_row;
    StreamTimer timer(s->stream);  // rotate + moments; order_timer below: order + sum (the host draws in between)
    TMI_HIP(timer.status);
    const dim3 edge_grid((E + 255) / 256), block(256);
    TMI_HIP(timer.mark());
    if (d_rot) hipLaunchKernelGGL(rotate_translations_kernel, edge_grid, block, 0, s->stream, E, d_rot, d_v1, d_pos, d_t);
    std::vector<double> axes_h((size_t)3 * K);
    if (axes_given) {
      TMI_HIP(timer.mark());
      std::copy(axes, axes + (size_t)3 * K, axes_h.begin());
    } else {
      hipLaunchKernelGGL(translation_moments_kernel, dim3(1), block, 0, s->stream, E, d_t, d_moments);
      TMI_HIP(timer.mark());
      TMI_HIP(hipGetLastError());
      TMI_HIP(s->download(h_moments, d_moments, 6));
      TMI_HIP(hipStreamSynchronize(s->stream));
      // :216-221 -- the variance goes where RandGaussian takes a standard deviation, as in the reference
      AxisDeviates rng(opt->seed);
      for (int i = 0; i < K; ++i) {
        double a[3];
        for (int k = 0; k < 3; ++k) a[k] = h_moments[k] + h_moments[3 + k] * rng.normal();
        const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int k = 0; k < 3; ++k) axes_h[(size_t)3 * i + k] = n > 0.0 ? a[k] / n : a[k];
      }
      if (!all_finite(axes_h.data(), axes_h.size())) {
        s->error = "translation filter: the drawn axes are not finite (translations too large?)";
        return TMI_BA_ERR_INVALID_ARGUMENT;
      }
    }
    TMI_HIP(hipMemcpyAsync(d_axes, axes_h.data(), axes_h.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
    TMI_HIP(hipMemsetAsync(d_counter, 0, sizeof(int), s->stream));
    StreamTimer order_timer(s->stream);
    TMI_HIP(order_timer.status);
    TMI_HIP(order_timer.mark());
    if (lds) {
      static bool attr_set = false;
      if (!attr_set) {
        TMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mfas_order_kernel<true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)mfas_lds_bytes(kMfasLdsViews)));
        attr_set = true;
      }
      hipLaunchKernelGGL(mfas_order_kernel<true>, dim3(K), dim3(kMfasThreads), mfas_lds_bytes(V), s->stream, G, d_axes,
                         ordered, d_state, d_order, d_contrib);
    } else {
      hipLaunchKernelGGL(mfas_order_kernel<false>, dim3(K), dim3(kMfasThreads), kMfasLdsHeader, s->stream, G, d_axes,
                         ordered, d_state, d_order, d_contrib);
    }
    const double threshold = opt->translation_projection_tolerance * (double)K;
    hipLaunchKernelGGL(bad_weight_sum_kernel, edge_grid, block, 0, s->stream, E, K, d_contrib, threshold, d_flag,
                       d_weight, d_counter);
    TMI_HIP(order_timer.mark());
    ReadBack rb(s->stream);
    rb.add(h_counter, d_counter, 1);
    rb.add(pair_removed, d_flag, (size_t)E);
    rb.add(pair_bad_weight, d_weight, (size_t)E);
    rb.add(rotated_translation, d_t, (size_t)3 * E);
    rb.add(iteration_order, d_order, (size_t)K * V);
    TMI_HIP(rb.finish());
    if (axes) std::copy(axes_h.begin(), axes_h.end(), axes);
    sum->num_pairs = E;
    sum->num_pairs_removed = *h_counter;
    sum->num_iterations = K;
    sum->num_views_ordered = ordered;
    sum->kernel_seconds = timer.seconds(0, 1) + order_timer.seconds();
    return TMI_BA_OK;
  });
}

int32_t tmi_ba_filter_view_pairs_from_orientation(const tmi_ba_view_pair_batch* Bh,
                                                  double max_relative_rotation_difference_degrees, int32_t device,
                                                  uint8_t* pair_removed, double* pair_angle,
                                                  tmi_ba_view_pair_filter_summary* sum) {
  if (!Bh || !sum) return bad_argument("orientation filter: null batch or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  if (const char* why = check_view_pair_batch(Bh, true, Bh->pair_rotation2)) return bad_argument(why);
  if (!(max_relative_rotation_difference_degrees >= 0.0))  // filter_view_pairs_from_orientation.cc:77
    return bad_argument("orientation filter: negative threshold");
  const int V = Bh->num_views, E = Bh->num_pairs;
  const double max_rad = max_relative_rotation_difference_degrees * (M_PI / 180.0);  // :80-84
  return one_shot_batch(device, "orientation filter: no such device", E, t0, &sum->seconds, [&](OneShot* s) -> int {
    int *d_v1, *d_v2, *d_counter;
    double *d_rot, *d_rot2, *d_angle;
    unsigned char* d_flag;
    TMI_HIP(s->upload(&d_rot, Bh->view_rotation, (size_t)3 * V));
    TMI_HIP(s->upload(&d_v1, (const int*)Bh->pair_view1, (size_t)E));
    TMI_HIP(s->upload(&d_v2, (const int*)Bh->pair_view2, (size_t)E));
    TMI_HIP(s->upload(&d_rot2, Bh->pair_rotation2, (size_t)3 * E));
    TMI_HIP(s->alloc(&d_angle, (size_t)E));
    TMI_HIP(s->alloc(&d_flag, (size_t)E));
    TMI_HIP(s->alloc_filled(&d_counter, 1, 0));
    Pinned<int> pinned;
    TMI_HIP(pinned.alloc(1));
    int* h_counter = pinned.get();
    StreamTimer timer(s->stream);
    TMI_HIP(timer.status);
    TMI_HIP(timer.mark());
    hipLaunchKernelGGL(orientation_filter_kernel, dim3((E + 255) / 256), dim3(256), 0, s->stream, E, d_rot, d_v1, d_v2,
                       d_rot2, max_rad * max_rad, d_flag, d_angle, d_counter);
    TMI_HIP(timer.mark());
    ReadBack rb(s->stream);
    rb.add(h_counter, d_counter, 1);
    rb.add(pair_removed, d_flag, (size_t)E);
    rb.add(pair_angle, d_angle, (size_t)E);
    TMI_HIP(rb.finish());
    sum->num_pairs = E;
    sum->num_pairs_removed = *h_counter;
    sum->kernel_seconds = timer.seconds();
    return TMI_BA_OK;
  });
}
}  // extern "C"

// ---- the sample-consensus scaffold of the batched RANSAC calls (ransac_core.h) -----------------
namespace {
// SampleConsensusEstimator::ComputeMaxIterations (sample_consensus_estimator.h:215-243) for a sample of sample_size,
// without the T(d,d) test.
int ransac_max_iterations(double inlier_ratio, double log_failure_prob, int min_iterations, int max_iterations,
                          double sample_size) {
  if (inlier_ratio == 1.0) return min_iterations;
  const double log_prob = std::log(1.0 - std::pow(inlier_ratio, sample_size)) - std::numeric_limits<double>::epsilon();
  const double num_iterations = log_failure_prob / log_prob;
  return (int)std::max((double)min_iterations, std::min(num_iterations, (double)max_iterations));
}

// The CHECKs of the SampleConsensusEstimator constructor (sample_consensus_estimator.h:191-197) and the limits of the
// chunked loop, on either options struct.  Null: nothing is wrong; else the message, for the call to prefix.
template <class Options>
const char* ransac_options_error(const Options* L, const int32_t* samples, int32_t samples_given) {
  if (!(L->failure_probability > 0.0 && L->failure_probability < 1.0)) return "failure_probability must be in (0, 1)";
  if (!(L->min_inlier_ratio >= 0.0 && L->min_inlier_ratio <= 1.0)) return "min_inlier_ratio must be in [0, 1]";
  if (L->min_iterations < 0 || L->max_iterations < L->min_iterations)
    return "max_iterations < min_iterations, or a negative count";
  if (L->max_iterations > kRansacMaxIterations) return "max_iterations above 2^20";
  if (L->chunk_iterations < 0) return "negative chunk_iterations";
  if (samples_given && !samples) return "samples_given without samples";
  return nullptr;
}

// The caller's per-item arrays (each may be null).
struct RansacItemArrays {
  int8_t* status;
  int32_t *num_inliers, *num_iterations, *best_iteration, *best_solution;
  double* confidence;
};

// One call's host half of the chunked evaluate-then-replay loop over S attempted items (a view, a view pair) with M
// correspondences in all: plan(), upload<P>() and chunks<P>(), then the call's final kernel into d_status,
// d_num_inliers and d_slot_inlier, then read_back() and item_results() per item.  P is the problem of ransac_core.h.
struct RansacRun {
  std::vector<long long> sel_ptr;  // [S + 1] the call fills this before plan()
  int S = 0, K = 0, chunk = 1, chunks_run = 0;
  size_t M = 0;
  double sample_size = 0.0;
  std::vector<int> bound;
  std::vector<RansacState> state;
  RansacBatch B;
  int* d_active = nullptr;
  unsigned char* d_slot_inlier = nullptr;
  int* d_num_inliers = nullptr;
  signed char* d_status = nullptr;
  std::vector<signed char> status;
  std::vector<int> num_inliers;
  std::vector<unsigned char> slot_inlier;

  // ComputeMaxIterations per item and inlier count with the host's log and pow, the initial bound from
  // min_inlier_ratio, the states and the chunk length.
  template <class Options>
  void plan(const Options* L, int sample) {
    S = (int)sel_ptr.size() - 1;
    K = L->max_iterations;
    M = (size_t)sel_ptr[S];
    sample_size = (double)sample;
    const double log_failure_prob = std::log(L->failure_probability);
    bound.resize(M + (size_t)S);
    state.resize((size_t)S);
    int initial_bound = K;
    if (L->min_inlier_ratio > 0.0)
      initial_bound =
          std::min(ransac_max_iterations(L->min_inlier_ratio, log_failure_prob, L->min_iterations, K, sample_size), K);
    for (int s = 0; s < S; ++s) {
      const int n = (int)(sel_ptr[(size_t)s + 1] - sel_ptr[s]);
      int* row = bound.data() + sel_ptr[s] + s;
      for (int k = 0; k <= n; ++k)
        row[k] = k < sample ? K
                            : ransac_max_iterations((double)k / (double)n, log_failure_prob, L->min_iterations, K, sample_size);
      RansacState& st = state[s];
      memset(&st, 0, sizeof(st));
      st.best_cost = INT32_MAX;
      st.best_iteration = st.best_solution = -1;
      st.max_iterations = initial_bound;
      st.done = initial_bound <= 0;
    }
    // the engine's choice of chunk: the common case -- the run stops at min_iterations -- is a single chunk
    chunk = L->chunk_iterations ? L->chunk_iterations : std::max(L->min_iterations, 64);
    chunk = std::max(1, std::min(chunk, std::max(K, 1)));
  }

  // Everything of B but the correspondence planes, and the final kernel's outputs.  samples: the caller's table of
  // num_items rows, or null.
  template <class P>
  int upload(OneShot* s, uint64_t seed, const std::vector<int>& sel_item, const std::vector<unsigned>& sel_stream,
             const std::vector<double>& thresh, const int32_t* samples, size_t num_items, bool want_hypothesis_cost) {
    memset(&B, 0, sizeof(B));
    const size_t slots = (size_t)S * chunk * P::kSlots, hyp = (size_t)S * K * P::kSlots;
    int *d_sel_item, *d_bound, *d_samples = nullptr;
    unsigned* d_sel_stream;
    long long* d_sel_ptr;
    double* d_thresh;
    TMI_HIP(s->upload(&d_sel_item, sel_item.data(), sel_item.size()));
    TMI_HIP(s->upload(&d_sel_stream, sel_stream.data(), sel_stream.size()));
    TMI_HIP(s->upload(&d_sel_ptr, (const long long*)sel_ptr.data(), sel_ptr.size()));
    TMI_HIP(s->upload(&d_thresh, thresh.data(), thresh.size()));
    TMI_HIP(s->upload(&d_bound, (const int*)bound.data(), bound.size()));
    TMI_HIP(s->upload(&B.state, (const RansacState*)state.data(), state.size()));
    if (samples) TMI_HIP(s->upload(&d_samples, (const int*)samples, (size_t)P::kSample * K * num_items));
    TMI_HIP(s->alloc(&d_active, (size_t)S));
    TMI_HIP(s->alloc(&B.models, slots * P::kModel));
    TMI_HIP(s->alloc(&B.has_model, slots));
    TMI_HIP(s->alloc(&B.cost, slots));
    TMI_HIP(s->alloc(&d_slot_inlier, M));
    TMI_HIP(s->alloc(&d_num_inliers, (size_t)S));
    TMI_HIP(s->alloc(&d_status, (size_t)S));
    if (want_hypothesis_cost) TMI_HIP(s->alloc_filled(&B.hypothesis_cost, hyp, 0xff));
    B.num_selected = S;
    B.max_iterations = K;
    B.chunk = chunk;
    B.seed = seed;
    B.sel_item = d_sel_item;
    B.sel_stream = d_sel_stream;
    B.sel_ptr = d_sel_ptr;
    B.threshold = d_thresh;
    B.samples = d_samples;
    B.bound_table = d_bound;
    B.active = d_active;
    return TMI_BA_OK;
  }

  // The chunk loop: bounded by ceil(max_iterations / chunk) whatever the device reports.  phases (or null): the
  // summary that has fields for the device time of the three launches.
  template <class P>
  int chunks(OneShot* s, tmi_ba_two_view_ransac_summary* phases) {
    const hipStream_t stream = s->stream;
    std::vector<int> active;
    const int max_chunks = (K + chunk - 1) / chunk;
    for (int ch = 0; ch < max_chunks; ++ch) {
      active.clear();
      for (int v = 0; v < S; ++v)
        if (!state[v].done) active.push_back(v);
      if (active.empty()) break;
      TMI_HIP(hipMemcpyAsync(d_active, active.data(), active.size() * sizeof(int), hipMemcpyHostToDevice, stream));
      B.num_active = (int)active.size();
      B.chunk_start = ch * chunk;
      const long long items = (long long)B.num_active * chunk;
      StreamTimer phase(stream, phases ? 4 : 0);
      TMI_HIP(phase.status);
      if (phases) TMI_HIP(phase.mark());
      hipLaunchKernelGGL(ransac_hypothesis_kernel<P>, dim3((unsigned)((items + P::kThreads - 1) / P::kThreads)),
                         dim3(P::kThreads), 0, stream, B);
      if (phases) TMI_HIP(phase.mark());
      hipLaunchKernelGGL(ransac_score_kernel<P>, dim3((unsigned)((items * (P::kSlots / P::kScoreSlots) + 3) / 4)),
                         dim3(256), 0, stream, B);
      if (phases) TMI_HIP(phase.mark());
      hipLaunchKernelGGL(ransac_replay_kernel<P>, dim3((unsigned)((B.num_active + 63) / 64)), dim3(64), 0, stream, B);
      if (phases) TMI_HIP(phase.mark());
      TMI_HIP(hipGetLastError());
      TMI_HIP(s->download(state.data(), B.state, state.size()));
      TMI_HIP(hipStreamSynchronize(stream));  // (also: `active` is free to change)
      if (phases) {
        phases->hypothesis_seconds += phase.seconds(0, 1);
        phases->score_seconds += phase.seconds(1, 2);
        phases->replay_seconds += phase.seconds(2, 3);
      }
      ++chunks_run;
    }
    return TMI_BA_OK;
  }

  // After the final kernel: the statuses, the inlier counts and (want_mask) the inlier mask come to the host, the
  // stream is synchronised, and the costs of attempted item v go to row sel_rank[v] of the caller's hypothesis_cost.
  int read_back(OneShot* s, bool want_mask, int slots, const std::vector<int>& sel_rank, int32_t* hypothesis_cost) {
    const size_t KS = (size_t)K * slots;
    status.resize((size_t)S);
    num_inliers.resize((size_t)S);
    slot_inlier.resize(want_mask ? M : 0);
    std::vector<int> hyp_h(hypothesis_cost ? (size_t)S * KS : 0);
    TMI_HIP(s->download(status.data(), d_status, status.size()));
    TMI_HIP(s->download(num_inliers.data(), d_num_inliers, num_inliers.size()));
    TMI_HIP(s->download(slot_inlier.data(), d_slot_inlier, slot_inlier.size()));
    TMI_HIP(s->download(hyp_h.data(), B.hypothesis_cost, hyp_h.size()));
    TMI_HIP(hipStreamSynchronize(s->stream));
    if (hypothesis_cost)
      for (int v = 0; v < S; ++v)
        std::copy(hyp_h.begin() + (size_t)v * KS, hyp_h.begin() + ((size_t)v + 1) * KS,
                  hypothesis_cost + (size_t)sel_rank[v] * KS);
    return TMI_BA_OK;
  }

  // Attempted item v with status `code` into entry `item` of the caller's arrays.
  void item_results(int v, int item, int code, const RansacItemArrays& out) const {
    const RansacState& st = state[v];
    if (out.status) out.status[item] = (int8_t)code;
    if (out.num_inliers) out.num_inliers[item] = num_inliers[v];
    if (out.num_iterations) out.num_iterations[item] = st.num_iterations;
    if (out.best_iteration) out.best_iteration[item] = st.best_iteration;
    if (out.best_solution) out.best_solution[item] = st.best_solution;
    if (out.confidence) {
      const int n = (int)(sel_ptr[(size_t)v + 1] - sel_ptr[v]);
      const double ratio = (double)num_inliers[v] / (double)n;  // sample_consensus_estimator.h:336-340
      out.confidence[item] = 1.0 - std::pow(1.0 - std::pow(ratio, sample_size), (double)st.num_iterations);
    }
  }
};
}  // namespace

extern "C" {
// ---- batched LocalizeViewToReconstruction: P3P RANSAC (localize_kernels.h) ---------------------
void tmi_ba_localization_options_init(tmi_ba_localization_options* o) {
  if (!o) return;
  o->failure_probability = 0.01;  // sample_consensus_estimator.h:57-65
  o->min_inlier_ratio = 0.0;
  o->min_iterations = 100;
  o->max_iterations = 1000;       // (the reference's struct default is INT_MAX; the estimators set ransac_max_iterations)
  o->min_num_inliers = 30;        // localize_view_to_reconstruction.h:71
  o->bundle_adjust_view = 1;
  o->chunk_iterations = 0;
  o->seed = 0;
}

int32_t tmi_ba_localize_views(tmi_ba_problem* P, const tmi_ba_localization_options* L, const tmi_ba_options* O,
                              const uint8_t* view_mask, const double* view_error_threshold, const int32_t* samples,
                              int32_t samples_given, int8_t* view_status, int32_t* view_num_correspondences,
                              int32_t* view_num_inliers, int32_t* view_num_iterations, int32_t* view_best_iteration,
                              int32_t* view_best_solution, double* view_confidence, uint8_t* obs_inlier,
                              int32_t* hypothesis_cost, tmi_ba_localization_summary* sum) {
  if (!P || !L || !O || !sum) return bad_argument("localize views: null problem, options or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is looked for
  const int Nc = P->num_cameras, G = P->num_groups, Np = P->num_points;
  const int64_t No = P->num_observations;
  if (Nc < 0 || G < 0 || Np < 0 || No < 0) return bad_argument("localize views: negative size");
  if ((Nc && (!P->extrinsics || !P->camera_group)) || (G && (!P->group_model || !P->group_offset)) ||
      (Np && !P->points) || (No && (!P->obs_camera || !P->obs_point || !P->obs_xy)))
    return bad_argument("localize views: missing array");
  if (No >= (int64_t)0x7fffffffLL) return bad_argument("localize views: more than 2^31 observations");
  if (const char* why = ransac_options_error(L, samples, samples_given))
    return bad_argument((std::string("localize views: ") + why).c_str());
  const int n_intr = G ? P->group_offset[G] : 0;
  if (n_intr && !P->intrinsics) return bad_argument("localize views: missing intrinsics");
  std::vector<uint32_t> grp_free((size_t)G, 0);
  for (int g = 0; g < G; ++g) {
    const int o = P->group_offset[g], nk = P->group_offset[g + 1] - o;
    if (P->group_model[g] < 0 || P->group_model[g] > 4 || nk != tmi_ba_intrinsics_size(P->group_model[g]) || o < 0)
      return bad_argument("localize views: bad intrinsics group");
    for (int j = 0; j < nk; ++j)
      if (!P->intrinsics_constant || !P->intrinsics_constant[o + j]) grp_free[g] |= 1u << j;
  }
  std::vector<int4> cam((size_t)Nc);
  for (int c = 0; c < Nc; ++c) {
    const int g = P->camera_group[c];
    if (g < 0 || g >= G) return bad_argument("localize views: bad camera group");
    const int o = P->group_offset[g];
    cam[c] = view_cam_record(P->camera_flags ? P->camera_flags[c] : 0, P->group_model[g], o,
                             P->group_offset[g + 1] - o, grp_free[g]);
  }
  std::vector<long long> optr((size_t)Nc + 1, 0);
  for (int64_t i = 0; i < No; ++i) {
    const int c = P->obs_camera[i], p = P->obs_point[i];
    if (c < 0 || c >= Nc || p < 0 || p >= Np) return bad_argument("localize views: bad observation index");
    optr[(size_t)c + 1]++;
  }
  for (int c = 0; c < Nc; ++c) optr[(size_t)c + 1] += optr[c];
  // the selected views; attempted: enough correspondences for min_num_inliers (:141-145) and for a sample (the
  // reference's sampler refuses fewer than three)
  const int K = L->max_iterations;
  const int need = std::max(L->min_num_inliers, 3);
  std::vector<int> selected, sel_view;       // camera indices; sel_view: the attempted ones, the device's slots
  std::vector<int> sel_rank;                 // rank of a device slot among the selected views
  for (int c = 0; c < Nc; ++c) {
    if (view_mask && !view_mask[c]) continue;
    const long long n = optr[(size_t)c + 1] - optr[c];
    if (n >= need) {
      if (!view_error_threshold) return bad_argument("localize views: missing view_error_threshold");
      if (!(view_error_threshold[c] > 0.0)) return bad_argument("localize views: error threshold must be positive");
      if (samples_given)
        for (int64_t i = 0; i < K; ++i) {
          const int32_t* t = samples + 3 * ((int64_t)K * c + i);
          if (t[0] < 0 || t[1] < 0 || t[2] < 0 || t[0] >= n || t[1] >= n || t[2] >= n || t[0] == t[1] || t[0] == t[2] ||
              t[1] == t[2])
            return bad_argument("localize views: a sample with a repeated or out-of-range index");
        }
      sel_view.push_back(c);
      sel_rank.push_back((int)selected.size());
    }
    selected.push_back(c);
  }
  const int num_selected = (int)selected.size(), S = (int)sel_view.size();
  // nothing below fails on an argument: preset the outputs
  for (int c = 0; c < Nc; ++c) {
    const bool sel = !view_mask || view_mask[c];
    const long long n = optr[(size_t)c + 1] - optr[c];
    if (view_status) view_status[c] = (int8_t)(sel ? 1 : -1);
    if (view_num_correspondences) view_num_correspondences[c] = sel ? (int32_t)n : 0;
    if (view_num_inliers) view_num_inliers[c] = 0;
    if (view_num_iterations) view_num_iterations[c] = 0;
    if (view_best_iteration) view_best_iteration[c] = -1;
    if (view_best_solution) view_best_solution[c] = -1;
    if (view_confidence) view_confidence[c] = 0.0;
  }
  if (obs_inlier && No) memset(obs_inlier, 0, (size_t)No);
  if (hypothesis_cost)
    std::fill(hypothesis_cost, hypothesis_cost + (size_t)num_selected * (size_t)K * 4, -1);
  sum->num_views = num_selected;
  sum->num_too_few_correspondences = num_selected - S;
  // the attempted views' observations in view-major order, ascending observation index inside a view (the gather of
  // tmi_ba_adjust_views, which the adjustment below then runs on)
  std::vector<uint8_t> attempted((size_t)Nc, 0);
  for (const int c : sel_view) attempted[c] = 1;
  std::vector<long long> vptr((size_t)Nc + 1, 0);
  for (int c = 0; c < Nc; ++c) vptr[(size_t)c + 1] = vptr[c] + (attempted[c] ? optr[(size_t)c + 1] - optr[c] : 0);
  const size_t M = (size_t)vptr[Nc];
  std::vector<unsigned long long> keys(M);
  std::vector<int> slot_pt(M);
  std::vector<int64_t> slot_obs(M);
  std::vector<double> xy(2 * M);
  if (M) {
    std::vector<long long> fill(vptr.begin(), vptr.end() - 1);
    for (int64_t i = 0; i < No; ++i) {
      const int c = P->obs_camera[i];
      if (!attempted[c]) continue;
      const size_t o = (size_t)fill[c]++;
      keys[o] = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)o;
      slot_pt[o] = P->obs_point[i];
      slot_obs[o] = i;
      xy[2 * o] = P->obs_xy[2 * i];
      xy[2 * o + 1] = P->obs_xy[2 * i + 1];
    }
  }
  RansacRun run;
  run.sel_ptr.assign((size_t)S + 1, 0);
  std::vector<double> thresh((size_t)S);
  for (int s = 0; s < S; ++s) {
    const int c = sel_view[s];
    run.sel_ptr[s] = vptr[c];
    run.sel_ptr[(size_t)s + 1] = vptr[(size_t)c + 1];
    thresh[s] = view_error_threshold[c];
  }
  run.plan(L, LocalizeProblem::kSample);
  const std::vector<unsigned> sel_stream(sel_view.begin(), sel_view.end());  // a view's sample stream is its camera index
  return one_shot_batch(O->device, "localize views: no such device", S, t0, &sum->seconds, [&](OneShot* s) -> int {
    const hipStream_t stream = s->stream;
    ViewBatch VB;
    memset(&VB, 0, sizeof(VB));
    int4* d_cam;
    long long* d_vptr;
    unsigned long long* d_keys;
    int* d_slot_pt;
    double *d_xy, *d_pts, *d_pose_out;
    TMI_HIP(s->upload(&VB.ext, (const double*)P->extrinsics, (size_t)6 * Nc));
    TMI_HIP(s->upload(&VB.intr, (const double*)P->intrinsics, (size_t)n_intr));
    TMI_HIP(s->upload(&d_cam, cam.data(), cam.size()));
    TMI_HIP(s->upload(&d_vptr, vptr.data(), vptr.size()));
    TMI_HIP(s->upload(&d_keys, keys.data(), keys.size()));
    TMI_HIP(s->upload(&d_slot_pt, slot_pt.data(), slot_pt.size()));
    TMI_HIP(s->upload(&d_xy, xy.data(), xy.size()));
    TMI_HIP(s->upload(&d_pts, (const double*)P->points, (size_t)4 * Np));
    if (const int rc = run.upload<LocalizeProblem>(s, L->seed, sel_view, sel_stream, thresh,
                                                   samples_given ? samples : nullptr, (size_t)Nc, hypothesis_cost != nullptr))
      return rc;
    RansacBatch& B = run.B;
    for (int q = 0; q < LocalizeProblem::kPlanes; ++q) TMI_HIP(s->alloc(&B.plane[q], M));
    TMI_HIP(s->alloc(&d_pose_out, (size_t)6 * S));
    StreamTimer timer(stream);
    TMI_HIP(timer.status);
    TMI_HIP(timer.mark());
    hipLaunchKernelGGL(localize_prepare_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, (long long)M,
                       d_keys, d_slot_pt, d_xy, d_pts, d_cam, VB.intr, B);
    if (const int rc = run.chunks<LocalizeProblem>(s, nullptr)) return rc;
    hipLaunchKernelGGL(localize_final_kernel, dim3(S), dim3(64), 0, stream, B, (int)L->min_num_inliers,
                       run.d_slot_inlier, run.d_num_inliers, run.d_status, d_pose_out, VB.ext);
    TMI_HIP(timer.mark());
    TMI_HIP(hipGetLastError());
    if (const int rc = run.read_back(s, obs_inlier != nullptr, LocalizeProblem::kSlots, sel_rank, hypothesis_cost))
      return rc;
    sum->kernel_seconds = timer.seconds();
    sum->num_chunks = run.chunks_run;
    // BundleAdjustView on exactly the localised views, on the data already uploaded
    std::vector<uint8_t> localised((size_t)Nc, 0);
    int num_localised = 0;
    for (int v = 0; v < S; ++v)
      if (run.status[v] == 0) {
        localised[sel_view[v]] = 1;
        ++num_localised;
      }
    if (L->bundle_adjust_view && num_localised) {
      std::vector<int> chain_ptr, chain_views;
      build_view_chains(Nc, cam, P->camera_group, G, vptr, localised.data(), &chain_ptr, &chain_views);
      VB.cam = d_cam;
      VB.vptr = d_vptr;
      VB.keys = d_keys;
      VB.slot_pt = d_slot_pt;
      VB.obs_xy = d_xy;
      VB.pts = d_pts;
      std::vector<int8_t> term((size_t)Nc, -1);
      tmi_ba_view_batch_summary vs;
      memset(&vs, 0, sizeof(vs));
      const int rc = run_view_batch(s, VB, O, Nc, cam, chain_ptr, chain_views, {term.data(), nullptr, nullptr, nullptr},
                                    &vs);
      if (rc) return rc;
      sum->kernel_seconds += vs.kernel_seconds;
      for (int v = 0; v < S; ++v)
        if (run.status[v] == 0 && term[sel_view[v]] != 0 && term[sel_view[v]] != 1) run.status[v] = 4;
      // (the kernel wrote back exactly the usable views' free intrinsics)
      TMI_HIP(s->download(P->intrinsics, VB.intr, (size_t)n_intr));
    }
    std::vector<double> ext_h((size_t)6 * Nc);
    TMI_HIP(s->download(ext_h.data(), VB.ext, ext_h.size()));
    TMI_HIP(hipStreamSynchronize(stream));
    const RansacItemArrays out = {view_status,         view_num_inliers,   view_num_iterations,
                                  view_best_iteration, view_best_solution, view_confidence};
    for (int v = 0; v < S; ++v) {
      const int c = sel_view[v];
      const int code = run.status[v];
      if (code == 0 || code == 4) std::copy(ext_h.begin() + 6 * (size_t)c, ext_h.begin() + 6 * (size_t)c + 6, P->extrinsics + 6 * (size_t)c);
      switch (code) {
        case 0: sum->num_localized++; break;
        case 2: sum->num_no_model++; break;
        case 3: sum->num_too_few_inliers++; break;
        default: sum->num_failed_ba++; break;
      }
      sum->total_iterations += run.state[v].num_iterations;
      run.item_results(v, c, code, out);
      if (obs_inlier)
        for (long long o = run.sel_ptr[v]; o < run.sel_ptr[(size_t)v + 1]; ++o)
          obs_inlier[slot_obs[(size_t)o]] = run.slot_inlier[(size_t)o];
    }
    return TMI_BA_OK;
  });
}

// ---- batched BruteForceFeatureMatcher: exact squared-L2 matching (match_kernels.h) -------------
void tmi_ba_match_options_init(tmi_ba_match_options* o) {
  if (!o) return;
  o->use_lowes_ratio = 1;  // feature_matcher_options.h:45-71
  o->lowes_ratio = 0.8f;
  o->keep_only_symmetric_matches = 1;
  o->min_num_feature_matches = 30;
  o->device = -1;
  o->pairs_per_chunk = 0;
}
}  // extern "C"
namespace {
// Work memory of a chunk of pairs, per descriptor row and direction: the nearest-neighbour triple (12), the two flags
// (2), the scan's input and output (8) and the compacted matches (12).
constexpr long long kMatchRowBytes = 34;
constexpr long long kMatchWorkBudgetBytes = 64ll << 20;
constexpr long long kMatchMaxChunkRows = 0x7ffffff0ll;


// The call the two matchers share.  Cascade == false: tmi_ba_match_features (match_nn_kernel gives every row its
// neighbour triple).  Cascade == true: tmi_ba_match_features_cascade (the images are hashed once, then
// cascade_candidates_kernel gives the triple; projections, image_hash and image_bucket_ids are its alone).  The chunk
// plan, the finish kernels and the read-back are one code.
template <bool Cascade, class Options, class Summary>
int32_t match_features_call(const Options* M, int32_t num_images, const int64_t* image_begin, const float* descriptors,
                            int32_t dim, const float* projections, int32_t num_pairs, const int32_t* pair_image1,
                            const int32_t* pair_image2, int64_t match_capacity, int8_t* pair_status,
                            int32_t* pair_num_forward, int64_t* pair_match_begin, int32_t* match_feature1,
                            int32_t* match_feature2, float* match_distance, uint32_t* image_hash,
                            uint16_t* image_bucket_ids, Summary* sum) {
  const std::string what = Cascade ? "cascade match features" : "match features";
  auto bad = [&](const char* why) { return bad_argument((what + ": " + why).c_str()); };
  if (!M || !sum) return bad("null options or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is looked for
  if (num_images < 0 || num_pairs < 0 || match_capacity < 0) return bad("negative count");
  if (dim < 1) return bad("dim < 1");
  if (!image_begin) return bad("missing image_begin");
  if (M->min_num_feature_matches < 0 || M->pairs_per_chunk < 0)
    return bad("negative min_num_feature_matches or pairs_per_chunk");
  if (Cascade && !projections) return bad("missing projections");
  if (image_begin[0] != 0) return bad("image_begin must start at 0");
  for (int m = 0; m < num_images; ++m) {
    if (image_begin[m + 1] < image_begin[m]) return bad("image_begin decreases");
    if (image_begin[m + 1] - image_begin[m] >= 0x7fffffffLL) return bad("an image of 2^31 rows");
  }
  const int64_t total_rows = image_begin[num_images];
  if (total_rows && !descriptors) return bad("missing descriptors");
  if (num_pairs && (!pair_image1 || !pair_image2 || !pair_status || !pair_num_forward))
    return bad("missing pair array");
  if (!pair_match_begin) return bad("missing pair_match_begin");
  if (match_capacity && (!match_feature1 || !match_feature2 || !match_distance))
    return bad("missing match array");
  for (int p = 0; p < num_pairs; ++p)
    if (pair_image1[p] < 0 || pair_image1[p] >= num_images || pair_image2[p] < 0 || pair_image2[p] >= num_images)
      return bad("image index out of range");
  const bool symmetric = M->keep_only_symmetric_matches != 0;
  const int min_matches = M->min_num_feature_matches;
  const float ratio_f = M->lowes_ratio * M->lowes_ratio;  // formed in fp32 (brute_force_feature_matcher.cc:58-59)
  // cascade: formed in double, 1.0 without the ratio test (cascade_hasher.cc:180, cascade_hashing_feature_matcher.cc:144)
  const double ratio_sq = !Cascade ? (double)ratio_f
                          : M->use_lowes_ratio ? (double)M->lowes_ratio * (double)M->lowes_ratio : 1.0;
  // the chunks of consecutive pairs
  auto rows_of = [&](int p) -> long long {
    const long long n1 = image_begin[pair_image1[p] + 1] - image_begin[pair_image1[p]];
    const long long n2 = image_begin[pair_image2[p] + 1] - image_begin[pair_image2[p]];
    return n1 + (symmetric ? n2 : 0);
  };
  std::vector<int> chunk_begin(1, 0);
  long long max_rows = 0;
  int max_pairs = 0;
  for (int p = 0; p < num_pairs;) {
    long long rows = 0;
    int q = p;
    while (q < num_pairs) {
      const long long r = rows_of(q);
      if (r > kMatchMaxChunkRows) {
        g_last_error = what + ": a pair with more than 2^31 rows over its directions";
        return TMI_BA_ERR_UNSUPPORTED;
      }
      if (q > p) {
        if (M->pairs_per_chunk ? q - p >= M->pairs_per_chunk : (rows + r) * kMatchRowBytes > kMatchWorkBudgetBytes) break;
        if (rows + r > kMatchMaxChunkRows) break;
      }
      rows += r;
      ++q;
    }
    max_rows = std::max(max_rows, rows);
    max_pairs = std::max(max_pairs, q - p);
    chunk_begin.push_back(q);
    p = q;
  }
  if constexpr (!Cascade)
    for (int p = 0; p < num_pairs; ++p) {
      const long long n1 = image_begin[pair_image1[p] + 1] - image_begin[pair_image1[p]];
      const long long n2 = image_begin[pair_image2[p] + 1] - image_begin[pair_image2[p]];
      sum->distance_evaluations += n1 * n2 * (symmetric ? 2 : 1);
    }
  pair_match_begin[0] = 0;
  const std::string no_device = what + ": no such device";
  const int rc = one_shot_batch(M->device, no_device.c_str(), num_pairs, t0, &sum->total_seconds, [&](OneShot* s) -> int {
    const hipStream_t stream = s->stream;
    float* d_desc;
    TMI_HIP(s->upload(&d_desc, descriptors, (size_t)total_rows * (size_t)dim));
    // cascade: every image is hashed once, however many pairs name it
    CascadeRecord* d_rec = nullptr;
    int *d_bucket_begin = nullptr, *d_bucket_rows = nullptr, *d_task_image = nullptr;
    unsigned long long* d_counters = nullptr;
    std::vector<int> task_image;
    if constexpr (Cascade) {
      float *d_proj, *d_mean;
      long long* d_image_begin;
      int2* d_hash_blocks;
      std::vector<long long> begin_h(image_begin, image_begin + num_images + 1);
      std::vector<int2> hash_blocks;
      for (int m = 0; m < num_images; ++m)
        for (long long r = 0; r * kCascadeHashRows < begin_h[m + 1] - begin_h[m]; ++r) hash_blocks.push_back(make_int2(m, (int)r));
      TMI_HIP(s->upload(&d_proj, projections, (size_t)kCascadeProjRows * (size_t)dim));
      TMI_HIP(s->upload(&d_image_begin, begin_h.data(), begin_h.size()));
      TMI_HIP(s->upload(&d_hash_blocks, hash_blocks.data(), hash_blocks.size()));
      TMI_HIP(s->alloc(&d_mean, (size_t)num_images * (size_t)dim));
      TMI_HIP(s->alloc(&d_rec, (size_t)total_rows));
      TMI_HIP(s->alloc(&d_bucket_begin, (size_t)num_images * kCascadeGroups * (kCascadeBuckets + 1)));
      TMI_HIP(s->alloc(&d_bucket_rows, (size_t)kCascadeGroups * (size_t)total_rows));
      TMI_HIP(s->alloc(&d_task_image, 2 * (size_t)max_pairs));
      TMI_HIP(s->alloc_filled(&d_counters, 4 * (size_t)kCascadeCounterShards, 0));
      StreamTimer timer(stream);
      TMI_HIP(timer.status);
      TMI_HIP(timer.mark());
      if (num_images) {
        const long long cells = (long long)num_images * dim;
        hipLaunchKernelGGL(cascade_mean_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, d_desc, (int)dim,
                           d_image_begin, (int)num_images, d_mean);
        if (!hash_blocks.empty())
          hipLaunchKernelGGL(cascade_hash_kernel, dim3((unsigned)hash_blocks.size()), dim3(256), 0, stream, d_desc, (int)dim,
                             d_proj, d_mean, d_image_begin, d_hash_blocks, d_rec);
        hipLaunchKernelGGL(cascade_bucket_kernel, dim3((unsigned)num_images * kCascadeGroups), dim3(256), 0, stream, d_rec,
                           d_image_begin, d_bucket_begin, d_bucket_rows);
      }
      TMI_HIP(timer.mark());
      TMI_HIP(hipGetLastError());
      std::vector<CascadeRecord> rec_h((image_hash || image_bucket_ids) ? (size_t)total_rows : 0);
      TMI_HIP(s->download(rec_h.data(), d_rec, rec_h.size()));
      TMI_HIP(hipStreamSynchronize(stream));  // (also: begin_h and hash_blocks are free to go)
      sum->kernel_seconds += timer.seconds();
      for (size_t r = 0; r < rec_h.size(); ++r) {
        if (image_hash) std::copy(rec_h[r].code, rec_h[r].code + 4, image_hash + 4 * r);
        if (image_bucket_ids) std::copy(rec_h[r].ids, rec_h[r].ids + kCascadeGroups, image_bucket_ids + kCascadeGroups * r);
      }
    }
    const size_t R = (size_t)max_rows;
    MatchNn nn;
    MatchTask* d_tasks;
    int2* d_blocks;
    int *d_fwd_task, *d_pair_counts, *d_flag, *d_scan, *d_counts;
    MatchRecord* d_out;
    unsigned char *d_pass, *d_keep;
    const size_t max_blocks = (R + kMatchTile - 1) / kMatchTile + 2 * (size_t)max_pairs;
    TMI_HIP(s->alloc(&nn.best_d, R));
    TMI_HIP(s->alloc(&nn.best_i, R));
    TMI_HIP(s->alloc(&nn.second_d, R));
    TMI_HIP(s->alloc(&d_tasks, 2 * (size_t)max_pairs));
    TMI_HIP(s->alloc(&d_blocks, max_blocks));
    TMI_HIP(s->alloc(&d_fwd_task, (size_t)max_pairs));
    TMI_HIP(s->alloc(&d_pair_counts, 2 * (size_t)max_pairs));
    TMI_HIP(s->alloc(&d_pass, R));
    TMI_HIP(s->alloc(&d_keep, R));
    TMI_HIP(s->alloc(&d_flag, R + 1));
    TMI_HIP(s->alloc(&d_scan, R + 1));
    TMI_HIP(s->alloc(&d_counts, 4 * (size_t)max_pairs + 1));
    TMI_HIP(s->alloc(&d_out, R));
    size_t scan_bytes = 0;
    TMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, d_flag, d_scan, (int)(R + 1), stream));
    unsigned char* d_scan_tmp;
    TMI_HIP(s->alloc(&d_scan_tmp, std::max<size_t>(scan_bytes, 16)));
    Pinned<int> h_counts_buf;
    Pinned<MatchRecord> h_out_buf;
    TMI_HIP(h_counts_buf.alloc(4 * (size_t)max_pairs + 1));
    TMI_HIP(h_out_buf.alloc(R));
    int* const h_counts = h_counts_buf.get();
    MatchRecord* const rec = h_out_buf.get();
    const size_t lds = match_lds_bytes(dim);
    const bool staged = dim <= kMatchMaxStagedDim;
    int64_t total = 0;
    std::vector<MatchTask> tasks;
    std::vector<int2> blocks;
    std::vector<int> fwd_task;
    for (size_t c = 0; c + 1 < chunk_begin.size(); ++c) {
      const int p0 = chunk_begin[c], np = chunk_begin[c + 1] - p0;
      tasks.clear();
      blocks.clear();
      fwd_task.clear();
      task_image.clear();
      long long rows = 0;
      for (int p = 0; p < np; ++p) {
        const int i1 = pair_image1[p0 + p], i2 = pair_image2[p0 + p];
        const int n1 = (int)(image_begin[i1 + 1] - image_begin[i1]), n2 = (int)(image_begin[i2 + 1] - image_begin[i2]);
        MatchTask f = {image_begin[i1], image_begin[i2], n1, n2, (int)rows, p, 1, symmetric ? (int)(rows + n1) : -1};
        fwd_task.push_back((int)tasks.size());
        tasks.push_back(f);
        task_image.push_back(i2);  // the image whose buckets the task's rows look into
        rows += n1;
        if (symmetric) {
          MatchTask r = {image_begin[i2], image_begin[i1], n2, n1, (int)rows, p, 0, f.out_base};
          tasks.push_back(r);
          task_image.push_back(i1);
          rows += n2;
        }
      }
      if constexpr (!Cascade)
        for (size_t t = 0; t < tasks.size(); ++t)
          for (int b = 0; b * kMatchTile < tasks[t].n_rows; ++b) blocks.push_back(make_int2((int)t, b));
      const int num_rows = (int)rows, num_tasks = (int)tasks.size();
      if (blocks.size() > max_blocks || (size_t)num_rows > R) {  // (the plan above bounds both)
        s->error = what + ": chunk plan exceeded";
        return TMI_BA_ERR_DEVICE;
      }
      TMI_HIP(hipMemcpyAsync(d_tasks, tasks.data(), tasks.size() * sizeof(MatchTask), hipMemcpyHostToDevice, stream));
      if (!blocks.empty())
        TMI_HIP(hipMemcpyAsync(d_blocks, blocks.data(), blocks.size() * sizeof(int2), hipMemcpyHostToDevice, stream));
      if constexpr (Cascade)
        TMI_HIP(hipMemcpyAsync(d_task_image, task_image.data(), task_image.size() * sizeof(int), hipMemcpyHostToDevice, stream));
      TMI_HIP(hipMemcpyAsync(d_fwd_task, fwd_task.data(), fwd_task.size() * sizeof(int), hipMemcpyHostToDevice, stream));
      TMI_HIP(hipMemsetAsync(d_pair_counts, 0, 2 * (size_t)np * sizeof(int), stream));
      int* d_num_forward = d_pair_counts;
      int* d_num_kept = d_pair_counts + np;
      StreamTimer timer(stream);
      TMI_HIP(timer.status);
      TMI_HIP(timer.mark());
      const unsigned row_grid = (unsigned)((num_rows + 255) / 256);
      if constexpr (Cascade) {
        if (num_rows)
          hipLaunchKernelGGL(cascade_candidates_kernel, dim3((unsigned)((num_rows + 3) / 4)), dim3(256), 0, stream, d_desc,
                             (int)dim, d_tasks, d_task_image, num_tasks, num_rows, d_rec, d_bucket_begin, d_bucket_rows, nn,
                             d_counters);
      } else if (!blocks.empty()) {
        if (staged)
          hipLaunchKernelGGL(match_nn_kernel<true>, dim3((unsigned)blocks.size()), dim3(256), lds, stream, d_desc, (int)dim,
                             d_tasks, d_blocks, nn);
        else
          hipLaunchKernelGGL(match_nn_kernel<false>, dim3((unsigned)blocks.size()), dim3(256), lds, stream, d_desc, (int)dim,
                             d_tasks, d_blocks, nn);
      }
      if (num_rows) {
        hipLaunchKernelGGL(match_ratio_kernel<Cascade>, dim3(row_grid), dim3(256), 0, stream, d_tasks, num_tasks, num_rows, nn,
                           (int)(M->use_lowes_ratio != 0), ratio_sq, d_pass, d_num_forward);
        hipLaunchKernelGGL(match_symmetric_kernel, dim3(row_grid), dim3(256), 0, stream, d_tasks, num_tasks, num_rows, nn,
                           d_pass, d_num_forward, (int)symmetric, min_matches, d_keep, d_num_kept);
      }
      hipLaunchKernelGGL(match_flag_kernel, dim3((unsigned)(num_rows / 256 + 1)), dim3(256), 0, stream, d_tasks, num_tasks,
                         num_rows, d_keep, d_num_kept, min_matches, d_flag);
      TMI_HIP(hipcub::DeviceScan::ExclusiveSum(d_scan_tmp, scan_bytes, d_flag, d_scan, num_rows + 1, stream));
      if (num_rows)
        hipLaunchKernelGGL(match_compact_kernel, dim3(row_grid), dim3(256), 0, stream, d_tasks, num_tasks, num_rows, nn,
                           d_flag, d_scan, d_out);
      hipLaunchKernelGGL(match_pair_kernel, dim3((unsigned)(np / 256 + 1)), dim3(256), 0, stream, d_tasks, d_fwd_task, np,
                         num_rows, d_num_forward, d_num_kept, min_matches, d_scan, d_counts);
      TMI_HIP(timer.mark());
      TMI_HIP(hipGetLastError());
      // the counts, then exactly the chunk's matches
      TMI_HIP(s->download(h_counts, d_counts, 4 * (size_t)np + 1));
      TMI_HIP(hipStreamSynchronize(stream));  // (also: tasks, blocks and fwd_task are free to change)
      sum->kernel_seconds += timer.seconds();
      const int chunk_total = h_counts[4 * np];
      if (chunk_total < 0 || chunk_total > num_rows) {
        s->error = what + ": the device reported an impossible match count";
        return TMI_BA_ERR_DEVICE;
      }
      for (int p = 0; p < np; ++p) {
        pair_status[p0 + p] = (int8_t)h_counts[4 * p];
        pair_num_forward[p0 + p] = h_counts[4 * p + 1];
        pair_match_begin[p0 + p] = total + h_counts[4 * p + 2];
        if (h_counts[4 * p] == 0) sum->num_pairs_ok++;
      }
      if (chunk_total && total + chunk_total <= match_capacity) {
        const size_t n = (size_t)chunk_total;
        TMI_HIP(s->download(rec, d_out, n));
        TMI_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < n; ++i) {
          match_feature1[total + i] = rec[i].feature1;
          match_feature2[total + i] = rec[i].feature2;
          match_distance[total + i] = rec[i].distance;
        }
      }
      total += chunk_total;
      pair_match_begin[p0 + np] = total;
      sum->num_chunks++;
    }
    sum->num_matches = total;
    if constexpr (Cascade) {
      unsigned long long counters_h[4 * kCascadeCounterShards];
      TMI_HIP(s->download(counters_h, d_counters, (size_t)4 * kCascadeCounterShards));
      TMI_HIP(hipStreamSynchronize(stream));
      for (int i = 0; i < kCascadeCounterShards; ++i) {
        sum->candidates_examined += (int64_t)counters_h[4 * i];
        sum->distance_evaluations += (int64_t)counters_h[4 * i + 1];
        sum->rows_skipped += (int64_t)counters_h[4 * i + 2];
      }
    }
    return TMI_BA_OK;
  });
  sum->total_seconds = now_s() - t0;
  if (rc == TMI_BA_OK && sum->num_matches > match_capacity) {
    g_last_error = what + ": match_capacity is smaller than the number of matches (summary->num_matches)";
    return TMI_BA_ERR_CAPACITY;
  }
  return rc;
}
}  // namespace
extern "C" {

int32_t tmi_ba_match_features(const tmi_ba_match_options* M, int32_t num_images, const int64_t* image_begin,
                              const float* descriptors, int32_t dim, int32_t num_pairs, const int32_t* pair_image1,
                              const int32_t* pair_image2, int64_t match_capacity, int8_t* pair_status,
                              int32_t* pair_num_forward, int64_t* pair_match_begin, int32_t* match_feature1,
                              int32_t* match_feature2, float* match_distance, tmi_ba_match_summary* sum) {
  return match_features_call<false>(M, num_images, image_begin, descriptors, dim, nullptr, num_pairs, pair_image1,
                                    pair_image2, match_capacity, pair_status, pair_num_forward, pair_match_begin,
                                    match_feature1, match_feature2, match_distance, nullptr, nullptr, sum);
}

// ---- batched CascadeHashingFeatureMatcher (cascade_match_kernels.h) ----------------------------
void tmi_ba_cascade_match_options_init(tmi_ba_cascade_match_options* o) {
  if (!o) return;
  o->use_lowes_ratio = 1;  // feature_matcher_options.h:45-71
  o->lowes_ratio = 0.8f;
  o->keep_only_symmetric_matches = 1;
  o->min_num_feature_matches = 30;
  o->device = -1;
  o->pairs_per_chunk = 0;
}

int32_t tmi_ba_match_features_cascade(const tmi_ba_cascade_match_options* options, int32_t num_images,
                                      const int64_t* image_begin, const float* descriptors, int32_t dim,
                                      const float* projections, int32_t num_pairs, const int32_t* pair_image1,
                                      const int32_t* pair_image2, int64_t match_capacity, int8_t* pair_status,
                                      int32_t* pair_num_forward, int64_t* pair_match_begin, int32_t* match_feature1,
                                      int32_t* match_feature2, float* match_distance, uint32_t* image_hash,
                                      uint16_t* image_bucket_ids, tmi_ba_cascade_match_summary* summary) {
  return match_features_call<true>(options, num_images, image_begin, descriptors, dim, projections, num_pairs,
                                   pair_image1, pair_image2, match_capacity, pair_status, pair_num_forward,
                                   pair_match_begin, match_feature1, match_feature2, match_distance, image_hash,
                                   image_bucket_ids, summary);
}
}  // extern "C"

// ---- TrackBuilder: tracks from matches by union-find (track_build_kernels.h) -------------------
namespace {
// Stable radix sort of (key, value) pairs on bits [0, end_bit) and an exclusive sum, each with work memory of the
// call's own.
template <class K>
int tb_sort_pairs(OneShot* s, const K* key_in, K* key_out, const unsigned* value_in, unsigned* value_out, size_t n,
                  int end_bit) {
  size_t bytes = 0;
  unsigned char* tmp = nullptr;
  TMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, key_in, key_out, value_in, value_out, (int)n, 0, end_bit, s->stream));
  TMI_HIP(s->alloc(&tmp, std::max<size_t>(bytes, 16)));
  TMI_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, key_in, key_out, value_in, value_out, (int)n, 0, end_bit, s->stream));
  return TMI_BA_OK;
}

int tb_exclusive_sum(OneShot* s, const unsigned* in, unsigned* out, size_t n) {
  size_t bytes = 0;
  unsigned char* tmp = nullptr;
  TMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)n, s->stream));
  TMI_HIP(s->alloc(&tmp, std::max<size_t>(bytes, 16)));
  TMI_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, (int)n, s->stream));
  return TMI_BA_OK;
}

// The bits that hold every value below n (at least one).
int tb_bits(unsigned n) {
  int bits = 1;
  while (bits < 32 && (1ull << bits) < n) ++bits;
  return bits;
}

#define TMI_TB(call)                  \
  do {                                \
    const int rc_ = (call);           \
    if (rc_ != TMI_BA_OK) return rc_; \
  } while (0)
}  // namespace
extern "C" {

void tmi_ba_track_build_options_init(tmi_ba_track_build_options* o) {
  if (!o) return;
  o->min_track_length = 2;  // reconstruction_builder.h:81-85
  o->max_track_length = 50;
  o->device = -1;
}

int32_t tmi_ba_build_tracks(const tmi_ba_track_build_options* O, int64_t num_edges, const uint32_t* endpoint_view,
                            const uint32_t* endpoint_feature, int64_t track_capacity, int64_t obs_capacity,
                            int64_t* track_begin, uint32_t* obs_view, uint32_t* obs_feature, uint32_t* endpoint_node,
                            uint32_t* endpoint_label, tmi_ba_track_build_summary* sum) {
  if (!O || !sum) return bad_argument("build tracks: null options or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is looked for
  if (num_edges < 0 || track_capacity < 0 || obs_capacity < 0) return bad_argument("build tracks: negative count");
  if (num_edges >= (1ll << 30)) return bad_argument("build tracks: 2^30 edges or more");
  if (O->max_track_length < 1) return bad_argument("build tracks: max_track_length < 1");
  if (O->min_track_length < 1) return bad_argument("build tracks: min_track_length < 1");
  if (num_edges && (!endpoint_view || !endpoint_feature)) return bad_argument("build tracks: missing endpoint array");
  if (!track_begin) return bad_argument("build tracks: missing track_begin");
  if (obs_capacity && (!obs_view || !obs_feature)) return bad_argument("build tracks: missing observation array");
  for (int64_t e = 0; e < num_edges; ++e)
    if (endpoint_view[2 * e] == endpoint_view[2 * e + 1])
      return bad_argument("build tracks: an edge joins two features of the same view");
  const long long E = num_edges, N2 = 2 * E;
  const unsigned cap = (unsigned)O->max_track_length;
  const unsigned min_length = (unsigned)std::max(O->min_track_length, 2);  // a set of one node is always dropped
  bool too_small = false;
  const int rc = one_shot_batch(O->device, "build tracks: no such device", (int)E, t0, &sum->seconds, [&](OneShot* s) -> int {
    const hipStream_t stream = s->stream;
    auto grid = [](long long n) { return dim3((unsigned)((n + 255) / 256)); };
    StreamTimer nodes_timer(stream), components_timer(stream), cap_timer(stream, 4), output_timer(stream, 4);
    TMI_HIP(nodes_timer.status);
    TMI_HIP(components_timer.status);
    TMI_HIP(cap_timer.status);
    TMI_HIP(output_timer.status);
    unsigned long long* d_counters;
    TMI_HIP(s->alloc_filled(&d_counters, (size_t)kTbCounters, 0));
    unsigned long long counters[kTbCounters];
    auto read_counters = [&]() -> int {
      TMI_HIP(s->download(counters, d_counters, (size_t)kTbCounters));
      TMI_HIP(hipStreamSynchronize(stream));
      if (counters[kTbError]) {
        s->error = "build tracks: a device loop reached its bound";
        return TMI_BA_ERR_DEVICE;
      }
      return TMI_BA_OK;
    };

    // step 1: node ids
    unsigned *d_view, *d_feature, *d_index, *d_index_sorted, *d_head, *d_first, *d_heads_before, *d_firsts_before;
    unsigned *d_run_node, *d_node_view, *d_node_feature, *d_endpoint_node;
    unsigned long long *d_key, *d_key_sorted;
    TMI_HIP(s->upload(&d_view, endpoint_view, (size_t)N2));
    TMI_HIP(s->upload(&d_feature, endpoint_feature, (size_t)N2));
    TMI_HIP(s->alloc(&d_key, (size_t)N2));
    TMI_HIP(s->alloc(&d_key_sorted, (size_t)N2));
    TMI_HIP(s->alloc(&d_index, (size_t)N2));
    TMI_HIP(s->alloc(&d_index_sorted, (size_t)N2));
    TMI_HIP(s->alloc_filled(&d_head, (size_t)N2 + 1, 0));
    TMI_HIP(s->alloc_filled(&d_first, (size_t)N2 + 1, 0));
    TMI_HIP(s->alloc(&d_heads_before, (size_t)N2 + 1));
    TMI_HIP(s->alloc(&d_firsts_before, (size_t)N2 + 1));
    TMI_HIP(s->alloc(&d_run_node, (size_t)N2));
    TMI_HIP(s->alloc(&d_node_view, (size_t)N2));
    TMI_HIP(s->alloc(&d_node_feature, (size_t)N2));
    TMI_HIP(s->alloc(&d_endpoint_node, (size_t)N2));
    TMI_HIP(nodes_timer.mark());
    hipLaunchKernelGGL(tb_keys_kernel, grid(N2), dim3(256), 0, stream, d_view, d_feature, N2, d_key, d_index);
    TMI_TB(tb_sort_pairs(s, d_key, d_key_sorted, d_index, d_index_sorted, (size_t)N2, 64));
    hipLaunchKernelGGL(tb_run_heads_kernel, grid(N2), dim3(256), 0, stream, d_key_sorted, d_index_sorted, N2, d_head, d_first);
    TMI_TB(tb_exclusive_sum(s, d_head, d_heads_before, (size_t)N2 + 1));
    TMI_TB(tb_exclusive_sum(s, d_first, d_firsts_before, (size_t)N2 + 1));
    hipLaunchKernelGGL(tb_run_nodes_kernel, grid(N2), dim3(256), 0, stream, d_key_sorted, d_index_sorted, d_head,
                       d_heads_before, d_firsts_before, N2, d_run_node, d_node_view, d_node_feature);
    hipLaunchKernelGGL(tb_endpoint_nodes_kernel, grid(N2), dim3(256), 0, stream, d_index_sorted, d_head, d_heads_before,
                       d_run_node, N2, d_endpoint_node);
    TMI_HIP(nodes_timer.mark());
    TMI_HIP(hipGetLastError());
    unsigned num_nodes = 0;
    TMI_HIP(s->download(&num_nodes, d_firsts_before + N2, 1));
    TMI_HIP(hipStreamSynchronize(stream));
    if (num_nodes < 2 || (long long)num_nodes > N2) {
      s->error = "build tracks: the device reported an impossible node count";
      return TMI_BA_ERR_DEVICE;
    }
    const size_t N = num_nodes;
    const int node_bits = tb_bits(num_nodes);
    sum->num_nodes = num_nodes;
    sum->phase_seconds[0] = nodes_timer.seconds();

    // step 2: the components of the unconstrained graph and their sizes
    unsigned *d_parent, *d_component, *d_size, *d_iota;
    TMI_HIP(s->alloc(&d_parent, N));
    TMI_HIP(s->alloc(&d_iota, N));
    TMI_HIP(s->alloc(&d_component, N));
    TMI_HIP(s->alloc_filled(&d_size, N, 0));
    TMI_HIP(components_timer.mark());
    hipLaunchKernelGGL(tb_iota_kernel, grid(N), dim3(256), 0, stream, d_parent, num_nodes);
    hipLaunchKernelGGL(tb_iota_kernel, grid(N), dim3(256), 0, stream, d_iota, num_nodes);  // the sorts' values
    hipLaunchKernelGGL(tb_union_kernel, grid(E), dim3(256), 0, stream, d_endpoint_node, E, num_nodes, d_parent, d_counters);
    hipLaunchKernelGGL(tb_flatten_kernel, grid(N), dim3(256), 0, stream, d_parent, num_nodes, d_component, d_counters);
    hipLaunchKernelGGL(tb_sizes_kernel, grid(N), dim3(256), 0, stream, d_component, num_nodes, d_size);
    hipLaunchKernelGGL(tb_component_stats_kernel, grid(N), dim3(256), 0, stream, d_component, d_size, num_nodes, cap,
                       d_counters);
    TMI_HIP(components_timer.mark());
    TMI_HIP(hipGetLastError());
    TMI_TB(read_counters());
    sum->num_components = (int64_t)counters[kTbComponents];
    sum->num_oversize_components = (int64_t)counters[kTbOversize];
    sum->phase_seconds[1] = components_timer.seconds();
    const unsigned num_oversize = (unsigned)counters[kTbOversize];
    if (counters[kTbComponents] > N || counters[kTbOversize] > counters[kTbComponents]) {
      s->error = "build tracks: the device reported an impossible component count";
      return TMI_BA_ERR_DEVICE;
    }

    // nodes sorted by (label, node id): for the replay by component, for the output by final label
    auto sort_nodes_by = [&](const unsigned* label, unsigned** sorted_label, unsigned** sorted_node) -> int {
      TMI_HIP(s->alloc(sorted_label, N));
      TMI_HIP(s->alloc(sorted_node, N));
      return tb_sort_pairs(s, label, *sorted_label, d_iota, *sorted_node, N, node_bits);
    };

    // step 3: the cap.  Without an oversize component the components are the final sets.
    unsigned *d_final = d_component, *d_set_size = d_size, *d_out_label = nullptr, *d_out_node = nullptr;
    unsigned *d_flag, *d_before;  // flags over the nodes and their sums, used by one step at a time
    TMI_HIP(s->alloc(&d_flag, N + 1));
    TMI_HIP(s->alloc(&d_before, N + 1));
    if (num_oversize) {
      unsigned *d_edge_flag, *d_edge_before, *d_edge_count, *d_by_component, *d_by_component_node, *d_position;
      unsigned *d_list_node_begin, *d_list_num_nodes, *d_list_num_edges, *d_list_edge_begin, *d_work_parent, *d_work_size;
      const size_t K = num_oversize;
      TMI_HIP(s->alloc(&d_edge_flag, (size_t)E + 1));
      TMI_HIP(s->alloc(&d_edge_before, (size_t)E + 1));
      TMI_HIP(s->alloc(&d_edge_count, N));
      TMI_HIP(s->alloc(&d_position, N));
      TMI_HIP(s->alloc(&d_list_node_begin, K));
      TMI_HIP(s->alloc(&d_list_num_nodes, K));
      TMI_HIP(s->alloc(&d_list_num_edges, K + 1));
      TMI_HIP(s->alloc(&d_list_edge_begin, K + 1));
      TMI_HIP(s->alloc(&d_work_parent, N));
      TMI_HIP(s->alloc(&d_work_size, N));
      TMI_HIP(s->alloc(&d_final, N));
      TMI_HIP(s->alloc(&d_set_size, N));
      TMI_HIP(hipMemsetAsync(d_edge_flag, 0, ((size_t)E + 1) * sizeof(unsigned), stream));
      TMI_HIP(hipMemsetAsync(d_edge_count, 0, N * sizeof(unsigned), stream));
      TMI_HIP(hipMemsetAsync(d_flag, 0, (N + 1) * sizeof(unsigned), stream));
      TMI_HIP(hipMemsetAsync(d_list_num_edges, 0, (K + 1) * sizeof(unsigned), stream));
      TMI_HIP(hipMemsetAsync(d_set_size, 0, N * sizeof(unsigned), stream));
      TMI_HIP(cap_timer.mark());
      hipLaunchKernelGGL(tb_replay_edges_kernel, grid(E), dim3(256), 0, stream, d_endpoint_node, d_component, d_size, E, cap,
                         d_edge_flag, d_edge_count);
      TMI_TB(tb_exclusive_sum(s, d_edge_flag, d_edge_before, (size_t)E + 1));
      TMI_TB(sort_nodes_by(d_component, &d_by_component, &d_by_component_node));
      hipLaunchKernelGGL(tb_component_heads_kernel, grid(N), dim3(256), 0, stream, d_by_component, d_by_component_node,
                         d_size, num_nodes, cap, d_position, d_flag);
      TMI_TB(tb_exclusive_sum(s, d_flag, d_before, N + 1));
      hipLaunchKernelGGL(tb_component_list_kernel, grid(N), dim3(256), 0, stream, d_by_component, d_flag, d_before, d_size,
                         d_edge_count, num_nodes, d_list_node_begin, d_list_num_nodes, d_list_num_edges);
      TMI_TB(tb_exclusive_sum(s, d_list_num_edges, d_list_edge_begin, K + 1));
      TMI_HIP(cap_timer.mark());
      TMI_HIP(hipGetLastError());
      unsigned num_replayed = 0, listed = 0;
      TMI_HIP(s->download(&num_replayed, d_edge_before + E, 1));
      TMI_HIP(s->download(&listed, d_before + N, 1));
      TMI_HIP(hipStreamSynchronize(stream));
      if (listed != num_oversize || num_replayed < 1 || (long long)num_replayed > E) {
        s->error = "build tracks: the device reported an impossible replay plan";
        return TMI_BA_ERR_DEVICE;
      }
      sum->num_replayed_edges = num_replayed;
      unsigned *d_replay_key, *d_replay_edge, *d_replay_key_sorted, *d_replay_edge_sorted;
      TMI_HIP(s->alloc(&d_replay_key, (size_t)num_replayed));
      TMI_HIP(s->alloc(&d_replay_edge, (size_t)num_replayed));
      TMI_HIP(s->alloc(&d_replay_key_sorted, (size_t)num_replayed));
      TMI_HIP(s->alloc(&d_replay_edge_sorted, (size_t)num_replayed));
      TMI_HIP(hipMemcpyAsync(d_final, d_component, N * sizeof(unsigned), hipMemcpyDeviceToDevice, stream));
      TMI_HIP(cap_timer.mark());
      hipLaunchKernelGGL(tb_replay_compact_kernel, grid(E), dim3(256), 0, stream, d_endpoint_node, d_component, d_edge_flag,
                         d_edge_before, E, d_replay_key, d_replay_edge);
      // stable: the edges of a component stay in ascending edge index
      TMI_TB(tb_sort_pairs(s, d_replay_key, d_replay_key_sorted, d_replay_edge, d_replay_edge_sorted, (size_t)num_replayed,
                           node_bits));
      hipLaunchKernelGGL(tb_iota_kernel, grid(N), dim3(256), 0, stream, d_work_parent, num_nodes);
      TMI_HIP(hipMemsetD32Async((hipDeviceptr_t)d_work_size, 1, N, stream));
      hipLaunchKernelGGL(tb_replay_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, stream, d_list_node_begin,
                         d_list_num_nodes, d_list_edge_begin, num_oversize, d_replay_edge_sorted, d_endpoint_node, d_position,
                         d_by_component_node, cap, d_work_parent, d_work_size, d_final, d_counters);
      hipLaunchKernelGGL(tb_sizes_kernel, grid(N), dim3(256), 0, stream, d_final, num_nodes, d_set_size);
      TMI_HIP(cap_timer.mark());
      TMI_HIP(hipGetLastError());
      TMI_HIP(output_timer.mark());
      TMI_TB(sort_nodes_by(d_final, &d_out_label, &d_out_node));
    } else {
      TMI_HIP(output_timer.mark());
      TMI_TB(sort_nodes_by(d_component, &d_out_label, &d_out_node));
    }

    // steps 4 to 6: small sets, consistency, the CSR
    unsigned long long *d_view_key, *d_view_key_sorted;
    unsigned *d_by_view_node, *d_keep, *d_obs_flag, *d_obs_before;
    TMI_HIP(s->alloc(&d_view_key, N));
    TMI_HIP(s->alloc(&d_view_key_sorted, N));
    TMI_HIP(s->alloc(&d_by_view_node, N));
    TMI_HIP(s->alloc(&d_keep, N));
    TMI_HIP(s->alloc_filled(&d_obs_flag, N + 1, 0));
    TMI_HIP(s->alloc(&d_obs_before, N + 1));
    TMI_HIP(hipMemsetAsync(d_flag, 0, (N + 1) * sizeof(unsigned), stream));
    hipLaunchKernelGGL(tb_view_keys_kernel, grid(N), dim3(256), 0, stream, d_final, d_node_view, num_nodes, d_view_key);
    TMI_TB(tb_sort_pairs(s, d_view_key, d_view_key_sorted, d_iota, d_by_view_node, N, 32 + node_bits));
    hipLaunchKernelGGL(tb_keep_kernel, grid(N), dim3(256), 0, stream, d_view_key_sorted, d_by_view_node, d_set_size,
                       num_nodes, min_length, d_keep, d_counters);
    hipLaunchKernelGGL(tb_output_flags_kernel, grid(N), dim3(256), 0, stream, d_out_label, d_out_node, d_set_size, d_keep,
                       num_nodes, min_length, d_obs_flag, d_flag, d_counters);
    TMI_TB(tb_exclusive_sum(s, d_obs_flag, d_obs_before, N + 1));
    TMI_TB(tb_exclusive_sum(s, d_flag, d_before, N + 1));
    TMI_HIP(output_timer.mark());
    TMI_HIP(hipGetLastError());
    unsigned num_obs = 0, num_tracks = 0;
    TMI_HIP(s->download(&num_obs, d_obs_before + N, 1));
    TMI_HIP(s->download(&num_tracks, d_before + N, 1));
    TMI_TB(read_counters());
    if (num_oversize) sum->phase_seconds[2] = cap_timer.seconds(0, 1) + cap_timer.seconds(2, 3);
    sum->num_sets = (int64_t)counters[kTbSets];
    sum->num_small_tracks = (int64_t)counters[kTbSmall];
    sum->num_inconsistent_features = (int64_t)counters[kTbInconsistent];
    sum->num_tracks = num_tracks;
    sum->num_observations = num_obs;
    if (num_obs > num_nodes || (unsigned long long)num_tracks + counters[kTbSmall] != counters[kTbSets] ||
        counters[kTbInconsistent] + num_obs > N) {
      s->error = "build tracks: the device reported impossible totals";
      return TMI_BA_ERR_DEVICE;
    }
    too_small = (int64_t)num_tracks > track_capacity || (int64_t)num_obs > obs_capacity;
    long long* d_track_begin = nullptr;
    unsigned *d_obs_view = nullptr, *d_obs_feature = nullptr, *d_endpoint_label = nullptr;
    TMI_HIP(output_timer.mark());
    if (!too_small) {
      TMI_HIP(s->alloc(&d_track_begin, (size_t)num_tracks + 1));
      TMI_HIP(s->alloc(&d_obs_view, (size_t)num_obs));
      TMI_HIP(s->alloc(&d_obs_feature, (size_t)num_obs));
      hipLaunchKernelGGL(tb_emit_kernel, grid((long long)N + 1), dim3(256), 0, stream, d_out_node, d_obs_flag, d_obs_before,
                         d_flag, d_before, d_node_view, d_node_feature, num_nodes, d_track_begin, d_obs_view, d_obs_feature);
    }
    if (endpoint_label) {
      TMI_HIP(s->alloc(&d_endpoint_label, (size_t)N2));
      hipLaunchKernelGGL(tb_endpoint_labels_kernel, grid(N2), dim3(256), 0, stream, d_endpoint_node, d_final, N2,
                         d_endpoint_label);
    }
    TMI_HIP(output_timer.mark());
    TMI_HIP(hipGetLastError());
    if (!too_small) {
      static_assert(sizeof(long long) == sizeof(int64_t), "track_begin is read back as it is");
      TMI_HIP(s->download((long long*)track_begin, d_track_begin, (size_t)num_tracks + 1));
      TMI_HIP(s->download(obs_view, d_obs_view, (size_t)num_obs));
      TMI_HIP(s->download(obs_feature, d_obs_feature, (size_t)num_obs));
    }
    TMI_HIP(s->download(endpoint_node, d_endpoint_node, (size_t)N2));
    TMI_HIP(s->download(endpoint_label, d_endpoint_label, (size_t)N2));
    TMI_HIP(hipStreamSynchronize(stream));
    sum->phase_seconds[3] = output_timer.seconds(0, 1) + output_timer.seconds(2, 3);
    sum->kernel_seconds = sum->phase_seconds[0] + sum->phase_seconds[1] + sum->phase_seconds[2] + sum->phase_seconds[3];
    return TMI_BA_OK;
  });
  if (rc == TMI_BA_OK && E == 0) track_begin[0] = 0;
  sum->seconds = now_s() - t0;
  if (rc == TMI_BA_OK && too_small) {
    g_last_error = "build tracks: track_capacity or obs_capacity is too small (summary->num_tracks, num_observations)";
    return TMI_BA_ERR_CAPACITY;
  }
  return rc;
}
#undef TMI_TB
}  // extern "C"

// ---- the view-graph steps: largest component, MST orientations (view_graph_kernels.h) -----------
namespace {
// What both calls ask of the batch, the mask and (need_weights) the weights.  null: fine.
const char* check_view_graph_arguments(const tmi_ba_view_pair_batch* B, const uint8_t* mask, bool need_weights,
                                       const int32_t* weight) {
  const int V = B->num_views, E = B->num_pairs;
  if (V < 0 || E < 0) return "view graph: negative size";
  if (E > 0 && (!B->pair_view1 || !B->pair_view2)) return "view graph: missing array";
  if (need_weights && E > 0 && (!weight || !B->pair_rotation2)) return "view graph: missing array";
  if (E > (1 << 30)) return "view graph: more than 2^30 pairs";
  for (int e = 0; e < E; ++e) {
    const int a = B->pair_view1[e], b = B->pair_view2[e];
    if (a < 0 || a >= V || b < 0 || b >= V) return "view graph: view index out of range";
    if (a == b) return "view graph: a view paired with itself";
    if (need_weights && (!mask || mask[e]) && weight[e] < 0)
      return "view graph: negative num_verified_matches on an alive edge";
  }
  return nullptr;
}

struct ViewGraphDevice {
  int *view1, *view2;
  unsigned char *mask, *keep;
  unsigned *label, *size;
  unsigned long long* counters;
};

#define TMI_VG(call)                  \
  do {                                \
    const int rc_ = (call);           \
    if (rc_ != TMI_BA_OK) return rc_; \
  } while (0)

// Uploads the edges and queues steps 1 to 3 of tmi_ba_largest_connected_component: label [V], keep [E], counters.
int vg_queue_components(OneShot* s, const tmi_ba_view_pair_batch* B, const uint8_t* mask, ViewGraphDevice* D,
                        StreamTimer* timer) {
  const int V = B->num_views, E = B->num_pairs;
  const hipStream_t stream = s->stream;
  auto grid = [](long long n) { return dim3((unsigned)((n + 255) / 256)); };
  unsigned* d_parent;
  D->mask = nullptr;
  TMI_HIP(s->upload(&D->view1, (const int*)B->pair_view1, (size_t)E));
  TMI_HIP(s->upload(&D->view2, (const int*)B->pair_view2, (size_t)E));
  if (mask) TMI_HIP(s->upload(&D->mask, (const unsigned char*)mask, (size_t)E));
  TMI_HIP(s->alloc(&D->keep, (size_t)E));
  TMI_HIP(s->alloc(&d_parent, (size_t)V));
  TMI_HIP(s->alloc(&D->label, (size_t)V));
  TMI_HIP(s->alloc_filled(&D->size, (size_t)V, 0));
  TMI_HIP(s->alloc_filled(&D->counters, (size_t)kVgCounters, 0));
  TMI_HIP(timer->mark());
  hipLaunchKernelGGL(tb_iota_kernel, grid(V), dim3(256), 0, stream, d_parent, (unsigned)V);
  hipLaunchKernelGGL(vg_union_kernel, grid(E), dim3(256), 0, stream, D->view1, D->view2, D->mask, E, (unsigned)V, d_parent,
                     D->counters);
  hipLaunchKernelGGL(tb_flatten_kernel, grid(V), dim3(256), 0, stream, d_parent, (unsigned)V, D->label, D->counters);
  hipLaunchKernelGGL(tb_sizes_kernel, grid(V), dim3(256), 0, stream, D->label, (unsigned)V, D->size);
  hipLaunchKernelGGL(vg_component_stats_kernel, grid(V), dim3(256), 0, stream, D->label, D->size, (unsigned)V, D->counters);
  hipLaunchKernelGGL(vg_keep_kernel, grid(E), dim3(256), 0, stream, D->view1, D->mask, D->label, E, D->keep, D->counters);
  return TMI_BA_OK;
}

// The component summary from the counters; false: the device reported impossible totals.
bool vg_component_summary(const unsigned long long* c, int V, int E, tmi_ba_view_graph_component_summary* sum) {
  const unsigned long long best = c[kVgBest];
  const unsigned long long size = best >> 32, label = 0xffffffffull - (best & 0xffffffffull);
  if (c[kVgAlive] > (unsigned long long)E || c[kVgKept] > c[kVgAlive] || c[kVgEdgeViews] > (unsigned long long)V ||
      size > c[kVgEdgeViews] || (best && (label >= (unsigned long long)V || size < 2 || !c[kVgKept])) ||
      (!best && (c[kVgAlive] || c[kVgComponents])))
    return false;
  sum->num_components = (int32_t)c[kVgComponents];
  sum->largest_label = best ? (int32_t)label : -1;
  sum->largest_num_views = (int32_t)size;
  sum->num_pairs_kept = (int32_t)c[kVgKept];
  sum->num_pairs_removed = (int32_t)(c[kVgAlive] - c[kVgKept]);
  sum->num_views_removed = (int32_t)(c[kVgEdgeViews] - size);
  return true;
}
}  // namespace
extern "C" {

int32_t tmi_ba_largest_connected_component(const tmi_ba_view_pair_batch* Bh, const uint8_t* pair_mask, int32_t device,
                                           int32_t* view_label, uint8_t* view_in_largest, uint8_t* pair_keep,
                                           tmi_ba_view_graph_component_summary* summary) {
  if (!Bh || !summary) return bad_argument("largest component: null batch or summary");
  const double t0 = now_s();
  // argument errors before the device is looked for
  if (const char* why = check_view_graph_arguments(Bh, pair_mask, false, nullptr)) return bad_argument(why);
  const int V = Bh->num_views, E = Bh->num_pairs;
  tmi_ba_view_graph_component_summary sum;  // the caller's is written on success only
  memset(&sum, 0, sizeof(sum));
  sum.largest_label = -1;
  std::vector<int32_t> label_h((size_t)V);
  std::vector<uint8_t> in_largest_h((size_t)V, 0), keep_h((size_t)E, 0);
  for (int v = 0; v < V; ++v) label_h[v] = v;  // (E == 0: every view is its own component)
  const int rc = one_shot_batch(device, "largest component: no such device", E, t0, &sum.seconds, [&](OneShot* s) -> int {
    const hipStream_t stream = s->stream;
    ViewGraphDevice D;
    unsigned char* d_in_largest;
    StreamTimer timer(stream);
    TMI_HIP(timer.status);
    TMI_HIP(s->alloc(&d_in_largest, (size_t)V));
    TMI_VG(vg_queue_components(s, Bh, pair_mask, &D, &timer));
    hipLaunchKernelGGL(vg_view_flags_kernel, dim3((V + 255) / 256), dim3(256), 0, stream, D.label, (unsigned)V, D.counters,
                       d_in_largest);
    TMI_HIP(timer.mark());
    TMI_HIP(hipGetLastError());
    unsigned long long counters[kVgCounters];
    static_assert(sizeof(unsigned) == sizeof(int32_t), "labels are read back as they are");
    TMI_HIP(s->download(counters, D.counters, (size_t)kVgCounters));
    TMI_HIP(s->download((unsigned*)label_h.data(), D.label, label_h.size()));
    TMI_HIP(s->download(in_largest_h.data(), d_in_largest, in_largest_h.size()));
    TMI_HIP(s->download(keep_h.data(), D.keep, keep_h.size()));
    TMI_HIP(hipStreamSynchronize(stream));
    if (counters[kVgError]) {
      s->error = "largest component: a device loop reached its bound";
      return TMI_BA_ERR_DEVICE;
    }
    if (!vg_component_summary(counters, V, E, &sum)) {
      s->error = "largest component: the device reported impossible totals";
      return TMI_BA_ERR_DEVICE;
    }
    sum.kernel_seconds = timer.seconds();
    return TMI_BA_OK;
  });
  if (rc != TMI_BA_OK) return rc;
  if (view_label) std::copy(label_h.begin(), label_h.end(), view_label);
  if (view_in_largest) std::copy(in_largest_h.begin(), in_largest_h.end(), view_in_largest);
  if (pair_keep) std::copy(keep_h.begin(), keep_h.end(), pair_keep);
  sum.seconds = now_s() - t0;
  *summary = sum;
  return TMI_BA_OK;
}

int32_t tmi_ba_orientations_from_maximum_spanning_tree(const tmi_ba_view_pair_batch* Bh,
                                                       const int32_t* pair_num_verified_matches,
                                                       const uint8_t* pair_mask, int32_t root_view, int32_t device,
                                                       double* view_orientation, int32_t* view_parent,
                                                       int32_t* view_parent_pair, int32_t* view_depth,
                                                       uint8_t* pair_in_tree, tmi_ba_spanning_tree_summary* summary) {
  if (!Bh || !summary) return bad_argument("spanning tree: null batch or summary");
  const double t0 = now_s();
  // argument errors before the device is looked for
  if (const char* why = check_view_graph_arguments(Bh, pair_mask, true, pair_num_verified_matches)) return bad_argument(why);
  const int V = Bh->num_views, E = Bh->num_pairs;
  if (root_view < -1 || root_view >= V) return bad_argument("spanning tree: root_view outside [-1, num_views)");
  tmi_ba_spanning_tree_summary sum;  // the caller's is written on success only
  memset(&sum, 0, sizeof(sum));
  sum.component.largest_label = -1;
  sum.root_view = -1;
  std::vector<double> orientation_h;
  std::vector<int32_t> parent_h, parent_pair_h, depth_h;
  std::vector<uint8_t> in_tree_h;
  const int rc = one_shot_batch(device, "spanning tree: no such device", E, t0, &sum.component.seconds, [&](OneShot* s) -> int {
    const hipStream_t stream = s->stream;
    auto grid = [](long long n) { return dim3((unsigned)((n + 255) / 256)); };
    ViewGraphDevice D;
    StreamTimer timer(stream);
    TMI_HIP(timer.status);
    int *d_weight, *d_tree;  // d_tree [5 V]: parent, parent pair, depth, the two frontiers
    unsigned *d_index, *d_by_pair, *d_weight_key, *d_weight_key_sorted, *d_edge_of_rank, *d_comp, *d_hook, *d_best;
    unsigned *d_degree, *d_row_ptr, *d_cursor;
    unsigned long long *d_pair_key, *d_pair_key_sorted;
    unsigned char* d_in_tree;
    int2* d_row;
    double *d_relative, *d_orientation;
    const size_t Vs = (size_t)V, Es = (size_t)E;
    TMI_HIP(s->upload(&d_weight, (const int*)pair_num_verified_matches, Es));
    TMI_HIP(s->upload(&d_relative, Bh->pair_rotation2, 3 * Es));
    TMI_HIP(s->alloc(&d_pair_key, Es));
    TMI_HIP(s->alloc(&d_pair_key_sorted, Es));
    TMI_HIP(s->alloc(&d_index, Es));
    TMI_HIP(s->alloc(&d_by_pair, Es));
    TMI_HIP(s->alloc(&d_weight_key, Es));
    TMI_HIP(s->alloc(&d_weight_key_sorted, Es));
    TMI_HIP(s->alloc(&d_edge_of_rank, Es));
    TMI_HIP(s->alloc_filled(&d_in_tree, Es, 0));
    TMI_HIP(s->alloc(&d_row, 2 * Es));  // (a tree has fewer edges than views; the flags can never exceed E)
    TMI_HIP(s->alloc(&d_comp, Vs));
    TMI_HIP(s->alloc(&d_hook, Vs));
    TMI_HIP(s->alloc(&d_best, Vs));
    TMI_HIP(s->alloc_filled(&d_degree, Vs + 1, 0));
    TMI_HIP(s->alloc(&d_row_ptr, Vs + 1));
    TMI_HIP(s->alloc(&d_cursor, Vs + 1));
    TMI_HIP(s->alloc(&d_tree, 5 * Vs));
    TMI_HIP(hipMemsetAsync(d_tree, 0xff, 3 * Vs * sizeof(int), stream));
    TMI_HIP(s->alloc_filled(&d_orientation, 3 * Vs, 0));
    // step 1
    TMI_VG(vg_queue_components(s, Bh, pair_mask, &D, &timer));
    // step 2: the ranks of the reference's order, then the Boruvka rounds
    hipLaunchKernelGGL(vg_pair_keys_kernel, grid(E), dim3(256), 0, stream, D.view1, D.view2, E, d_pair_key, d_index);
    TMI_VG(tb_sort_pairs(s, d_pair_key, d_pair_key_sorted, d_index, d_by_pair, Es, 32 + tb_bits((unsigned)V)));
    hipLaunchKernelGGL(vg_weight_keys_kernel, grid(E), dim3(256), 0, stream, d_by_pair, d_weight, D.keep, E, d_weight_key);
    TMI_VG(tb_sort_pairs(s, d_weight_key, d_weight_key_sorted, d_by_pair, d_edge_of_rank, Es, 32));
    hipLaunchKernelGGL(tb_iota_kernel, grid(V), dim3(256), 0, stream, d_comp, (unsigned)V);
    int rounds = 1;  // ceil(log2 V) + 1
    while ((1ll << (rounds - 1)) < (long long)V) ++rounds;
    for (int round = 0; round < rounds; ++round) {
      TMI_HIP(hipMemsetAsync(d_best, 0xff, Vs * sizeof(unsigned), stream));
      hipLaunchKernelGGL(vg_min_edge_kernel, grid(E), dim3(256), 0, stream, d_edge_of_rank, D.keep, D.view1, D.view2, d_comp,
                         E, d_best);
      hipLaunchKernelGGL(vg_hook_kernel, grid(V), dim3(256), 0, stream, d_edge_of_rank, D.view1, D.view2, d_comp, d_best,
                         (unsigned)V, d_hook, d_in_tree);
      hipLaunchKernelGGL(tb_flatten_kernel, grid(V), dim3(256), 0, stream, d_hook, (unsigned)V, d_comp, D.counters);
    }
    // steps 3 and 4: the tree's CSR and the walk from the root
    hipLaunchKernelGGL(vg_tree_degree_kernel, grid(E), dim3(256), 0, stream, d_in_tree, D.view1, D.view2, E, d_degree,
                       D.counters);
    TMI_VG(tb_exclusive_sum(s, d_degree, d_row_ptr, Vs + 1));
    TMI_HIP(hipMemcpyAsync(d_cursor, d_row_ptr, (Vs + 1) * sizeof(unsigned), hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(vg_tree_fill_kernel, grid(E), dim3(256), 0, stream, d_in_tree, D.view1, D.view2, E, d_cursor, d_row);
    hipLaunchKernelGGL(vg_root_kernel, dim3(1), dim3(kVgRootThreads), 0, stream, V, (int)root_view, D.label, d_row_ptr,
                       d_row, d_relative, d_orientation, d_tree, D.counters);
    TMI_HIP(timer.mark());
    TMI_HIP(hipGetLastError());
    unsigned long long counters[kVgCounters];
    orientation_h.resize(3 * Vs);
    parent_h.resize(Vs);
    parent_pair_h.resize(Vs);
    depth_h.resize(Vs);
    in_tree_h.resize(Es);
    TMI_HIP(s->download(counters, D.counters, (size_t)kVgCounters));
    TMI_HIP(s->download(orientation_h.data(), d_orientation, 3 * Vs));
    TMI_HIP(s->download(parent_h.data(), d_tree, Vs));
    TMI_HIP(s->download(parent_pair_h.data(), d_tree + Vs, Vs));
    TMI_HIP(s->download(depth_h.data(), d_tree + 2 * Vs, Vs));
    TMI_HIP(s->download(in_tree_h.data(), d_in_tree, Es));
    TMI_HIP(hipStreamSynchronize(stream));
    if (counters[kVgError]) {
      s->error = "spanning tree: a device loop reached its bound";
      return TMI_BA_ERR_DEVICE;
    }
    if (!vg_component_summary(counters, V, E, &sum.component)) {
      s->error = "spanning tree: the device reported impossible totals";
      return TMI_BA_ERR_DEVICE;
    }
    if (counters[kVgBadRoot]) {
      s->error = "spanning tree: root_view is outside the largest component";
      return TMI_BA_ERR_INVALID_ARGUMENT;
    }
    if (counters[kVgBest]) {
      const unsigned long long views = (unsigned long long)sum.component.largest_num_views;
      if (counters[kVgTreePairs] + 1 != views || counters[kVgReached] != views || counters[kVgDepth] >= views ||
          counters[kVgRoot] >= (unsigned long long)V) {
        s->error = "spanning tree: the device's tree does not span the largest component";
        return TMI_BA_ERR_DEVICE;
      }
      sum.usable = 1;
      sum.num_tree_pairs = (int32_t)counters[kVgTreePairs];
      sum.tree_depth = (int32_t)counters[kVgDepth];
      sum.root_view = (int32_t)counters[kVgRoot];
    }
    sum.component.kernel_seconds = timer.seconds();
    return TMI_BA_OK;
  });
  if (rc != TMI_BA_OK) return rc;
  if (sum.usable) {
    for (int v = 0; v < V && view_orientation; ++v)
      if (depth_h[v] >= 0) std::copy(&orientation_h[3 * (size_t)v], &orientation_h[3 * (size_t)v] + 3, view_orientation + 3 * (size_t)v);
    if (view_parent) std::copy(parent_h.begin(), parent_h.end(), view_parent);
    if (view_parent_pair) std::copy(parent_pair_h.begin(), parent_pair_h.end(), view_parent_pair);
    if (view_depth) std::copy(depth_h.begin(), depth_h.end(), view_depth);
    if (pair_in_tree) std::copy(in_tree_h.begin(), in_tree_h.end(), pair_in_tree);
  }
  sum.component.seconds = now_s() - t0;
  *summary = sum;
  return TMI_BA_OK;
}
#undef TMI_VG
}  // extern "C"

// ---- batched EstimateUncalibratedRelativePose: eight-point RANSAC (two_view_ransac_kernels.h) ----
extern "C" {
void tmi_ba_two_view_ransac_options_init(tmi_ba_two_view_ransac_options* o) {
  if (!o) return;
  o->failure_probability = 0.01;  // sample_consensus_estimator.h:57-65
  o->min_inlier_ratio = 0.0;
  o->min_iterations = 10;         // estimate_twoview_info.h:70
  o->max_iterations = 1000;       // estimate_twoview_info.h:71
  o->chunk_iterations = 0;
  o->device = -1;
  o->seed = 0;
}
}  // extern "C"
namespace {
// What the two RANSAC calls over view pairs share beyond the scaffold.  P = EightPointProblem: model_a = the
// fundamental matrix, focal lengths out.  P = FivePointProblem: model_a = the essential matrix, pair_best_solution out.
template <class P>
int32_t two_view_ransac_call(
    const char* name, const tmi_ba_two_view_ransac_options* L, int32_t num_pairs, const int64_t* pair_offset, const double* feature1,
    const double* feature2, const double* pair_error_threshold, const uint8_t* pair_mask, const uint32_t* pair_stream,
    const int32_t* samples, int32_t samples_given, int8_t* pair_status, int32_t* pair_num_correspondences,
    int32_t* pair_num_inliers, int32_t* pair_num_iterations, int32_t* pair_best_iteration, int32_t* pair_best_solution,
    double* pair_confidence, double* fundamental_matrix, double* focal_length1, double* focal_length2, double* rotation,
    double* position, uint8_t* corr_inlier, int32_t* hypothesis_cost, tmi_ba_two_view_ransac_summary* sum) {
  constexpr int kSample = P::kSample, kSlots = P::kSlots;
  const std::string what = name;
  auto bad = [&](const char* why) { return bad_argument((what + ": " + why).c_str()); };
  if (!L || !sum) return bad("null options or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is looked for
  const int Npair = num_pairs;
  if (Npair < 0) return bad("negative size");
  if (!pair_offset) return bad("missing array");
  if (pair_offset[0] != 0) return bad("pair_offset must start at 0");
  for (int p = 0; p < Npair; ++p)
    if (pair_offset[p + 1] < pair_offset[p]) return bad("pair_offset decreases");
  const int64_t total = pair_offset[Npair];
  if (total >= (int64_t)0x7fffffffLL) return bad("more than 2^31 correspondences");
  if (total && (!feature1 || !feature2)) return bad("missing array");
  if (const char* why = ransac_options_error(L, samples, samples_given)) return bad(why);
  const int K = L->max_iterations;
  std::vector<int> selected, sel_pair, sel_rank;  // sel_pair: the attempted ones, the device's slots
  for (int p = 0; p < Npair; ++p) {
    if (pair_mask && !pair_mask[p]) continue;
    const int64_t n = pair_offset[p + 1] - pair_offset[p];
    if (n >= kSample) {
      if (!pair_error_threshold) return bad("missing pair_error_threshold");
      if (!(pair_error_threshold[p] > 0.0))
        return bad("error threshold must be positive");
      if (samples_given)
        for (int64_t i = 0; i < K; ++i) {
          const int32_t* t = samples + kSample * ((int64_t)K * p + i);
          for (int a = 0; a < kSample; ++a) {
            bool wrong = t[a] < 0 || t[a] >= n;
            for (int b = 0; b < a; ++b) wrong = wrong || t[a] == t[b];
            if (wrong) return bad("a sample with a repeated or out-of-range index");
          }
        }
      sel_pair.push_back(p);
      sel_rank.push_back((int)selected.size());
    }
    selected.push_back(p);
  }
  const int num_selected = (int)selected.size(), S = (int)sel_pair.size();
  // nothing below fails on an argument: preset the outputs
  for (int p = 0; p < Npair; ++p) {
    const bool sel = !pair_mask || pair_mask[p];
    if (pair_status) pair_status[p] = (int8_t)(sel ? 1 : -1);
    if (pair_num_correspondences) pair_num_correspondences[p] = sel ? (int32_t)(pair_offset[p + 1] - pair_offset[p]) : 0;
    if (pair_num_inliers) pair_num_inliers[p] = 0;
    if (pair_num_iterations) pair_num_iterations[p] = 0;
    if (pair_best_iteration) pair_best_iteration[p] = -1;
    if (pair_best_solution) pair_best_solution[p] = -1;
    if (pair_confidence) pair_confidence[p] = 0.0;
    if (fundamental_matrix) std::fill(fundamental_matrix + 9 * (size_t)p, fundamental_matrix + 9 * (size_t)p + 9, 0.0);
    if (focal_length1) focal_length1[p] = 0.0;
    if (focal_length2) focal_length2[p] = 0.0;
    if (rotation) std::fill(rotation + 3 * (size_t)p, rotation + 3 * (size_t)p + 3, 0.0);
    if (position) std::fill(position + 3 * (size_t)p, position + 3 * (size_t)p + 3, 0.0);
  }
  if (corr_inlier && total) memset(corr_inlier, 0, (size_t)total);
  if (hypothesis_cost) std::fill(hypothesis_cost, hypothesis_cost + (size_t)num_selected * (size_t)K * kSlots, -1);
  sum->num_pairs = num_selected;
  sum->num_too_few_correspondences = num_selected - S;
  // the attempted pairs' correspondences, pair-major, structure of arrays
  RansacRun run;
  std::vector<long long>& sel_ptr = run.sel_ptr;
  sel_ptr.assign((size_t)S + 1, 0);
  for (int s = 0; s < S; ++s) sel_ptr[(size_t)s + 1] = sel_ptr[s] + (pair_offset[sel_pair[s] + 1] - pair_offset[sel_pair[s]]);
  const size_t M = (size_t)sel_ptr[S];
  std::vector<double> xs(4 * std::max<size_t>(M, 1));
  double *hx1 = xs.data(), *hy1 = hx1 + M, *hx2 = hy1 + M, *hy2 = hx2 + M;
  std::vector<double> thresh((size_t)S);
  std::vector<unsigned> stream_id((size_t)S);
  for (int s = 0; s < S; ++s) {
    const int p = sel_pair[s];
    const int64_t o0 = pair_offset[p];
    const int n = (int)(pair_offset[p + 1] - o0);
    for (int m = 0; m < n; ++m) {
      const size_t o = (size_t)sel_ptr[s] + m;
      hx1[o] = feature1[2 * (o0 + m)];
      hy1[o] = feature1[2 * (o0 + m) + 1];
      hx2[o] = feature2[2 * (o0 + m)];
      hy2[o] = feature2[2 * (o0 + m) + 1];
    }
    thresh[s] = pair_error_threshold[p];
    stream_id[s] = pair_stream ? pair_stream[p] : (unsigned)p;
  }
  run.plan(L, kSample);
  const std::string no_device = what + ": no such device";
  return one_shot_batch(L->device, no_device.c_str(), S, t0, &sum->seconds, [&](OneShot* s) -> int {
    const hipStream_t stream = s->stream;
    double *d_xs, *d_model_out;
    TMI_HIP(s->upload(&d_xs, (const double*)xs.data(), xs.size()));
    if (const int rc = run.upload<P>(s, L->seed, sel_pair, stream_id, thresh, samples_given ? samples : nullptr,
                                     (size_t)Npair, hypothesis_cost != nullptr))
      return rc;
    RansacBatch& B = run.B;
    for (int q = 0; q < P::kPlanes; ++q) B.plane[q] = d_xs + q * M;  // x1, y1, x2, y2
    TMI_HIP(s->alloc(&d_model_out, (size_t)17 * S));
    StreamTimer timer(stream);
    TMI_HIP(timer.status);
    TMI_HIP(timer.mark());
    if (const int rc = run.chunks<P>(s, sum)) return rc;
    hipLaunchKernelGGL(two_view_final_kernel, dim3(S), dim3(64), 0, stream, B, run.d_slot_inlier, run.d_num_inliers,
                       run.d_status, d_model_out);
    TMI_HIP(timer.mark());
    TMI_HIP(hipGetLastError());
    std::vector<double> model_h((size_t)17 * S);
    TMI_HIP(s->download(model_h.data(), d_model_out, model_h.size()));
    if (const int rc = run.read_back(s, corr_inlier != nullptr, kSlots, sel_rank, hypothesis_cost)) return rc;
    sum->kernel_seconds = timer.seconds();
    sum->num_chunks = run.chunks_run;
    const RansacItemArrays out = {pair_status,         pair_num_inliers,   pair_num_iterations,
                                  pair_best_iteration, pair_best_solution, pair_confidence};
    for (int v = 0; v < S; ++v) {
      const int p = sel_pair[v];
      const int n = (int)(sel_ptr[(size_t)v + 1] - sel_ptr[v]);
      const int code = run.status[v];
      const RansacState& st = run.state[v];
      const double* mo = model_h.data() + 17 * (size_t)v;
      if (code == 0) sum->num_estimated++; else sum->num_no_model++;
      sum->total_iterations += st.num_iterations;
      sum->total_scores += (int64_t)st.num_iterations * n;
      run.item_results(v, p, code, out);
      if (fundamental_matrix) std::copy(mo, mo + 9, fundamental_matrix + 9 * (size_t)p);
      if (focal_length1) focal_length1[p] = mo[9];
      if (focal_length2) focal_length2[p] = mo[10];
      if (rotation) std::copy(mo + 11, mo + 14, rotation + 3 * (size_t)p);
      if (position) std::copy(mo + 14, mo + 17, position + 3 * (size_t)p);
      if (corr_inlier)
        std::copy(run.slot_inlier.begin() + (size_t)sel_ptr[v], run.slot_inlier.begin() + (size_t)sel_ptr[(size_t)v + 1],
                  corr_inlier + pair_offset[p]);
    }
    return TMI_BA_OK;
  });
}
}  // namespace
extern "C" {

int32_t tmi_ba_estimate_uncalibrated_relative_poses(
    const tmi_ba_two_view_ransac_options* L, int32_t num_pairs, const int64_t* pair_offset, const double* feature1,
    const double* feature2, const double* pair_error_threshold, const uint8_t* pair_mask, const uint32_t* pair_stream,
    const int32_t* samples, int32_t samples_given, int8_t* pair_status, int32_t* pair_num_correspondences,
    int32_t* pair_num_inliers, int32_t* pair_num_iterations, int32_t* pair_best_iteration, double* pair_confidence,
    double* fundamental_matrix, double* focal_length1, double* focal_length2, double* rotation, double* position,
    uint8_t* corr_inlier, int32_t* hypothesis_cost, tmi_ba_two_view_ransac_summary* sum) {
  return two_view_ransac_call<EightPointProblem>(
      "uncalibrated relative poses", L, num_pairs, pair_offset, feature1, feature2, pair_error_threshold, pair_mask,
      pair_stream, samples, samples_given, pair_status, pair_num_correspondences, pair_num_inliers, pair_num_iterations,
      pair_best_iteration, nullptr, pair_confidence, fundamental_matrix, focal_length1, focal_length2, rotation, position,
      corr_inlier, hypothesis_cost, sum);
}

// ---- batched EstimateRelativePose: five-point RANSAC (two_view_calibrated_kernels.h) ----
int32_t tmi_ba_estimate_calibrated_relative_poses(
    const tmi_ba_two_view_ransac_options* L, int32_t num_pairs, const int64_t* pair_offset, const double* feature1,
    const double* feature2, const double* pair_error_threshold, const uint8_t* pair_mask, const uint32_t* pair_stream,
    const int32_t* samples, int32_t samples_given, int8_t* pair_status, int32_t* pair_num_correspondences,
    int32_t* pair_num_inliers, int32_t* pair_num_iterations, int32_t* pair_best_iteration, int32_t* pair_best_solution,
    double* pair_confidence, double* essential_matrix, double* rotation, double* position, uint8_t* corr_inlier,
    int32_t* hypothesis_cost, tmi_ba_two_view_ransac_summary* sum) {
  return two_view_ransac_call<FivePointProblem>(
      "calibrated relative poses", L, num_pairs, pair_offset, feature1, feature2, pair_error_threshold, pair_mask,
      pair_stream, samples, samples_given, pair_status, pair_num_correspondences, pair_num_inliers, pair_num_iterations,
      pair_best_iteration, pair_best_solution, pair_confidence, essential_matrix, nullptr, nullptr, rotation, position,
      corr_inlier, hypothesis_cost, sum);
}
}  // extern "C"

// ---- batched EstimateHomography: four-point RANSAC, either scoring (homography_kernels.h) ----
namespace {
// The MLESAC half of a RansacRun: the double costs, the inlier counts and the double best cost beside RansacBatch, and
// the chunk loop over the MLE kernels.  (The loop is written out once more rather than shared with
// RansacRun::chunks: the two differ in the kernels launched, and the integer calls' loop stays as it is.)
struct RansacMleRun : RansacRun {
  RansacMle E = {};

  template <class P>
  int upload_mle(OneShot* s, bool want_hypothesis_cost_real) {
    memset(&E, 0, sizeof(E));
    const size_t slots = (size_t)S * chunk * P::kSlots, hyp = (size_t)S * K * P::kSlots;
    const std::vector<double> best((size_t)S, std::numeric_limits<double>::max());
    TMI_HIP(s->alloc(&E.cost, slots));
    TMI_HIP(s->alloc(&E.inliers, slots));
    TMI_HIP(s->upload(&E.best_cost, best.data(), best.size()));
    TMI_HIP(hipStreamSynchronize(s->stream));  // (`best` goes out of scope)
    if (want_hypothesis_cost_real) {
      const std::vector<double> nan(hyp, std::numeric_limits<double>::quiet_NaN());
      TMI_HIP(s->upload(&E.hypothesis_cost, nan.data(), nan.size()));
      TMI_HIP(hipStreamSynchronize(s->stream));
    }
    return TMI_BA_OK;
  }

  template <class P>
  int chunks_mle(OneShot* s, tmi_ba_two_view_ransac_summary* phases) {
    const hipStream_t stream = s->stream;
    std::vector<int> active;
    const int max_chunks = (K + chunk - 1) / chunk;
    for (int ch = 0; ch < max_chunks; ++ch) {
      active.clear();
      for (int v = 0; v < S; ++v)
        if (!state[v].done) active.push_back(v);
      if (active.empty()) break;
      TMI_HIP(hipMemcpyAsync(d_active, active.data(), active.size() * sizeof(int), hipMemcpyHostToDevice, stream));
      B.num_active = (int)active.size();
      B.chunk_start = ch * chunk;
      const long long items = (long long)B.num_active * chunk;
      StreamTimer phase(stream, 4);
      TMI_HIP(phase.status);
      TMI_HIP(phase.mark());
      hipLaunchKernelGGL(ransac_hypothesis_kernel<P>, dim3((unsigned)((items + P::kThreads - 1) / P::kThreads)),
                         dim3(P::kThreads), 0, stream, B);
      TMI_HIP(phase.mark());
      hipLaunchKernelGGL(ransac_score_mle_kernel<P>, dim3((unsigned)((items * (P::kSlots / P::kScoreSlots) + 3) / 4)),
                         dim3(256), 0, stream, B, E);
      TMI_HIP(phase.mark());
      hipLaunchKernelGGL(ransac_replay_mle_kernel<P>, dim3((unsigned)((B.num_active + 63) / 64)), dim3(64), 0, stream,
                         B, E);
      TMI_HIP(phase.mark());
      TMI_HIP(hipGetLastError());
      TMI_HIP(s->download(state.data(), B.state, state.size()));
      TMI_HIP(hipStreamSynchronize(stream));  // (also: `active` is free to change)
      phases->hypothesis_seconds += phase.seconds(0, 1);
      phases->score_seconds += phase.seconds(1, 2);
      phases->replay_seconds += phase.seconds(2, 3);
      ++chunks_run;
    }
    return TMI_BA_OK;
  }
};
}  // namespace

extern "C" {
void tmi_ba_homography_ransac_options_init(tmi_ba_homography_ransac_options* o) {
  if (!o) return;
  o->failure_probability = 0.01;  // sample_consensus_estimator.h:57-65
  o->min_inlier_ratio = 0.0;
  o->min_iterations = 10;         // estimate_twoview_info.h:70
  o->max_iterations = 1000;       // estimate_twoview_info.h:71
  o->chunk_iterations = 0;
  o->device = -1;
  o->seed = 0;
  o->use_mle = 0;
  o->reserved = 0;
}

// The argument checks, the presets and the packing are those of two_view_ransac_call with a sample of four, written out
// again: that function's outputs and instantiations stay as they are.
int32_t tmi_ba_estimate_homographies(
    const tmi_ba_homography_ransac_options* L, int32_t num_pairs, const int64_t* pair_offset, const double* feature1,
    const double* feature2, const double* pair_error_threshold, const uint8_t* pair_mask, const uint32_t* pair_stream,
    const int32_t* samples, int32_t samples_given, int8_t* pair_status, int32_t* pair_num_correspondences,
    int32_t* pair_num_inliers, int32_t* pair_num_iterations, int32_t* pair_best_iteration, double* pair_confidence,
    double* homography, uint8_t* corr_inlier, int32_t* hypothesis_cost, double* hypothesis_cost_real,
    tmi_ba_two_view_ransac_summary* sum) {
  using P = HomographyProblem;
  constexpr int kSample = P::kSample;
  auto bad = [&](const char* why) { return bad_argument((std::string("homographies: ") + why).c_str()); };
  if (!L || !sum) return bad("null options or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is looked for
  const int Npair = num_pairs;
  if (Npair < 0) return bad("negative size");
  if (!pair_offset) return bad("missing array");
  if (pair_offset[0] != 0) return bad("pair_offset must start at 0");
  for (int p = 0; p < Npair; ++p)
    if (pair_offset[p + 1] < pair_offset[p]) return bad("pair_offset decreases");
  const int64_t total = pair_offset[Npair];
  if (total >= (int64_t)0x7fffffffLL) return bad("more than 2^31 correspondences");
  if (total && (!feature1 || !feature2)) return bad("missing array");
  if (const char* why = ransac_options_error(L, samples, samples_given)) return bad(why);
  const bool mle = L->use_mle != 0;
  if (hypothesis_cost_real && !mle) return bad("hypothesis_cost_real without use_mle");
  const int K = L->max_iterations;
  std::vector<int> selected, sel_pair, sel_rank;  // sel_pair: the attempted ones, the device's slots
  for (int p = 0; p < Npair; ++p) {
    if (pair_mask && !pair_mask[p]) continue;
    const int64_t n = pair_offset[p + 1] - pair_offset[p];
    if (n >= kSample) {
      if (!pair_error_threshold) return bad("missing pair_error_threshold");
      if (!(pair_error_threshold[p] > 0.0)) return bad("error threshold must be positive");
      if (samples_given)
        for (int64_t i = 0; i < K; ++i) {
          const int32_t* t = samples + kSample * ((int64_t)K * p + i);
          for (int a = 0; a < kSample; ++a) {
            bool wrong = t[a] < 0 || t[a] >= n;
            for (int b = 0; b < a; ++b) wrong = wrong || t[a] == t[b];
            if (wrong) return bad("a sample with a repeated or out-of-range index");
          }
        }
      sel_pair.push_back(p);
      sel_rank.push_back((int)selected.size());
    }
    selected.push_back(p);
  }
  const int num_selected = (int)selected.size(), S = (int)sel_pair.size();
  // nothing below fails on an argument: preset the outputs
  for (int p = 0; p < Npair; ++p) {
    const bool sel = !pair_mask || pair_mask[p];
    if (pair_status) pair_status[p] = (int8_t)(sel ? 1 : -1);
    if (pair_num_correspondences) pair_num_correspondences[p] = sel ? (int32_t)(pair_offset[p + 1] - pair_offset[p]) : 0;
    if (pair_num_inliers) pair_num_inliers[p] = 0;
    if (pair_num_iterations) pair_num_iterations[p] = 0;
    if (pair_best_iteration) pair_best_iteration[p] = -1;
    if (pair_confidence) pair_confidence[p] = 0.0;
    if (homography) std::fill(homography + 9 * (size_t)p, homography + 9 * (size_t)p + 9, 0.0);
  }
  if (corr_inlier && total) memset(corr_inlier, 0, (size_t)total);
  const size_t hyp_all = (size_t)num_selected * (size_t)K;
  if (hypothesis_cost) std::fill(hypothesis_cost, hypothesis_cost + hyp_all, -1);
  if (hypothesis_cost_real)
    std::fill(hypothesis_cost_real, hypothesis_cost_real + hyp_all, std::numeric_limits<double>::quiet_NaN());
  sum->num_pairs = num_selected;
  sum->num_too_few_correspondences = num_selected - S;
  // the attempted pairs' correspondences, pair-major, structure of arrays
  RansacMleRun run;
  std::vector<long long>& sel_ptr = run.sel_ptr;
  sel_ptr.assign((size_t)S + 1, 0);
  for (int s = 0; s < S; ++s) sel_ptr[(size_t)s + 1] = sel_ptr[s] + (pair_offset[sel_pair[s] + 1] - pair_offset[sel_pair[s]]);
  const size_t M = (size_t)sel_ptr[S];
  std::vector<double> xs(4 * std::max<size_t>(M, 1));
  double *hx1 = xs.data(), *hy1 = hx1 + M, *hx2 = hy1 + M, *hy2 = hx2 + M;
  std::vector<double> thresh((size_t)S);
  std::vector<unsigned> stream_id((size_t)S);
  for (int s = 0; s < S; ++s) {
    const int p = sel_pair[s];
    const int64_t o0 = pair_offset[p];
    const int n = (int)(pair_offset[p + 1] - o0);
    for (int m = 0; m < n; ++m) {
      const size_t o = (size_t)sel_ptr[s] + m;
      hx1[o] = feature1[2 * (o0 + m)];
      hy1[o] = feature1[2 * (o0 + m) + 1];
      hx2[o] = feature2[2 * (o0 + m)];
      hy2[o] = feature2[2 * (o0 + m) + 1];
    }
    thresh[s] = pair_error_threshold[p];
    stream_id[s] = pair_stream ? pair_stream[p] : (unsigned)p;
  }
  run.plan(L, kSample);
  return one_shot_batch(L->device, "homographies: no such device", S, t0, &sum->seconds, [&](OneShot* s) -> int {
    const hipStream_t stream = s->stream;
    double *d_xs, *d_model_out;
    TMI_HIP(s->upload(&d_xs, (const double*)xs.data(), xs.size()));
    if (const int rc = run.upload<P>(s, L->seed, sel_pair, stream_id, thresh, samples_given ? samples : nullptr,
                                     (size_t)Npair, hypothesis_cost != nullptr))
      return rc;
    if (mle)
      if (const int rc = run.upload_mle<P>(s, hypothesis_cost_real != nullptr)) return rc;
    RansacBatch& B = run.B;
    for (int q = 0; q < P::kPlanes; ++q) B.plane[q] = d_xs + q * M;  // x1, y1, x2, y2
    TMI_HIP(s->alloc(&d_model_out, (size_t)9 * S));
    StreamTimer timer(stream);
    TMI_HIP(timer.status);
    TMI_HIP(timer.mark());
    if (const int rc = mle ? run.chunks_mle<P>(s, sum) : run.chunks<P>(s, sum)) return rc;
    hipLaunchKernelGGL(homography_final_kernel, dim3(S), dim3(64), 0, stream, B, run.d_slot_inlier, run.d_num_inliers,
                       run.d_status, d_model_out);
    TMI_HIP(timer.mark());
    TMI_HIP(hipGetLastError());
    std::vector<double> model_h((size_t)9 * S), real_h(hypothesis_cost_real ? (size_t)S * K : 0);
    TMI_HIP(s->download(model_h.data(), d_model_out, model_h.size()));
    TMI_HIP(s->download(real_h.data(), run.E.hypothesis_cost, real_h.size()));
    if (const int rc = run.read_back(s, corr_inlier != nullptr, 1, sel_rank, hypothesis_cost)) return rc;
    sum->kernel_seconds = timer.seconds();
    sum->num_chunks = run.chunks_run;
    const RansacItemArrays out = {pair_status,         pair_num_inliers, pair_num_iterations,
                                  pair_best_iteration, nullptr,          pair_confidence};
    for (int v = 0; v < S; ++v) {
      const int p = sel_pair[v];
      const int n = (int)(sel_ptr[(size_t)v + 1] - sel_ptr[v]);
      const int code = run.status[v];
      const RansacState& st = run.state[v];
      if (code == 0) sum->num_estimated++; else sum->num_no_model++;
      sum->total_iterations += st.num_iterations;
      sum->total_scores += (int64_t)st.num_iterations * n;
      run.item_results(v, p, code, out);
      if (homography) std::copy(model_h.begin() + 9 * (size_t)v, model_h.begin() + 9 * (size_t)v + 9, homography + 9 * (size_t)p);
      if (corr_inlier)
        std::copy(run.slot_inlier.begin() + (size_t)sel_ptr[v], run.slot_inlier.begin() + (size_t)sel_ptr[(size_t)v + 1],
                  corr_inlier + pair_offset[p]);
      if (hypothesis_cost_real)
        std::copy(real_h.begin() + (size_t)v * K, real_h.begin() + ((size_t)v + 1) * K,
                  hypothesis_cost_real + (size_t)sel_rank[v] * K);
    }
    return TMI_BA_OK;
  });
}
}  // extern "C"

// ---- the two known-orientation position RANSACs: a sample of two, either scoring (known_orientation_kernels.h) ----
namespace {
// What one of the two calls hands to the shared body below.  feature[k] [2n] are rotated on the device by
// orientation[k] [3 per item] into planes (2k, 2k + 1); extra [extra_width n] (the world points) fills the planes after
// them unrotated.  rotated[k] (optional): the caller's [2n] for the features the RANSAC saw.
struct KnownOrientationInput {
  int num_features;              // 1 (absolute) or 2 (relative)
  const double* feature[2];
  const double* orientation[2];
  double* rotated[2];
  const double* extra;
  int extra_width;               // 3 or 0
};

// The argument checks, the presets and the packing are those of tmi_ba_estimate_homographies with a sample of two; the
// rotation launches come before the chunk loop and are part of kernel_seconds.
template <class P, class Final>
int32_t known_orientation_call(const char* what, const tmi_ba_homography_ransac_options* L, int32_t num_items,
                               const int64_t* item_offset, const KnownOrientationInput& in,
                               const double* item_error_threshold, const uint8_t* item_mask,
                               const uint32_t* item_stream, const int32_t* samples, int32_t samples_given,
                               int8_t* item_status, int32_t* item_num_correspondences, int32_t* item_num_inliers,
                               int32_t* item_num_iterations, int32_t* item_best_iteration, double* item_confidence,
                               double* model, uint8_t* corr_inlier, int32_t* hypothesis_cost,
                               double* hypothesis_cost_real, tmi_ba_two_view_ransac_summary* sum, Final final_kernel) {
  constexpr int kSample = P::kSample;
  auto bad = [&](const char* why) { return bad_argument((std::string(what) + ": " + why).c_str()); };
  if (!L || !sum) return bad("null options or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is looked for
  const int N = num_items;
  if (N < 0) return bad("negative size");
  if (!item_offset) return bad("missing array");
  if (item_offset[0] != 0) return bad("item_offset must start at 0");
  for (int p = 0; p < N; ++p)
    if (item_offset[p + 1] < item_offset[p]) return bad("item_offset decreases");
  const int64_t total = item_offset[N];
  if (total >= (int64_t)0x7fffffffLL) return bad("more than 2^31 correspondences");
  for (int k = 0; k < in.num_features; ++k)
    if ((total && !in.feature[k]) || (N && !in.orientation[k])) return bad("missing array");
  if (total && in.extra_width && !in.extra) return bad("missing array");
  if (const char* why = ransac_options_error(L, samples, samples_given)) return bad(why);
  const bool mle = L->use_mle != 0;
  if (hypothesis_cost_real && !mle) return bad("hypothesis_cost_real without use_mle");
  const int K = L->max_iterations;
  std::vector<int> selected, sel_item, sel_rank;  // sel_item: the attempted ones, the device's slots
  for (int p = 0; p < N; ++p) {
    if (item_mask && !item_mask[p]) continue;
    const int64_t n = item_offset[p + 1] - item_offset[p];
    if (n >= kSample) {
      if (!item_error_threshold) return bad("missing error threshold");
      if (!(item_error_threshold[p] > 0.0)) return bad("error threshold must be positive");
      if (samples_given)
        for (int64_t i = 0; i < K; ++i) {
          const int32_t* t = samples + kSample * ((int64_t)K * p + i);
          for (int a = 0; a < kSample; ++a) {
            bool wrong = t[a] < 0 || t[a] >= n;
            for (int b = 0; b < a; ++b) wrong = wrong || t[a] == t[b];
            if (wrong) return bad("a sample with a repeated or out-of-range index");
          }
        }
      sel_item.push_back(p);
      sel_rank.push_back((int)selected.size());
    }
    selected.push_back(p);
  }
  const int num_selected = (int)selected.size(), S = (int)sel_item.size();
  // nothing below fails on an argument: preset the outputs
  for (int p = 0; p < N; ++p) {
    const bool sel = !item_mask || item_mask[p];
    if (item_status) item_status[p] = (int8_t)(sel ? 1 : -1);
    if (item_num_correspondences) item_num_correspondences[p] = sel ? (int32_t)(item_offset[p + 1] - item_offset[p]) : 0;
    if (item_num_inliers) item_num_inliers[p] = 0;
    if (item_num_iterations) item_num_iterations[p] = 0;
    if (item_best_iteration) item_best_iteration[p] = -1;
    if (item_confidence) item_confidence[p] = 0.0;
    if (model) std::fill(model + 3 * (size_t)p, model + 3 * (size_t)p + 3, 0.0);
  }
  if (corr_inlier && total) memset(corr_inlier, 0, (size_t)total);
  for (int k = 0; k < in.num_features; ++k)
    if (in.rotated[k] && total) std::fill(in.rotated[k], in.rotated[k] + 2 * (size_t)total, 0.0);
  const size_t hyp_all = (size_t)num_selected * (size_t)K;
  if (hypothesis_cost) std::fill(hypothesis_cost, hypothesis_cost + hyp_all, -1);
  if (hypothesis_cost_real)
    std::fill(hypothesis_cost_real, hypothesis_cost_real + hyp_all, std::numeric_limits<double>::quiet_NaN());
  sum->num_pairs = num_selected;
  sum->num_too_few_correspondences = num_selected - S;
  // the attempted items' correspondences, item-major, structure of arrays
  RansacMleRun run;
  std::vector<long long>& sel_ptr = run.sel_ptr;
  sel_ptr.assign((size_t)S + 1, 0);
  for (int s = 0; s < S; ++s) sel_ptr[(size_t)s + 1] = sel_ptr[s] + (item_offset[sel_item[s] + 1] - item_offset[sel_item[s]]);
  const size_t M = (size_t)sel_ptr[S];
  std::vector<double> xs((size_t)P::kPlanes * std::max<size_t>(M, 1));
  std::vector<double> thresh((size_t)S), orient((size_t)in.num_features * 3 * std::max(S, 1));
  std::vector<unsigned> stream_id((size_t)S);
  for (int s = 0; s < S; ++s) {
    const int p = sel_item[s];
    const int64_t o0 = item_offset[p];
    const int n = (int)(item_offset[p + 1] - o0);
    for (int m = 0; m < n; ++m) {
      const size_t o = (size_t)sel_ptr[s] + m;
      for (int k = 0; k < in.num_features; ++k) {
        xs[(size_t)(2 * k) * M + o] = in.feature[k][2 * (o0 + m)];
        xs[(size_t)(2 * k + 1) * M + o] = in.feature[k][2 * (o0 + m) + 1];
      }
      for (int q = 0; q < in.extra_width; ++q)
        xs[(size_t)(2 * in.num_features + q) * M + o] = in.extra[(size_t)in.extra_width * (o0 + m) + q];
    }
    for (int k = 0; k < in.num_features; ++k)
      for (int q = 0; q < 3; ++q) orient[(size_t)3 * ((size_t)k * S + s) + q] = in.orientation[k][3 * (size_t)p + q];
    thresh[s] = item_error_threshold[p];
    stream_id[s] = item_stream ? item_stream[p] : (unsigned)p;
  }
  run.plan(L, kSample);
  const std::string no_device = std::string(what) + ": no such device";
  return one_shot_batch(L->device, no_device.c_str(), S, t0, &sum->seconds, [&](OneShot* s) -> int {
    const hipStream_t stream = s->stream;
    double *d_xs, *d_orient, *d_model_out;
    TMI_HIP(s->upload(&d_xs, (const double*)xs.data(), xs.size()));
    TMI_HIP(s->upload(&d_orient, (const double*)orient.data(), orient.size()));
    if (const int rc = run.upload<P>(s, L->seed, sel_item, stream_id, thresh, samples_given ? samples : nullptr,
                                     (size_t)N, hypothesis_cost != nullptr))
      return rc;
    if (mle)
      if (const int rc = run.upload_mle<P>(s, hypothesis_cost_real != nullptr)) return rc;
    RansacBatch& B = run.B;
    for (int q = 0; q < P::kPlanes; ++q) B.plane[q] = d_xs + q * M;
    TMI_HIP(s->alloc(&d_model_out, (size_t)3 * S));
    StreamTimer timer(stream);
    TMI_HIP(timer.status);
    TMI_HIP(timer.mark());
    for (int k = 0; k < in.num_features && M > 0; ++k)
      hipLaunchKernelGGL(rotate_features_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, S, B.sel_ptr,
                         d_orient + (size_t)3 * k * S, B.plane[2 * k], B.plane[2 * k + 1]);
    if (const int rc = mle ? run.chunks_mle<P>(s, sum) : run.chunks<P>(s, sum)) return rc;
    hipLaunchKernelGGL(final_kernel, dim3(S), dim3(64), 0, stream, B, run.d_slot_inlier, run.d_num_inliers, run.d_status,
                       d_model_out);
    TMI_HIP(timer.mark());
    TMI_HIP(hipGetLastError());
    const bool want_rotated = in.rotated[0] || (in.num_features > 1 && in.rotated[1]);
    std::vector<double> model_h((size_t)3 * S), real_h(hypothesis_cost_real ? (size_t)S * K : 0),
        rot_h(want_rotated ? (size_t)2 * in.num_features * M : 0);
    TMI_HIP(s->download(model_h.data(), d_model_out, model_h.size()));
    TMI_HIP(s->download(real_h.data(), run.E.hypothesis_cost, real_h.size()));
    TMI_HIP(s->download(rot_h.data(), d_xs, rot_h.size()));
    if (const int rc = run.read_back(s, corr_inlier != nullptr, 1, sel_rank, hypothesis_cost)) return rc;
    sum->kernel_seconds = timer.seconds();
    sum->num_chunks = run.chunks_run;
    const RansacItemArrays out = {item_status,         item_num_inliers, item_num_iterations,
                                  item_best_iteration, nullptr,          item_confidence};
    for (int v = 0; v < S; ++v) {
      const int p = sel_item[v];
      const int n = (int)(sel_ptr[(size_t)v + 1] - sel_ptr[v]);
      const int code = run.status[v];
      const RansacState& st = run.state[v];
      if (code == 0) sum->num_estimated++; else sum->num_no_model++;
      sum->total_iterations += st.num_iterations;
      sum->total_scores += (int64_t)st.num_iterations * n;
      run.item_results(v, p, code, out);
      if (model) std::copy(model_h.begin() + 3 * (size_t)v, model_h.begin() + 3 * (size_t)v + 3, model + 3 * (size_t)p);
      if (corr_inlier)
        std::copy(run.slot_inlier.begin() + (size_t)sel_ptr[v], run.slot_inlier.begin() + (size_t)sel_ptr[(size_t)v + 1],
                  corr_inlier + item_offset[p]);
      if (hypothesis_cost_real)
        std::copy(real_h.begin() + (size_t)v * K, real_h.begin() + ((size_t)v + 1) * K,
                  hypothesis_cost_real + (size_t)sel_rank[v] * K);
      for (int k = 0; k < in.num_features; ++k)
        if (in.rotated[k])
          for (int m = 0; m < n; ++m) {
            const size_t o = (size_t)sel_ptr[v] + m;
            in.rotated[k][2 * (item_offset[p] + m)] = rot_h[(size_t)(2 * k) * M + o];
            in.rotated[k][2 * (item_offset[p] + m) + 1] = rot_h[(size_t)(2 * k + 1) * M + o];
          }
    }
    return TMI_BA_OK;
  });
}
}  // namespace

extern "C" {
int32_t tmi_ba_estimate_positions_known_orientation(
    const tmi_ba_homography_ransac_options* L, int32_t num_items, const int64_t* item_offset, const double* feature,
    const double* world_point, const double* item_orientation, const double* item_error_threshold,
    const uint8_t* item_mask, const uint32_t* item_stream, const int32_t* samples, int32_t samples_given,
    int8_t* item_status, int32_t* item_num_correspondences, int32_t* item_num_inliers, int32_t* item_num_iterations,
    int32_t* item_best_iteration, double* item_confidence, double* position, uint8_t* corr_inlier,
    int32_t* hypothesis_cost, double* hypothesis_cost_real, double* rotated_feature,
    tmi_ba_two_view_ransac_summary* sum) {
  const KnownOrientationInput in = {1, {feature, nullptr}, {item_orientation, nullptr}, {rotated_feature, nullptr},
                                    world_point, 3};
  return known_orientation_call<KnownOrientationAbsoluteProblem>(
      "positions with known orientation", L, num_items, item_offset, in, item_error_threshold, item_mask, item_stream,
      samples, samples_given, item_status, item_num_correspondences, item_num_inliers, item_num_iterations,
      item_best_iteration, item_confidence, position, corr_inlier, hypothesis_cost, hypothesis_cost_real, sum,
      known_orientation_absolute_final_kernel);
}

int32_t tmi_ba_estimate_relative_positions_known_orientation(
    const tmi_ba_homography_ransac_options* L, int32_t num_pairs, const int64_t* pair_offset, const double* feature1,
    const double* feature2, const double* pair_orientation1, const double* pair_orientation2,
    const double* pair_error_threshold, const uint8_t* pair_mask, const uint32_t* pair_stream, const int32_t* samples,
    int32_t samples_given, int8_t* pair_status, int32_t* pair_num_correspondences, int32_t* pair_num_inliers,
    int32_t* pair_num_iterations, int32_t* pair_best_iteration, double* pair_confidence, double* position,
    uint8_t* corr_inlier, int32_t* hypothesis_cost, double* hypothesis_cost_real, double* rotated_feature1,
    double* rotated_feature2, tmi_ba_two_view_ransac_summary* sum) {
  const KnownOrientationInput in = {2, {feature1, feature2}, {pair_orientation1, pair_orientation2},
                                    {rotated_feature1, rotated_feature2}, nullptr, 0};
  return known_orientation_call<KnownOrientationRelativeProblem>(
      "relative positions with known orientation", L, num_pairs, pair_offset, in, pair_error_threshold, pair_mask,
      pair_stream, samples, samples_given, pair_status, pair_num_correspondences, pair_num_inliers, pair_num_iterations,
      pair_best_iteration, pair_confidence, position, corr_inlier, hypothesis_cost, hypothesis_cost_real, sum,
      known_orientation_relative_final_kernel);
}
}  // extern "C"

// ---- batched GuidedEpipolarMatcher (guided_match_kernels.h) ------------------------------------
#define TMI_GM(call)                  \
  do {                                \
    const int rc_ = (call);           \
    if (rc_ != TMI_BA_OK) return rc_; \
  } while (0)
extern "C" {
void tmi_ba_guided_match_options_init(tmi_ba_guided_match_options* o) {
  if (!o) return;
  o->guided_matching_max_distance_pixels = 2.0;  // guided_epipolar_matcher.h:64-75
  o->lowes_ratio = 0.8;
  o->min_num_candidates = 50;  // kMinNumMatchesFound, guided_epipolar_matcher.cc:279
  o->device = -1;
  o->seed = 0;
  o->reserved[0] = o->reserved[1] = 0;
}

int32_t tmi_ba_guided_epipolar_match(const tmi_ba_guided_match_options* O, int32_t num_images,
                                     const int64_t* image_begin, const float* descriptors, int32_t dim,
                                     const double* keypoints, int32_t num_pairs, const int32_t* pair_image1,
                                     const int32_t* pair_image2, const double* fundamental_matrix,
                                     const int64_t* pair_match_begin, const int32_t* match_feature1,
                                     const int32_t* match_feature2, const uint8_t* pair_mask,
                                     const uint32_t* pair_stream, int64_t added_capacity, int8_t* pair_status,
                                     int32_t* pair_num_groups, int64_t* pair_added_begin, int32_t* added_feature1,
                                     int32_t* added_feature2, float* added_distance, int32_t* feature_group,
                                     double* group_endpoints, int32_t* group_num_candidates,
                                     tmi_ba_guided_match_summary* sum) {
  auto bad = [&](const char* why) { return bad_argument((std::string("guided epipolar match: ") + why).c_str()); };
  if (!O || !sum) return bad("null options or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is looked for
  if (num_images < 0 || num_pairs < 0 || added_capacity < 0) return bad("negative count");
  if (dim < 1) return bad("dim < 1");
  if (!image_begin) return bad("missing image_begin");
  const double c = O->guided_matching_max_distance_pixels;
  if (!(c > 0.0) || !std::isfinite(c)) return bad("guided_matching_max_distance_pixels is not in (0, inf)");
  if (c < 0.0625) {  // a supported-range limit, not an argument error: it bounds a walk at 2^21 steps
    g_last_error = "guided epipolar match: guided_matching_max_distance_pixels below 1/16 is not supported";
    return TMI_BA_ERR_UNSUPPORTED;
  }
  if (!std::isfinite(O->lowes_ratio)) return bad("lowes_ratio is not finite");
  if (O->min_num_candidates < 0 || O->min_num_candidates > kGmMaxCandidatesFill)
    return bad("min_num_candidates is not in [0, 64]");
  if (image_begin[0] != 0) return bad("image_begin must start at 0");
  for (int m = 0; m < num_images; ++m) {
    if (image_begin[m + 1] < image_begin[m]) return bad("image_begin decreases");
    if (image_begin[m + 1] - image_begin[m] > kGmMaxImageRows) return bad("an image of more than 131072 rows");
  }
  const int64_t total_rows = image_begin[num_images];
  if (total_rows && (!descriptors || !keypoints)) return bad("missing descriptors or keypoints");
  if (num_pairs && (!pair_image1 || !pair_image2 || !fundamental_matrix || !pair_status || !pair_num_groups))
    return bad("missing pair array");
  if (!pair_match_begin || !pair_added_begin) return bad("missing pair_match_begin or pair_added_begin");
  if (pair_match_begin[0] != 0) return bad("pair_match_begin must start at 0");
  for (int p = 0; p < num_pairs; ++p)
    if (pair_match_begin[p + 1] < pair_match_begin[p]) return bad("pair_match_begin decreases");
  const int64_t num_matches = pair_match_begin[num_pairs];
  if (num_matches && (!match_feature1 || !match_feature2)) return bad("missing match array");
  if (added_capacity && (!added_feature1 || !added_feature2 || !added_distance)) return bad("missing added array");
  for (int p = 0; p < num_pairs; ++p) {
    const int i1 = pair_image1[p], i2 = pair_image2[p];
    if (i1 < 0 || i1 >= num_images || i2 < 0 || i2 >= num_images) return bad("image index out of range");
    const int64_t n1 = image_begin[i1 + 1] - image_begin[i1], n2 = image_begin[i2 + 1] - image_begin[i2];
    for (int64_t m = pair_match_begin[p]; m < pair_match_begin[p + 1]; ++m)
      if (match_feature1[m] < 0 || match_feature1[m] >= n1 || match_feature2[m] < 0 || match_feature2[m] >= n2)
        return bad("match index out of range");
  }
  // the selected pairs, their ROW1 / ROW2 and the rows of the test outputs; every named image gets its device rows
  std::vector<GmPair> pairs;
  std::vector<int> sel_pair;
  std::vector<int64_t> out_row((size_t)num_pairs + 1, 0);
  std::vector<long long> device_row((size_t)num_images, -1);
  std::vector<int> match_row1, match_row2;
  long long rows1 = 0, rows2 = 0, uploaded = 0;
  int max_n2 = 0;
  for (int p = 0; p < num_pairs; ++p) {
    const int i1 = pair_image1[p], i2 = pair_image2[p];
    const int n1 = (int)(image_begin[i1 + 1] - image_begin[i1]), n2 = (int)(image_begin[i2 + 1] - image_begin[i2]);
    out_row[(size_t)p + 1] = out_row[p] + n1;
    pair_status[p] = -1;
    pair_num_groups[p] = 0;
    pair_added_begin[p] = 0;
    if (pair_mask && !pair_mask[p]) continue;
    for (int im : {i1, i2})
      if (device_row[im] < 0) {
        device_row[im] = uploaded;
        uploaded += image_begin[im + 1] - image_begin[im];
      }
    GmPair P;
    memset(&P, 0, sizeof(P));
    P.row1 = device_row[i1];
    P.row2 = device_row[i2];
    P.n1 = n1;
    P.n2 = n2;
    P.base1 = (int)rows1;
    P.base2 = (int)rows2;
    P.stream = pair_stream ? pair_stream[p] : (unsigned)p;
    std::copy(fundamental_matrix + 9 * (size_t)p, fundamental_matrix + 9 * (size_t)p + 9, P.F);
    rows1 += n1;
    rows2 += n2;
    if (rows1 >= 0x7fffffffLL || 4 * rows2 >= 0x7fffffffLL || num_matches >= 0x7fffffffLL) {
      g_last_error = "guided epipolar match: the rows of the selected pairs exceed 2^31";
      return TMI_BA_ERR_UNSUPPORTED;
    }
    for (int64_t m = pair_match_begin[p]; m < pair_match_begin[p + 1]; ++m) {
      match_row1.push_back(P.base1 + match_feature1[m]);
      match_row2.push_back(P.base2 + match_feature2[m]);
    }
    max_n2 = std::max(max_n2, n2);
    pairs.push_back(P);
    sel_pair.push_back(p);
  }
  pair_added_begin[num_pairs] = 0;
  const int64_t out_rows = out_row[num_pairs];
  if (feature_group) std::fill(feature_group, feature_group + out_rows, -1);
  if (group_endpoints) std::fill(group_endpoints, group_endpoints + 4 * out_rows, 0.0);
  if (group_num_candidates) std::fill(group_num_candidates, group_num_candidates + out_rows, 0);
  const int S = (int)pairs.size();
  sum->num_pairs = S;
  const double ratio_sq = O->lowes_ratio * O->lowes_ratio;  // formed in double (guided_epipolar_matcher.cc:150)
  const int rc = one_shot_batch(O->device, "guided epipolar match: no such device", S, t0, &sum->seconds, [&](OneShot* s) -> int {
    const hipStream_t stream = s->stream;
    auto grid = [](long long n) { return dim3((unsigned)((n + 255) / 256)); };
    const size_t R1 = (size_t)rows1, R2 = (size_t)rows2, E = 4 * R2, M = match_row1.size();
    // every named image once
    float* d_desc;
    double* d_keys;
    TMI_HIP(s->alloc(&d_desc, (size_t)uploaded * (size_t)dim));
    TMI_HIP(s->alloc(&d_keys, 2 * (size_t)uploaded));
    for (int m = 0; m < num_images; ++m) {
      const size_t n = (size_t)(image_begin[m + 1] - image_begin[m]);
      if (device_row[m] < 0 || n == 0) continue;
      TMI_HIP(hipMemcpyAsync(d_desc + (size_t)device_row[m] * dim, descriptors + (size_t)image_begin[m] * dim,
                             n * (size_t)dim * sizeof(float), hipMemcpyHostToDevice, stream));
      TMI_HIP(hipMemcpyAsync(d_keys + 2 * (size_t)device_row[m], keypoints + 2 * (size_t)image_begin[m],
                             2 * n * sizeof(double), hipMemcpyHostToDevice, stream));
    }
    sum->rows_uploaded = uploaded;
    GmPair* d_pairs;
    GmPairState* d_state;
    int *d_match_row1, *d_match_row2, *d_slot_first, *d_slot_size, *d_row_group, *d_num_groups, *d_slot_num_candidates;
    int* d_counts;
    unsigned char *d_matched1, *d_matched2;
    unsigned *d_u2, *d_ubegin, *d_num_lines, *d_vbegin, *d_pair_key, *d_pair_key_gathered, *d_pair_key_sorted;
    unsigned *d_iota1, *d_row_by_code, *d_pos_row, *d_segment_key, *d_segment_key_gathered, *d_segment_key_sorted;
    unsigned *d_iota2, *d_entry_by_cell, *d_entry_sorted, *d_pass, *d_scan;
    unsigned long long *d_code, *d_code_sorted, *d_cell_key, *d_cell_key_sorted, *d_counters;
    double* d_slot_endpoints;
    GmNn nn;
    GmRecord* d_out;
    TMI_HIP(s->upload(&d_pairs, pairs.data(), (size_t)S));
    TMI_HIP(s->upload(&d_match_row1, match_row1.data(), M));
    TMI_HIP(s->upload(&d_match_row2, match_row2.data(), M));
    TMI_HIP(s->alloc(&d_state, (size_t)S));
    TMI_HIP(s->alloc_filled(&d_matched1, R1, 0));
    TMI_HIP(s->alloc_filled(&d_matched2, R2, 0));
    TMI_HIP(s->alloc_filled(&d_u2, (size_t)S + 1, 0));
    TMI_HIP(s->alloc(&d_ubegin, (size_t)S + 1));
    TMI_HIP(s->alloc_filled(&d_num_lines, (size_t)S + 1, 0));
    TMI_HIP(s->alloc(&d_vbegin, (size_t)S + 1));
    TMI_HIP(s->alloc(&d_code, R1));
    TMI_HIP(s->alloc(&d_code_sorted, R1));
    TMI_HIP(s->alloc(&d_pair_key, R1));
    TMI_HIP(s->alloc(&d_pair_key_gathered, R1));
    TMI_HIP(s->alloc(&d_pair_key_sorted, R1));
    TMI_HIP(s->alloc(&d_iota1, R1));
    TMI_HIP(s->alloc(&d_row_by_code, R1));
    TMI_HIP(s->alloc(&d_pos_row, R1));
    TMI_HIP(s->alloc(&d_cell_key, E));
    TMI_HIP(s->alloc(&d_cell_key_sorted, E));
    TMI_HIP(s->alloc(&d_segment_key, E));
    TMI_HIP(s->alloc(&d_segment_key_gathered, E));
    TMI_HIP(s->alloc(&d_segment_key_sorted, E));
    TMI_HIP(s->alloc(&d_iota2, E));
    TMI_HIP(s->alloc(&d_entry_by_cell, E));
    TMI_HIP(s->alloc(&d_entry_sorted, E));
    TMI_HIP(s->alloc_filled(&d_slot_first, R1, 0));
    TMI_HIP(s->alloc_filled(&d_slot_size, R1, 0));
    TMI_HIP(s->alloc_filled(&d_slot_endpoints, 4 * R1, 0));
    TMI_HIP(s->alloc_filled(&d_slot_num_candidates, R1, 0));
    TMI_HIP(s->alloc_filled(&d_row_group, R1, 0xff));
    TMI_HIP(s->alloc_filled(&d_num_groups, (size_t)S, 0));
    TMI_HIP(s->alloc(&nn.best_d, R1));
    TMI_HIP(s->alloc(&nn.best_i, R1));
    TMI_HIP(s->alloc(&nn.second_d, R1));
    TMI_HIP(s->alloc_filled(&d_pass, R1 + 1, 0));
    TMI_HIP(s->alloc(&d_scan, R1 + 1));
    TMI_HIP(s->alloc(&d_out, R1));
    TMI_HIP(s->alloc(&d_counts, 4 * (size_t)S + 1));
    TMI_HIP(s->alloc_filled(&d_counters, (size_t)4, 0));
    const int bitmap_words = ((max_n2 + 31) / 32 + 3) & ~3;
    const size_t lds = (size_t)bitmap_words * sizeof(unsigned) + (size_t)kGmListCap * sizeof(int);
    const int* vbegin = reinterpret_cast<const int*>(d_vbegin);
    const int* ubegin = reinterpret_cast<const int*>(d_ubegin);
    StreamTimer timer(stream);
    TMI_HIP(timer.status);
    TMI_HIP(timer.mark());
    // a, b
    if (M) hipLaunchKernelGGL(gm_mark_kernel, grid((long long)M), dim3(256), 0, stream, d_match_row1, d_match_row2, (long long)M, d_matched1, d_matched2);
    hipLaunchKernelGGL(gm_box_kernel, dim3((unsigned)S), dim3(256), 0, stream, d_pairs, d_keys, d_matched1, d_matched2, d_state, d_u2);
    TMI_GM(tb_exclusive_sum(s, d_u2, d_ubegin, (size_t)S + 1));
    if (R1) {
      hipLaunchKernelGGL(gm_lines_kernel, grid((long long)R1), dim3(256), 0, stream, d_pairs, S, (int)R1, d_keys, d_matched1, d_state, d_code,
                         d_pair_key, d_iota1, d_num_lines);
      // c: (pair, code, feature) by two stable sorts, the feature order being the initial one
      TMI_GM(tb_sort_pairs(s, d_code, d_code_sorted, d_iota1, d_row_by_code, R1, 64));
      hipLaunchKernelGGL(gm_gather_kernel, grid((long long)R1), dim3(256), 0, stream, d_pair_key, d_row_by_code, (int)R1, d_pair_key_gathered);
      TMI_GM(tb_sort_pairs(s, d_pair_key_gathered, d_pair_key_sorted, d_row_by_code, d_pos_row, R1, tb_bits((unsigned)S + 1)));
    }
    TMI_GM(tb_exclusive_sum(s, d_num_lines, d_vbegin, (size_t)S + 1));
    hipLaunchKernelGGL(gm_group_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, stream, d_pairs, S, vbegin, d_pos_row, d_code, c,
                       d_slot_first, d_slot_size, d_slot_endpoints, d_row_group, d_num_groups);
    // d
    if (E) {
      hipLaunchKernelGGL(gm_cells_kernel, grid((long long)E), dim3(256), 0, stream, d_pairs, S, (int)R2, d_keys, d_matched2, d_state, c,
                         d_cell_key, d_segment_key, d_iota2);
      TMI_GM(tb_sort_pairs(s, d_cell_key, d_cell_key_sorted, d_iota2, d_entry_by_cell, E, 64));
      hipLaunchKernelGGL(gm_gather_kernel, grid((long long)E), dim3(256), 0, stream, d_segment_key, d_entry_by_cell, (int)E, d_segment_key_gathered);
      TMI_GM(tb_sort_pairs(s, d_segment_key_gathered, d_segment_key_sorted, d_entry_by_cell, d_entry_sorted, E, tb_bits(4u * (unsigned)S + 1)));
    }
    // e, f: a workgroup per slot
    if (R1) {
      hipLaunchKernelGGL(gm_search_kernel, dim3((unsigned)R1), dim3(kGmThreads), lds, stream, d_pairs, S, vbegin, ubegin, d_u2, d_num_groups,
                         d_slot_first, d_slot_size, d_slot_endpoints, d_pos_row, d_entry_sorted, d_cell_key, d_desc, (int)dim, c, ratio_sq,
                         (int)O->min_num_candidates, (unsigned long long)O->seed, bitmap_words, nn, d_pass, d_slot_num_candidates,
                         d_counters);
    }
    TMI_GM(tb_exclusive_sum(s, d_pass, d_scan, R1 + 1));
    if (R1) hipLaunchKernelGGL(gm_compact_kernel, grid((long long)R1), dim3(256), 0, stream, d_pairs, S, vbegin, d_pos_row, nn, d_pass, d_scan, d_out);
    hipLaunchKernelGGL(gm_pair_kernel, dim3((unsigned)(S / 256 + 1)), dim3(256), 0, stream, d_state, vbegin, d_num_groups, d_scan, S, d_counts);
    TMI_HIP(timer.mark());
    // the read-back: counts and the test outputs, then exactly the added matches
    std::vector<int> counts(4 * (size_t)S + 1), vbegin_h((size_t)S + 1);
    const bool want_slots = group_endpoints || group_num_candidates;
    std::vector<int> row_group_h(feature_group ? R1 : 0), slot_nc_h(group_num_candidates ? R1 : 0);
    std::vector<double> slot_ep_h(group_endpoints ? 4 * R1 : 0);
    unsigned long long counters_h[4] = {0, 0, 0, 0};
    ReadBack rb(stream);
    rb.add(counts.data(), d_counts, counts.size());
    rb.add(vbegin_h.data(), vbegin, want_slots ? vbegin_h.size() : 0);
    rb.add(row_group_h.data(), d_row_group, row_group_h.size());
    rb.add(slot_nc_h.data(), d_slot_num_candidates, slot_nc_h.size());
    rb.add(slot_ep_h.data(), d_slot_endpoints, slot_ep_h.size());
    rb.add(counters_h, d_counters, (size_t)4);
    TMI_HIP(rb.finish());
    sum->kernel_seconds = timer.seconds();
    sum->num_groups = (int64_t)counters_h[0];
    sum->num_candidates = (int64_t)counters_h[1];
    sum->distance_evaluations = (int64_t)counters_h[2];
    const int total = counts[4 * (size_t)S];
    if (total < 0 || (size_t)total > R1) {
      s->error = "guided epipolar match: the device reported an impossible match count";
      return TMI_BA_ERR_DEVICE;
    }
    for (int i = 0; i < S; ++i) {
      const int p = sel_pair[i], ng = counts[4 * (size_t)i + 1];
      if (ng < 0 || ng > pairs[i].n1 || counts[4 * (size_t)i + 2] < 0 || counts[4 * (size_t)i + 2] > total) {
        s->error = "guided epipolar match: the device reported an impossible group count";
        return TMI_BA_ERR_DEVICE;
      }
      pair_status[p] = (int8_t)counts[4 * (size_t)i];
      pair_num_groups[p] = ng;
      if (counts[4 * (size_t)i] == 0) sum->num_pairs_ok++;
      if (feature_group) std::copy(row_group_h.begin() + pairs[i].base1, row_group_h.begin() + pairs[i].base1 + pairs[i].n1, feature_group + out_row[p]);
      if (want_slots && (vbegin_h[i] < 0 || (size_t)vbegin_h[i] + (size_t)ng > R1)) {
        s->error = "guided epipolar match: the device reported an impossible group table";
        return TMI_BA_ERR_DEVICE;
      }
      for (int g = 0; g < ng && want_slots; ++g) {
        const size_t slot = (size_t)vbegin_h[i] + (size_t)g;
        if (group_num_candidates) group_num_candidates[out_row[p] + g] = slot_nc_h[slot];
        if (group_endpoints) std::copy(slot_ep_h.begin() + 4 * slot, slot_ep_h.begin() + 4 * slot + 4, group_endpoints + 4 * (out_row[p] + g));
      }
    }
    // pair_added_begin over ALL pairs: a pair that is masked out begins where its successor does
    {
      int next = total;
      int i = S - 1;
      pair_added_begin[num_pairs] = total;
      for (int p = num_pairs - 1; p >= 0; --p) {
        if (i >= 0 && sel_pair[i] == p) {
          next = counts[4 * (size_t)i + 2];
          --i;
        }
        pair_added_begin[p] = next;
      }
    }
    sum->num_added = total;
    if (total && total <= added_capacity) {
      std::vector<GmRecord> rec((size_t)total);
      ReadBack rb2(stream);
      rb2.add(rec.data(), d_out, rec.size());
      TMI_HIP(rb2.finish());
      for (size_t i = 0; i < rec.size(); ++i) {
        added_feature1[i] = rec[i].feature1;
        added_feature2[i] = rec[i].feature2;
        added_distance[i] = rec[i].distance;
      }
    }
    return TMI_BA_OK;
  });
  sum->seconds = now_s() - t0;
  if (rc == TMI_BA_OK && sum->num_added > added_capacity) {
    g_last_error = "guided epipolar match: added_capacity is smaller than the number of added matches (summary->num_added)";
    return TMI_BA_ERR_CAPACITY;
  }
  return rc;
}
}  // extern "C"
#undef TMI_GM
