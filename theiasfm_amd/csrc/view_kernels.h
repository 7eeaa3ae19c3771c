// Batched single-view bundle adjustment: theia::BundleAdjustView (bundle_adjustment.cc:83-93, called per
// localised view from localize_view_to_reconstruction.cc:248-252) for many views in one launch.
//
// A view's problem is its own observations, every point constant, the view's free extrinsics plus the free
// entries of its intrinsics group: D <= 16 unknowns against hundreds to thousands of residuals.  One
// workgroup of 256 threads runs one CHAIN of such problems, one after another: the views of a shared
// intrinsics group with free entries (ascending camera index; each starts from the intrinsics the previous
// one left, kept in LDS along the chain), or a single view.  Per LM iteration:
//   linearise   thread per observation: residual and the 2 x 16 Jacobian [extrinsics | intrinsics] from the
//               prepared camera record (camera_models.h), loss corrector and Jacobi scale applied, the free
//               columns and the residual staged as rows [J | r] into an LDS tile of kViewTile observations;
//   Gram        thread t < (D+1)(D+2)/2 owns one entry of the upper triangle of [J|r]^T [J|r] and adds it
//               up over the tile's rows in row order: J^T J and J^T r in one pass, a fixed summation order;
//   solve       one lane factors J^T J + diag(clamp(diag J^T J) / radius) (D x D Cholesky in LDS);
//   trial pass  cost only at x + step, wave butterflies then the four wave sums in order.
// The trust-region loop (small_lm.h) runs on a problem whose point side is empty, replicated and uniform in every
// thread, reading the values lane 0 publishes through LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "camera_models.h"
#include "kernels.h"
#include "small_lm.h"

namespace tmi {

constexpr int kViewTile = 256;  // observations per LDS tile (one per thread)
constexpr int kViewCols = 17;   // <= 16 free columns + the residual

struct ViewBatch {
  double* ext;                        // [6 Nc] in/out
  double* intr;                       // intrinsics of the groups, in/out
  const int4* cam;                    // [Nc] (model, intrinsics offset, intrinsics size, free mask over [ext(6) | intr(10)])
  const unsigned long long* keys;     // view-major observations: (view << 32) | slot, ascending
  const long long* vptr;              // [Nc + 1] range of each view in keys
  const int* slot_pt;                 // slot -> point index
  const double* obs_xy;               // [2 slots]
  const double* pts;                  // [4 points] homogeneous, constant
  const int* chain_ptr;               // [n_chains + 1]
  const int* chain_views;             // views of the chains, in order
  SmallLmOut out;                     // [Nc] per-view outputs (written for the views of the chains)
};

struct ViewLds {
  double tile[2 * kViewTile * kViewCols];
  double prep[kPrepStride];
  double x[16], xc[16], sp[16], kchain[10];
  double A[16 * 16];  // J^T J (free columns, dense)
  double g[16];
  double y[16], z[16];
  double L[16 * 16];
  double part[256];   // the Gram's per-class partial sums
  double red[2][4];
  double scal[8];
  int col[16];        // compact column of parameter a, or -1
  int par[16];        // parameter of compact column d
};

// prepared record of the parameter set p (lane 0); with the scales sp the angle-axis columns come out scaled
__device__ __forceinline__ void vb_prepare(ViewLds& S, const double* p, int nk) {
  if (threadIdx.x == 0) prepare_camera_record(p, p + 6, nk, S.sp, S.prep);
  __syncthreads();
}

// sum over the workgroup in a fixed order: wave butterflies, then the four wave sums in wave order
__device__ __forceinline__ void vb_block_sum2(ViewLds& S, double a, double b, double* ra, double* rb) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    S.red[0][w] = a;
    S.red[1][w] = b;
  }
  __syncthreads();
  *ra = ((S.red[0][0] + S.red[0][1]) + S.red[0][2]) + S.red[0][3];
  *rb = ((S.red[1][0] + S.red[1][1]) + S.red[1][2]) + S.red[1][3];
  __syncthreads();
}

// One pass over the view's observations at the record S.prep.  JAC: J^T J -> S.A, J^T r -> S.g (scaled by
// S.sp, loss-corrected).  Returns the cost 1/2 sum rho(|r|^2); *bad = 1 if a residual cannot be evaluated.
template <bool JAC, int UMODEL>
__device__ double vb_pass(const ViewBatch& B, ViewLds& S, int model, int D, long long beg, long long end,
                          int loss_type, double loss_width, double* bad) {
  const int tid = threadIdx.x;
  const int D1 = D + 1;
  const int NS = D1 * (D1 + 1) / 2;
  // the threads not needed for one copy of the triangle split the rows: nsplit interleaved row classes, each summed by
  // its own copy of the NS owners (D <= 10: four copies, one per wave; D <= 14: two), finished in class order below
  const int nsplit = NS <= 64 ? 4 : (NS <= 128 ? 2 : 1);
  const int stride = 256 / nsplit;
  const int ent = tid % stride, part = tid / stride;
  int gi = 0, gj = 0;
  if (JAC && ent < NS) {  // (gi, gj) = entry `ent` of the row-wise packed upper triangle
    int t = ent;
    while (t >= D1 - gi) {
      t -= D1 - gi;
      ++gi;
    }
    gj = gi + t;
  }
  double acc = 0.0, acc2 = 0.0, c = 0.0, nbad = 0.0;
  for (long long t0 = beg; t0 < end; t0 += kViewTile) {
    const long long o = t0 + tid;
    const int nrow = (int)min((long long)kViewTile, end - t0);
    if (o < end) {
      const unsigned slot = (unsigned)(B.keys[o] & 0xffffffffull);
      const int p = B.slot_pt[slot];
      double X[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) X[i] = B.pts[(size_t)p * 4 + i];
      double r[2], Jext[2][6], Jint[2][10], Jpt[2][4];
      const bool ok = reprojection_error_prepared<JAC, double>(UMODEL >= 0 ? UMODEL : model, S.prep, X,
                                                               B.obs_xy[2 * (size_t)slot], B.obs_xy[2 * (size_t)slot + 1],
                                                               r, Jext, Jint, Jpt);
      double* row0 = S.tile + (size_t)(2 * tid) * kViewCols;
      double* row1 = row0 + kViewCols;
      if (!ok) {
        nbad = 1.0;
        if (JAC)
          for (int d = 0; d <= D; ++d) {
            row0[d] = 0.0;
            row1[d] = 0.0;
          }
      } else {
        const double sq = r[0] * r[0] + r[1] * r[1];
        double sqrt_rho1 = 1.0, asn = 0.0, rscale = 1.0;
        if (loss_type != 0) {
          double rho[3];
          loss_eval(loss_type, loss_width, sq, rho);
          c += 0.5 * rho[0];
          if (JAC) {
            sqrt_rho1 = sqrt(rho[1]);
            rscale = sqrt_rho1;
            if (!(sq == 0.0 || rho[2] <= 0.0)) {
              const double Dd = 1.0 + 2.0 * sq * rho[2] / rho[1];
              const double alpha = 1.0 - sqrt(Dd);
              rscale = sqrt_rho1 / (1.0 - alpha);
              asn = alpha / sq;
            }
          }
        } else {
          c += 0.5 * sq;
        }
        if (JAC) {
#pragma unroll
          for (int a = 0; a < 16; ++a) {
            const int d = S.col[a];
            if (d < 0) continue;
            // angle-axis columns: scaled inside the prepared record; the others here
            double j0 = a < 6 ? Jext[0][a] : Jint[0][a - 6];
            double j1 = a < 6 ? Jext[1][a] : Jint[1][a - 6];
            if (a < 3 || a >= 6) {
              j0 *= S.sp[a];
              j1 *= S.sp[a];
            }
            if (loss_type != 0) {
              const double rtj = j0 * r[0] + j1 * r[1];
              j0 = sqrt_rho1 * (j0 - asn * r[0] * rtj);
              j1 = sqrt_rho1 * (j1 - asn * r[1] * rtj);
            }
            row0[d] = j0;
            row1[d] = j1;
          }
          row0[D] = r[0] * rscale;
          row1[D] = r[1] * rscale;
        }
      }
    }
    if (JAC) {
      __syncthreads();
      if (ent < NS) {
        // rows part, part + nsplit, ...: two accumulators (alternate rows of the class) halve the dependent chain
        const int nr = 2 * nrow;
        int rr = part;
        for (; rr + nsplit < nr; rr += 2 * nsplit) {
          const double* r0 = S.tile + (size_t)rr * kViewCols;
          const double* r1 = r0 + (size_t)nsplit * kViewCols;
          acc += r0[gi] * r0[gj];
          acc2 += r1[gi] * r1[gj];
        }
        if (rr < nr) {
          const double* r0 = S.tile + (size_t)rr * kViewCols;
          acc += r0[gi] * r0[gj];
        }
      }
      __syncthreads();
    }
  }
  if (JAC) {
    if (ent < NS) S.part[tid] = acc + acc2;
    __syncthreads();
    if (tid < NS) {
      double sum = S.part[tid];
      for (int q = 1; q < nsplit; ++q) sum += S.part[q * stride + tid];
      if (gj < D) {
        S.A[gi * 16 + gj] = sum;
        S.A[gj * 16 + gi] = sum;
      } else if (gi < D) {
        S.g[gi] = sum;
      }
    }
  }
  double cost, b;
  vb_block_sum2(S, c, nbad, &cost, &b);  // (its barriers also publish S.A / S.g)
  *bad = b;
  return cost;
}

// Termination per view as in SmallLmOut.  Extrinsics and the group's intrinsics are written back for 0 and 1.
// The solve is small_lm.h's loop, but the gradient is tested at the top of an iteration (which then does not count)
// and the D <= 16 system is factored by lane 0 in LDS: D is known at run time only.
template <int UMODEL = -1>
__global__ __launch_bounds__(256) void view_lm_kernel(ViewBatch B, SmallLmArgs A) {
  __shared__ ViewLds S;
  const int tid = threadIdx.x;
  const int cb = B.chain_ptr[blockIdx.x], ce = B.chain_ptr[blockIdx.x + 1];
  for (int ci = cb; ci < ce; ++ci) {
    const int c = B.chain_views[ci];
    const int4 rec = B.cam[c];
    const int model = rec.x, nk = rec.z;
    const unsigned fm = (unsigned)rec.w;
    const int D = __popc(fm);
    const long long beg = B.vptr[c], end = B.vptr[c + 1];
    if (ci == cb && tid == 0)  // the chain's intrinsics: from memory once, then what the chain's views leave
      for (int j = 0; j < 10; ++j) S.kchain[j] = j < nk ? B.intr[rec.y + j] : 0.0;
    if (D == 0 || beg == end || D > 16) {
      if (tid == 0) B.out.write(c, -1, 0, 0.0, 0.0);
      continue;
    }
    if (tid == 0) {
      for (int a = 0; a < 6; ++a) S.x[a] = B.ext[(size_t)c * 6 + a];
      for (int j = 0; j < 10; ++j) S.x[6 + j] = S.kchain[j];
      int d = 0;
      for (int a = 0; a < 16; ++a) {
        S.sp[a] = 1.0;
        if (fm & (1u << a)) {
          S.col[a] = d;
          S.par[d++] = a;
        } else {
          S.col[a] = -1;
        }
      }
    }
    __syncthreads();
    const int lt = A.loss_type;
    const double lw = A.loss_width;
    double bad = 0.0;
    vb_prepare(S, S.x, nk);
    double cost = vb_pass<true, UMODEL>(B, S, model, D, beg, end, lt, lw, &bad);
    if (bad > 0.0) {
      // tmi_ba_solve stops with TMI_BA_ERR_EVALUATION_FAILED before it reports a cost
      if (tid == 0) B.out.write(c, 3, 0, 0.0, 0.0);
      __syncthreads();
      continue;
    }
    const double initial_cost = cost;
    if (A.jacobi_scaling) {
      // 1 / (1 + |column|) from the unscaled (loss-corrected) Jacobian at the start point
      if (tid == 0)
        for (int d = 0; d < D; ++d) S.sp[S.par[d]] = 1.0 / (1.0 + sqrt(S.A[d * 16 + d]));
      __syncthreads();
      vb_prepare(S, S.x, nk);
      cost = vb_pass<true, UMODEL>(B, S, model, D, beg, end, lt, lw, &bad);
    }
    auto x_norm_of = [&](const double* p) {
      double n = 0.0;
      if (fm & 0x3fu)
        for (int a = 0; a < 6; ++a) n += p[a] * p[a];
      if (fm >> 6)
        for (int j = 0; j < 10; ++j) n += p[6 + j] * p[6 + j];
      return n;
    };
    double x_norm = sqrt(x_norm_of(S.x));
    TrustRegion tr(A);
    int iter = 0, term = 1;
    bool need_gradient_check = true;
    for (;;) {
      if (iter >= A.max_num_iterations) break;
      ++iter;
      if (need_gradient_check) {
        need_gradient_check = false;
        double gmax = 0.0;
        for (int d = 0; d < D; ++d) gmax = fmax(gmax, fabs(S.g[d] / S.sp[S.par[d]]));
        if (gmax <= A.gradient_tolerance) {
          term = 0;
          --iter;
          break;
        }
      }
      const double inv_radius = 1.0 / tr.radius;
      if (tid == 0) {
        // (J^T J + diag) y = g by Cholesky; model cost change of the step -y: y^T g - 1/2 y^T J^T J y
        double ok = 1.0;
        for (int j = 0; j < D; ++j) {
          const double dj = S.A[j * 16 + j];
          double d = dj + TrustRegion::lm_diag(A, dj) * inv_radius;
          for (int m = 0; m < j; ++m) d -= S.L[j * 16 + m] * S.L[j * 16 + m];
          if (!(d > 0.0)) {
            ok = 0.0;
            d = 1.0;
          }
          const double l = sqrt(d);
          S.L[j * 16 + j] = l;
          const double il = 1.0 / l;
          for (int i = j + 1; i < D; ++i) {
            double t = S.A[j * 16 + i];
            for (int m = 0; m < j; ++m) t -= S.L[i * 16 + m] * S.L[j * 16 + m];
            S.L[i * 16 + j] = t * il;
          }
        }
        double mcc = 0.0;
        if (ok != 0.0) {
          double* z = S.z;  // (in LDS: a runtime-indexed register array would live in scratch)
          for (int i = 0; i < D; ++i) {
            double t = S.g[i];
            for (int m = 0; m < i; ++m) t -= S.L[i * 16 + m] * z[m];
            z[i] = t / S.L[i * 16 + i];
          }
          for (int i = D - 1; i >= 0; --i) {
            double t = z[i];
            for (int m = i + 1; m < D; ++m) t -= S.L[m * 16 + i] * S.y[m];
            S.y[i] = t / S.L[i * 16 + i];
          }
          double yg = 0.0, yVy = 0.0;
          for (int a = 0; a < D; ++a) {
            yg += S.y[a] * S.g[a];
            double t = 0.0;
            for (int b = 0; b < D; ++b) t += S.A[a * 16 + b] * S.y[b];
            yVy += S.y[a] * t;
          }
          mcc = yg - 0.5 * yVy;
          if (!(mcc > 0.0)) ok = 0.0;
        }
        if (ok != 0.0) {
          // candidate x - scale .* y on the free coordinates
          double step_sq = 0.0;
          for (int a = 0; a < 16; ++a) {
            double v = S.x[a];
            const int d = S.col[a];
            if (d >= 0) {
              const double dd = -S.y[d] * S.sp[a];
              v += dd;
              step_sq += dd * dd;
            }
            S.xc[a] = v;
          }
          S.scal[2] = step_sq;
          S.scal[3] = x_norm_of(S.xc);
        }
        S.scal[0] = ok;
        S.scal[1] = mcc;
      }
      __syncthreads();
      const bool usable = S.scal[0] != 0.0;
      const double mcc = S.scal[1], step_sq = S.scal[2], cand_xn_sq = S.scal[3];
      __syncthreads();
      if (!usable) {
        if (tr.invalid_step(A, &term)) break;
        continue;
      }
      vb_prepare(S, S.xc, nk);
      double cand_bad = 0.0;
      double cand_cost = vb_pass<false, UMODEL>(B, S, model, D, beg, end, lt, lw, &cand_bad);
      if (cand_bad > 0.0) cand_cost = 1.7976931348623157e308;
      if (tr.converged(A, sqrt(step_sq), x_norm, cost, cand_cost, &term)) break;
      if (tr.accept(A, (cost - cand_cost) / mcc)) {
        if (tid == 0)
          for (int a = 0; a < 16; ++a) S.x[a] = S.xc[a];
        __syncthreads();
        cost = cand_cost;
        x_norm = sqrt(cand_xn_sq);
        vb_prepare(S, S.x, nk);
        vb_pass<true, UMODEL>(B, S, model, D, beg, end, lt, lw, &bad);
        need_gradient_check = true;
      }
      if (tr.too_small(A, &term)) break;
    }
    if (tid == 0) {
      B.out.write(c, term, iter, initial_cost, cost);
      if (term != 2) {  // IsSolutionUsable
        for (int a = 0; a < 6; ++a) B.ext[(size_t)c * 6 + a] = S.x[a];
        if (fm >> 6) {
          for (int j = 0; j < nk; ++j) B.intr[rec.y + j] = S.x[6 + j];
          for (int j = 0; j < 10; ++j) S.kchain[j] = S.x[6 + j];
        }
      }
    }
    __syncthreads();
  }
}

// ---- the resident form's view-major index (tmi_ba_solver_adjust_views) ------------------------------
// keys[e] = (view << 32) | e for every observation slot e of the SELL layout (~0 for padding), slot_pt[e] = the
// slot's padded track index; sorted by a device radix sort, the views' ranges come from select_view_ptr_kernel.
__global__ __launch_bounds__(256) void view_keys_kernel(DeviceView v, unsigned long long* __restrict__ keys,
                                                        int* __restrict__ slot_pt) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * kSlicesPerBlock + (threadIdx.x >> 6);
  if (s >= v.nslices) return;
  const int lp = s * 64 + lane;
  const int k = v.pt_k[lp];
  const int K = (v.slice_ptr[s + 1] - v.slice_ptr[s]) >> 6;
  const size_t base = (size_t)v.slice_ptr[s] + lane;
  for (int j = 0; j < K; ++j) {
    const size_t e = base + (size_t)j * 64;
    keys[e] = (j < k) ? (((unsigned long long)(unsigned)v.obs_cam[e] << 32) | (unsigned long long)e) : ~0ull;
    slot_pt[e] = lp;
  }
}

}  // namespace tmi
