// The scaffold of the one-shot calls (side_calls.h, pose_graph_calls.h): the memory and stream of one call (OneShot,
// Pinned), device time between marks (StreamTimer), the typed way out (download, ReadBack), the batched small-problem
// solve (run_small_lm), the frame of a batch call (one_shot_batch, with_light_handle) and the argument checks two or
// more calls share.  Included by engine.hip after the driver: TMI_HIP, g_last_error, now_s, create_impl and
// tmi_ba_solver are the driver's.
#pragma once

#include "read_back_error.h"

namespace {
// n elements from the device to the host, queued on `stream`; nothing where there is nothing to copy or nobody asked.
template <class T>
hipError_t download(hipStream_t stream, T* host, const T* device, size_t n) {
  if (n == 0 || !host) return hipSuccess;
  return hipMemcpyAsync(host, device, n * sizeof(T), hipMemcpyDeviceToHost, stream);
}

// Device memory of one call, freed on every way out, and the stream it runs on: a stream of its own (open) or a
// borrowed one.  error: what TMI_HIP reports.
struct OneShot {
  std::string error;
  std::vector<void*> allocs;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  explicit OneShot(hipStream_t borrowed = nullptr) : stream(borrowed) {}
  OneShot(const OneShot&) = delete;
  OneShot& operator=(const OneShot&) = delete;
  // a stream of its own on `device` (< 0: the current device)
  int open(int device) {
    OneShot* s = this;
    if (device >= 0) TMI_HIP(hipSetDevice(device));
    TMI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    own_stream = true;
    return TMI_BA_OK;
  }
  template <class T>
  hipError_t alloc(T** p, size_t n) {
    *p = nullptr;
    const hipError_t e = hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) allocs.push_back((void*)*p);
    return e;
  }
  // alloc, then every byte of the buffer set to `byte` on the stream
  template <class T>
  hipError_t alloc_filled(T** p, size_t n, int byte) {
    hipError_t e = alloc(p, n);
    if (e == hipSuccess) e = hipMemsetAsync(*p, byte, std::max<size_t>(n, 1) * sizeof(T), stream);
    return e;
  }
  template <class T>
  hipError_t upload(T** p, const T* h, size_t n) {
    hipError_t e = alloc(p, n);
    if (e == hipSuccess && n) e = hipMemcpyAsync(*p, h, n * sizeof(T), hipMemcpyHostToDevice, stream);
    return e;
  }
  template <class T>
  hipError_t download(T* host, const T* device, size_t n) {
    return ::download(stream, host, device, n);
  }
  // per-item outputs of a batched solve, preset to "nothing to solve" (-1, 0, 0, 0)
  int alloc_outputs(SmallLmOut* o, size_t n) {
    OneShot* s = this;
    TMI_HIP(alloc_filled(&o->term, n, 0xff));
    TMI_HIP(alloc_filled(&o->iters, n, 0));
    TMI_HIP(alloc_filled(&o->c0, n, 0));
    TMI_HIP(alloc_filled(&o->c1, n, 0));
    return TMI_BA_OK;
  }
  ~OneShot() {
    if (own_stream) hipStreamDestroy(stream);
    for (void* p : allocs) hipFree(p);
  }
};

// Pinned host memory of one call, n elements (16 bytes at least), freed on every way out.
template <class T>
struct Pinned {
  T* p = nullptr;
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  hipError_t alloc(size_t n) {
    return hipHostMalloc((void**)&p, std::max<size_t>(n * sizeof(T), 16), hipHostMallocDefault);
  }
  T* get() const { return p; }
  ~Pinned() {
    if (p) hipHostFree(p);
  }
};

// The finish of a call, made when its last launch has been queued: the launch error is taken then, add() queues the
// read-backs until one fails, and finish() always synchronises the stream and answers the launch, copy or sync error,
// in that order (read_back_error.h), for TMI_HIP to report.
struct ReadBack {
  hipStream_t stream;
  hipError_t launch;
  hipError_t copy = hipSuccess;
  explicit ReadBack(hipStream_t stream_) : stream(stream_), launch(hipGetLastError()) {}
  template <class T>
  void add(T* host, const T* device, size_t n) {
    if (copy == hipSuccess) copy = download(stream, host, device, n);
  }
  hipError_t finish() { return read_back_error(launch, copy, hipStreamSynchronize(stream)); }
};

// Device time between marks on a stream: every mark() records the next event; seconds(a, b) is the time from mark a to
// mark b once the stream has been synchronised (0 where the runtime cannot tell).  The events are destroyed on every
// way out.
struct StreamTimer {
  static constexpr int kMaxMarks = 4;
  hipStream_t stream;
  hipEvent_t ev[kMaxMarks] = {};
  hipError_t status = hipSuccess;  // of creating the events: TMI_HIP(timer.status) before the first mark
  int marked = 0;
  explicit StreamTimer(hipStream_t stream_, int marks = 2) : stream(stream_) {
    for (int i = 0; i < marks && status == hipSuccess; ++i) status = hipEventCreate(&ev[i]);
  }
  StreamTimer(const StreamTimer&) = delete;
  StreamTimer& operator=(const StreamTimer&) = delete;
  hipError_t mark() { return hipEventRecord(ev[marked++], stream); }
  double seconds(int a = 0, int b = 1) const {
    float ms = 0.f;
    hipEventElapsedTime(&ms, ev[a], ev[b]);
    return 1e-3 * ms;
  }
  ~StreamTimer() {
    for (hipEvent_t e : ev)
      if (e) hipEventDestroy(e);
  }
};

// The caller's per-item arrays (each may be null).
struct ItemArrays {
  int8_t* term;
  int32_t* iters;
  double* c0;
  double* c1;
};

// One batched small-problem solve: launch() queues it on `stream` between two events (sum->kernel_seconds), then the n
// per-item outputs d are read back, counted (*num_items: termination >= 0; successes 0 and 1) and item i is written to
// the caller's arrays at map[i] (null: the identity; map[i] < 0: padding).  term_h (optional): the terminations.
// TMI_HIP reports into s->error.
template <class Holder, class Sum, class Launch>
int run_small_lm(Holder* s, hipStream_t stream, const SmallLmOut& d, size_t n, const int* map, Launch launch,
                 const ItemArrays& out, Sum* sum, int64_t* num_items, std::vector<signed char>* term_h = nullptr) {
  StreamTimer timer(stream);
  TMI_HIP(timer.status);
  timer.mark();
  launch();
  timer.mark();
  ReadBack rb(stream);
  std::vector<signed char> term(n);
  std::vector<int> iters(n);
  std::vector<double> c0(out.c0 ? n : 0), c1(out.c1 ? n : 0);
  rb.add(term.data(), d.term, n);
  rb.add(iters.data(), d.iters, n);
  rb.add(c0.data(), d.c0, c0.size());
  rb.add(c1.data(), d.c1, c1.size());
  TMI_HIP(rb.finish());
  for (size_t i = 0; i < n; ++i) {
    const int p = map ? map[i] : (int)i;
    if (p < 0) continue;
    const int t = term[i];
    if (t >= 0) {
      ++*num_items;
      if (t == 0 || t == 1) sum->num_success++;
      sum->total_iterations += iters[i];
    }
    if (out.term) out.term[p] = (int8_t)t;
    if (out.iters) out.iters[p] = iters[i];
    if (out.c0) out.c0[p] = c0[i];
    if (out.c1) out.c1[p] = c1[i];
  }
  sum->kernel_seconds = timer.seconds();
  if (term_h) term_h->swap(term);
  return TMI_BA_OK;
}

// One-shot form of a resident track entry point: call(s) on a light handle of P, the points downloaded into
// `download` afterwards if it is given (the cameras are constant on these paths), the handle destroyed on every way
// out.
template <class Call>
int with_light_handle(const tmi_ba_problem* P, const tmi_ba_options* O, tmi_ba_problem* download, Call call) {
  tmi_ba_solver* s = new tmi_ba_solver();
  int rc = create_impl(s, P, O, 0, 1, /*light=*/true);
  if (rc == TMI_BA_OK) rc = call(s);
  if (rc == TMI_BA_OK && download) rc = tmi_ba_solver_download(s, download);
  if (rc != TMI_BA_OK) g_last_error = s->error;
  tmi_ba_solver_destroy(s);
  return rc;
}

// An argument error and its message, before the device is touched.
int bad_argument(const char* why) {
  g_last_error = why;
  return TMI_BA_ERR_INVALID_ARGUMENT;
}

// The device part of a one-shot batch call, after its argument checks: TMI_BA_ERR_NO_DEVICE without a device, `device`
// checked against the count (no_such_device: the message, or null for none), nothing to do for an empty batch; then
// body(OneShot*) on a stream of its own, its error handed to tmi_ba_last_error, and *seconds since t0.
template <class Body>
int one_shot_batch(int device, const char* no_such_device, int num_items, double t0, double* seconds, Body body) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_last_error = "no HIP device visible (the device path has no CPU fallback)";
    return TMI_BA_ERR_NO_DEVICE;
  }
  if (device >= ndev) {
    if (no_such_device) g_last_error = no_such_device;
    return TMI_BA_ERR_INVALID_ARGUMENT;
  }
  if (num_items == 0) return TMI_BA_OK;
  OneShot s;
  int rc = s.open(device);
  if (rc == TMI_BA_OK) rc = body(&s);
  if (rc) g_last_error = s.error;
  *seconds = now_s() - t0;
  return rc;
}

bool all_finite(const double* x, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) return false;
  return true;
}

// What the calls on a view-pair batch ask of it; `pair_values` is the per-edge array the call reads.  null: fine.
const char* check_view_pair_batch(const tmi_ba_view_pair_batch* B, bool need_rotation, const double* pair_values) {
  const int V = B->num_views, E = B->num_pairs;
  if (V < 0 || E < 0) return "view pairs: negative size";
  if (need_rotation && V > 0 && !B->view_rotation) return "view pairs: missing view_rotation";
  if (E > 0 && (!B->pair_view1 || !B->pair_view2 || !pair_values)) return "view pairs: missing array";
  if (E > (1 << 30)) return "view pairs: more than 2^30 pairs";
  std::vector<uint64_t> keys((size_t)E);
  for (int e = 0; e < E; ++e) {
    const int a = B->pair_view1[e], b = B->pair_view2[e];
    if (a < 0 || a >= V || b < 0 || b >= V) return "view pairs: view index out of range";
    if (a == b) return "view pairs: a view paired with itself";
    keys[e] = ((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b);
  }
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return "view pairs: an unordered pair appears twice";
  if (B->view_rotation && !all_finite(B->view_rotation, (size_t)3 * V)) return "view pairs: non-finite view_rotation";
  if (!all_finite(pair_values, (size_t)3 * E)) return "view pairs: non-finite pair value";
  return nullptr;
}
}  // namespace
