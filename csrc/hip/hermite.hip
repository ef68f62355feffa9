// Runtime of the 4th-order Hermite integrator on one GPU (gs_hermite_* in gravsim.h).
//
// Device-resident state x, v, a, j (4 components per body, n_pad rows, ghost rows zero) and a
// control block (t, h, steps; gs_hermite.h). A step is four launches on one stream: control,
// predict, evaluate (the hot acceleration+jerk kernel, nbody_hermite.hip), reduce + correct.
// The step size and the time live on the device, so enqueueing steps never waits for one.
#include <limits>
#include <utility>
#include <vector>

#include "gs_hermite.h"
#include "gs_stepper.h"

struct gs_hermite {
  gs_config cfg;
  int64_t n = 0, n_pad = 0;
  int32_t chunk = 0, n_chunks = 0, ipl = 0, groups = 0;
  size_t esz = 4;
  hipStream_t stream = nullptr;
  void *X = nullptr, *V = nullptr, *A = nullptr, *J = nullptr, *XP = nullptr, *VP = nullptr;
  void *PA = nullptr, *PJ = nullptr, *a_out = nullptr, *j_out = nullptr;
  gs::HermiteCtrl* ctrl = nullptr;
  double* wgmin = nullptr;
  double* mass_dev = nullptr;
  unsigned long long* nonfinite = nullptr;
  std::vector<double> mass_host;
  double eta = 0.0, t_end = 0.0;
  bool has_end = false;
};

namespace {

size_t rows_bytes(const gs_hermite* h) { return (size_t)h->n_pad * 4 * h->esz; }
int nwg(const gs_hermite* h) { return (int)(h->n_pad / gs::kForceBlock); }

template <typename T>
gs::HArgs<T> make_args(const gs_hermite* h, int mode, bool phi) {
  gs::HArgs<T> a{};
  a.X = static_cast<T*>(h->X); a.V = static_cast<T*>(h->V);
  a.A = static_cast<T*>(h->A); a.J = static_cast<T*>(h->J);
  a.XP = static_cast<T*>(h->XP); a.VP = static_cast<T*>(h->VP);
  a.PA = static_cast<T*>(h->PA); a.PJ = static_cast<T*>(h->PJ);
  a.a_out = static_cast<T*>(h->a_out); a.j_out = static_cast<T*>(h->j_out);
  a.ctrl = h->ctrl;
  a.wgmin = h->wgmin;
  a.n_real = h->n; a.n_pad = h->n_pad; a.chunk = h->chunk; a.n_chunks = h->n_chunks;
  a.mode = mode;
  a.phi = phi ? 1 : 0;
  a.cut2 = (T)(h->cfg.cutoff * h->cfg.cutoff);
  a.eps2 = (T)(h->cfg.softening * h->cfg.softening);
  return a;
}

// Write the control block for a run that stands at time t (stream-ordered).
int write_ctrl(gs_hermite* h, double t, uint64_t steps, double dt_last, double dt_min) {
  gs::HermiteCtrl c{};
  c.t = t;
  c.h = 0.0;
  c.dt_last = dt_last;
  c.dt_min = dt_min;
  c.dt_max = h->cfg.dt;
  c.eta = h->eta;
  c.t_end = h->t_end;
  c.steps = steps;
  c.has_end = h->has_end ? 1 : 0;
  c.active = 0;
  GS_HIP(hipMemcpyAsync(h->ctrl, &c, sizeof(c), hipMemcpyHostToDevice, h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));  // (c is on this frame)
  return 0;
}

int read_ctrl(gs_hermite* h, gs::HermiteCtrl* c) {
  GS_HIP(hipMemcpyAsync(c, h->ctrl, sizeof(*c), hipMemcpyDeviceToHost, h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// Derivatives of the current (x, v) through the step's own kernel, then the reduce in `mode`.
template <typename T>
int eval_current(gs_hermite* h, int mode, bool phi) {
  gs::HArgs<T> a = make_args<T>(h, mode, phi);
  a.XP = a.X;
  a.VP = a.V;
  GS_HIP(gs::launch_hermite_eval<T>(a, h->ipl, h->groups, false, h->stream));
  GS_HIP(gs::launch_hermite_reduce<T>(a, h->stream));
  return 0;
}

template <typename T>
int step_t(gs_hermite* h, int32_t nsteps) {
  const gs::HArgs<T> a = make_args<T>(h, gs::HM_STEP, false);
  for (int32_t k = 0; k < nsteps; ++k) {
    GS_HIP(gs::launch_hermite_ctrl<T>(a, h->stream));
    GS_HIP(gs::launch_hermite_predict<T>(a, h->stream));
    GS_HIP(gs::launch_hermite_eval<T>(a, h->ipl, h->groups, true, h->stream));
    GS_HIP(gs::launch_hermite_reduce<T>(a, h->stream));
  }
  return 0;
}

// Host fp64 (n x 3 [+ w]) -> device rows of 4 (ghost rows zero).
template <typename T>
int upload_rows(gs_hermite* h, void* dst, const double* src3, const double* w, double wscale) {
  std::vector<T> buf((size_t)h->n_pad * 4, T(0));
  for (int64_t i = 0; i < h->n; ++i) {
    for (int d = 0; d < 3; ++d) buf[4 * i + d] = (T)src3[3 * i + d];
    if (w) buf[4 * i + 3] = (T)(wscale * w[i]);
  }
  GS_HIP(hipMemcpyAsync(dst, buf.data(), rows_bytes(h), hipMemcpyHostToDevice, h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

template <typename T>
int download_rows(gs_hermite* h, const void* src, int64_t rows, double* out, int comps) {
  if (!out) return 0;
  std::vector<T> buf((size_t)rows * 4);
  GS_HIP(hipMemcpyAsync(buf.data(), src, (size_t)rows * 4 * sizeof(T), hipMemcpyDeviceToHost,
                        h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  for (int64_t i = 0; i < rows; ++i)
    for (int d = 0; d < comps; ++d) out[comps * i + d] = (double)buf[4 * i + d];
  return 0;
}

int set_wgmin(gs_hermite* h, double first) {
  std::vector<double> w((size_t)nwg(h), std::numeric_limits<double>::infinity());
  w[0] = first;
  GS_HIP(hipMemcpyAsync(h->wgmin, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice,
                        h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int start_from_state(gs_hermite* h) {
  if (write_ctrl(h, 0.0, 0, 0.0, std::numeric_limits<double>::infinity())) return -1;
  return h->esz == 4 ? eval_current<float>(h, gs::HM_INIT, false)
                     : eval_current<double>(h, gs::HM_INIT, false);
}

}  // namespace

extern "C" {

int gs_hermite_create(const gs_config* cfg, gs_hermite** out) {
  if (!cfg || !out) { gs_set_error("hermite: null argument"); return -1; }
  if (cfg->nranks != 1 || cfg->rank != 0) {
    gs_set_error("hermite runs on one rank (nranks must be 1)");
    return -1;
  }
  if (cfg->n < 1) { gs_set_error("hermite: n must be >= 1"); return -1; }
  if (!(cfg->dt > 0.0)) { gs_set_error("hermite: dt must be > 0"); return -1; }
  if (!(cfg->cutoff > 0.0) && !(cfg->softening > 0.0)) {
    gs_set_error("hermite: cutoff and softening cannot both be 0 (the self term)");
    return -1;
  }
  const int fp64 = cfg->dtype == GS_FP64;
  const int32_t chunk = cfg->chunk > 0 ? cfg->chunk : gs::auto_chunk(cfg->n);
  if (chunk % 1024) { gs_set_error("hermite: chunk must be a multiple of 1024"); return -1; }
  gs_hermite* h = new gs_hermite();
  h->cfg = *cfg;
  h->esz = fp64 ? 8 : 4;
  h->n = cfg->n;
  h->chunk = chunk;
  h->n_pad = gs::round_up(cfg->n, chunk);
  h->n_chunks = (int32_t)(h->n_pad / chunk);
  // Launch shape (any choice gives the same bits): the widest lane tile that still leaves
  // about four workgroups per CU, then as many chunk groups as reach that count.
  const int64_t want = 1024;
  int ipl = cfg->ipl;
  if (ipl == 0) {
    ipl = fp64 ? 2 : 4;
    while (ipl > (fp64 ? 1 : 2) && h->n_pad / (gs::kForceBlock * ipl) * h->n_chunks < want)
      ipl >>= 1;
  }
  if (!gs::hermite_ipl_ok(fp64, ipl) || h->n_pad % (gs::kForceBlock * ipl)) {
    gs_set_error("hermite: ipl must be 1, 2 (or 4 for fp32)");
    delete h;
    return -1;
  }
  h->ipl = ipl;
  const int64_t blocks = h->n_pad / (gs::kForceBlock * ipl);
  int64_t groups = cfg->split_groups > 0 ? cfg->split_groups : (2 * want + blocks - 1) / blocks;
  if (groups > h->n_chunks) groups = h->n_chunks;
  if (groups < 1) groups = 1;
  h->groups = (int32_t)groups;
  auto fail = [&](const char*) {
    gs_hermite_destroy(h);
    return -1;
  };
#define HM_TRY(call)                                                                  \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) {                                                           \
      char b_[256];                                                                   \
      snprintf(b_, sizeof(b_), "hermite create: %s: %s", #call, hipGetErrorString(e_)); \
      gs_set_error(b_);                                                               \
      return fail(b_);                                                                \
    }                                                                                 \
  } while (0)
  HM_TRY(hipSetDevice(cfg->device));
  HM_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const size_t rb = rows_bytes(h);
  for (void** p : {&h->X, &h->V, &h->A, &h->J, &h->XP, &h->VP, &h->a_out, &h->j_out}) {
    HM_TRY(hipMalloc(p, rb));
    HM_TRY(hipMemsetAsync(*p, 0, rb, h->stream));
  }
  HM_TRY(hipMalloc(&h->PA, rb * (size_t)h->n_chunks));
  HM_TRY(hipMalloc(&h->PJ, rb * (size_t)h->n_chunks));
  HM_TRY(hipMalloc((void**)&h->ctrl, sizeof(gs::HermiteCtrl)));
  HM_TRY(hipMalloc((void**)&h->wgmin, (size_t)nwg(h) * sizeof(double)));
  HM_TRY(hipMalloc((void**)&h->mass_dev, (size_t)h->n_pad * sizeof(double)));
  HM_TRY(hipMalloc((void**)&h->nonfinite, sizeof(unsigned long long)));
  HM_TRY(hipStreamSynchronize(h->stream));
#undef HM_TRY
  h->mass_host.assign((size_t)h->n, 0.0);
  if (set_wgmin(h, std::numeric_limits<double>::infinity()) ||
      write_ctrl(h, 0.0, 0, 0.0, std::numeric_limits<double>::infinity())) {
    gs_hermite_destroy(h);
    return -1;
  }
  *out = h;
  return 0;
}

int gs_hermite_destroy(gs_hermite* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : {h->X, h->V, h->A, h->J, h->XP, h->VP, h->a_out, h->j_out, h->PA, h->PJ,
                  (void*)h->ctrl, (void*)h->wgmin, (void*)h->mass_dev, (void*)h->nonfinite})
    if (p) (void)hipFree(p);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

int gs_hermite_layout(gs_hermite* h, gs_layout* out) {
  if (!h || !out) { gs_set_error("hermite layout: null argument"); return -1; }
  *out = gs_layout{};
  out->n = h->n;
  out->n_pad = h->n_pad;
  out->n_local = h->n_pad;
  out->local_begin = 0;
  out->chunk = h->chunk;
  out->n_chunks = h->n_chunks;
  out->ipl = h->ipl;
  out->kernel = GS_KERNEL_LDS;
  out->mode = GS_MODE_SPLIT;
  out->split_groups = h->groups;
  return 0;
}

int gs_hermite_set_adaptive(gs_hermite* h, double eta, double dt_max, double t_end) {
  if (!(eta >= 0.0) || !(dt_max > 0.0)) {
    gs_set_error("hermite: eta must be >= 0 and dt_max > 0");
    return -1;
  }
  GS_HIP(hipSetDevice(h->cfg.device));
  h->eta = eta;
  h->cfg.dt = dt_max;
  h->has_end = t_end >= 0.0;  // (a negative or NaN t_end: no end time)
  h->t_end = h->has_end ? t_end : 0.0;
  gs::HermiteCtrl c;
  if (read_ctrl(h, &c)) return -1;
  return write_ctrl(h, c.t, c.steps, c.dt_last, c.dt_min);
}

int gs_hermite_init_ics(gs_hermite* h, int32_t ic, uint64_t seed) {
  GS_HIP(hipSetDevice(h->cfg.device));
  hipError_t e;
  if (h->esz == 4)
    e = gs::launch_init_ics<float>(ic, seed, h->n, h->n_pad, 0, h->n_pad, h->cfg.G,
                                   static_cast<float*>(h->X), static_cast<float*>(h->V),
                                   h->mass_dev, h->stream);
  else
    e = gs::launch_init_ics<double>(ic, seed, h->n, h->n_pad, 0, h->n_pad, h->cfg.G,
                                    static_cast<double*>(h->X), static_cast<double*>(h->V),
                                    h->mass_dev, h->stream);
  GS_HIP(e);
  GS_HIP(hipMemcpyAsync(h->mass_host.data(), h->mass_dev, (size_t)h->n * sizeof(double),
                        hipMemcpyDeviceToHost, h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  return start_from_state(h);
}

int gs_hermite_set_state(gs_hermite* h, const double* pos, const double* vel, const double* mass,
                         const double* acc, const double* jerk, double t, double dt_next,
                         double dt_min) {
  if (!pos || !vel || !mass) { gs_set_error("hermite set_state: null argument"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  const bool f32 = h->esz == 4;
  if (f32 ? upload_rows<float>(h, h->X, pos, mass, h->cfg.G)
          : upload_rows<double>(h, h->X, pos, mass, h->cfg.G))
    return -1;
  if (f32 ? upload_rows<float>(h, h->V, vel, nullptr, 0.0)
          : upload_rows<double>(h, h->V, vel, nullptr, 0.0))
    return -1;
  h->mass_host.assign(mass, mass + h->n);
  if (!acc || !jerk) {
    if (start_from_state(h)) return -1;
    gs::HermiteCtrl c;
    if (read_ctrl(h, &c)) return -1;  // (also waits for the evaluation)
    return write_ctrl(h, t, 0, 0.0,
                      dt_min > 0.0 ? dt_min : std::numeric_limits<double>::infinity());
  }
  // A resumed run: a, j as the last step left them, and the step size its criterion chose.
  if (f32 ? upload_rows<float>(h, h->A, acc, nullptr, 0.0)
          : upload_rows<double>(h, h->A, acc, nullptr, 0.0))
    return -1;
  if (f32 ? upload_rows<float>(h, h->J, jerk, nullptr, 0.0)
          : upload_rows<double>(h, h->J, jerk, nullptr, 0.0))
    return -1;
  if (set_wgmin(h, dt_next > 0.0 ? dt_next : std::numeric_limits<double>::infinity())) return -1;
  return write_ctrl(h, t, 0, 0.0,
                    dt_min > 0.0 ? dt_min : std::numeric_limits<double>::infinity());
}

int gs_hermite_get_state(gs_hermite* h, double* pos, double* vel, double* mass, double* acc,
                         double* jerk) {
  GS_HIP(hipSetDevice(h->cfg.device));
  const bool f32 = h->esz == 4;
  const std::pair<const void*, double*> rows[4] = {{h->X, pos}, {h->V, vel}, {h->A, acc},
                                                   {h->J, jerk}};
  for (const auto& r : rows)
    if (f32 ? download_rows<float>(h, r.first, h->n, r.second, 3)
            : download_rows<double>(h, r.first, h->n, r.second, 3))
      return -1;
  if (mass)
    for (int64_t i = 0; i < h->n; ++i) mass[i] = h->mass_host[(size_t)i];
  return 0;
}

int gs_hermite_derivs(gs_hermite* h, double* acc4, double* jerk4) {
  GS_HIP(hipSetDevice(h->cfg.device));
  const bool f32 = h->esz == 4;
  if (f32 ? eval_current<float>(h, gs::HM_OUT, true) : eval_current<double>(h, gs::HM_OUT, true))
    return -1;
  if (f32 ? download_rows<float>(h, h->a_out, h->n, acc4, 4)
          : download_rows<double>(h, h->a_out, h->n, acc4, 4))
    return -1;
  return f32 ? download_rows<float>(h, h->j_out, h->n, jerk4, 4)
             : download_rows<double>(h, h->j_out, h->n, jerk4, 4);
}

int gs_hermite_step(gs_hermite* h, int32_t nsteps) {
  GS_HIP(hipSetDevice(h->cfg.device));
  return h->esz == 4 ? step_t<float>(h, nsteps) : step_t<double>(h, nsteps);
}

int gs_hermite_sync(gs_hermite* h) {
  GS_HIP(hipSetDevice(h->cfg.device));
  GS_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int gs_hermite_status(gs_hermite* h, gs_hermite_info* out) {
  if (!h || !out) { gs_set_error("hermite status: null argument"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  gs::HermiteCtrl c;
  if (read_ctrl(h, &c)) return -1;
  double next = c.dt_max;
  if (c.eta > 0.0) {
    std::vector<double> w((size_t)nwg(h));
    GS_HIP(hipMemcpyAsync(w.data(), h->wgmin, w.size() * sizeof(double), hipMemcpyDeviceToHost,
                          h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    for (double v : w)
      if (v < next) next = v;
  }
  out->time = c.t;
  out->dt_last = c.dt_last;
  out->dt_next = next;
  out->dt_min = c.dt_min;
  out->steps = (int64_t)c.steps;
  out->finished = c.has_end && c.t >= c.t_end;
  out->ipl = h->ipl;
  return 0;
}

int64_t gs_hermite_count_nonfinite(gs_hermite* h) {
  if (hipSetDevice(h->cfg.device) != hipSuccess ||
      hipMemsetAsync(h->nonfinite, 0, sizeof(unsigned long long), h->stream) != hipSuccess) {
    gs_set_error("hermite count_nonfinite: device error");
    return -1;
  }
  hipError_t e = h->esz == 4
      ? gs::launch_count_nonfinite<float>(static_cast<const float*>(h->X), 0, h->n_pad,
                                          static_cast<const float*>(h->V), h->nonfinite, h->stream)
      : gs::launch_count_nonfinite<double>(static_cast<const double*>(h->X), 0, h->n_pad,
                                           static_cast<const double*>(h->V), h->nonfinite,
                                           h->stream);
  unsigned long long cnt = 0;
  if (e != hipSuccess ||
      hipMemcpyAsync(&cnt, h->nonfinite, sizeof(cnt), hipMemcpyDeviceToHost, h->stream) !=
          hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess) {
    gs_set_error("hermite count_nonfinite: device error");
    return -1;
  }
  return (int64_t)cnt;
}

}  // extern "C"
