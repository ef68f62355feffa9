// Runtime of the Hermite integrators, 4th and 6th order (gs_hermite_* in gravsim.h).
//
// Device-resident state x, v, a, j (4 components per body, n_pad rows, ghost rows zero) and a
// control block (t, h, steps; gs_hermite.h). A step is four launches on one stream: control,
// predict, evaluate (the hot acceleration+jerk kernel, nbody_hermite.hip), reduce + correct.
// The step size and the time live on the device, so enqueueing steps never waits for one.
// The order is a property of the run (gs_hermite_set_order): order 6 also carries snap and
// crackle rows, its chain is the same four launches with the kernels of nbody_hermite6.hip, and
// the one path below asks the order where the two differ (with_args, launch_shape, eval_current,
// the carried rows). It runs on one rank in fp32 or fp64; gs_hermite_set_block keeps refusing it,
// and its block steps (fp64 only) are switched on by gs_hermite_set_block6 (refuse6).
// Block mode (gs_hermite_set_block): per-body times and levels, an active list and a second
// control block; a block step is a chain of seven launches, and gs_hermite_step advances whole
// macro steps of dt against a device-side target time, one status read per 32 chains. Both orders
// take the one path: block_chain and derivs_active call gs::launch_block_* on the run's kernel
// arguments, and the overloads for H6Args run order 4's next, control and compact kernels on
// base_view(a) and order 6's own predict-all, narrow, wide and correct kernels.
// Three precisions: fp32 and fp64 throughout, and mixed (GS_MIXED): the state rows, the reduce
// and the corrector in fp64, the predicted rows (position as double-single hi + lo) and the
// partial sums of the pair kernels in fp32.
// Ranks (shared steps only): rank r owns whole units of 1024 rows (gs_hermite_partition) and runs
// the slice forms of predict, evaluate and reduce + correct on them; every array but the
// partials keeps its full length. A step is control -> predict (slice) -> gather of XP, VP (XL)
// -> evaluate (slice) -> reduce + correct (slice) -> gather of wgmin, all on the engine's one
// stream; every rank runs the control kernel on the gathered wgmin and so holds the same h, t
// and steps. The gathers are RCCL collectives (gs_hermite_comm_init) or, for the shards of a
// virtual group in one process, device copies ordered by events (gs_hermite_group_*).
#include <chrono>
#include <cmath>
#include <initializer_list>
#include <limits>
#include <memory>
#include <utility>
#include <vector>

#include "gs_hermite.h"
#include "gs_stepper.h"

struct gs_hermite {
  gs_config cfg;
  int64_t n = 0, n_pad = 0;
  int32_t chunk = 0, n_chunks = 0, ipl = 0, groups = 0;
  size_t esz = 4;  // bytes per element of the state rows (x, v, a, j, the outputs)
  size_t psz = 4;  // ... of the predicted rows and the partial sums (mixed: 4 against esz 8)
  hipStream_t stream = nullptr;
  // Device buffers are owned in groups (gs_devmem.h; docs/DESIGN.md §24): each is complete or
  // empty, and a pointer is null exactly while its group does not hold it.
  gs::rt::DevMem base;  // while the engine lives: the buffers from here to `nonfinite`
  void *X = nullptr, *V = nullptr, *A = nullptr, *J = nullptr, *XP = nullptr, *VP = nullptr;
  void* XL = nullptr;  // mixed: lo rows of the predicted position
  void *PA = nullptr, *PJ = nullptr, *a_out = nullptr, *j_out = nullptr;
  gs::HermiteCtrl* ctrl = nullptr;
  double* wgmin = nullptr;
  double* mass_dev = nullptr;
  unsigned long long* nonfinite = nullptr;
  std::vector<double> mass_host;
  double eta = 0.0, t_end = 0.0;
  bool has_end = false;
  // block time steps (gs_hermite_set_block)
  bool block = false;
  int32_t max_level = 24, narrow_max = 0;
  gs::HBlock blk{};
  gs::rt::DevMem blockg;  // while `block`: blk.bc, tb, level, list, wgcount, wgnext
  // while `block` with blk.cap > 0 slots, the partials of the narrow path (size_narrow): blk.NA,
  // blk.NJ, the snap's NS for order 6, the neighbour's NNI where collisions are on
  gs::rt::DevMem narrow;
  void* NS = nullptr;
  int32_t* NNI = nullptr;
  int64_t macro0 = 0;  // macro steps of dt the run stood at when its state was set
  // collisions (gs_hermite_set_collisions): 0 off, 1 record, 2 record and stop the shared step
  int32_t nn = 0;
  gs::rt::DevMem coll;  // while `nn`: the eight below
  void* R = nullptr;  // radii, state precision
  int32_t *PN = nullptr, *nn_i = nullptr, *ca_i = nullptr, *nn_out = nullptr;
  double *nn_q = nullptr, *ca_q = nullptr, *q_out = nullptr;
  // ranks: the rows this one owns, and every rank's (in units of 1024 rows)
  int64_t row0 = 0, n_loc = 0;
  std::vector<int64_t> ubeg, ucnt;
  bool uniform = true;        // equal slices: in-place ncclAllGather
  bool wgmin_open = false;    // the first step minima wait for a gather (a shard of a group)
  hipEvent_t ev = nullptr;    // this shard's rows are ready (virtual group)
  ncclComm_t comm = nullptr;
  std::atomic<ncclComm_t> comm_live{nullptr};
  int32_t comm_count = 0, comm_user_rank = -1, comm_cu_device = -1;
  double step_timeout_s = 0.0;
  // bounded waits (RCCL runs): an event per chain in a ring; `seen` of `rec` have completed
  std::vector<hipEvent_t> ring;
  int64_t rec = 0, seen = 0;
  // 6th-order scheme (gs_hermite_set_order): snap and crackle rows, the predicted acceleration,
  // the snap partials and output
  int32_t order = 4;
  void *S = nullptr, *C = nullptr, *AP = nullptr, *PS = nullptr, *s_out = nullptr;
  gs::rt::DevMem six;  // while `order` is 6: the five above
};

namespace {

size_t rows_bytes(const gs_hermite* h) { return (size_t)h->n_pad * 4 * h->esz; }
size_t pair_rows_bytes(const gs_hermite* h) { return (size_t)h->n_pad * 4 * h->psz; }
bool is_mixed(const gs_hermite* h) { return h->psz != h->esz; }

// f(T pair type, S state type) for the run's precision.
template <typename F>
int by_dtype(const gs_hermite* h, F f) {
  if (is_mixed(h)) return f(float(), double());
  return h->esz == 4 ? f(float(), float()) : f(double(), double());
}
// f(S state type): fp32 rows for an fp32 run, fp64 rows for fp64 and mixed.
template <typename F>
auto by_state(const gs_hermite* h, F f) {
  return h->esz == 4 ? f(float()) : f(double());
}
int nwg(const gs_hermite* h) { return (int)(h->n_pad / gs::kForceBlock); }
bool multi(const gs_hermite* h) { return h->cfg.nranks > 1; }
constexpr int64_t kUnit = 1024;  // rows per ownership unit (gs_hermite_partition)

// The kernel arguments of a launch. What both structs hold: P the type of the predicted rows, the
// partials and the pair law, S of the state rows and the outputs.
template <typename P, typename S, typename A>
void set_shared(const gs_hermite* h, int mode, bool phi, A& a) {
  a.X = static_cast<S*>(h->X); a.V = static_cast<S*>(h->V);
  a.A = static_cast<S*>(h->A); a.J = static_cast<S*>(h->J);
  a.XP = static_cast<P*>(h->XP); a.VP = static_cast<P*>(h->VP);
  a.PA = static_cast<P*>(h->PA); a.PJ = static_cast<P*>(h->PJ);
  a.a_out = static_cast<S*>(h->a_out); a.j_out = static_cast<S*>(h->j_out);
  a.ctrl = h->ctrl;
  a.wgmin = h->wgmin;
  a.n_real = h->n; a.n_pad = h->n_pad; a.chunk = h->chunk; a.n_chunks = h->n_chunks;
  a.mode = mode;
  a.phi = phi ? 1 : 0;
  a.cut2 = (P)(h->cfg.cutoff * h->cfg.cutoff);
  a.eps2 = (P)(h->cfg.softening * h->cfg.softening);
  a.blk = h->blk;
}

// Order 4 (T the pair type, S the state type) and order 6.
template <typename T, typename S>
void set_args(const gs_hermite* h, int mode, bool phi, gs::HArgs<T, S>& a) {
  set_shared<T, S>(h, mode, phi, a);
  a.XL = static_cast<T*>(h->XL);
  a.nn = h->nn ? 1 : 0;
  a.R = static_cast<S*>(h->R);
  a.PN = h->PN; a.NNI = h->NNI;
  a.nn_q = h->nn_q; a.nn_i = h->nn_i; a.ca_q = h->ca_q; a.ca_i = h->ca_i;
  a.q_out = h->q_out; a.nn_out = h->nn_out;
  a.row0 = h->row0; a.n_loc = h->n_loc;
}

template <typename T>
void set_args(const gs_hermite* h, int mode, bool phi, gs::H6Args<T>& a) {
  set_shared<T, T>(h, mode, phi, a);
  a.S = static_cast<T*>(h->S); a.C = static_cast<T*>(h->C);
  a.AP = static_cast<T*>(h->AP); a.PS = static_cast<T*>(h->PS);
  a.s_out = static_cast<T*>(h->s_out);
  a.NS = static_cast<T*>(h->NS);
}

template <typename A>
A make_args(const gs_hermite* h, int mode, bool phi) {
  A a{};
  set_args(h, mode, phi, a);
  return a;
}

// f(the kernel arguments of the run's precision and order): HArgs<T, S>, or H6Args<T> for a run
// of order 6 (fp32 or fp64: refuse6).
template <typename F>
int with_args(const gs_hermite* h, int mode, bool phi, F f) {
  if (h->order == 6)
    return h->esz == 4 ? f(make_args<gs::H6Args<float>>(h, mode, phi))
                       : f(make_args<gs::H6Args<double>>(h, mode, phi));
  return by_dtype(h, [&](auto t, auto s) {
    return f(make_args<gs::HArgs<decltype(t), decltype(s)>>(h, mode, phi));
  });
}

// The kernel arguments of order 6; and of order 6 in fp32, which has no block steps (refuse6
// R6_BLOCK6 keeps them from being switched on, so what asks this never runs).
template <typename A> struct is_six : std::false_type {};
template <typename T> struct is_six<gs::H6Args<T>> : std::true_type {};
template <typename A> constexpr bool kNoBlock = std::is_same<A, gs::H6Args<float>>::value;

// The four launches of a shared step, by the type of the kernel arguments.
template <typename T, typename S>
hipError_t launch_ctrl(const gs::HArgs<T, S>& a, hipStream_t s) {
  return gs::launch_hermite_ctrl<T, S>(a, s);
}
template <typename T, typename S>
hipError_t launch_predict(const gs::HArgs<T, S>& a, hipStream_t s) {
  return gs::launch_hermite_predict<T, S>(a, s);
}
template <typename T, typename S>
hipError_t launch_eval(const gs::HArgs<T, S>& a, int ipl, int groups, bool gated, hipStream_t s) {
  return gs::launch_hermite_eval<T, S>(a, ipl, groups, gated, s);
}
template <typename T, typename S>
hipError_t launch_reduce(const gs::HArgs<T, S>& a, hipStream_t s) {
  return gs::launch_hermite_reduce<T, S>(a, s);
}
template <typename T>
hipError_t launch_ctrl(const gs::H6Args<T>& a, hipStream_t s) {
  return gs::launch_hermite_ctrl<T, T>(gs::base_view(a), s);  // (order 4's control kernel)
}
template <typename T>
hipError_t launch_predict(const gs::H6Args<T>& a, hipStream_t s) {
  return gs::launch_hermite6_predict<T>(a, s);
}
template <typename T>
hipError_t launch_eval(const gs::H6Args<T>& a, int ipl, int groups, bool gated, hipStream_t s) {
  return gs::launch_hermite6_eval<T>(a, ipl, groups, gated, s);
}
template <typename T>
hipError_t launch_reduce(const gs::H6Args<T>& a, hipStream_t s) {
  return gs::launch_hermite6_reduce<T>(a, s);
}

int read_ctrl(gs_hermite* h, gs::HermiteCtrl* c);

// Launch shape (any choice gives the same bits): the widest lane tile that still leaves about
// four workgroups per CU, then as many chunk groups as reach that count. Order 4: mixed
// precision with collisions on has no 4-body tile (it would need all 256 VGPRs): 2 bodies per
// lane there, also where the configuration asks for 4, and the layout reports what runs.
// Order 6 is built with 1 or (fp32) 2 bodies per lane.
int launch_shape(gs_hermite* h) {
  const int fp64 = h->cfg.dtype == GS_FP64;
  const bool six = h->order == 6;
  const int top = six ? (fp64 ? 1 : 2) : (fp64 || (is_mixed(h) && h->nn) ? 2 : 4);
  const int low = six || fp64 ? 1 : 2;  // (the automatic choice goes no narrower)
  const int64_t want = 1024;
  int ipl = h->cfg.ipl;
  if (ipl == 0) {
    ipl = top;
    while (ipl > low && h->n_loc / (gs::kForceBlock * ipl) * h->n_chunks < want) ipl >>= 1;
  }
  if (!(six ? gs::hermite6_ipl_ok(fp64, ipl) : gs::hermite_ipl_ok(fp64, ipl)) ||
      h->n_loc % (gs::kForceBlock * ipl)) {
    gs_set_error(six ? "hermite order 6: ipl must be 1 (or 2 for fp32)"
                     : "hermite: ipl must be 1, 2 (or 4 for fp32 and mixed)");
    return -1;
  }
  if (ipl > top) ipl = top;
  h->ipl = ipl;
  const int64_t blocks = h->n_loc / (gs::kForceBlock * ipl);  // (of the rows this rank owns)
  int64_t groups =
      h->cfg.split_groups > 0 ? h->cfg.split_groups : (2 * want + blocks - 1) / blocks;
  if (groups > h->n_chunks) groups = h->n_chunks;
  if (groups < 1) groups = 1;
  h->groups = (int32_t)groups;
  return 0;
}

// Write the control block for a run that stands at time t (stream-ordered).
int write_ctrl(gs_hermite* h, double t, uint64_t steps, double dt_last, double dt_min,
               unsigned long long overlaps) {
  gs::HermiteCtrl c{};
  c.overlaps = overlaps;
  c.ov_stop = h->nn == 2 ? 1 : 0;
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

// The engine's settings changed: rewrite the control block where the run stands. overlaps < 0:
// the overlap count stays as it is.
int update_ctrl(gs_hermite* h, int64_t overlaps = -1) {
  gs::HermiteCtrl c;
  if (read_ctrl(h, &c)) return -1;
  return write_ctrl(h, c.t, c.steps, c.dt_last, c.dt_min,
                    overlaps < 0 ? c.overlaps : (unsigned long long)overlaps);
}

// The evaluate kernels read the current (x, v) instead of a predicted state: in place, or
// (mixed) through the split of X, V into the fp32 rows.
template <typename T, typename S>
int point_at_current(gs_hermite* h, gs::HArgs<T, S>& a) {
  if (a.nn) {  // (the radii ride in the VP rows)
    GS_HIP((gs::launch_hermite_stage<T, S>(a, h->stream)));
    return 0;
  }
  if constexpr (sizeof(T) == sizeof(S)) {
    a.XP = a.X;
    a.VP = a.V;
  } else {
    GS_HIP(gs::launch_hermite_split(a, h->stream));
  }
  return 0;
}

template <typename T>
int point_at_current(gs_hermite*, gs::H6Args<T>& a) {
  a.XP = a.X;
  a.VP = a.V;
  return 0;
}

// Derivatives of the current (x, v) through the step's own kernel, then the reduce in a.mode
// (HM_INIT: into the carried rows, and the first step's minima; HM_OUT: the outputs).
template <typename A>
int eval_current(gs_hermite* h, A a) {
  if (point_at_current(h, a)) return -1;
  if constexpr (is_six<A>::value) {
    // Order 6 takes two passes: this one with ap = 0 gives a (and j), the one below with ap = a
    // gives s (and phi where asked).
    A first = a;
    first.phi = 0;
    GS_HIP(hipMemsetAsync(h->AP, 0, rows_bytes(h), h->stream));
    GS_HIP(launch_eval(first, h->ipl, h->groups, false, h->stream));
    GS_HIP(launch_reduce(first, h->stream));
    GS_HIP(hipMemcpyAsync(h->AP, a.mode == gs::HM_INIT ? h->A : h->a_out, rows_bytes(h),
                          hipMemcpyDeviceToDevice, h->stream));
  }
  GS_HIP(launch_eval(a, h->ipl, h->groups, false, h->stream));
  GS_HIP(launch_reduce(a, h->stream));
  return 0;
}

// What order 6 does not run with, each stated once: the settings of the engine itself, then
// what a caller is about to switch on (`asked`). Null: nothing stands in the way.
enum { R6_NONE, R6_BLOCK, R6_BLOCK6, R6_NN, R6_GROUP };
const char* refuse6(const gs_hermite* h, int asked = R6_NONE) {
  if (multi(h)) return "hermite order 6 runs on one rank (nranks > 1, --gpus, is refused)";
  if (h->cfg.dtype == GS_MIXED)
    return "hermite order 6 has no mixed precision (GS_MIXED, --dtype mixed, is refused)";
  // (block mode that gs_hermite_set_block switched on is order 4's)
  if ((h->block && h->order != 6) || asked == R6_BLOCK)
    return "hermite order 6 has no block steps through gs_hermite_set_block (--block-steps): its "
           "own are gs_hermite_set_block6 (--block-steps6), in fp64";
  if (asked == R6_BLOCK6 && h->cfg.dtype != GS_FP64)
    return "hermite order 6 runs block steps (gs_hermite_set_block6, --block-steps6) in fp64 only: "
           "fp32 pair arithmetic collapses its step criterion (fp32 with block steps is refused)";
  if (h->nn || asked == R6_NN)
    return "hermite order 6 has no collisions (gs_hermite_set_collisions, --collisions)";
  if (asked == R6_GROUP)
    return "hermite group: order 6 runs on one rank (no virtual group, gs_hermite_group_*)";
  return nullptr;
}

// ---- ranks -----------------------------------------------------------------------------
// The arrays a multi-rank run gathers: base address and bytes per ownership unit.
enum { G_XP, G_VP, G_XL, G_X, G_V, G_A, G_J, G_AOUT, G_JOUT, G_WGMIN };

char* gbuf(gs_hermite* h, int w, size_t* ub) {
  const size_t rs = (size_t)kUnit * 4 * h->esz, rp = (size_t)kUnit * 4 * h->psz;
  void* p = nullptr;
  switch (w) {
    case G_XP: *ub = rp; p = h->XP; break;
    case G_VP: *ub = rp; p = h->VP; break;
    case G_XL: *ub = rp; p = h->XL; break;
    case G_X: *ub = rs; p = h->X; break;
    case G_V: *ub = rs; p = h->V; break;
    case G_A: *ub = rs; p = h->A; break;
    case G_J: *ub = rs; p = h->J; break;
    case G_AOUT: *ub = rs; p = h->a_out; break;
    case G_JOUT: *ub = rs; p = h->j_out; break;
    default: *ub = (size_t)(kUnit / gs::kForceBlock) * sizeof(double); p = h->wgmin; break;
  }
  return static_cast<char*>(p);
}

bool abort_comm(gs_hermite* h) {
  ncclComm_t c = h->comm_live.exchange(nullptr);
  if (!c) return false;
  (void)ncclCommAbort(c);
  return true;
}

// One rank's gather over RCCL, in place on the engine's stream: ncclAllGather for equal slices,
// else every rank broadcasts its own slice, all P in one group call (as gather() of the stepper).
int gather_comm(gs_hermite* h, int w) {
  if (h->comm_live.load() == nullptr) {
    gs_set_error("hermite: this rank of a multi-rank run has no live communicator "
                 "(gs_hermite_comm_init) and is no shard of a gs_hermite_group_* call");
    return -1;
  }
  size_t ub = 0;
  char* buf = gbuf(h, w, &ub);
  const int P = h->cfg.nranks, r = h->cfg.rank;
  if (h->uniform) {
    GS_NCCL(ncclAllGather(buf + (size_t)h->ubeg[r] * ub, buf, (size_t)h->ucnt[r] * ub, ncclChar,
                          h->comm, h->stream));
    return 0;
  }
  GS_NCCL(ncclGroupStart());
  for (int q = 0; q < P; ++q) {
    char* sl = buf + (size_t)h->ubeg[q] * ub;
    GS_NCCL(ncclBroadcast(sl, sl, (size_t)h->ucnt[q] * ub, ncclChar, q, h->comm, h->stream));
  }
  GS_NCCL(ncclGroupEnd());
  return 0;
}

// The shards of a virtual group: every shard's stream waits until the others' rows are ready,
// then copies their slices into its own arrays.
int gather_group(gs_hermite* const* sh, int P, std::initializer_list<int> ws) {
  for (int r = 0; r < P; ++r) GS_HIP(hipEventRecord(sh[r]->ev, sh[r]->stream));
  for (int d = 0; d < P; ++d)
    for (int q = 0; q < P; ++q)
      if (q != d) GS_HIP(hipStreamWaitEvent(sh[d]->stream, sh[q]->ev, 0));
  for (int w : ws)
    for (int d = 0; d < P; ++d)
      for (int q = 0; q < P; ++q) {
        if (q == d) continue;
        size_t ub = 0;
        char* dst = gbuf(sh[d], w, &ub);
        const char* src = gbuf(sh[q], w, &ub);
        const size_t off = (size_t)sh[d]->ubeg[q] * ub;
        GS_HIP(hipMemcpyAsync(dst + off, src + off, (size_t)sh[d]->ucnt[q] * ub,
                              hipMemcpyDeviceToDevice, sh[d]->stream));
      }
  return 0;
}

// Gather the listed arrays: nothing on one rank, RCCL for a lone rank of P, copies for a group.
int gather(gs_hermite* const* sh, int P, std::initializer_list<int> ws) {
  if (P > 1) return gather_group(sh, P, ws);
  if (!multi(sh[0])) return 0;
  for (int w : ws)
    if (gather_comm(sh[0], w)) return -1;
  return 0;
}

// shards[r] is rank r of P of one run on one device (or: one engine, whatever its rank).
int check_group(gs_hermite* const* sh, int P) {
  if (!sh || P < 1) { gs_set_error("hermite group: bad arguments"); return -1; }
  for (int r = 0; r < P; ++r)
    if (!sh[r]) { gs_set_error("hermite group: null shard"); return -1; }
  for (int r = 0; r < P; ++r)
    if (sh[r]->order == 6) {
      gs_set_error(refuse6(sh[r], R6_GROUP));
      return -1;
    }
  if (P == 1) return 0;
  for (int r = 0; r < P; ++r) {
    const gs_hermite* h = sh[r];
    if (h->cfg.nranks != P || h->cfg.rank != r) {
      gs_set_error("hermite group: shards[r] must be rank r of P (shards out of order, or "
                   "created for another P)");
      return -1;
    }
    if (h->n != sh[0]->n || h->chunk != sh[0]->chunk || h->cfg.dtype != sh[0]->cfg.dtype ||
        h->cfg.device != sh[0]->cfg.device || h->comm_live.load() != nullptr) {
      gs_set_error("hermite group: the shards differ in n, chunk, dtype or device, or hold a "
                   "communicator");
      return -1;
    }
  }
  return 0;
}

// The first step minima of a group whose shards had their states set one by one.
int close_wgmin(gs_hermite* const* sh, int P) {
  bool open = false;
  for (int r = 0; r < P; ++r) open = open || sh[r]->wgmin_open;
  if (!open) return 0;
  if (gather(sh, P, {G_WGMIN})) return -1;
  for (int r = 0; r < P; ++r) sh[r]->wgmin_open = false;
  return 0;
}

int wait_seen(gs_hermite* h, int64_t target);

// nsteps shared steps of the P shards; A: the kernel arguments (with_args; order 6: P is 1).
template <typename A>
int step_t(gs_hermite* const* sh, int P, int32_t nsteps) {
  if (close_wgmin(sh, P)) return -1;
  std::vector<A> a;
  for (int r = 0; r < P; ++r) a.push_back(make_args<A>(sh[r], gs::HM_STEP, false));
  const bool mixed = is_mixed(sh[0]);
  for (int32_t k = 0; k < nsteps; ++k) {
    for (int r = 0; r < P; ++r) {
      GS_HIP(launch_ctrl(a[r], sh[r]->stream));
      GS_HIP(launch_predict(a[r], sh[r]->stream));
    }
    // (the same collectives on every rank whatever ctrl->active is: a chain past t_end gathers
    // stale rows and changes nothing)
    if (mixed ? gather(sh, P, {G_XP, G_VP, G_XL}) : gather(sh, P, {G_XP, G_VP})) return -1;
    for (int r = 0; r < P; ++r) {
      GS_HIP(launch_eval(a[r], sh[r]->ipl, sh[r]->groups, true, sh[r]->stream));
      GS_HIP(launch_reduce(a[r], sh[r]->stream));
    }
    if (gather(sh, P, {G_WGMIN})) return -1;
    gs_hermite* h = sh[0];
    if (P == 1 && !h->ring.empty()) {  // (an RCCL run: the progress record of the bounded waits)
      const int64_t cap = (int64_t)h->ring.size();
      if (h->rec - h->seen == cap && wait_seen(h, h->seen + 1)) return -1;
      GS_HIP(hipEventRecord(h->ring[(size_t)(h->rec % cap)], h->stream));
      h->rec += 1;
    }
  }
  return 0;
}

// Host fp64 (n x 3 [+ w]) -> device state rows of 4 (ghost rows zero).
int upload_rows(gs_hermite* h, void* dst, const double* src3, const double* w, double wscale) {
  return by_state(h, [&](auto s) {
    using T = decltype(s);
    std::vector<T> buf((size_t)h->n_pad * 4, T(0));
    for (int64_t i = 0; i < h->n; ++i) {
      for (int d = 0; d < 3; ++d) buf[4 * i + d] = (T)src3[3 * i + d];
      if (w) buf[4 * i + 3] = (T)(wscale * w[i]);
    }
    GS_HIP(hipMemcpyAsync(dst, buf.data(), rows_bytes(h), hipMemcpyHostToDevice, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

// The first `comps` components of `rows` device state rows -> host fp64 (out null: nothing).
int download_rows(gs_hermite* h, const void* src, int64_t rows, double* out, int comps) {
  if (!out) return 0;
  return by_state(h, [&](auto s) {
    using T = decltype(s);
    std::vector<T> buf((size_t)rows * 4);
    GS_HIP(hipMemcpyAsync(buf.data(), src, (size_t)rows * 4 * sizeof(T), hipMemcpyDeviceToHost,
                          h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < rows; ++i)
      for (int d = 0; d < comps; ++d) out[comps * i + d] = (double)buf[4 * i + d];
    return 0;
  });
}

// The first `rows` entries of a (q, neighbour) pair of device arrays (a null output: skipped).
int download_pair(gs_hermite* h, const double* dq, const int32_t* di, int64_t rows, double* q,
                  int32_t* nn) {
  if (q)
    GS_HIP(hipMemcpyAsync(q, dq, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (nn)
    GS_HIP(hipMemcpyAsync(nn, di, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost,
                          h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// Two events around a stretch of a stream's work; destroyed on every way out of the scope.
struct EventTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  int create() {
    GS_HIP(hipEventCreate(&e0));
    GS_HIP(hipEventCreate(&e1));
    return 0;
  }
  int start(hipStream_t s) {
    GS_HIP(hipEventRecord(e0, s));
    return 0;
  }
  // Waits for the stretch to end; *ms: its milliseconds.
  int stop(hipStream_t s, double* ms) {
    float t = 0.0f;
    GS_HIP(hipEventRecord(e1, s));
    GS_HIP(hipEventSynchronize(e1));
    GS_HIP(hipEventElapsedTime(&t, e0, e1));
    *ms = (double)t;
    return 0;
  }
};

// The per-body records of a run that starts: no neighbour yet, no approach.
int clear_records(gs_hermite* h, bool latest) {
  if (!h->nn) return 0;
  const std::vector<double> inf((size_t)h->n_pad, std::numeric_limits<double>::infinity());
  const std::vector<int32_t> none((size_t)h->n_pad, -1);
  for (int k = latest ? 0 : 1; k < 2; ++k) {
    GS_HIP(hipMemcpyAsync(k ? h->ca_q : h->nn_q, inf.data(), inf.size() * sizeof(double),
                          hipMemcpyHostToDevice, h->stream));
    GS_HIP(hipMemcpyAsync(k ? h->ca_i : h->nn_i, none.data(), none.size() * sizeof(int32_t),
                          hipMemcpyHostToDevice, h->stream));
  }
  GS_HIP(hipStreamSynchronize(h->stream));  // (the vectors are on this frame)
  return 0;
}

using gs::rt::DevMem;

// A buffer of group g with every byte set to `fill`, on the engine's stream.
template <typename T>
int dev_buf(gs_hermite* h, DevMem& g, T** slot, size_t bytes, const char* tag, int fill = 0) {
  if (g.alloc(slot, bytes, tag)) return -1;
  GS_HIP(hipMemsetAsync(*slot, fill, bytes, h->stream));
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

// ---- block time steps ------------------------------------------------------------------

int read_bctrl(gs_hermite* h, gs::HermiteBlockCtrl* c) {
  GS_HIP(hipMemcpyAsync(c, h->blk.bc, sizeof(*c), hipMemcpyDeviceToHost, h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int write_bctrl(gs_hermite* h, const gs::HermiteBlockCtrl& c) {
  GS_HIP(hipMemcpyAsync(h->blk.bc, &c, sizeof(c), hipMemcpyHostToDevice, h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));  // (c may be on the caller's frame)
  return 0;
}

// The default narrow_max for n_pad bodies (a function of n and dtype only: it changes bits).
int32_t default_narrow_max(const gs_hermite* h) {
  // The measured crossover of the two evaluate paths, down to a power of two (docs/DESIGN.md
  // §15): 4096 (fp32) and 2048 (fp64) at 65,536 bodies, 32,768 for both at 262,144. Between and
  // beyond the measured sizes: n_pad / 8 from 262,144 up, n_pad / 16 (fp32), / 32 (fp64) below.
  // Mixed (§16): 8192 at 65,536 and 32,768 at 262,144, n_pad / 8 at both and elsewhere (its wide
  // path pays a third LDS read per j, its narrow path only one more coalesced load).
  // Order 6 (fp64; §23): 4096 at 65,536 and 32,768 at 262,144 (profiles/hermite6_block_sweep.json),
  // n_pad / 16 and n_pad / 8; the same rule between and beyond the two measured sizes.
  const int64_t div = h->n_pad >= 262144 || is_mixed(h) ? 8
                      : h->order == 6 ? 16 : (h->esz == 4 ? 16 : 32);
  int64_t d = 1;
  while (2 * d <= h->n_pad / div) d *= 2;
  return (int32_t)d;
}

// The control block's narrow_max follows the host's.
int push_narrow_max(gs_hermite* h) {
  gs::HermiteBlockCtrl c;
  if (read_bctrl(h, &c)) return -1;
  c.narrow_max = h->narrow_max;
  return write_bctrl(h, c);
}

// The partials of the narrow path for `cap` slots (0 outside block mode), the one place that
// sizes them: acceleration and jerk, the snap for order 6, the neighbour where collisions (`nn`)
// are on. A resize that fails leaves no slots, on the host and in the control block: every step
// then takes the wide path.
int size_narrow(gs_hermite* h, int32_t cap, bool nn) {
  const size_t slots = (size_t)h->blk.n_slices * (size_t)cap, bytes = slots * 4 * h->psz;
  const int rc = h->narrow.rebuild([&](DevMem& g) {
    return cap > 0 && (g.alloc(&h->blk.NA, bytes, "NA") || g.alloc(&h->blk.NJ, bytes, "NJ") ||
                       (h->order == 6 && g.alloc(&h->NS, bytes, "NS")) ||
                       (nn && g.alloc(&h->NNI, slots * sizeof(int32_t), "NNI")));
  });
  h->blk.cap = h->narrow_max = rc ? 0 : cap;
  if (rc && h->blk.bc) (void)push_narrow_max(h);  // (it sets no error unless it fails itself)
  return rc;
}

// Block mode off: the narrow slots and the block arrays go.
void drop_block(gs_hermite* h) {
  (void)size_narrow(h, 0, false);
  h->blockg.release();
  h->blk = gs::HBlock{};
  h->block = false;
}

// Narrow partials for narrow_max slots (< 0: the default), and the control block told.
int set_narrow(gs_hermite* h, int32_t narrow_max) {
  if (narrow_max < 0) narrow_max = default_narrow_max(h);
  if (narrow_max > h->n_pad) narrow_max = (int32_t)h->n_pad;
  GS_HIP(hipStreamSynchronize(h->stream));
  if (size_narrow(h, narrow_max, h->nn != 0)) return -1;
  return push_narrow_max(h);
}

// Control block of a block run that stands at `macro` whole steps of dt, counters zero.
int reset_bctrl(gs_hermite* h, int64_t macro) {
  gs::HermiteBlockCtrl c{};
  c.t_ticks = macro << h->max_level;
  c.target = c.t_ticks;
  c.dt_max = h->cfg.dt;
  c.eta = h->eta;
  c.L = h->max_level;
  c.narrow_max = h->narrow_max;
  h->macro0 = macro;
  return write_bctrl(h, c);
}

template <typename T, typename S>
int block_start_t(gs_hermite* h, int64_t macro) {
  if (reset_bctrl(h, macro)) return -1;
  const gs::HArgs<T, S> a = make_args<gs::HArgs<T, S>>(h, gs::HM_STEP, false);
  GS_HIP((gs::launch_block_init<T, S>(a, macro << h->max_level, h->stream)));
  return 0;
}

// Levels afresh from the carried a, j; every body stands at `macro` steps of dt.
int block_start(gs_hermite* h, int64_t macro) {
  return by_dtype(h, [&](auto t, auto s) {
    return block_start_t<decltype(t), decltype(s)>(h, macro);
  });
}

// One block step of either order: next + control, predict-all + mark + compact, narrow, wide,
// correct (the overloads of gs_hermite.h).
template <typename A>
int block_chain(gs_hermite* h, const A& a) {
  if constexpr (kNoBlock<A>) {
    gs_set_error(refuse6(h, R6_BLOCK6));
    return -1;
  } else {
    GS_HIP(gs::launch_block_next(a, h->stream));
    GS_HIP(gs::launch_block_predict(a, h->stream));
    GS_HIP(gs::launch_block_narrow(a, h->stream));
    GS_HIP(gs::launch_block_wide(a, h->ipl, h->groups, h->stream));
    GS_HIP(gs::launch_block_correct(a, h->stream));
    return 0;
  }
}

// n macro steps: chains in batches of 32 against the device-side target, one status read each.
// A: the kernel arguments of the run's precision and order (with_args).
template <typename A>
int block_step_t(gs_hermite* h, int32_t nsteps) {
  gs::HermiteBlockCtrl c;
  if (read_bctrl(h, &c)) return -1;
  const int L = h->max_level;
  int64_t target = ((c.t_ticks >> L) + nsteps) << L;
  if (h->has_end) {
    const int64_t end = (int64_t)llround(h->t_end / h->cfg.dt) << L;
    if (target > end) target = end;
  }
  if (target <= c.t_ticks) return 0;
  c.target = target;
  if (write_bctrl(h, c)) return -1;
  const A a = make_args<A>(h, gs::HM_STEP, false);
  while (c.t_ticks < target) {
    const int64_t before = c.t_ticks;
    for (int k = 0; k < 32; ++k)
      if (block_chain(h, a)) return -1;
    if (read_bctrl(h, &c)) return -1;
    if (c.t_ticks == before) {
      gs_set_error("hermite block steps: no progress (body times out of step)");
      return -1;
    }
  }
  return 0;
}

// Derivatives of the listed bodies at the current state through one block path's evaluate and
// correct (a: HM_OUT with the potential), `reps` times between two events where ms is asked. The
// block control is put back as it was. Order 6: one pass at the rows (x, v, carried a), and the
// snap where asked.
template <typename A>
int derivs_active(gs_hermite* h, A a, const int32_t* idx, int32_t n_idx, int32_t path, int32_t reps,
                  double* ms, double* acc4, double* jerk4, double* snap4, double* q, int32_t* nn) {
  if constexpr (kNoBlock<A>) {
    gs_set_error(refuse6(h, R6_BLOCK6));
    return -1;
  } else {
    gs::HermiteBlockCtrl keep;
    if (read_bctrl(h, &keep)) return -1;
    gs::HermiteBlockCtrl c = keep;
    c.n_act = n_idx;
    c.path = path;
    c.active = 1;
    GS_HIP(hipMemcpyAsync(h->blk.list, idx, (size_t)n_idx * sizeof(int32_t),
                          hipMemcpyHostToDevice, h->stream));
    if (write_bctrl(h, c)) return -1;
    if (point_at_current(h, a)) return -1;
    if constexpr (is_six<A>::value) a.AP = a.A;
    EventTimer timer;
    if (ms && (timer.create() || timer.start(h->stream))) return -1;
    for (int32_t r = 0; r < reps; ++r) {
      if (path == gs::HP_NARROW)
        GS_HIP(gs::launch_block_narrow(a, h->stream));
      else
        GS_HIP(gs::launch_block_wide(a, h->ipl, h->groups, h->stream));
      GS_HIP(gs::launch_block_correct(a, h->stream));
    }
    if (ms) {
      if (timer.stop(h->stream, ms)) return -1;
      *ms /= reps;
    }
    if (download_rows(h, h->a_out, n_idx, acc4, 4) || download_rows(h, h->j_out, n_idx, jerk4, 4) ||
        (h->order == 6 && download_rows(h, h->s_out, n_idx, snap4, 4)) ||
        ((q || nn) && download_pair(h, h->q_out, h->nn_out, n_idx, q, nn)))
      return -1;
    return write_bctrl(h, keep);
  }
}

// The arrays order 6 adds to the run's (snap and crackle rows, the predicted acceleration, the
// snap output, the snap partials), zeroed but for the partials (a row per chunk, written before
// they are read): they exist exactly while the order is 6.
int fill_order6(gs_hermite* h, DevMem& g) {
  const size_t rb = rows_bytes(h);
  if (dev_buf(h, g, &h->S, rb, "S") || dev_buf(h, g, &h->C, rb, "C") ||
      dev_buf(h, g, &h->AP, rb, "AP") || dev_buf(h, g, &h->s_out, rb, "s_out") ||
      g.alloc(&h->PS, rb * (size_t)h->n_chunks, "PS"))
    return -1;
  GS_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// The state rows a run carries from step to step beside x, v: (A, J), order 6 (A, J, S, C).
std::vector<void*> carried_rows(const gs_hermite* h) {
  if (h->order == 6) return {h->A, h->J, h->S, h->C};
  return {h->A, h->J};
}

int start_from_state(gs_hermite* h) {
  if (write_ctrl(h, 0.0, 0, 0.0, std::numeric_limits<double>::infinity(), 0)) return -1;
  if (clear_records(h, true)) return -1;
  if (with_args(h, gs::HM_INIT, false, [&](auto a) { return eval_current(h, a); })) return -1;
  if (multi(h)) {
    // every rank holds all of x, v (uploaded or generated whole), so only the step minima of
    // the other ranks' rows are missing: gathered now (RCCL), or by the group's next call
    if (h->comm_live.load() != nullptr) {
      if (gather_comm(h, G_WGMIN)) return -1;
    } else {
      h->wgmin_open = true;
    }
  }
  return h->block ? block_start(h, 0) : 0;
}

// Bounded wait of an RCCL run for its chain number `target` (see gs_hermite_sync).
int wait_seen(gs_hermite* h, int64_t target) {
  using clock = std::chrono::steady_clock;
  auto last = clock::now();
  const int64_t cap = (int64_t)h->ring.size();
  while (h->seen < target) {
    const hipError_t e = hipEventQuery(h->ring[(size_t)(h->seen % cap)]);
    if (e == hipSuccess) {
      h->seen += 1;
      last = clock::now();
      continue;
    }
    if (e != hipErrorNotReady) GS_HIP(e);
    if (gs_hermite_comm_check(h)) return -1;
    if (h->step_timeout_s > 0.0 &&
        std::chrono::duration<double>(clock::now() - last).count() > h->step_timeout_s) {
      abort_comm(h);
      gs_set_error("hermite: no step completed within the step timeout; RCCL communicator "
                   "aborted");
      return -1;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
  return 0;
}

int get_state_group(gs_hermite* const* sh, int P, double* pos, double* vel, double* mass,
                    double* acc, double* jerk) {
  gs_hermite* h = sh[0];
  GS_HIP(hipSetDevice(h->cfg.device));
  if (gather(sh, P, {G_X, G_V, G_A, G_J})) return -1;
  const std::pair<const void*, double*> rows[4] = {{h->X, pos}, {h->V, vel}, {h->A, acc},
                                                   {h->J, jerk}};
  for (const auto& r : rows)
    if (download_rows(h, r.first, h->n, r.second, 3)) return -1;
  if (mass)
    for (int64_t i = 0; i < h->n; ++i) mass[i] = h->mass_host[(size_t)i];
  for (int r = 1; r < P; ++r) GS_HIP(hipStreamSynchronize(sh[r]->stream));
  return 0;
}

// snap4: order 6 only (null otherwise).
int derivs_group(gs_hermite* const* sh, int P, double* acc4, double* jerk4, double* snap4,
                 double* q, int32_t* nn) {
  gs_hermite* h = sh[0];
  GS_HIP(hipSetDevice(h->cfg.device));
  if (gather(sh, P, {G_X, G_V})) return -1;  // (each rank's corrector moved its own rows only)
  for (int r = 0; r < P; ++r)
    if (with_args(sh[r], gs::HM_OUT, true, [&](auto a) { return eval_current(sh[r], a); }))
      return -1;
  if (gather(sh, P, {G_AOUT, G_JOUT})) return -1;
  if (download_rows(h, h->a_out, h->n, acc4, 4) || download_rows(h, h->j_out, h->n, jerk4, 4) ||
      (h->order == 6 && download_rows(h, h->s_out, h->n, snap4, 4)))
    return -1;
  for (int r = 1; r < P; ++r) GS_HIP(hipStreamSynchronize(sh[r]->stream));
  return q || nn ? download_pair(h, h->q_out, h->nn_out, h->n, q, nn) : 0;
}

// Milliseconds per evaluate launch at the engine's current predicted rows.
template <typename T, typename S>
int time_eval_t(gs_hermite* h, int32_t reps, double* ms) {
  const gs::HArgs<T, S> a = make_args<gs::HArgs<T, S>>(h, gs::HM_STEP, false);
  EventTimer timer;
  if (timer.create()) return -1;
  GS_HIP((gs::launch_hermite_eval<T, S>(a, h->ipl, h->groups, false, h->stream)));  // warm
  if (timer.start(h->stream)) return -1;
  for (int32_t k = 0; k < reps; ++k)
    GS_HIP((gs::launch_hermite_eval<T, S>(a, h->ipl, h->groups, false, h->stream)));
  if (timer.stop(h->stream, ms)) return -1;
  *ms /= reps;
  return 0;
}

// The one implementation behind gs_hermite_set_state and gs_hermite_set_state6. given: the
// carried rows the caller has, in the order of carried_rows(); with every one of the run's
// order the run resumes, else its derivatives start afresh.
int set_state(gs_hermite* h, const double* pos, const double* vel, const double* mass,
              std::initializer_list<const double*> given, double t, double dt_next,
              double dt_min) {
  GS_HIP(hipSetDevice(h->cfg.device));
  if (upload_rows(h, h->X, pos, mass, h->cfg.G) || upload_rows(h, h->V, vel, nullptr, 0.0))
    return -1;
  h->mass_host.assign(mass, mass + h->n);
  // block mode: the run stands at a whole number of steps of dt (a synchronised state)
  const int64_t macro = h->block ? (int64_t)llround(t / h->cfg.dt) : 0;
  if (h->block && (double)macro * h->cfg.dt != t) {
    gs_set_error("hermite block steps: the state's time must be a whole multiple of dt");
    return -1;
  }
  const double inf = std::numeric_limits<double>::infinity();
  const std::vector<void*> rows = carried_rows(h);
  bool all = true;
  for (size_t k = 0; k < rows.size(); ++k) all = all && given.begin()[k];
  if (!all) {
    if (start_from_state(h)) return -1;
    if (h->block && block_start(h, macro)) return -1;
    gs::HermiteCtrl c;
    if (read_ctrl(h, &c)) return -1;  // (also waits for the evaluation)
    return write_ctrl(h, t, 0, 0.0, dt_min > 0.0 ? dt_min : inf, c.overlaps);
  }
  // A resumed run: the carried rows as the last step left them, and the step size its criterion
  // chose.
  if (clear_records(h, true)) return -1;
  for (size_t k = 0; k < rows.size(); ++k)
    if (upload_rows(h, rows[k], given.begin()[k], nullptr, 0.0)) return -1;
  if (set_wgmin(h, dt_next > 0.0 ? dt_next : inf)) return -1;
  if (h->block && block_start(h, macro)) return -1;  // (levels afresh until set_block_state)
  return write_ctrl(h, t, 0, 0.0, dt_min > 0.0 ? dt_min : inf, 0);
}

}  // namespace

extern "C" {

int gs_hermite_create(const gs_config* cfg, gs_hermite** out) {
  if (!cfg || !out) { gs_set_error("hermite: null argument"); return -1; }
  if (cfg->nranks < 1 || cfg->rank < 0 || cfg->rank >= cfg->nranks) {
    gs_set_error("hermite: bad rank/nranks");
    return -1;
  }
  if (cfg->n < 1) { gs_set_error("hermite: n must be >= 1"); return -1; }
  if (!(cfg->dt > 0.0)) { gs_set_error("hermite: dt must be > 0"); return -1; }
  if (!(cfg->cutoff > 0.0) && !(cfg->softening > 0.0)) {
    gs_set_error("hermite: cutoff and softening cannot both be 0 (the self term)");
    return -1;
  }
  if (cfg->dtype != GS_FP32 && cfg->dtype != GS_FP64 && cfg->dtype != GS_MIXED) {
    gs_set_error("hermite: dtype must be GS_FP32, GS_FP64 or GS_MIXED");
    return -1;
  }
  const int fp64 = cfg->dtype == GS_FP64;  // (the pair kernels': mixed takes fp32's launch shape)
  const int32_t chunk = cfg->chunk > 0 ? cfg->chunk : gs::auto_chunk(cfg->n);
  if (chunk % 1024) { gs_set_error("hermite: chunk must be a multiple of 1024"); return -1; }
  // (a half-built engine is destroyed on every way out but the last)
  std::unique_ptr<gs_hermite, int (*)(gs_hermite*)> guard(new gs_hermite(), gs_hermite_destroy);
  gs_hermite* h = guard.get();
  h->cfg = *cfg;
  h->esz = cfg->dtype == GS_FP32 ? 4 : 8;
  h->psz = fp64 ? 8 : 4;
  h->n = cfg->n;
  h->chunk = chunk;
  h->n_pad = gs::round_up(cfg->n, chunk);
  h->n_chunks = (int32_t)(h->n_pad / chunk);
  for (int32_t q = 0; q < cfg->nranks; ++q) {
    int64_t b = 0, c = 0;
    if (gs_hermite_partition(cfg->n, chunk, cfg->nranks, q, &b, &c)) return -1;
    if (b >= cfg->n) {
      gs_set_error("hermite: more ranks than units of 1024 rows that hold a body (a rank would "
                   "own ghost rows only)");
      return -1;
    }
    h->ubeg.push_back(b / kUnit);
    h->ucnt.push_back(c / kUnit);
    if (c != h->n_pad / cfg->nranks) h->uniform = false;
  }
  h->row0 = h->ubeg[(size_t)cfg->rank] * kUnit;
  h->n_loc = h->ucnt[(size_t)cfg->rank] * kUnit;
  if (launch_shape(h)) return -1;
  GS_HIP(hipSetDevice(cfg->device));
  GS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  GS_HIP(hipEventCreateWithFlags(&h->ev, hipEventDisableTiming));
  const size_t rb = rows_bytes(h), prb = pair_rows_bytes(h);
  const size_t pb = (size_t)h->n_loc * 4 * h->psz * (size_t)h->n_chunks;  // (partials: own rows)
  DevMem& g = h->base;
  if (dev_buf(h, g, &h->X, rb, "X") || dev_buf(h, g, &h->V, rb, "V") ||
      dev_buf(h, g, &h->A, rb, "A") || dev_buf(h, g, &h->J, rb, "J") ||
      dev_buf(h, g, &h->a_out, rb, "a_out") || dev_buf(h, g, &h->j_out, rb, "j_out") ||
      dev_buf(h, g, &h->XP, prb, "XP") || dev_buf(h, g, &h->VP, prb, "VP") ||
      (is_mixed(h) && dev_buf(h, g, &h->XL, prb, "XL")) ||
      g.alloc(&h->PA, pb, "PA") || g.alloc(&h->PJ, pb, "PJ") ||
      g.alloc(&h->ctrl, sizeof(gs::HermiteCtrl), "ctrl") ||
      g.alloc(&h->wgmin, (size_t)nwg(h) * sizeof(double), "wgmin") ||
      g.alloc(&h->mass_dev, (size_t)h->n_pad * sizeof(double), "mass") ||
      g.alloc(&h->nonfinite, sizeof(unsigned long long), "nonfinite"))
    return -1;
  GS_HIP(hipStreamSynchronize(h->stream));
  h->mass_host.assign((size_t)h->n, 0.0);
  if (set_wgmin(h, std::numeric_limits<double>::infinity()) ||
      write_ctrl(h, 0.0, 0, 0.0, std::numeric_limits<double>::infinity(), 0))
    return -1;
  *out = guard.release();
  return 0;
}

int gs_hermite_destroy(gs_hermite* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (ncclComm_t c = h->comm_live.exchange(nullptr)) (void)ncclCommDestroy(c);
  for (hipEvent_t e : h->ring) (void)hipEventDestroy(e);
  if (h->ev) (void)hipEventDestroy(h->ev);
  const hipStream_t stream = h->stream;
  delete h;  // (the five groups free their buffers)
  if (stream) (void)hipStreamDestroy(stream);
  return 0;
}

int gs_hermite_layout(gs_hermite* h, gs_layout* out) {
  if (!h || !out) { gs_set_error("hermite layout: null argument"); return -1; }
  *out = gs_layout{};
  out->n = h->n;
  out->n_pad = h->n_pad;
  out->n_local = h->n_loc;
  out->local_begin = h->row0;
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
  return update_ctrl(h);
}

int gs_hermite_init_ics(gs_hermite* h, int32_t ic, uint64_t seed) {
  GS_HIP(hipSetDevice(h->cfg.device));
  const hipError_t launched = by_state(h, [&](auto s) {
    using T = decltype(s);
    return gs::launch_init_ics<T>(ic, seed, h->n, h->n_pad, 0, h->n_pad, h->cfg.G,
                                  static_cast<T*>(h->X), static_cast<T*>(h->V), h->mass_dev,
                                  h->stream);
  });
  GS_HIP(launched);
  GS_HIP(hipMemcpyAsync(h->mass_host.data(), h->mass_dev, (size_t)h->n * sizeof(double),
                        hipMemcpyDeviceToHost, h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  return start_from_state(h);
}

int gs_hermite_set_state(gs_hermite* h, const double* pos, const double* vel, const double* mass,
                         const double* acc, const double* jerk, double t, double dt_next,
                         double dt_min) {
  if (!pos || !vel || !mass) { gs_set_error("hermite set_state: null argument"); return -1; }
  // (order 6 carries a, j, s, c: without the last two the derivatives start afresh)
  return set_state(h, pos, vel, mass, {acc, jerk, nullptr, nullptr}, t, dt_next, dt_min);
}

int gs_hermite_get_state(gs_hermite* h, double* pos, double* vel, double* mass, double* acc,
                         double* jerk) {
  return get_state_group(&h, 1, pos, vel, mass, acc, jerk);
}

int gs_hermite_derivs(gs_hermite* h, double* acc4, double* jerk4) {
  return gs_hermite_derivs_nn(h, acc4, jerk4, nullptr, nullptr);
}

int gs_hermite_derivs_nn(gs_hermite* h, double* acc4, double* jerk4, double* q, int32_t* nn) {
  if ((q || nn) && !h->nn) { gs_set_error("hermite derivs_nn: collisions are off"); return -1; }
  return derivs_group(&h, 1, acc4, jerk4, nullptr, q, nn);
}

int gs_hermite_step(gs_hermite* h, int32_t nsteps) {
  GS_HIP(hipSetDevice(h->cfg.device));
  if (h->block)
    return with_args(h, gs::HM_STEP, false,
                     [&](auto a) { return block_step_t<decltype(a)>(h, nsteps); });
  return with_args(h, gs::HM_STEP, false,
                   [&](auto a) { return step_t<decltype(a)>(&h, 1, nsteps); });
}

int gs_hermite_sync(gs_hermite* h) {
  GS_HIP(hipSetDevice(h->cfg.device));
  if (!h->ring.empty()) {
    // An RCCL run: a peer that never arrives must not block this rank for ever. Wait for the
    // recorded chains one by one, watching the communicator's async error; when none completes
    // for the step timeout the communicator is aborted, which releases the stream.
    if (wait_seen(h, h->rec)) return -1;
    if (h->comm_live.load() == nullptr) { gs_set_error("hermite: communicator aborted"); return -1; }
  }
  GS_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int gs_hermite_status(gs_hermite* h, gs_hermite_info* out) {
  if (!h || !out) { gs_set_error("hermite status: null argument"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  if (!h->ring.empty() && wait_seen(h, h->rec)) return -1;  // (an RCCL run: a bounded wait)
  *out = gs_hermite_info{};
  out->ipl = h->ipl;
  gs::HermiteBlockCtrl b;
  if (h->block && read_bctrl(h, &b)) return -1;
  gs::HermiteCtrl c;  // (block runs: the evaluation a run starts with counts its overlaps here)
  if (read_ctrl(h, &c)) return -1;
  if (h->block) {
    const int64_t macro = b.t_ticks >> b.L;
    out->time = b.dt_max * ldexp((double)b.t_ticks, -b.L);
    out->dt_last = out->dt_next = b.dt_max;
    out->dt_min = ldexp(b.dt_max, -b.level_max);
    out->steps = macro - h->macro0;
    out->finished = h->has_end && out->time >= h->t_end;
    out->block_steps = (int64_t)b.block_steps;
    out->body_steps = (int64_t)b.body_steps;
    out->level_clamped = (int64_t)b.level_clamped;
    out->level_max = b.level_max;
    out->narrow_max = b.narrow_max;
    out->overlaps = (int64_t)(b.overlaps + c.overlaps);
    return 0;
  }
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
  out->overlaps = (int64_t)c.overlaps;
  return 0;
}

// Block mode on or off: gs_hermite_set_block (order 4) and gs_hermite_set_block6 (order 6).
static int set_block_mode(gs_hermite* h, int32_t on, int32_t max_level, int32_t order) {
  if (!h) { gs_set_error("hermite set_block: null argument"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  if (!on) {
    GS_HIP(hipStreamSynchronize(h->stream));
    drop_block(h);
    return 0;
  }
  if (multi(h)) {
    gs_set_error("hermite block steps (block_steps) run on one rank");
    return -1;
  }
  if (order == 6 && h->order != 6) {
    gs_set_error("hermite set_block6: the order is not 6 (gs_hermite_set_order)");
    return -1;
  }
  if (h->order == 6)
    if (const char* why = refuse6(h, order == 6 ? R6_BLOCK6 : R6_BLOCK)) {
      gs_set_error(why);
      return -1;
    }
  if (max_level < 0 || max_level > 40) {
    gs_set_error("hermite block steps: max_level must be in 0..40");
    return -1;
  }
  if (!(h->eta > 0.0)) { gs_set_error("hermite block steps need eta > 0"); return -1; }
  if (h->has_end && (double)llround(h->t_end / h->cfg.dt) * h->cfg.dt != h->t_end) {
    gs_set_error("hermite block steps: t_end must be a whole multiple of dt");
    return -1;
  }
  GS_HIP(hipStreamSynchronize(h->stream));
  drop_block(h);
  h->max_level = max_level;
  const size_t np = (size_t)h->n_pad, wg = (size_t)nwg(h);
  gs::HBlock& b = h->blk;
  const int built = h->blockg.rebuild([&](DevMem& g) {
    return g.alloc(&b.bc, sizeof(gs::HermiteBlockCtrl), "block ctrl") ||
           dev_buf(h, g, &b.tb, np * sizeof(int64_t), "block tb") ||
           dev_buf(h, g, &b.level, np * sizeof(int32_t), "block level") ||
           dev_buf(h, g, &b.list, np * sizeof(int32_t), "block list") ||
           dev_buf(h, g, &b.wgcount, wg * sizeof(int32_t), "block wgcount") ||
           g.alloc(&b.wgnext, wg * sizeof(int64_t), "block wgnext");
  });
  b.slice = gs::hermite_narrow_slice(h->n_pad);
  b.n_slices = (int32_t)((h->n_pad + b.slice - 1) / b.slice);
  // (block mode is on once its arrays and the narrow slots stand; else it stays off, with neither)
  if (built || reset_bctrl(h, 0) || set_narrow(h, -1)) {
    drop_block(h);
    return -1;
  }
  h->block = true;
  return 0;
}

int gs_hermite_set_block(gs_hermite* h, int32_t on, int32_t max_level) {
  return set_block_mode(h, on, max_level, 4);
}

int gs_hermite_set_block6(gs_hermite* h, int32_t on, int32_t max_level) {
  return set_block_mode(h, on, max_level, 6);
}

int gs_hermite_set_block_tuning(gs_hermite* h, int32_t narrow_max) {
  if (!h || !h->block) { gs_set_error("hermite block tuning: not in block mode"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  return set_narrow(h, narrow_max);
}

int gs_hermite_get_block_state(gs_hermite* h, int64_t* tb, int32_t* level) {
  if (!h || !h->block) { gs_set_error("hermite block state: not in block mode"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  if (tb)
    GS_HIP(hipMemcpyAsync(tb, h->blk.tb, (size_t)h->n * sizeof(int64_t), hipMemcpyDeviceToHost,
                          h->stream));
  if (level)
    GS_HIP(hipMemcpyAsync(level, h->blk.level, (size_t)h->n * sizeof(int32_t),
                          hipMemcpyDeviceToHost, h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int gs_hermite_set_block_state(gs_hermite* h, const int64_t* tb, const int32_t* level) {
  if (!h || !h->block) { gs_set_error("hermite block state: not in block mode"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  gs::HermiteBlockCtrl c;
  if (read_bctrl(h, &c)) return -1;
  const int L = h->max_level;
  std::vector<int32_t> lv((size_t)h->n);
  std::vector<int64_t> tv((size_t)h->n);
  if (!level) GS_HIP(hipMemcpy(lv.data(), h->blk.level, lv.size() * 4, hipMemcpyDeviceToHost));
  if (!tb) GS_HIP(hipMemcpy(tv.data(), h->blk.tb, tv.size() * 8, hipMemcpyDeviceToHost));
  int64_t tmin = std::numeric_limits<int64_t>::max();
  for (int64_t i = 0; i < h->n; ++i) {
    if (level) lv[(size_t)i] = level[i];
    if (tb) tv[(size_t)i] = tb[i];
    const int32_t k = lv[(size_t)i];
    if (k < 0 || k > L || tv[(size_t)i] < 0 || (tv[(size_t)i] & (((int64_t)1 << (L - k)) - 1))) {
      gs_set_error("hermite block state: level out of 0..max_level, or a body time that is no "
                   "multiple of its step");
      return -1;
    }
    if (tv[(size_t)i] < tmin) tmin = tv[(size_t)i];
    if (k > c.level_max) c.level_max = k;
  }
  GS_HIP(hipMemcpyAsync(h->blk.level, lv.data(), lv.size() * 4, hipMemcpyHostToDevice, h->stream));
  GS_HIP(hipMemcpyAsync(h->blk.tb, tv.data(), tv.size() * 8, hipMemcpyHostToDevice, h->stream));
  c.t_ticks = tmin;
  c.target = tmin;
  return write_bctrl(h, c);  // (waits for the copies: lv, tv are on this frame)
}

// The checks of every derivs_active / time_active entry; *path 0 becomes the path narrow_max picks.
static int active_args_ok(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t* path_io) {
  int32_t path = *path_io;
  if (!h || !h->block) { gs_set_error("hermite derivs_active: not in block mode"); return -1; }
  if (!idx || n_idx < 1 || n_idx > h->n || path < 0 || path > 2) {
    gs_set_error("hermite derivs_active: bad arguments");
    return -1;
  }
  for (int32_t k = 0; k < n_idx; ++k)
    if (idx[k] < 0 || idx[k] >= h->n) {
      gs_set_error("hermite derivs_active: index out of range");
      return -1;
    }
  if (path == 0) path = n_idx <= h->narrow_max ? gs::HP_NARROW : gs::HP_WIDE;
  if (path == gs::HP_NARROW && n_idx > h->narrow_max) {
    gs_set_error("hermite derivs_active: narrow path needs n_idx <= narrow_max");
    return -1;
  }
  *path_io = path;
  return 0;
}

// The one way in of the entries below. six: an entry of order 6 (the engine's order must be 6);
// the others take an engine of either order (of order 6: its a and j).
static int active_entry(gs_hermite* h, bool six, const int32_t* idx, int32_t n_idx, int32_t path,
                        int32_t reps, double* ms, double* acc4, double* jerk4, double* snap4,
                        double* q, int32_t* nn) {
  if (active_args_ok(h, idx, n_idx, &path)) return -1;
  if (six && h->order != 6) { gs_set_error("hermite derivs_active6: the order is not 6"); return -1; }
  if (reps < 1) reps = 1;
  GS_HIP(hipSetDevice(h->cfg.device));
  return with_args(h, gs::HM_OUT, true, [&](auto a) {
    return derivs_active(h, a, idx, n_idx, path, reps, ms, acc4, jerk4, snap4, q, nn);
  });
}

int gs_hermite_derivs_active(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t path,
                             double* acc4, double* jerk4) {
  return active_entry(h, false, idx, n_idx, path, 1, nullptr, acc4, jerk4, nullptr, nullptr,
                      nullptr);
}

int gs_hermite_time_active(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t path,
                           int32_t reps, double* ms, double* acc4, double* jerk4) {
  return active_entry(h, false, idx, n_idx, path, reps, ms, acc4, jerk4, nullptr, nullptr, nullptr);
}

int gs_hermite_derivs_active_nn(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t path,
                                double* acc4, double* jerk4, double* q, int32_t* nn) {
  if (h && (q || nn) && !h->nn) {
    gs_set_error("hermite derivs_active_nn: collisions are off");
    return -1;
  }
  return active_entry(h, false, idx, n_idx, path, 1, nullptr, acc4, jerk4, nullptr, q, nn);
}

int gs_hermite_derivs_active6(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t path,
                              double* acc4, double* jerk4, double* snap4) {
  return active_entry(h, true, idx, n_idx, path, 1, nullptr, acc4, jerk4, snap4, nullptr, nullptr);
}

int gs_hermite_time_active6(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t path,
                            int32_t reps, double* ms, double* acc4, double* jerk4,
                            double* snap4) {
  return active_entry(h, true, idx, n_idx, path, reps, ms, acc4, jerk4, snap4, nullptr, nullptr);
}

int gs_hermite_set_collisions(gs_hermite* h, int32_t on) {
  if (!h || on < 0 || on > 2) { gs_set_error("hermite set_collisions: bad arguments"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  GS_HIP(hipStreamSynchronize(h->stream));
  if (!on) {
    h->coll.release();
    h->nn = 0;
    const int narrow = size_narrow(h, h->blk.cap, false);  // (without the neighbour partials)
    if (launch_shape(h) || update_ctrl(h, 0)) return -1;
    return narrow;
  }
  if (multi(h)) {
    gs_set_error("hermite collisions run on one rank");
    return -1;
  }
  if (h->order == 6) { gs_set_error(refuse6(h, R6_NN)); return -1; }
  if (h->n_pad > (int64_t)std::numeric_limits<int32_t>::max()) {
    gs_set_error("hermite set_collisions: too many bodies for int32 neighbour indices");
    return -1;
  }
  if (!h->nn) {
    const size_t np = (size_t)h->n_pad, ib = np * sizeof(int32_t), qb = np * sizeof(double);
    const int built = h->coll.rebuild([&](DevMem& g) {
      return dev_buf(h, g, &h->R, np * h->esz, "R") ||
             g.alloc(&h->PN, ib * (size_t)h->n_chunks, "PN") ||  // (the indices: -1, all bits set)
             dev_buf(h, g, &h->nn_i, ib, "nn_i", 0xff) ||
             dev_buf(h, g, &h->ca_i, ib, "ca_i", 0xff) ||
             dev_buf(h, g, &h->nn_out, ib, "nn_out", 0xff) ||
             dev_buf(h, g, &h->nn_q, qb, "nn_q") || dev_buf(h, g, &h->ca_q, qb, "ca_q") ||
             dev_buf(h, g, &h->q_out, qb, "q_out");
    });
    // (collisions are on once their arrays and the narrow path's neighbour partials stand)
    if (built || size_narrow(h, h->blk.cap, true)) {
      h->coll.release();
      return -1;
    }
  }
  h->nn = on;
  if (launch_shape(h)) return -1;
  if (clear_records(h, true)) return -1;
  return update_ctrl(h, 0);
}

int gs_hermite_set_radii(gs_hermite* h, const double* r) {
  if (!h || !r) { gs_set_error("hermite set_radii: null argument"); return -1; }
  if (!h->nn) { gs_set_error("hermite set_radii: collisions are off"); return -1; }
  for (int64_t i = 0; i < h->n; ++i)
    if (!(r[i] >= 0.0) || !std::isfinite(r[i])) {
      gs_set_error("hermite set_radii: a radius must be finite and >= 0");
      return -1;
    }
  GS_HIP(hipSetDevice(h->cfg.device));
  return by_state(h, [&](auto s) {
    using T = decltype(s);
    std::vector<T> d((size_t)h->n_pad, T(0));
    for (int64_t i = 0; i < h->n; ++i) d[(size_t)i] = (T)r[i];
    GS_HIP(hipMemcpyAsync(h->R, d.data(), d.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int gs_hermite_set_order(gs_hermite* h, int32_t order) {
  if (!h || (order != 4 && order != 6)) {
    gs_set_error("hermite set_order: the order must be 4 or 6");
    return -1;
  }
  GS_HIP(hipSetDevice(h->cfg.device));
  GS_HIP(hipStreamSynchronize(h->stream));
  if (order == 6)
    if (const char* why = refuse6(h)) { gs_set_error(why); return -1; }
  const int32_t was = h->order;
  if (order != was && h->block) {  // (the narrow partials and the chain are the order's)
    gs_set_error("hermite set_order: switch block steps off first (gs_hermite_set_block6)");
    return -1;
  }
  // (the order and its launch shape change once order 6's arrays stand; a switch that fails
  // leaves the order, the shape and the arrays of before)
  if (order == 6 && was != 6 && h->six.rebuild([&](DevMem& g) { return fill_order6(h, g); }))
    return -1;
  h->order = order;
  if (launch_shape(h)) {
    h->order = was;
    if (was != 6) h->six.release();
    return -1;
  }
  if (order != 6) h->six.release();
  return 0;
}

int32_t gs_hermite_get_order(gs_hermite* h) { return h ? h->order : 0; }

int32_t gs_hermite6_ipl_ok(int32_t fp64, int32_t ipl) {
  return gs::hermite6_ipl_ok(fp64, ipl) ? 1 : 0;
}

int gs_hermite_set_state6(gs_hermite* h, const double* pos, const double* vel, const double* mass,
                          const double* acc, const double* jerk, const double* snap,
                          const double* crackle, double t, double dt_next, double dt_min) {
  if (!h || h->order != 6) { gs_set_error("hermite set_state6: the order is not 6"); return -1; }
  if (!pos || !vel || !mass) { gs_set_error("hermite set_state6: null argument"); return -1; }
  return set_state(h, pos, vel, mass, {acc, jerk, snap, crackle}, t, dt_next, dt_min);
}

int gs_hermite_get_carried6(gs_hermite* h, double* snap, double* crackle) {
  if (!h || h->order != 6) { gs_set_error("hermite get_carried6: the order is not 6"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  return download_rows(h, h->S, h->n, snap, 3) || download_rows(h, h->C, h->n, crackle, 3) ? -1
                                                                                            : 0;
}

int gs_hermite_derivs6(gs_hermite* h, double* acc4, double* jerk4, double* snap4) {
  if (!h || h->order != 6) { gs_set_error("hermite derivs6: the order is not 6"); return -1; }
  return derivs_group(&h, 1, acc4, jerk4, snap4, nullptr, nullptr);
}

int gs_hermite_neighbours(gs_hermite* h, double* q, int32_t* nn) {
  if (!h || !h->nn) { gs_set_error("hermite neighbours: collisions are off"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  return download_pair(h, h->nn_q, h->nn_i, h->n, q, nn);
}

int gs_hermite_closest(gs_hermite* h, double* q, int32_t* nn, int32_t clear) {
  if (!h || !h->nn) { gs_set_error("hermite closest: collisions are off"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  if (download_pair(h, h->ca_q, h->ca_i, h->n, q, nn)) return -1;
  return clear ? clear_records(h, false) : 0;
}

int gs_hermite_clear_overlap(gs_hermite* h) {
  if (!h) { gs_set_error("hermite clear_overlap: null argument"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  if (update_ctrl(h, 0)) return -1;
  if (h->block) {
    gs::HermiteBlockCtrl b;
    if (read_bctrl(h, &b)) return -1;
    b.overlaps = 0;
    return write_bctrl(h, b);
  }
  return 0;
}

int64_t gs_hermite_count_nonfinite(gs_hermite* h) {
  if (hipSetDevice(h->cfg.device) != hipSuccess ||
      hipMemsetAsync(h->nonfinite, 0, sizeof(unsigned long long), h->stream) != hipSuccess) {
    gs_set_error("hermite count_nonfinite: device error");
    return -1;
  }
  const hipError_t e = by_state(h, [&](auto s) {  // (the rows this rank owns)
    using T = decltype(s);
    return gs::launch_count_nonfinite<T>(static_cast<const T*>(h->X), h->row0, h->n_loc,
                                         static_cast<const T*>(h->V) + 4 * h->row0, h->nonfinite,
                                         h->stream);
  });
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

// ---- ranks: virtual group and RCCL -----------------------------------------------------

int gs_hermite_group_step(gs_hermite** shards, int32_t P, int32_t nsteps) {
  if (check_group(shards, P)) return -1;
  for (int r = 0; r < P; ++r)
    if (shards[r]->block) { gs_set_error("hermite group: block steps run on one rank"); return -1; }
  GS_HIP(hipSetDevice(shards[0]->cfg.device));
  return with_args(shards[0], gs::HM_STEP, false,
                   [&](auto a) { return step_t<decltype(a)>(shards, P, nsteps); });
}

int gs_hermite_group_get_state(gs_hermite** shards, int32_t P, double* pos, double* vel,
                               double* mass, double* acc, double* jerk) {
  if (check_group(shards, P)) return -1;
  return get_state_group(shards, P, pos, vel, mass, acc, jerk);
}

int gs_hermite_group_derivs(gs_hermite** shards, int32_t P, double* acc4, double* jerk4) {
  if (check_group(shards, P)) return -1;
  return derivs_group(shards, P, acc4, jerk4, nullptr, nullptr, nullptr);
}

int gs_hermite_group_time_eval(gs_hermite** shards, int32_t P, int32_t reps, double* ms) {
  if (check_group(shards, P) || !ms) return -1;
  if (reps < 1) reps = 1;
  GS_HIP(hipSetDevice(shards[0]->cfg.device));
  for (int r = 0; r < P; ++r) GS_HIP(hipStreamSynchronize(shards[r]->stream));
  for (int r = 0; r < P; ++r)  // (one shard at a time: each has the device to itself)
    if (by_dtype(shards[r], [&](auto t, auto s) {
          return time_eval_t<decltype(t), decltype(s)>(shards[r], reps, ms + r);
        }))
      return -1;
  return 0;
}

int gs_hermite_comm_init(gs_hermite* h, const void* id128, int32_t rank, int32_t nranks) {
  if (!h || !id128) { gs_set_error("hermite comm_init: null argument"); return -1; }
  if (rank != h->cfg.rank || nranks != h->cfg.nranks) {
    gs_set_error("hermite comm_init: rank/nranks differ from the engine's");
    return -1;
  }
  if (h->comm) { gs_set_error("hermite comm_init: called twice"); return -1; }
  GS_HIP(hipSetDevice(h->cfg.device));
  if (nranks == 1) return 0;  // (one rank gathers nothing: no communicator is kept)
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  GS_NCCL(ncclCommInitRank(&h->comm, nranks, id, rank));
  h->comm_live.store(h->comm);
  int32_t info[3] = {0, -1, -1};
  const int bad = gs::rt::comm_verify(h->comm, nranks, rank, h->cfg.device, info,
                                      "hermite comm_init");
  h->comm_count = info[0];
  h->comm_user_rank = info[1];
  h->comm_cu_device = info[2];
  if (bad) {
    const std::string why = gs_last_error();  // (kept across the abort)
    abort_comm(h);
    gs_set_error(why.c_str());
    return -1;
  }
  h->ring.resize(32);
  for (hipEvent_t& e : h->ring) GS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  // Warm-up (RCCL builds its transports on the first collective): the gather of the step minima,
  // which are all +inf before a state is set, waited for like a step.
  if (gather_comm(h, G_WGMIN)) return -1;
  GS_HIP(hipEventRecord(h->ring[0], h->stream));
  h->rec = 1;
  h->seen = 0;
  return wait_seen(h, 1);
}

int gs_hermite_comm_info(gs_hermite* h, int32_t* count, int32_t* user_rank, int32_t* cu_device) {
  if (!h) return -1;
  if (count) *count = h->comm_live.load() != nullptr ? h->comm_count : 0;
  if (user_rank) *user_rank = h->comm_user_rank;
  if (cu_device) *cu_device = h->comm_cu_device;
  return 0;
}

int gs_hermite_comm_check(gs_hermite* h) {
  if (!h || !h->comm) return 0;
  ncclComm_t c = h->comm_live.load();
  if (!c) { gs_set_error("RCCL communicator aborted (timeout or async error)"); return -1; }
  if (gs::rt::comm_async_check(c)) {
    const std::string why = gs_last_error();
    abort_comm(h);
    gs_set_error(why.c_str());
    return -1;
  }
  return 0;
}

int32_t gs_hermite_abort(gs_hermite* h) { return h && abort_comm(h) ? 1 : 0; }

int gs_hermite_set_step_timeout(gs_hermite* h, double timeout_s) {
  if (!h || !(timeout_s >= 0.0)) { gs_set_error("hermite: bad step timeout"); return -1; }
  h->step_timeout_s = timeout_s;
  return 0;
}

}  // extern "C"
