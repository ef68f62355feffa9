// gravsim native C ABI — MI355X (gfx950) N-body runtime.
//
// One header for both native libraries:
//   libgravsim_hip.so  (hipcc, gfx950): device kernels + the GPU Stepper (streams, events,
//                      hipGraph replay, RCCL all-gather over xGMI).
//   libgravsim_cpu.so  (g++ -fopenmp): fp64/fp32 direct-sum CPU engine (mpi.c world_size=1
//                      analogue and fast native oracle).
// Python binds these with ctypes (gravsim/ops/_native.py); there is no torch ABI coupling,
// so the libraries also serve the standalone C++ driver in csrc/tools/.
//
// Reference parity (what these replace, /root/reference):
//   cuda.cu:32-60   calculate_force_between + calculate_forces_kernel  -> gs force kernels
//   cuda.cu:63-78   host update()                                      -> fused KD epilogue
//   cuda.cu:145-160 cudaMalloc/Memcpy/DeviceSynchronize per step       -> device-resident Stepper
//   mpi.c:160-236   MPI_Bcast / MPI_Allgatherv / MPI_Barrier           -> RCCL in-place all-gather
//   mpi.c:196-216   per-rank O(N^2/P) loop + in-place integrate       -> gs_cpu_step (Jacobi)
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// GS_MIXED (the Hermite integrator only): fp64 state, fp32 pair arithmetic on double-single
// predicted positions.
enum gs_dtype { GS_FP32 = 0, GS_FP64 = 1, GS_MIXED = 2 };

// Force kernel variants (the j-body source).
enum gs_kernel {
  GS_KERNEL_AUTO = 0,
  GS_KERNEL_LDS = 1,   // j-tiles staged into LDS by global_load_lds (LDS-DMA), broadcast ds_read_b128
  GS_KERNEL_SMEM = 2,  // wave-uniform j read through the scalar cache into SGPRs (s_load_dwordx16)
  GS_KERNEL_MFMA = 3,  // experimental fp32: r^2 as a 16x16x4 f32 MFMA GEMM, re-centred tiles
};

// Step schedule.
enum gs_mode {
  GS_MODE_AUTO = 0,
  GS_MODE_FUSED = 1,   // one workgroup per i-block sweeps every j-chunk, KD integrate in the epilogue
  GS_MODE_SPLIT = 2,   // i-block x chunk-group grid writes per-chunk partials; reduce+integrate kernel
  GS_MODE_SYM = 3,     // fp32 Newton-3: each unordered pair once, both sides (nbody_sym.hip)
};

// Initial-condition families (models). Same formulas in gravsim/models/initial_conditions.py.
// Multi-rank exchange strategies.
enum gs_strategy {
  GS_STRATEGY_ALLGATHER = 0,  // one in-place ncclAllGather, overlapped with the local chunks
  GS_STRATEGY_RING = 1,       // P-1 neighbour ncclSend/ncclRecv, each slice computed on arrival
};

enum gs_ic {
  GS_IC_SOLAR_RANDOM = 0,  // Sun/Earth/Mars + uniform cube bodies (cuda.cu:81-96,129-131)
  GS_IC_RANDOM = 1,        // uniform cube bodies only
};

typedef struct gs_config {
  int64_t n;          // real (global) body count
  int32_t dtype;      // gs_dtype
  int32_t kernel;     // gs_kernel
  int32_t mode;       // gs_mode
  int32_t ipl;        // i-bodies per lane (0 = auto)
  int32_t chunk;      // canonical j-chunk length (0 = auto, from n only)
  int32_t rank;       // this process' rank
  int32_t nranks;     // world size (bodies are block-partitioned over ranks)
  int32_t device;     // HIP device ordinal
  int32_t use_graph;  // capture the step loop into a hipGraph and replay it
  int32_t split_groups;  // SPLIT mode: chunk groups per i-block (0 = auto)
  int32_t cutoff_mode;   // 0 auto, 1 exact hard cutoff (select), 2 fast (overflow-safe core)
  int32_t strategy;      // 0 all-gather (default), 1 ring pass (neighbour send/recv, pipelined)
  double dt;          // time step [s]
  double G;           // gravitational constant
  double cutoff;      // hard cutoff radius [m]: zero force below it (mpi.c:64)
  double softening;   // Plummer softening length [m] (0 = reference semantics)
} gs_config;

typedef struct gs_layout {
  int64_t n;            // real bodies
  int64_t n_pad;        // padded global length (multiple of nranks*chunk)
  int64_t n_local;      // bodies per rank (padded)
  int64_t local_begin;  // global index of this rank's slice
  int32_t chunk;        // canonical j-chunk length
  int32_t n_chunks;     // chunks that contain at least one real body
  int32_t ipl;          // resolved i-bodies per lane
  int32_t kernel;       // resolved kernel variant
  int32_t mode;         // resolved schedule
  int32_t split_groups; // resolved chunk groups (SPLIT)
} gs_layout;

// ---------------------------------------------------------------- layout (host-only math)
// Canonical, world-size-independent decomposition (shared by CPU and GPU engines).
int gs_layout_compute(const gs_config* cfg, gs_layout* out);
int32_t gs_auto_chunk(int64_t n);
// Symmetric (Newton-3) schedule geometry for a padded body count, and its partial-buffer
// bytes per rank (GS_MODE_SYM).
int gs_sym_geometry(int64_t n_pad, int32_t* NC, int32_t* H, int32_t* L, int32_t* S,
                    int32_t* D);
int64_t gs_sym_bytes(int64_t n_pad, int32_t nranks, int32_t esz);
// Rows [a0, a0 + rows) of one rank (whole row blocks, mpi.c's remainder rule) and the
// reduction-tree nodes: B blocks of RB rows, nn nodes sent by this rank, nb by lower ranks,
// NN in all (gs_common.h).
int gs_sym_rank_rows(int64_t n_pad, int32_t nranks, int32_t rank, int32_t* a0, int32_t* rows);
// Rows a rank of a multi-rank Hermite run owns: n_pad = n rounded up to the chunk (0: auto), in
// units of 1024 rows dealt out contiguously by mpi.c's remainder rule (the first `units mod
// nranks` ranks hold one more). Refuses nranks above the unit count.
int gs_hermite_partition(int64_t n, int32_t chunk, int32_t nranks, int32_t rank,
                         int64_t* row_begin, int64_t* row_count);
int gs_sym_nodes(int64_t n_pad, int32_t nranks, int32_t rank, int32_t* B, int32_t* RB,
                 int32_t* nn, int32_t* nb, int32_t* NN);
// Busiest rank's work over the mean of the sym schedule's whole-row-block ownership
// (ceil(B / P) * P / B); mode auto picks sym only up to 1.25.
double gs_sym_imbalance(int64_t n_pad, int32_t nranks);
// Shell length of chunk row A (the antipodal pairs split between rows by parity).
int32_t gs_sym_shell_len(int32_t A, int32_t NC);
// Unit order of the gated sym launch for one rank (see layout.cpp); returns the entry count.
// 1 if rank src's node sums for rank dst's bodies can be nonzero, 0 if the geometry makes
// them +0.0 for every body (the exchange skips that send), -1 on bad arguments.
int32_t gs_sym_pair_live(int64_t n_pad, int32_t nranks, int32_t src, int32_t dst);
int64_t gs_sym_unit_map(int64_t n_pad, int32_t rank, int32_t nranks, int64_t fill,
                        int32_t* out, int64_t cap);
// ... with the last kr shell segments of every row split into np part units at the end (bit
// 30, part in bits 28-29; rows < 4096); the _kr form is np = 2.
int64_t gs_sym_unit_map_kr(int64_t n_pad, int32_t rank, int32_t nranks, int64_t fill,
                           int32_t kr, int32_t* out, int64_t cap);
int64_t gs_sym_unit_map_parts(int64_t n_pad, int32_t rank, int32_t nranks, int64_t fill,
                              int32_t kr, int32_t np, int32_t* out, int64_t cap);
// Split shell segments per row (SymArgs::Kr) for a geometry: S / 16 when a segment has at
// least 2 tiles of 128 bodies (L >= 2), else 0; and the parts each is split into (SymArgs::Np:
// 4 when L >= 4, else 2).
int32_t gs_sym_split_segments(int64_t n_pad);
int32_t gs_sym_split_parts(int64_t n_pad);
// The same for the ring strategy: entries carry the ring stage (bits 28-30) at which the last
// slice a unit reads arrives, and units are ordered by stage (rows < 4096, nranks <= 8).
int64_t gs_sym_unit_map_ring(int64_t n_pad, int32_t rank, int32_t nranks, int64_t fill,
                             int32_t* out, int64_t cap);

// ---------------------------------------------------------------- counter-based RNG / ICs (host)
// Fill bodies [begin, end) of the IC family into fp64 arrays (pos/vel: 3 per body, mass: 1).
void gs_ic_fill_host(int32_t ic, uint64_t seed, int64_t n, int64_t begin, int64_t end,
                     double* pos, double* vel, double* mass);

// ---------------------------------------------------------------- CPU engine (libgravsim_cpu)
// Accelerations for global bodies [i0, i1) against all j (positions X4 = x,y,z,mu; n_pad rows),
// summed in the canonical chunk order. acc4 gets (ax, ay, az, phi) per body. fp64 or fp32 (X4 type).
int gs_cpu_accel_f64(const double* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t chunk,
                     double cut2, double eps2, double* acc4);
int gs_cpu_accel_f32(const float* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t chunk,
                     float cut2, float eps2, float* acc4);
// One KD step for global bodies [i0, i1): reads X4 (full), vel4 (local, i0-based), writes
// Xnext4 rows [i0, i1) and vel4. Ghost rows (>= n_real) are zeroed.
// fp64 accelerations of rows [i0, i1) plus, per component, sum_j |term_ij| (8 doubles per
// row: a_x, a_y, a_z, 0, |.|_x, |.|_y, |.|_z, 0): the scale of a rounding-error bound.
int gs_cpu_accel_abs_f64(const double* X4, int64_t n_real, int64_t i0, int64_t i1, double cut2,
                         double eps2, double* out8);
// The same in long double (x87 extended): the reference of the fp64 accuracy gates.
int gs_cpu_accel_abs_ld(const double* X4, int64_t n_real, int64_t i0, int64_t i1, double cut2,
                        double eps2, double* out8);
int gs_cpu_step_f64(const double* X4, double* Xnext4, double* vel4, int64_t n_real, int64_t i0,
                    int64_t i1, int32_t chunk, double dt, double cut2, double eps2);
int gs_cpu_step_f32(const float* X4, float* Xnext4, float* vel4, int64_t n_real, int64_t i0,
                    int64_t i1, int32_t chunk, float dt, float cut2, float eps2);
// Hermite derivatives of global bodies [i0, i1) at (X4, V4 = vx, vy, vz, 0): acc4 gets
// (ax, ay, az, phi), jerk4 (jx, jy, jz, 0), with a_i = sum mu d / r^3 and
// j_i = sum mu (w - 3 (d.w) d / r^2) / r^3 (d = x_j - x_i, w = v_j - v_i, r^2 = |d|^2 + eps2),
// a pair contributing zero to all when r^2 < cut2; canonical chunk order, OpenMP over i.
int gs_cpu_accjerk_f64(const double* X4, const double* V4, int64_t n_real, int64_t i0, int64_t i1,
                       int32_t chunk, double cut2, double eps2, double* acc4, double* jerk4);
int gs_cpu_accjerk_f32(const float* X4, const float* V4, int64_t n_real, int64_t i0, int64_t i1,
                       int32_t chunk, float cut2, float eps2, float* acc4, float* jerk4);
// The same sums for the n_idx bodies idx[k] (a block step's active set, any order): row k of
// acc4 / jerk4 belongs to body idx[k] and is bit-equal to its row of gs_cpu_accjerk_*.
int gs_cpu_accjerk_idx_f64(const double* X4, const double* V4, int64_t n_real, const int32_t* idx,
                           int64_t n_idx, int32_t chunk, double cut2, double eps2, double* acc4,
                           double* jerk4);
int gs_cpu_accjerk_idx_f32(const float* X4, const float* V4, int64_t n_real, const int32_t* idx,
                           int64_t n_idx, int32_t chunk, float cut2, float eps2, float* acc4,
                           float* jerk4);
// One 4th-order Hermite step of size h on the n_real bodies, in place: predict, evaluate at the
// predicted state, correct; A4 / J4 carry the derivatives from step to step (scratch: 4 arrays
// of n_real * 4). *dt_min_out (if given and eta > 0) gets min_i of Aarseth's criterion
// (+inf when no body takes part).
// The first adaptive step of a run: (eta / 2) min_i |a_i| / |j_i| over the bodies with |j| > 0
// and a finite ratio (+inf when none is left). A4 / J4: n_real rows of 4.
double gs_cpu_hermite_first_dt_f64(const double* A4, const double* J4, int64_t n_real, double eta);
double gs_cpu_hermite_first_dt_f32(const float* A4, const float* J4, int64_t n_real, double eta);
int gs_cpu_hermite_step_f64(double* X4, double* V4, double* A4, double* J4, double* scratch,
                            int64_t n_real, int32_t chunk, double h, double cut2, double eps2,
                            double eta, double* dt_min_out);
int gs_cpu_hermite_step_f32(float* X4, float* V4, float* A4, float* J4, float* scratch,
                            int64_t n_real, int32_t chunk, double h, float cut2, float eps2,
                            double eta, double* dt_min_out);
// Mixed precision (GS_MIXED): arrays fp64 in and out. The evaluation sees each position as the
// double-single pair hi = float(x), lo = float(x - double(hi)) and forms d = (hi_j - hi_i) +
// (lo_j - lo_i) in fp32; v, mu, cut2 and eps2 are rounded to fp32 and the rest of the pair term
// and the chunk sums are gs_cpu_accjerk_f32's; the chunk sums are added in fp64 in chunk order.
// The step predicts, corrects and applies the criterion as gs_cpu_hermite_step_f64.
int gs_cpu_accjerk_mixed(const double* X4, const double* V4, int64_t n_real, int64_t i0,
                         int64_t i1, int32_t chunk, double cut2, double eps2, double* acc4,
                         double* jerk4);
int gs_cpu_accjerk_idx_mixed(const double* X4, const double* V4, int64_t n_real,
                             const int32_t* idx, int64_t n_idx, int32_t chunk, double cut2,
                             double eps2, double* acc4, double* jerk4);
int gs_cpu_hermite_step_mixed(double* X4, double* V4, double* A4, double* J4, double* scratch,
                              int64_t n_real, int32_t chunk, double h, double cut2, double eps2,
                              double eta, double* dt_min_out);
// Nearest neighbour of bodies [i0, i1) (or idx[0..n_idx)) by the pair measure
// q_ij = r^2 - (R_i + R_j)^2 of gs_hermite_set_collisions, with the arithmetic of the GPU
// kernels: r^2 as gs_cpu_accjerk_*, one add and one fma for q, a strict less in j order (the
// lowest j keeps a tie), pairs with r^2 < cut2 left out; (+inf, -1) when there is none. R: n_real
// radii. Row k of q / nn belongs to body i0 + k (idx[k]). mixed: as gs_cpu_accjerk_mixed.
int gs_cpu_nn_f64(const double* X4, const double* R, int64_t n_real, int64_t i0, int64_t i1,
                  double cut2, double eps2, double* q, int32_t* nn);
int gs_cpu_nn_f32(const float* X4, const float* R, int64_t n_real, int64_t i0, int64_t i1,
                  float cut2, float eps2, float* q, int32_t* nn);
int gs_cpu_nn_mixed(const double* X4, const double* R, int64_t n_real, int64_t i0, int64_t i1,
                    double cut2, double eps2, double* q, int32_t* nn);
int gs_cpu_nn_idx_f64(const double* X4, const double* R, int64_t n_real, const int32_t* idx,
                      int64_t n_idx, double cut2, double eps2, double* q, int32_t* nn);
int gs_cpu_nn_idx_f32(const float* X4, const float* R, int64_t n_real, const int32_t* idx,
                      int64_t n_idx, float cut2, float eps2, float* q, int32_t* nn);
int gs_cpu_nn_idx_mixed(const double* X4, const double* R, int64_t n_real, const int32_t* idx,
                        int64_t n_idx, double cut2, double eps2, double* q, int32_t* nn);
// k nearest neighbours of bodies [i0, i1) by distance (the definition of the k-nearest section
// below), with the arithmetic of the GPU kernel (explicit fma), so that the lists are bit-equal
// to gs_hip_knn's. X4: n_real rows of 4 (the fourth component is not read); k in 1..8; row r of
// r2 / idx (k entries each, ascending) belongs to body i0 + r. mixed: X4 fp64, the separation
// from the double-single rows of gs_cpu_accjerk_mixed, r2 widened to fp64.
int gs_cpu_knn_f64(const double* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t k,
                   double* r2, int32_t* idx);
int gs_cpu_knn_f32(const float* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t k, float* r2,
                   int32_t* idx);
int gs_cpu_knn_mixed(const double* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t k,
                     double* r2, int32_t* idx);
// 6th-order Hermite (Nitadori & Makino 2008). Derivatives of global bodies [i0, i1) at
// (X4, V4, A4 = ax, ay, az, 0 the acceleration the snap is taken at): acc4 (ax, ay, az, phi),
// jerk4, snap4 with s_i = sum mu q / r^3 - 6 alpha J_ij - 3 beta A_ij (q = a_j - a_i,
// alpha = (d.w) / r^2, beta = (|w|^2 + d.q) / r^2 + alpha^2); the pair law, the chunk order and
// the operations of the GPU pair term (nbody_hermite6.hip), a and j bit-equal to gs_cpu_accjerk_*.
int gs_cpu_accjerksnap_f64(const double* X4, const double* V4, const double* A4, int64_t n_real,
                           int64_t i0, int64_t i1, int32_t chunk, double cut2, double eps2,
                           double* acc4, double* jerk4, double* snap4);
int gs_cpu_accjerksnap_f32(const float* X4, const float* V4, const float* A4, int64_t n_real,
                           int64_t i0, int64_t i1, int32_t chunk, float cut2, float eps2,
                           float* acc4, float* jerk4, float* snap4);
// The same for listed bodies (an order-6 block step's active set): row k of the outputs is
// body idx[k]. fp64 only: order 6 runs its block steps in fp64.
int gs_cpu_accjerksnap_idx_f64(const double* X4, const double* V4, const double* A4,
                               int64_t n_real, const int32_t* idx, int64_t n_idx, int32_t chunk,
                               double cut2, double eps2, double* acc4, double* jerk4,
                               double* snap4);
// One 6th-order step of size h on the n_real bodies, in place: predict (x, v, a), evaluate,
// correct; A4, J4, S4, C4 carry a, j, snap and crackle from step to step (scratch: 6 arrays of
// n_real * 4: the predicted x, v, a rows, then a1, j1, s1). *dt_min_out (if given and eta > 0)
// gets min_i of the criterion of gs_hermite_set_order (+inf when no body takes part).
int gs_cpu_hermite6_step_f64(double* X4, double* V4, double* A4, double* J4, double* S4,
                             double* C4, double* scratch, int64_t n_real, int32_t chunk, double h,
                             double cut2, double eps2, double eta, double* dt_min_out);
int gs_cpu_hermite6_step_f32(float* X4, float* V4, float* A4, float* J4, float* S4, float* C4,
                             float* scratch, int64_t n_real, int32_t chunk, double h, float cut2,
                             float eps2, double eta, double* dt_min_out);
int gs_cpu_num_threads(void);
int gs_cpu_set_threads(int32_t n);  // OpenMP threads for the CPU engine (returns the new max)

// ---------------------------------------------------------------- GPU Stepper (libgravsim_hip)
typedef struct gs_stepper gs_stepper;

int gs_stepper_create(const gs_config* cfg, gs_stepper** out);
int gs_stepper_destroy(gs_stepper* s);
int gs_stepper_layout(gs_stepper* s, gs_layout* out);
// Generate ICs on device (every rank generates the full position set and its own velocities).
int gs_stepper_init_ics(gs_stepper* s, int32_t ic, uint64_t seed);
// Upload a global fp64 state (pos n*3, vel n*3, mass n). Every rank passes the full arrays.
int gs_stepper_set_state(gs_stepper* s, const double* pos, const double* vel, const double* mass);
// Download: full gathered positions (n*3), this rank's velocities (global layout n*3: only the
// rank's own rows are written), masses (n). Any pointer may be NULL.
int gs_stepper_get_state(gs_stepper* s, double* pos, double* vel, double* mass);
// Enqueue n steps (asynchronous w.r.t. the host).
int gs_stepper_step(gs_stepper* s, int32_t nsteps);
int gs_stepper_sync(gs_stepper* s);
// Bounded wait (timeout_s <= 0: unbounded) polling RCCL async errors; aborts the communicator
// when no enqueued step completes for timeout_s (the deadline bounds progress, not the run).
int gs_stepper_wait(gs_stepper* s, double timeout_s);
// Accelerations (+potential) of this rank's bodies for the current positions: acc4 = n_local*4.
int gs_stepper_accel(gs_stepper* s, double* acc4);
// Accelerations through the step's own force path (configured kernel and cutoff mode, no
// potential): what the integrator sees. acc4[:, 3] is 0.
int gs_stepper_accel_step_path(gs_stepper* s, double* acc4);
// Non-finite guard: returns number of non-finite position/velocity components on this rank.
int64_t gs_stepper_count_nonfinite(gs_stepper* s);
int64_t gs_stepper_steps_done(gs_stepper* s);
// 1 if the next step starts a replayable two-step period (an even step whose buffer still
// needs its gather, multi-rank): steps from here run from the graph / segmented plan.
int32_t gs_stepper_period_start(gs_stepper* s);
// Per-step phase timing of the last step (ms): up to the local/force phase, the step's
// collectives (all-gather + node-sum exchange spans on the comm stream), and the whole step.
int gs_stepper_phase_ms(gs_stepper* s, float* local_ms, float* comm_ms, float* total_ms);
// Eager steps record per-step phase events while on (hipGraph replay is off meanwhile).
int gs_stepper_set_timing(gs_stepper* s, int32_t on);
// Averages over the timed steps since the last call: out[0] steps, [1] step ms, [2] gather
// ms, [3] exchange ms, [4] exposed gather ms, [5] exposed exchange ms (compute-stream stalls),
// [6] the most force units a step deferred past the gather (overlap 3), [7] reserved.
int gs_stepper_phase_stats(gs_stepper* s, double* out8);
// Sym schedule work beside the all-gather: 0 wait then one launch, 3 one local-first launch
// whose remote units run once the gather is published or are deferred to a second launch
// behind it (the default for nranks > 1; GRAVSIM_SYM_OVERLAP sets another initial value).
int gs_stepper_set_overlap(gs_stepper* s, int32_t mode);
int32_t gs_stepper_get_overlap(gs_stepper* s);
// Units a dynamic-fetch workgroup may take after the first wave (<= 1: static units).
int32_t gs_stepper_get_dyn_cap(gs_stepper* s);
// Schedule knobs for an independent re-run (bench.py's replay audit): use_graph 0 eager,
// 1 single-rank graphs, 2 multi-rank capture too; dyn_cap <= 1 static units (one per
// workgroup), > 1 dynamic fetch with that many units per workgroup, < 0 unchanged.
int gs_stepper_set_schedule(gs_stepper* s, int32_t use_graph, int32_t dyn_cap);
// Test / A-B tuning of the sym schedule (< 0 or 0: unchanged): first_wave = workgroups of
// the dynamic launch that take one unit each (default: the resident slots; tests shrink it so
// small runs fetch dynamically too); fused_tail 1 / 0 forces the one-rank fused reduction
// tail / the three-kernel tail (default: fused up to 256K bodies). Same bits either way.
int gs_stepper_set_tuning(gs_stepper* s, int32_t first_wave, int32_t fused_tail);
// One-rank sym launches with persistent workgroups (1, the default) or round 4's workgroup
// turnover (0): same units and slots, same bits.
int gs_stepper_set_persist(gs_stepper* s, int32_t on);
// Re-resolve the force path with a new cutoff mode (0 auto, 1 exact select, 2 fast core).
int gs_stepper_set_cutoff_mode(gs_stepper* s, int32_t mode);
// Work audit of the sym schedule: force units completed since the last reset (waits for the
// compute stream) and the units one step must run on this rank (rows x (S + D + (Np - 1) Kr):
// a split segment counts as its Np parts, whichever way it runs); both 0 for the one-sided
// schedules.
int gs_stepper_audit(gs_stepper* s, uint64_t* units_done, uint64_t* units_per_step);
int gs_stepper_audit_reset(gs_stepper* s);
// Engine clock of the sym force launches since the last call (then reset; waits for the
// compute stream): out4[0] the duration-weighted shader clock (GHz, s_memtime against
// s_memrealtime per workgroup), [1] workgroup shader-cycles, [2] workgroup-seconds, [3]
// workgroups. All 0 for the one-sided schedules.
int gs_stepper_clock(gs_stepper* s, double* out4);
// Compiled force-tile shape of the sym kernels for fp64 (0) or fp32: *waves per workgroup,
// *ipl i-bodies and *jpl j-bodies per lane (bench.py builds its kernel label from this).
int gs_sym_tile_shape(int32_t fp64, int32_t* waves, int32_t* ipl, int32_t* jpl);
// What the last replayed steps ran from: *mode 0 eager, 1 one hipGraph per two steps, 2 a
// segmented plan (multi-rank: compute segments as graphs, collectives eager between them);
// *segments = graph segments per two steps (mode 2).
int gs_stepper_graph_info(gs_stepper* s, int32_t* mode, int32_t* segments);
// Steps per replayed one-rank graph launch (GRAVSIM_GRAPH_STEPS; 2 = one ping-pong period).
int gs_stepper_graph_steps(gs_stepper* s);
// Device memory ledger: entry i (name, bytes) of the HBM buffers this stepper owns; returns
// the entry count (i out of range: only the count).
int32_t gs_stepper_mem_entry(gs_stepper* s, int32_t i, const char** tag, uint64_t* bytes);
// Unit timeline of the last sym force launch (stepper created with GRAVSIM_UNIT_TRACE set):
// copies up to `cap` entries of 4 words {start, end (100 MHz ticks), HW_ID | XCC_ID << 32,
// row << 32 | segment} (all zero: the slot ran no unit) and clears them. Returns the count;
// out = nullptr returns the capacity; 0 when tracing is off.
int64_t gs_stepper_unit_trace(gs_stepper* s, uint64_t* out, int64_t cap);
// Bound on the host waiting for the oldest of the enqueued steps when it runs far ahead.
int gs_stepper_set_timeout(gs_stepper* s, double step_timeout_s);
// Resolved force path: *exact = 1 for the hard-cutoff select, *eps2 = r^2 offset in use.
int gs_stepper_force_mode(gs_stepper* s, int32_t* exact, double* eps2);
void* gs_stepper_compute_stream(gs_stepper* s);

// ---------------------------------------------------------------- Hermite (libgravsim_hip)
// 4th-order Hermite predictor-corrector (Makino & Aarseth 1992): hermite.hip, the
// acceleration+jerk kernel in nbody_hermite.hip. Uses cfg's n, dtype, device, dt (the fixed step,
// or the ceiling of the adaptive one), G, cutoff, softening, chunk, ipl (0 auto; 1, 2, fp32: 4)
// and split_groups (chunk groups of the evaluate grid, 0 auto); every launch shape gives the
// same bits. Refuses cutoff == softening == 0.
// nranks > 1 (shared steps only: block steps and collisions are refused there): rank r owns the
// rows of gs_hermite_partition and predicts, evaluates and corrects those against all j; the
// predicted rows and the per-workgroup step minima are gathered every step, so every rank holds
// the same control block and a P-rank run equals the one-rank run bit for bit. The gathers are
// RCCL collectives (gs_hermite_comm_init) or, for P shards in one process, device copies
// (gs_hermite_group_*). A rank that would own no real body is refused.
typedef struct gs_hermite gs_hermite;
typedef struct gs_hermite_info {
  double time;      // time reached [s]
  double dt_last;   // size of the last step taken
  double dt_next;   // min(dt, min_i dt_i): the next step before the t_end cut (fixed step: dt)
  double dt_min;    // smallest step so far (a last step cut short by t_end not counted)
  int64_t steps;    // steps taken (steps enqueued past t_end are no-ops and not counted)
  int32_t finished; // t_end is set and reached
  int32_t ipl;      // resolved i-bodies per lane
  // block mode (0 otherwise): `steps` above then counts macro steps of dt
  int64_t block_steps;    // block steps taken
  int64_t body_steps;     // sum of their active bodies (pair evaluations = body_steps * n)
  int64_t level_clamped;  // times a body wanted a step below dt 2^-max_level
  int32_t level_max;      // deepest level any body has had
  int32_t narrow_max;     // active-set size up to which the j-parallel evaluate runs
  // collisions (0 when off)
  int64_t overlaps;       // bodies the reduces have seen overlapping their nearest neighbour
} gs_hermite_info;
int gs_hermite_create(const gs_config* cfg, gs_hermite** out);
int gs_hermite_destroy(gs_hermite* h);
int gs_hermite_layout(gs_hermite* h, gs_layout* out);
// eta > 0: shared adaptive step by Aarseth's criterion (0: fixed dt_max); t_end >= 0: stop
// there (the last step is cut to reach it exactly), t_end < 0: none. Call before the state is
// set: the first adaptive step, (eta / 2) min |a| / |j|, is formed when the run starts.
int gs_hermite_set_adaptive(gs_hermite* h, double eta, double dt_max, double t_end);
int gs_hermite_init_ics(gs_hermite* h, int32_t ic, uint64_t seed);
// Upload a global fp64 state at time t; the step count restarts at 0. acc / jerk NULL:
// evaluated from (pos, vel). Given (a resumed run: n*3 each, with the dt_next and dt_min its
// status reported; <= 0: none): taken as they are.
int gs_hermite_set_state(gs_hermite* h, const double* pos, const double* vel, const double* mass,
                         const double* acc, const double* jerk, double t, double dt_next,
                         double dt_min);
// Download (any pointer may be NULL): pos, vel, acc, jerk n*3, mass n.
int gs_hermite_get_state(gs_hermite* h, double* pos, double* vel, double* mass, double* acc,
                         double* jerk);
// (ax, ay, az, phi) and (jx, jy, jz, 0) of the current state through the step's own kernel.
int gs_hermite_derivs(gs_hermite* h, double* acc4, double* jerk4);
// Enqueue n steps (asynchronous: the step size and the time live on the device).
int gs_hermite_step(gs_hermite* h, int32_t nsteps);
int gs_hermite_sync(gs_hermite* h);
int gs_hermite_status(gs_hermite* h, gs_hermite_info* out);  // waits for the enqueued steps
int64_t gs_hermite_count_nonfinite(gs_hermite* h);
// Individual block time steps (Makino 1991). Body i steps by dt 2^-k_i (k_i in 0..max_level,
// max_level in 0..40), time is an integer count of ticks of dt 2^-max_level, and a block step
// predicts every body to the earliest due time, evaluates and corrects the bodies due then.
// Needs eta > 0 and t_end (if any) a whole multiple of dt; call after set_adaptive and before
// the state is set. gs_hermite_step(h, n) then advances n macro steps of dt (every multiple of
// dt synchronises all bodies): it enqueues block-step chains against a device-side target time
// and reads the status back once per 32 chains.
int gs_hermite_set_block(gs_hermite* h, int32_t on, int32_t max_level);
// narrow_max: active sets up to this size take the j-parallel evaluate kernel, larger ones the
// gathered i-owned kernel (0: always the latter; n: always the former; < 0: the default for
// n and dtype). It changes the summation order, hence bits; (re)allocates the partial buffer.
int gs_hermite_set_block_tuning(gs_hermite* h, int32_t narrow_max);
// Per-body time (ticks) and level, n each (either may be NULL). Setting them makes the run
// stand at min tb; the carried a, j stay as they are.
int gs_hermite_get_block_state(gs_hermite* h, int64_t* tb, int32_t* level);
int gs_hermite_set_block_state(gs_hermite* h, const int64_t* tb, const int32_t* level);
// (ax, ay, az, phi) and (jx, jy, jz, 0) of the n_idx listed bodies (ascending or not, each
// < n) at the current (x, v) through the block path's evaluate and reduce; row k belongs to
// idx[k]. path: 0 by narrow_max, 1 narrow (n_idx <= narrow_max), 2 wide.
int gs_hermite_derivs_active(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t path,
                             double* acc4, double* jerk4);
// The same, `reps` times back to back between two events: *ms (if given) gets the milliseconds
// per evaluate + reduce (bench/hermite_rate.py --active-sweep); acc4 / jerk4 may be NULL.
int gs_hermite_time_active(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t path,
                           int32_t reps, double* ms, double* acc4, double* jerk4);

// Nearest neighbours and collision detection, from the acceleration+jerk kernels themselves.
// Every body has a radius R >= 0; the pair measure of bodies i and j is
//   q_ij = r^2_ij - (R_i + R_j)^2        (r^2 the kernel's own: |d|^2 + softening^2),
// one fma on the pair's r^2 in the pair type. The nearest neighbour of i is the real body
// j != i of the smallest q_ij (massless bodies take part; a pair the pair law zeroes, r^2 <
// cutoff^2, does not), the lowest j on an exact tie, and (+inf, -1) when there is none. With all
// radii 0 it is the nearest body by distance. Body i overlaps its neighbour when
// q_i < softening^2, that is |d|^2 < (R_i + R_j)^2. q and the neighbour of a body are
// bit-identical across ipl, chunk groups, the block paths, active sets and slots.
// on: 0 off (the default: the kernels of a run without collisions are unchanged), 1 record,
// 2 record and stop: a shared-step run takes no further step once a step has seen an overlap
// (later gs_hermite_step calls are no-ops, as past t_end) until gs_hermite_clear_overlap; a
// block-step run always runs on to the macro boundary. Call before the state is set. The call
// re-resolves the launch shape: a GS_MIXED run with collisions on has 2 i-bodies per lane at
// most (gs_hermite_layout and gs_hermite_info.ipl report what runs).
int gs_hermite_set_collisions(gs_hermite* h, int32_t on);
int gs_hermite_set_radii(gs_hermite* h, const double* r);  // n radii [m]; before the state
// The latest q and neighbour of every body (n each; either may be NULL): from the evaluation
// the run started with, or the last step that corrected the body.
int gs_hermite_neighbours(gs_hermite* h, double* q, int32_t* nn);
// Closest approach: the smallest q over the body's evaluations since the record was last
// cleared (by setting a state, or by clear != 0 here), and the neighbour then.
int gs_hermite_closest(gs_hermite* h, double* q, int32_t* nn, int32_t clear);
int gs_hermite_clear_overlap(gs_hermite* h);  // overlaps <- 0: a stopped run steps again
// gs_hermite_derivs / gs_hermite_derivs_active with q and the neighbour of each row too
// (either may be NULL); neither touches the records or the overlap count.
int gs_hermite_derivs_nn(gs_hermite* h, double* acc4, double* jerk4, double* q, int32_t* nn);
int gs_hermite_derivs_active_nn(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t path,
                                double* acc4, double* jerk4, double* q, int32_t* nn);

// 6th-order scheme (Nitadori & Makino 2008; gs_hermite_scheme.h, nbody_hermite6.hip): the state also
// carries the snap s = a'' and the crackle c = a''', and the one force pass of a step returns
// a, j and s at the predicted (x, v, a). One shared step (fixed, or adaptive with
//   dt_i = eta ((|a||s| + |j|^2) / (|c||a^(5)| + |a^(4)|^2))^(1/6),
// eta linear: useful values are 0.2 to 0.5), fp32 or fp64, one rank. gs_hermite_set_order(h, 6)
// refuses GS_MIXED, nranks > 1, block steps and collisions, and once the order is 6
// gs_hermite_set_block, gs_hermite_set_collisions and the gs_hermite_group_* calls refuse.
// Block steps of order 6 are an explicit choice, gs_hermite_set_block6 below. Call
// it before the state is set (like gs_hermite_set_block); order 4 frees the extra arrays again.
// cfg's ipl: 0 auto, 1, or 2 for fp32 (gs_hermite6_ipl_ok). A run starts with c = 0 and two
// evaluate passes: with ap = 0 for a and j, then with ap = a for s.
// gs_hermite_step, _sync, _status, _get_state, _set_adaptive and _count_nonfinite work as for
// order 4; gs_hermite_set_state starts the derivatives afresh from (pos, vel) at time t, and
// gs_hermite_derivs returns a and j of gs_hermite_derivs6.
int gs_hermite_set_order(gs_hermite* h, int32_t order);
int32_t gs_hermite_get_order(gs_hermite* h);
int32_t gs_hermite6_ipl_ok(int32_t fp64, int32_t ipl);  // 1 if that evaluate form is compiled
// gs_hermite_set_state with the carried snap and crackle too (n*3 each): with all four of acc,
// jerk, snap, crackle a resumed run continues bit for bit; with any of them NULL all start afresh.
int gs_hermite_set_state6(gs_hermite* h, const double* pos, const double* vel, const double* mass,
                          const double* acc, const double* jerk, const double* snap,
                          const double* crackle, double t, double dt_next, double dt_min);
// The carried snap and crackle, n*3 each (either may be NULL); a, j: gs_hermite_get_state.
int gs_hermite_get_carried6(gs_hermite* h, double* snap, double* crackle);
// (ax, ay, az, phi), (jx, jy, jz, 0) and (sx, sy, sz, 0) of the current (x, v), the snap at the
// acceleration of that state, through the step's own kernel (any pointer may be NULL).
int gs_hermite_derivs6(gs_hermite* h, double* acc4, double* jerk4, double* snap4);
// Block steps of an order-6 engine, fp64 only (in fp32 pair arithmetic, also with fp64 state and
// sums, the order-6 step criterion collapses: docs/DESIGN.md section 21): gs_hermite_set_block for
// order 6, with its arguments and conditions (one rank, eta > 0, t_end a multiple of dt); off (on
// = 0) before the order changes again. The block state, tuning and status calls are order 4's.
int gs_hermite_set_block6(gs_hermite* h, int32_t on, int32_t max_level);
// Order 6 in block mode: gs_hermite_derivs_active / gs_hermite_time_active with the snap. One
// pass at the rows (x, v, carried a) of the current state, so the snap is taken at the carried
// acceleration; row k belongs to idx[k], path as for order 4.
int gs_hermite_derivs_active6(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t path,
                              double* acc4, double* jerk4, double* snap4);
int gs_hermite_time_active6(gs_hermite* h, const int32_t* idx, int32_t n_idx, int32_t path,
                            int32_t reps, double* ms, double* acc4, double* jerk4,
                            double* snap4);

// ---------------------------------------------------------------- k nearest neighbours
// (nbody_knn.hip; the Casertano & Hut local density and the cluster read-outs rest on it.)
// The k nearest neighbours of body i are the first k entries of the ascending lexicographic
// order on (r^2_ij, j) over the real bodies j != i: the body itself is left out by index, not by
// distance (another body at the same position is a neighbour at r^2 = 0). r^2 is formed in the
// pair type, d = x_j - x_i per component (GS_MIXED: (hi_j - hi_i) + (lo_j - lo_i) on the
// double-single rows), r^2 = fma(dz, dz, fma(dy, dy, dx dx)); no softening, no cutoff. Entries
// past the n - 1 neighbours there are read (+inf, -1). The order is total: every launch shape
// (ipl, groups) gives the same bits, and they are the bits of gs_cpu_knn_*.
// gs_hip_knn is stateless: pos n*3 fp64 (rounded to the pair type as the engines do), k in 1..8,
// ipl 0 auto / 1 / 2, groups (chunk groups of the grid) 0 auto; r2 n*k doubles ascending, idx n*k.
// It pads, uploads, launches, merges, downloads and frees on a stream of its own, restores the
// caller's device and leaves no device state behind, so it may run beside a live engine.
int gs_hip_knn(const double* pos, int64_t n, int32_t dtype, int32_t k, int32_t ipl,
               int32_t groups, int32_t device, double* r2, int32_t* idx);
// The same pass `reps` times, nothing downloaded: ms[r] gets the milliseconds of launch + merge
// r between two events (bench/knn_rate.py); info4 (may be NULL): n_pad, ipl, groups, chunk.
int gs_hip_knn_time(const double* pos, int64_t n, int32_t dtype, int32_t k, int32_t ipl,
                    int32_t groups, int32_t device, int32_t reps, double* ms, int64_t* info4);
int32_t gs_knn_ipl_ok(int32_t dtype, int32_t ipl);  // 1 if that form is compiled (0: auto)
int32_t gs_knn_early_out(void);  // 1 if the insertion chain sits behind the wave-uniform test

// Virtual ranks on one device: shards[r] created with rank r of P; steps all of them in
// lockstep with the all-gather done by device copies (the RCCL schedule without RCCL).
int gs_group_step(gs_stepper** shards, int32_t P, int32_t nsteps);
// The same for Hermite shards (shards[r] created with rank r of P on one device, the state set on
// each): every shard runs the slice kernels and the control kernel of the RCCL path. nsteps 0
// only completes what setting the states left open (the gather of the first step minima).
// The reads return all n rows (as gs_hermite_get_state / gs_hermite_derivs on every rank of an
// RCCL run). gs_hermite_group_time_eval: milliseconds per evaluate launch of each shard
// (ms[P], device events around `reps` launches at the shard's current predicted rows).
int gs_hermite_group_step(gs_hermite** shards, int32_t P, int32_t nsteps);
int gs_hermite_group_get_state(gs_hermite** shards, int32_t P, double* pos, double* vel,
                               double* mass, double* acc, double* jerk);
int gs_hermite_group_derivs(gs_hermite** shards, int32_t P, double* acc4, double* jerk4);
int gs_hermite_group_time_eval(gs_hermite** shards, int32_t P, int32_t reps, double* ms);

// RCCL for a multi-rank Hermite run, one process per GPU (as gs_stepper_comm_init / _comm_info /
// _comm_check / gs_stepper_abort): the gathers of a step are in-place ncclAllGather calls on
// the engine's one stream (equal slices), or grouped in-place ncclBroadcast calls (uneven ones).
// Collective; call before the state is set. gs_hermite_sync then polls the stream and the
// communicator's async error, and aborts the communicator when nothing completes for
// timeout_s (gs_hermite_set_step_timeout; 0: no limit).
int gs_hermite_comm_init(gs_hermite* h, const void* id128, int32_t rank, int32_t nranks);
int gs_hermite_comm_info(gs_hermite* h, int32_t* count, int32_t* user_rank, int32_t* cu_device);
int gs_hermite_comm_check(gs_hermite* h);
int32_t gs_hermite_abort(gs_hermite* h);
int gs_hermite_set_step_timeout(gs_hermite* h, double timeout_s);

// RCCL: 128-byte unique id (rank 0 creates it; the launcher broadcasts it), then init.
int gs_rccl_unique_id(void* out128);
int gs_stepper_comm_init(gs_stepper* s, const void* id128, int32_t rank, int32_t nranks);
// Poll RCCL async errors; aborts the communicator on error. Returns 0 if healthy.
int gs_stepper_comm_check(gs_stepper* s);
// How far gs_stepper_comm_init got (safe to call from another thread, e.g. a watchdog):
// 0 not started, 1 in ncclCommInitRank, 2 warm-up all-gather, 3 warm-up ring send/recv,
// 4 warm-up peer send/recv, 5 waiting for the warm-up, 6 done, -1 aborted.
int32_t gs_stepper_comm_stage(gs_stepper* s);
// What the communicator is (ncclCommCount, ncclCommUserRank, ncclCommCuDevice, read at init
// and checked there against nranks / rank / the stepper's device): count 0 before comm_init
// or when none was kept (one rank).
int gs_stepper_comm_info(gs_stepper* s, int32_t* count, int32_t* user_rank, int32_t* cu_device);
// Abort the live RCCL communicator once (ncclCommAbort; callable from another thread to
// unblock collectives that will never complete). Returns 1 if it aborted, 0 if there was none.
int32_t gs_stepper_abort(gs_stepper* s);

int gs_hip_device_count(void);
const char* gs_hip_kernel_info(void);

// ---------------------------------------------------------------- HIP IPC (ipc.hip)
// Cross-process sharing of device memory and events on one node: what RCCL's intra-node P2P
// transport builds on (tests/test_ipc_gpu.py). Handles are HIP_IPC_HANDLE_SIZE (64) bytes.
int gs_dev_alloc(int32_t device, uint64_t bytes, void** out);
int gs_dev_free(void* p);
int gs_dev_copy(void* dst, const void* src, uint64_t bytes, int32_t to_device);
int gs_ipc_mem_handle(void* p, void* out64);
int gs_ipc_mem_open(int32_t device, const void* h64, void** out);
int gs_ipc_mem_close(void* p);
int gs_ipc_event_create(int32_t device, void** ev, void* out64);
int gs_ipc_event_open(int32_t device, const void* h64, void** ev);
int gs_event_record_sync(void* ev);
int gs_event_wait_sync(void* ev);
int gs_event_destroy(void* ev);

// ---------------------------------------------------------------- errors
const char* gs_last_error(void);

#ifdef __cplusplus
}
#endif
