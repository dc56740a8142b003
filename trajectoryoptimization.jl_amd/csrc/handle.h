// handle.h — host-side state behind a to_handle and the per-model launch table.  The kernels of one model are
// instantiated in their own translation units (ops_*.hip: the Quadrotor forward pass alone is a minute of compile
// time); trajopt_hip.hip holds the C-ABI and the model-independent kernels and reaches the rest through ModelOps.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "common.h"
#include "path_plan.h"
#include "rp_plan.h"

namespace to {

int fail(int code, const std::string& msg);  // records the message for to_last_error(), returns code
struct MpcDualCon;  // k_mpc.h (one translation unit only)

#define HIPCHECK(expr)                                                                         \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return ::to::fail(TO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
  } while (0)
#define TRY(expr) do { int r_ = (expr); if (r_ != TO_OK) return r_; } while (0)

constexpr int BLOCK = 64;  // one wave per workgroup: a small batch is spread over as many CUs as possible

// THE launch sequence of every kernel of the library.  enqueue() puts a kernel on a stream; launched() checks hipGetLastError() and returns
// TO_OK / TO_ERR_HIP; launch() is one after the other.  A launcher of several kernels enqueues all but the last: one check per launcher.
template <class... P, class... A>
inline void enqueue(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}
inline int launched() {
  HIPCHECK(hipGetLastError());
  return TO_OK;
}
template <class... P, class... A>
inline int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
  enqueue(kernel, grid, block, lds, stream, args...);
  return launched();
}

struct ModelOps;

}  // namespace to

struct to_handle_s {
  int device = 0;
  hipStream_t stream = nullptr;
  int model_key = -1;
  const to::ModelOps* ops = nullptr;
  int R = 0, G = 0;  // lanes per trajectory / trajectories per wave of the column-layout kernels
  to::KArgs a;       // host copy of the kernel argument block (device pointers inside)
  std::vector<to_cost_desc> costs;
  std::vector<to::DevCon> cons;
  std::vector<double> dt;
  std::vector<int> cost_index;
  std::vector<double> step_table;  // TO_MODEL_VECTOR: host copy of the per-step model table (models.h ModelVectorModel)
  std::vector<void*> allocs;
  double* stage = nullptr;  // device staging buffer in host layout
  size_t stage_bytes = 0;
  int* counter_host = nullptr;  // pinned
  int counter_len = 0;
  to::PathTraits traits;  // what `ops` tells the host logic (path_plan.h), built once at to_create
  to::PathPlan plan;      // the kernel path of this handle's solves and the candidate-buffer sizes that follow from it (path_plan.h plan_paths)
  int list_active = 0;    // list mode (KArgs::fwd_list): the last active count the solve loop has seen — what k_forward2's grid is sized for
  bool sync_debug = false;  // TRAJOPT_SYNC_DEBUG as the solve in flight read it (solve_loop.h read_solve_knobs): a synchronisation and a stderr line per batch step
  int accept_chunks = 1;  // grid.z of k_accept (a chunk is >= 32 elements of [X; U]: the copy is latency-bound per wave)
  // device copies of the descriptor tables
  to_cost_desc* d_costs = nullptr;
  to::DevCon* d_cons = nullptr;
  double* d_dt = nullptr;
  int* d_cost_index = nullptr;
  int* d_crow = nullptr;    // [64] compact_row table of the model (tangent-matrix getters)
  // Per-trajectory tables, all tiled (entry e of trajectory b at ((b >> 6) * L + e) * 64 + (b & 63)) and allocated on first use; the DevProblem
  // pointer of the same name is set while the table is in effect.  Two families:
  //  - zero-filled arrays of L * Bp doubles, written a block of rows at a time through upload_vec (tiled on the device): gl, cp, track_ref;
  //  - arrays with one spare tile whose lanes behind the batch hold the SHARED value of their row, written whole through upload_tiled (tiled on
  //    the host, desc_lower.h tile_rows): pm, dtb, cl, gw, ga.
  double* d_gl = nullptr;    // linear cost terms (DevProblem::gl), L = n_costs * (n + m); k_track.h lowers a tracking window into it
  std::vector<char> gl_set;  // [n_costs] cost i carries per-trajectory linear terms (all clear: DevProblem::gl goes back to null)
  double* d_cp = nullptr;    // constraint parameters (DevProblem::cp), L = (n + m) * number of constraints
  double* d_track_ref = nullptr;      // one tracking reference per trajectory (to_set_tracking_reference_batch), L = track_Nref * (n + m): rows
                                      // [x_ref[j]; u_ref[j]] (u rows zero while track_u is false)
  int* d_track_start = nullptr;       // [B] 1-based window starts, re-uploaded by every window call
  std::vector<int32_t> track_start;   // host copy of the starts (to_get_tracking_window)
  int track_Nref = 0, track_end = 0;  // knots of the stored reference (0: none) and its end mode (TO_TRACK_END_*)
  bool track_u = false;               // the reference carries controls
  to::MpcDualCon* d_dual_cons = nullptr;  // to_mpc_shift_duals (k_mpc.h): {dual_off, p, nk} per constraint, written on first use (the constraints are fixed at to_create)
  int* d_dual_action = nullptr;           // ... and the [Bp] actions of a call
  double* d_pm = nullptr;        // model parameters (DevProblem::pm), L = 16
  std::vector<double> pm_host;   // [16, B] host copy of what DevProblem::pm holds: what to_set_model_params_batch was given, or — pm_own false, the handle
                                 // carries per-trajectory time steps only — the shared parameters repeated (empty: DevProblem::pm is null)
  bool pm_own = false;           // to_set_model_params_batch is in effect (to_clear_model_params_batch / to_clear_time_steps_batch: which of the two keeps pm alive)
  double* d_dtb = nullptr;       // time steps (DevProblem::dtb), L = N - 1
  std::vector<double> dtb_host;  // [N-1, B] what to_set_time_steps_batch was given (empty: shared steps)
  double* d_cl = nullptr;        // constraint limits (DevProblem::cl), L = n_cl = summed p of the constraints
  std::vector<int> cl_base;                  // [n_cons] first row of constraint i's block in d_cl
  std::vector<std::vector<double>> cl_host;  // [n_cons] limits[q, B] as to_set_constraint_limits_batch was given them (empty: shared limits)
  double* d_gw = nullptr;        // cost weights (DevProblem::gw), L = n_costs * (n + m)
  std::vector<double> gw_host;   // [L, B] the diagonal Q / R every trajectory's costs are evaluated with (desc_lower.h cost_weights_fill; empty: DevProblem::gw is null)
  double* d_ga = nullptr;        // attitude references (DevProblem::ga), L = 4 * n_costs.  The device array is the truth after its first fill
                                 // (k_track_lower writes it); set with d_gw and cleared with it
  to::CostLaneState lane;        // why gw / ga are set: the caller's weights, the caller's attitudes, attitude tracking (path_plan.h cost_lane_step)
  double* d_tmp = nullptr;  // [Bp] scratch for reductions / outputs
  double* d_tmp2 = nullptr;
  // multi-GPU: RCCL communicator of the batch shards (to_comm_*; librccl is dlopen'ed on first use)
  void* comm = nullptr;
  int comm_rank = 0, comm_size = 1;
  std::vector<int32_t> comm_counts;  // shard size of every rank (exchanged at to_comm_init_rank)
  long long comm_offset = 0, comm_total = 0;  // global index of this rank's first trajectory; sum of the shards
  bool comm_equal = true;            // all shards equal: one in-place all-gather, else grouped broadcasts
  // projected-Newton polish (k_pn.h): workspace and tables, allocated on first use
  double* pn_ws = nullptr;
  size_t pn_ws_bytes = 0;
  int* pn_pak = nullptr;
  long long* pn_koff = nullptr;
  int* pn_list = nullptr;        // [Bp] device: the trajectory polished in workspace slot i
  int* pn_list_host = nullptr;   // [Bp] pinned: where the lists are assembled
  int pn_tab_len = 0;
  int pn_cap = 0, pn_nbmax = 0;  // workspace slots; max_k (ne + candidate rows of knot k)
  long long pn_per = 0;          // doubles per slot
  hipStream_t pn_stream = nullptr;  // low-priority stream of the early polish (altro_solve), created on first use
  hipEvent_t pn_ev[3] = {nullptr, nullptr, nullptr};  // snapshot taken / early polish enqueued up to here / timing
  int32_t *snap_status = nullptr, *snap_active = nullptr;  // pinned [Bp]: snapshots of the per-trajectory solver state
  double* snap_cmax = nullptr;
  int pn_early = 0;              // > 0 inside altro_solve: the AL loop hands finished trajectories to the polish up to this many times
  std::vector<char> pn_done_early;  // [B] polished while the AL stage was still running
  int pn_early_slots = 0;        // workspace slots handed out so far
  to_solver_opts pn_opts;        // the options the polish runs with (the AL stage runs with a looser constraint_tolerance)
  double pn_early_ms = 0.0;
  // repacked working set (k_generic.h k_repack_*): the per-trajectory arrays a solve carries from step to step, their home pointers,
  // two working copies (B/2 and B/4 trajectories: ping-pong) and the working position -> home index maps
  struct RpArr { size_t off; int kind; int L; };  // off: byte offset of the pointer field inside KArgs
  std::vector<RpArr> rp_arr;
  std::vector<void*> rp_home, rp_work[2];
  int* rp_map[2] = {nullptr, nullptr};
  to::RpSized rp_sized[2];  // what each working set's buffers were sized for (rp_plan.h: re-used only for the same arrays within the capacity)
  int rp_level = 0;      // 0: the kernels work on the home arrays; else on rp_work[(rp_level - 1) & 1]
  int rp_B = 0, rp_Bp = 0;  // the batch of the handle while a solve works on a smaller set
  // closed-loop policy rollouts (to_policy_rollout): start states and per-sample results, sized for the largest S*B seen so far, and
  // the sample-fastest staging of one chunk of waves when the trajectories are wanted
  double *pol_x0s = nullptr, *pol_J = nullptr, *pol_cmax = nullptr, *pol_dxmax = nullptr;
  int *pol_status = nullptr, *pol_klim = nullptr;
  size_t pol_cap = 0;        // samples the arrays above hold
  double *pol_xw = nullptr, *pol_uw = nullptr;
  int pol_waves = 0;         // waves the staging holds
  double* pol_plants = nullptr;  // to_policy_rollout_mc: [16, S*B] one plant per sample
  size_t pol_plants_cap = 0;     // samples it holds
  // asynchronous solves (to_*_solve_async / to_solve_wait)
  std::thread worker;
  std::atomic<bool> inflight{false};
  int async_rc = 0;
  std::string async_err;
  // progress of the solve in flight, as the solve loop last saw it (to_solve_progress / to_solve_wait_below: a host that
  // pipelines solves over several handles admits the next one when the one in flight has drained)
  std::atomic<int> prog_active{0};   // trajectories still iterating (B when a solve starts, 0 once its iLQR / AL stage has ended)
  std::atomic<int> prog_steps{0};    // batch steps whose counters have been read
  std::mutex prog_mu;
  std::condition_variable prog_cv;
  int last_steps = 0;     // batch steps and device time of the last solve (fill_stats)
  double last_ms = 0.0;
  // TRAJOPT_GUARD=1 (read at to_create): every device array of the handle sits between two red zones filled with a pattern, checked after
  // every batch step of a solve and every phase-API call — an out-of-bounds store of a kernel is reported where it happens, by array name,
  // instead of surfacing as a fault at whatever batch size happens to cross a mapping boundary (sanitizer hook; GPU ASan is
  // not available on this pool)
  bool guard = false;
  struct GuardRec { void* base; void* payload; size_t bytes; std::string name; };
  std::vector<GuardRec> guards;
  void* guard_tab = nullptr;   // device copy of the zone addresses (rebuilt when `guards` changes)
  int* guard_bad = nullptr;    // device: index of the first damaged zone, else INT_MAX
  bool guard_dirty = true;
  // measurement
  bool profile = false;
  std::vector<hipEvent_t> ev;  // event pool, 4 per batch step
  hipEvent_t sev[4] = {nullptr, nullptr, nullptr, nullptr};  // solve(): start, stop, two chunk read-back events (created once)
  double prof_ms[TO_PROFILE_SLOTS] = {0, 0, 0, 0};
  int64_t prof_launches[TO_PROFILE_SLOTS] = {0, 0, 0, 0};
};

namespace to {

// Launchers of the model-templated kernels (all enqueue on h->stream and return TO_OK / TO_ERR_HIP).
struct ModelOps {
  // model traits the host logic needs
  bool write_through = false;  // M::accept_write_through
  bool mfma_backward = false;  // M::mfma_backward: tangent-matrix expansion + one-wave-per-trajectory Riccati
  bool coop_backward = true;   // M::coop_backward: column-layout expansion + cooperative LDS Riccati
  bool lane_backward = false;  // M::lane_backward: lane-layout expansion + one-lane-per-trajectory Riccati (ne + m <= 6)
  bool lds_gains = false;      // forward pass stages gains through LDS
  int expand_knots = 1;
  int ls_first_round = 16;     // M::ls_first_round
  int gains_lds_pieces = 0;    // 16-byte pieces of one gains row (LDS sizing of the forward pass)
  int crow[64];                // compact_row(g, c) of the tangent-matrix layout
  int nep = 0, rs = 0;         // Tm<M>::NEP, Tm<M>::RS
  // Entries indexed [plants]: [1] is the flagged instance that loads one plant per trajectory (DevProblem::pm set, to_set_model_params_batch;
  // ops_plants_*.hip), null where a model has none.  A handle with pm set runs the general variants only (path_plan.h `plants`), so there is
  // one expansion per layout, the general forward variants (index = the mode, bit 3 set) and no fused / scan / packed / two-wave instance.
  int (*rollout[2])(to_handle*) = {};
  int (*cost)(to_handle*, int with_al, double* out, double* Jk) = nullptr;
  int (*violation)(to_handle*, double* out) = nullptr;
  int (*dual_update)(to_handle*) = nullptr;
  int (*outer)(to_handle*) = nullptr;
  int (*cost_derivs)(to_handle*, double* grad, double* hess) = nullptr;
  int (*discrete_jacobian[2])(to_handle*, double* F) = {};
  int (*constraint_eval)(to_handle*, int ci, double* vals, double* jac) = nullptr;
  int (*constraint_hessian)(to_handle*, int ci, const double* lambda, double* H) = nullptr;
  int (*expand[2])(to_handle*) = {};             // [0] picks layout, variant and kernel itself (ops.h op_expand); [1]: column and tangent-matrix layouts, general variant
  int (*expand_const)(to_handle*) = nullptr;     // packed expansion: the constant columns of [A B], written once per handle (k_expand_const_columns)
  int (*backward)(to_handle*) = nullptr;
  int (*expand_lane_k[2])(to_handle*) = {};      // lane-layout expansion, one lane per (trajectory, knot) (ops_lane.h; [0] null: column-per-lane kernel; [1]: general variant)
  int (*expand_backward)(to_handle*) = nullptr;  // fused lane expansion + Riccati (small models; null elsewhere)
  int (*expand_backward_scan)(to_handle*) = nullptr;  // fused expansion + scan Riccati, one wave per trajectory (k_scan.h)
  int (*expand_backward_coop)(to_handle*) = nullptr;  // fused expansion + cooperative Riccati (small models with <= 8 directions)
  int (*pn_prepare)(to_handle*, int want) = nullptr;  // projected-Newton polish (k_pn.h): tables + workspace slots ...
  int (*pn_launch[2])(to_handle*, int slot0, int count, hipStream_t stream, const to_solver_opts* opts) = {};  // ... and its launches
  int (*defect[2])(to_handle*, double* out) = {};               // max dynamics / initial-condition defect of the nominal trajectory
  int (*infeasible_controls)(to_handle*) = nullptr;             // InfeasibleModel only: slack controls from the current states (k_misc.h)
  // closed-loop policy rollout of `waves` waves from pa.g0 (k_policy.h): nz = the kernel's NZ, 0 (ops_policy.hip) or one of the stochastic
  // instances 1 .. 7 (ops_policy_mc.hip); noise_mask = the bits of nz this model has instances for
  int (*policy_rollout)(to_handle*, const PolicyArgs& pa, int waves) = nullptr;
  int (*policy_rollout_mc)(to_handle*, const PolicyArgs& pa, int waves, int nz) = nullptr;
  int policy_noise_mask = 0;
  int (*accept_roll)(to_handle*) = nullptr;  // accept by re-rolling the stored controls (k_forward.h; models without write-through)
  int (*forward[2][32])(to_handle*) = {};  // by kernel variant (k_forward.h MODE bits); variants a model never uses stay null
  int (*forward2[32])(to_handle*) = {};  // the same variants as two-wave workgroups (k_forward2; models with LDS-staged gains)
  // every kernel that reads model parameters has its flagged instance (lane: on the lane layout), the per-sample plant of the policy rollout included
  bool plants(bool lane) const {
    return rollout[1] && discrete_jacobian[1] && expand[1] && defect[1] && pn_launch[1] && forward[1][8] && (!lane || expand_lane_k[1]) && policy_rollout_mc &&
           (policy_noise_mask & 4);
  }
};

// each ops_*.hip fills the entries it instantiates; table indexed by model key (0..2 double integrator D=1..3, 3 Cartpole,
// 4 Quadrotor, 5 Quadrotor{MRP}, 6 Quadrotor{RodriguesParam}, 7 hybrid double integrator, 8 general model vector)
constexpr int N_MODEL_KEYS = 12;  // ... 9, 10 InfeasibleModel over the 1-D / 2-D double integrator, 11 over the Cartpole
// THE list of the ops_*.hip translation units: fill_ops_<unit> is declared and called (fill_model_ops) from here, so a unit cannot be one without the other
#define TO_OPS_UNITS(X)                                                                                                                          \
  X(small) X(small_forward) X(small_lane) X(quad_misc) X(quad_expand) X(quad_backward) X(quad_forward_a) X(quad_forward_b) X(quad_forward_c)      \
  X(quad_forward2_a) X(quad_forward2_b) X(quad_forward2_c) X(quadatt_misc) X(quadmrp_expand) X(quadrp_expand) X(quadmrp_forward) X(quadrp_forward) \
  X(hybrid) X(small_forward2) X(small_scan) X(pn) X(vector) X(infeasible_a) X(infeasible_b) X(policy) X(policy_mc)                                \
  X(plants_small) X(plants_lane) X(plants_forward) X(plants_quad) X(plants_quad_forward) X(plants_pn)
#define TO_OPS_DECLARE(unit) void fill_ops_##unit(ModelOps* table);
#define TO_OPS_CALL(unit) fill_ops_##unit(table);
TO_OPS_UNITS(TO_OPS_DECLARE)
inline void fill_model_ops(ModelOps* table) { TO_OPS_UNITS(TO_OPS_CALL) }
#undef TO_OPS_DECLARE
#undef TO_OPS_CALL

// handle-owned device memory (red zones around it in guard mode); g_free accepts what g_malloc returned
int g_malloc(to_handle* h, void** p, size_t bytes, const char* name);
void g_free(to_handle* h, void* p);
int check_guards(to_handle* h, const char* where);

inline dim3 grid_b(const to_handle* h, int y = 1, int z = 1) { return dim3(h->a.P.Bp / BLOCK, y, z); }

// Per-trajectory time steps (DevProblem::dtb) ride on the flagged instances, which exist twice (problem_dev.h step_dt_of): body(bool_constant<DT>)
// with DT = the handle carries them.  Chosen here, inside the launcher of entry [1] (ops.h, ops_lane.h, ops_pn.h): the ModelOps table does not grow, a handle with plants alone
// launches the kernels it always did, and the unflagged launchers (PM = false) never see a DT instance.
template <class M> struct TimeStepsModel : std::false_type {};  // the models to_set_time_steps_batch accepts
template <int D> struct TimeStepsModel<DoubleIntegratorModel<D>> : std::true_type {};
template <> struct TimeStepsModel<CartpoleModel> : std::true_type {};
template <> struct TimeStepsModel<QuadrotorModel> : std::true_type {};
template <class M, bool PM, class F>
int with_time_steps(const to_handle* h, F&& body) {
  if constexpr (PM && TimeStepsModel<M>::value) {
    if (h->a.P.dtb != nullptr) return body(std::true_type{});
  }
  return body(std::false_type{});
}

// Per-trajectory cost weights (DevProblem::gw, to_set_cost_weights_batch): body(bool_constant<GW>) with GW = the handle carries them.  The kernels
// that read a cost's diagonal outside the forward passes exist twice, and a handle without weights launches the instance it always did
// (problem_dev.h cost_wq); the expansion kernels carry the same choice as bit 3 of their variant (ops.h with_variant).  The models the setter
// refuses (desc_lower.h validate_cost_weights_target) have no second instance.
template <class M> struct CostWeightsModel : std::true_type {};
template <> struct CostWeightsModel<HybridDoubleIntegratorModel> : std::false_type {};
template <> struct CostWeightsModel<ModelVectorModel> : std::false_type {};
template <class Base> struct CostWeightsModel<InfeasibleModel<Base>> : std::false_type {};
template <class M, class F>
int with_weights(const to_handle* h, F&& body) {
  if constexpr (CostWeightsModel<M>::value) {
    if (h->a.P.gw != nullptr) return body(std::true_type{});
  }
  return body(std::false_type{});
}

}  // namespace to
