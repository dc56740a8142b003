// trajopt_hip.hip — host side of libtrajopt_hip.so: descriptor validation, device storage, kernel
// launches and the C-ABI declared in include/trajopt_hip.h.  gfx950 only; no CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <time.h>

#include <mutex>
#include <thread>

#include "desc_lower.h"
#include "fwd_list.h"
#include "handle.h"
#include "k_generic.h"
#include "k_mpc.h"
#include "k_track.h"
#include "policy_lower.h"
#include "solve_loop.h"

using namespace to;

namespace {
thread_local std::string g_err;
}
namespace to {
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}

namespace to {
// ---- guard mode (handle.h): red zones around every handle-owned device array ---------------------------------------------------------
constexpr size_t GUARD_BYTES = 4096;                          // per zone: half a tile row of the batch-fastest layout and then some
constexpr unsigned long long GUARD_WORD = 0xA5C3A5C3DEADBEEFull;
struct GuardZones { unsigned long long* front; unsigned long long* back; };
__global__ void k_guard_fill(unsigned long long* z) { z[blockIdx.x * 64 + threadIdx.x] = GUARD_WORD; }
__global__ void k_guard_check(const GuardZones* tab, int* bad) {
  const GuardZones g = tab[blockIdx.x];
  constexpr int words = (int)(GUARD_BYTES / 8);
  bool hit = false;
  for (int i = threadIdx.x; i < words; i += 64) hit = hit || g.front[i] != GUARD_WORD || g.back[i] != GUARD_WORD;
  if (hit) atomicMin(bad, (int)blockIdx.x);
}
__global__ void k_guard_poke(double* p, long long off) { p[off] = 1.0; }  // TRAJOPT_GUARD_SELFTEST: the overrun the check must find

int g_malloc(to_handle* h, void** p, size_t bytes, const char* name) {
  if (!h->guard) {
    HIPCHECK(hipMalloc(p, bytes));
    return TO_OK;
  }
  const size_t payload = (bytes + 255) / 256 * 256;  // the back zone starts right behind the (rounded-up) payload
  void* base = nullptr;
  HIPCHECK(hipMalloc(&base, payload + 2 * GUARD_BYTES));
  char* q = (char*)base + GUARD_BYTES;
  enqueue(k_guard_fill, dim3(GUARD_BYTES / 8 / 64), dim3(64), 0, h->stream, (unsigned long long*)base);
  enqueue(k_guard_fill, dim3(GUARD_BYTES / 8 / 64), dim3(64), 0, h->stream, (unsigned long long*)(q + payload));
  if (payload > bytes) HIPCHECK(hipMemsetAsync(q + bytes, 0, payload - bytes, h->stream));
  TRY(launched());
  h->guards.push_back({base, q, payload, name ? name : ""});
  h->guard_dirty = true;
  *p = q;
  return TO_OK;
}
void g_free(to_handle* h, void* p) {
  if (!p) return;
  if (h->guard)
    for (size_t i = 0; i < h->guards.size(); ++i)
      if (h->guards[i].payload == p) {
        hipFree(h->guards[i].base);
        h->guards.erase(h->guards.begin() + i);
        h->guard_dirty = true;
        return;
      }
  hipFree(p);
}
// every red zone of the handle intact?  Synchronises the stream (a debugging mode).
int check_guards(to_handle* h, const char* where) {
  if (!h->guard || h->guards.empty()) return TO_OK;
  if (!h->guard_bad) HIPCHECK(hipMalloc((void**)&h->guard_bad, sizeof(int)));
  if (h->guard_dirty) {
    std::vector<GuardZones> tab;
    for (const auto& g : h->guards) tab.push_back({(unsigned long long*)g.base, (unsigned long long*)((char*)g.payload + g.bytes)});
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (h->guard_tab) HIPCHECK(hipFree(h->guard_tab));
    HIPCHECK(hipMalloc(&h->guard_tab, tab.size() * sizeof(GuardZones)));
    HIPCHECK(hipMemcpy(h->guard_tab, tab.data(), tab.size() * sizeof(GuardZones), hipMemcpyHostToDevice));
    h->guard_dirty = false;
  }
  int bad = 0x7fffffff;
  HIPCHECK(hipMemcpyAsync(h->guard_bad, &bad, sizeof(int), hipMemcpyHostToDevice, h->stream));
  TRY(launch(k_guard_check, dim3((unsigned)h->guards.size()), dim3(64), 0, h->stream, (const GuardZones*)h->guard_tab, h->guard_bad));
  HIPCHECK(hipMemcpyAsync(&bad, h->guard_bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  if (bad != 0x7fffffff) {
    const auto& g = h->guards[bad];
    return fail(TO_ERR_HIP, "guard: a red zone of device array '" + g.name + "' (" + std::to_string(g.bytes) + " bytes) was overwritten — first seen after " + where);
  }
  return TO_OK;
}
}  // namespace to

namespace {

#define CHECK_H(h) do { if (!(h)) return fail(TO_ERR_NULL, "null handle"); } while (0)
#define CHECK_P(p) do { if (!(p)) return fail(TO_ERR_NULL, "null pointer"); } while (0)
#define CHECK_IDLE(h) do { if ((h)->inflight) return fail(TO_ERR_ARGUMENT, "an asynchronous solve is in flight on this handle (call to_solve_wait first)"); } while (0)

// launch table, one entry per model key; filled once by the ops_*.hip translation units
ModelOps g_ops[N_MODEL_KEYS];
std::once_flag g_ops_once;
const ModelOps* model_ops(int key) {
  std::call_once(g_ops_once, [] { fill_model_ops(g_ops); });
  return (key >= 0 && key < N_MODEL_KEYS) ? &g_ops[key] : nullptr;
}

template <class T>
int dev_alloc_named(to_handle* h, const char* name, T** p, size_t count, bool zero = true) {
  void* q = nullptr;
  TRY(g_malloc(h, &q, std::max<size_t>(count, 1) * sizeof(T), name));
  h->allocs.push_back(q);
  if (zero) HIPCHECK(hipMemsetAsync(q, 0, std::max<size_t>(count, 1) * sizeof(T), h->stream));
  *p = (T*)q;
  return TO_OK;
}
#define dev_alloc(h, p, ...) dev_alloc_named(h, #p, p, __VA_ARGS__)
// gives back an array of dev_alloc_named before to_destroy does (arrays that are re-sized)
template <class T>
void dev_release(to_handle* h, T** p) {
  if (!*p) return;
  h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), (void*)*p), h->allocs.end());
  g_free(h, *p);
  *p = nullptr;
}

int ensure_stage(to_handle* h, size_t bytes) {
  if (h->stage_bytes >= bytes) return TO_OK;
  if (h->stage) { HIPCHECK(hipStreamSynchronize(h->stream)); g_free(h, h->stage); h->stage = nullptr; h->stage_bytes = 0; }
  TRY(g_malloc(h, (void**)&h->stage, bytes, "stage"));
  h->stage_bytes = bytes;
  return TO_OK;
}

int use_device(to_handle* h) { HIPCHECK(hipSetDevice(h->device)); return TO_OK; }

// host (cnt per trajectory, column-major (dim, K, B)) -> tiled device array (elements e0..e0+cnt-1 of L) via the staging buffer
int upload_vec(to_handle* h, const double* host, double* d, int cnt, int L = -1, int e0 = 0) {
  if (L < 0) L = cnt;
  const size_t total = (size_t)cnt * h->a.P.B;
  TRY(ensure_stage(h, total * sizeof(double)));
  HIPCHECK(hipMemcpyAsync(h->stage, host, total * sizeof(double), hipMemcpyHostToDevice, h->stream));
  TRY(launch(k_to_device, grid_b(h, cnt), dim3(BLOCK), 0, h->stream, h->stage, d, L, e0, cnt, h->a.P.B));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
// host values[L, B] (NULL: the shared row for every trajectory) -> a spare-tile table (handle.h: pm, dtb, cl, gw, ga), whole: allocated on first
// use, tiled on the host (desc_lower.h tile_rows: the lanes behind the batch and the spare tile on shared[L]), one copy
int upload_tiled_named(to_handle* h, const char* name, double** d, size_t L, const double* values, const double* shared) {
  if (!*d) TRY(dev_alloc_named(h, name, d, tiled_len(L, h->a.P.Bp)));
  std::vector<double> tiled;
  tile_rows(L, h->a.P.B, h->a.P.Bp, values, shared, &tiled);
  HIPCHECK(hipMemcpyAsync(*d, tiled.data(), tiled.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
#define upload_tiled(h, p, ...) upload_tiled_named(h, #p, p, __VA_ARGS__)
// a DevProblem pointer goes back to null when the last flag behind it clears: the handle is back on the kernel variants it ran before
template <class T, class C, class F>
void null_unless_any(T** p, const C& flags, F set) {
  if (std::none_of(flags.begin(), flags.end(), set)) *p = nullptr;
}
// what the host-only validators of desc_lower.h take: the facts of a handle (make: cost_weight_facts, track_facts, below), NULL for a NULL handle
template <class F>
struct FactsOf {
  F f{};
  bool have;
  FactsOf(const to_handle* h, F (*make)(const to_handle*)) : have(h != nullptr) { if (h) f = make(h); }
  operator const F*() const { return have ? &f : nullptr; }
};
int download_vec(to_handle* h, double* host, const double* d, int cnt, int L = -1, int e0 = 0) {
  if (L < 0) L = cnt;
  const size_t total = (size_t)cnt * h->a.P.B;
  TRY(ensure_stage(h, total * sizeof(double)));
  TRY(launch(k_to_host, grid_b(h, cnt), dim3(BLOCK), 0, h->stream, d, h->stage, L, e0, cnt, h->a.P.B));
  HIPCHECK(hipMemcpyAsync(host, h->stage, total * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
// the nominal trajectory (slot 0 of a slotted X/U array) -> host layout or a caller-owned device buffer
int download_nominal(to_handle* h, double* host, const double* slot0, int cnt, void* dev_dst = nullptr) {
  const size_t total = (size_t)cnt * h->a.P.B;
  double* dst = (double*)dev_dst;
  if (!dst) { TRY(ensure_stage(h, total * sizeof(double))); dst = h->stage; }
  TRY(launch(k_to_host, grid_b(h, cnt), dim3(BLOCK), 0, h->stream, slot0, dst, cnt, 0, cnt, h->a.P.B));
  if (host) HIPCHECK(hipMemcpyAsync(host, dst, total * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
int download_scalar(to_handle* h, double* host, const double* d) {
  if (!host) return TO_OK;
  HIPCHECK(hipMemcpyAsync(host, d, sizeof(double) * h->a.P.B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
int download_int(to_handle* h, int32_t* host, const int* d) {
  if (!host) return TO_OK;
  HIPCHECK(hipMemcpyAsync(host, d, sizeof(int) * h->a.P.B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}

// Is the Q-function cost block of every knot block-diagonal (diagonal Qxx + the attitude block of Lie-group models, no
// Qux, any Quu)?  Then the tangent-matrix expansion stores ONE row per knot instead of NR (k_backward.h, compact_row).
bool compact_cost_blocks(const to_handle* h) {
  const int n = h->a.P.n;
  for (const auto& c : h->costs) if (c.kind != TO_COST_DIAGONAL && c.kind != TO_COST_DIAGONAL_QUAT) return false;
  for (const DevCon& c : h->cons) {
    if (c.d.kind == TO_CON_GOAL || c.d.kind == TO_CON_BOUND) continue;  // rows pick single entries of [x;u]: diagonal
    if (c.d.kind == TO_CON_NORM) {  // |z[inds]|: dense over inds — fine when they all sit in the control block
      bool ctrl = true;
      for (int i = 0; i < c.d.n_inds; ++i) ctrl = ctrl && c.d.inds[i] > n;
      if (ctrl) continue;
    }
    return false;
  }
  return true;
}

// Column layout (cooperative backward pass; vector-space models only): is the cost block of every knot DIAGONAL — diagonal
// costs, and constraints whose rows pick single entries of [x; u] (goal, bounds)?  Then lane j keeps one entry per knot.
bool diagonal_cost_blocks(const to_handle* h) {
  for (const auto& c : h->costs) if (c.kind != TO_COST_DIAGONAL) return false;
  for (const DevCon& c : h->cons) if (c.d.kind != TO_CON_GOAL && c.d.kind != TO_CON_BOUND) return false;
  return h->a.P.ne == h->a.P.n;
}

// what the host logic needs to know of a model's launch table (path_plan.h)
PathTraits path_traits(const ModelOps& o) {
  PathTraits t{o.write_through, o.mfma_backward, o.coop_backward, o.lane_backward, o.ls_first_round, o.expand_backward != nullptr, o.expand_backward_coop != nullptr,
               o.expand_backward_scan != nullptr, o.accept_roll != nullptr, o.expand_lane_k[0] != nullptr, o.expand_const != nullptr, 0u, 0u, 0u};
  for (int i = 0; i < 32; ++i) {
    if (o.forward[0][i]) t.forward |= 1u << i;
    if (o.forward[1][i]) t.forward_plants |= 1u << i;
    if (o.forward2[i]) t.forward2 |= 1u << i;
  }
  return t;
}

int upload_tables(to_handle* h) {
  {  // kernel-variant flags derived from the tables (refreshed whenever a cost or constraint is replaced)
    DevProblem& P = h->a.P;
    const int N = P.N;
    // simple_stage: one diagonal-kind cost on every stage knot and a uniform dt
    const int k0 = h->costs[h->cost_index[0]].kind;
    bool simple = k0 != TO_COST_QUADRATIC && k0 != TO_COST_ERROR_QUADRATIC;
    for (int k = 1; k < N - 1; ++k) simple = simple && h->cost_index[k] == h->cost_index[0] && h->dt[k] == h->dt[0];
    P.simple_stage = simple ? 1 : 0;
    TableFlags tf;
    for (const auto& c : h->costs) tf.dense_costs = tf.dense_costs || c.kind == TO_COST_QUADRATIC || c.kind == TO_COST_ERROR_QUADRATIC;
    tf.cons = !h->cons.empty();
    for (const auto& c : h->cons) {  // per-trajectory parameters / limits are read by the general variants only
      tf.non_selector = tf.non_selector || !c.selector; tf.con_params = tf.con_params || c.cp_off >= 0; tf.con_limits = tf.con_limits || c.cl_off >= 0;
    }
    tf.plants = P.pm != nullptr;  // ... and per-trajectory model parameters by the flagged instances of the general variants only
    tf.time_steps = P.dtb != nullptr;  // ... on which per-trajectory time steps ride
    tf.cost_weights = P.gw != nullptr;  // per-trajectory cost weights are read by the general variants only (their GW instances)
    P.expand_variant = expand_variant_of(tf);  // (path_plan.h)
    // unit-SOC forward-pass variants (problem_dev.h unit_soc_desc): at least one control-block constraint, and all of them unit
    bool any_ctrl = false, all_unit = true;
    for (const auto& c : h->cons)
      if (c.fast == 2) {
        any_ctrl = true;
        const bool u = P.m == 1 ? unit_soc_desc<1>(c.d.sense, c.fast, c.p, c.ssgn, c.soff) : P.m == 2 ? unit_soc_desc<2>(c.d.sense, c.fast, c.p, c.ssgn, c.soff)
                     : P.m == 3 ? unit_soc_desc<3>(c.d.sense, c.fast, c.p, c.ssgn, c.soff) : unit_soc_desc<4>(c.d.sense, c.fast, c.p, c.ssgn, c.soff);
        all_unit = all_unit && u && c.cl_off < 0;  // (the UNIT variants hold the shared bound in an SGPR: not while the cone carries per-trajectory limits)
      }
    P.unit_soc = (any_ctrl && all_unit) ? 1 : 0;
    if (const char* env = std::getenv("TRAJOPT_UNIT_SOC")) if (!std::atoi(env)) P.unit_soc = 0;  // A/B knob
    // (the compact cost block exists for the variants 0 and 2 of the tangent-matrix expansion; the general variant 7 — dense costs, generic
    // constraints, per-trajectory constraint parameters — writes the full block)
    h->a.h_compact = (h->a.bwd_mfma && compact_cost_blocks(h) && (P.expand_variant == 0 || P.expand_variant == 2)) ? 1 : 0;
    h->a.h_diag = (!h->a.bwd_mfma && !h->a.bwd_lane && diagonal_cost_blocks(h)) ? 1 : 0;
    if (const char* env = std::getenv("TRAJOPT_FULL_COST_BLOCKS")) if (std::atoi(env)) { h->a.h_compact = 0; h->a.h_diag = 0; }  // testing knob
  }
  // packed expansion (k_expand.h): whenever the compact cost block is (back) in use, the constant columns of [A B] are in place —
  // another variant of the expansion (general: full cost block) writes them from its dual numbers, equal to rounding only
  if (h->a.Mt && h->a.h_compact && h->plan.expand_pack && h->ops->expand_const) TRY(h->ops->expand_const(h));
  HIPCHECK(hipMemcpyAsync(h->d_costs, h->costs.data(), h->costs.size() * sizeof(to_cost_desc), hipMemcpyHostToDevice, h->stream));
  if (!h->cons.empty()) HIPCHECK(hipMemcpyAsync(h->d_cons, h->cons.data(), h->cons.size() * sizeof(DevCon), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}

int launch_set_active(to_handle* h, int v, int clear_bpfail = 1) {
  return launch(k_set_active, grid_b(h), dim3(BLOCK), 0, h->stream, h->a, v, clear_bpfail);
}
// THE plants choice: DevProblem::pm set — one plant per trajectory — selects entry [1] of the kernels that read model parameters (handle.h ModelOps)
// (per-trajectory time steps, DevProblem::dtb, ride on the same entries: path_plan.h routed_as_plants; pm is set while dtb is)
inline int plants(const to_handle* h) { return routed_as_plants(h->a.P.pm != nullptr, h->a.P.dtb != nullptr) ? 1 : 0; }
int launch_rollout(to_handle* h) { return h->ops->rollout[plants(h)](h); }
int launch_defect(to_handle* h, double* out) { return h->ops->defect[plants(h)](h, out); }
int launch_pn(to_handle* h, int slot0, int count, hipStream_t stream, const to_solver_opts* opts) {
  return h->ops->pn_launch[plants(h)](h, slot0, count, stream, opts);
}
int launch_discrete_jacobian(to_handle* h, double* F) { return h->ops->discrete_jacobian[plants(h)](h, F); }
int launch_cost(to_handle* h, int with_al, double* out, double* Jk) { return h->ops->cost(h, with_al, out, Jk); }
int launch_expand(to_handle* h) {
  // with plants the lane layout takes the lane instance and the other layouts the general column / tangent-matrix one (no expand_lane knob);
  // without, op_expand decides
  if (plants(h) && h->a.bwd_lane) return h->ops->expand_lane_k[1](h);
  return h->ops->expand[plants(h)](h);
}
int launch_backward(to_handle* h) { return h->ops->backward(h); }
int launch_accept(to_handle* h) {  // materialise accepted candidate slots on slot 0, then forget them
  if (!h->a.store_x) return h->ops->accept_roll(h);  // their states were not stored: rolled out again from the stored controls (clears acc itself)
  enqueue(k_accept, grid_b(h, 1, h->accept_chunks), dim3(BLOCK), 0, h->stream, h->a);
  return launch(k_clear_acc, grid_b(h), dim3(BLOCK), 0, h->stream, h->a);
}
// the forward-pass variant of the handle's problem (path_plan.h forward_mode) — among the instances that load one plant per trajectory (the
// general ones, stage cost read per knot), or among the others; < 0: not compiled for this model
int forward_variant(const to_handle* h, bool with_plants) {
  const DevProblem& P = h->a.P;  // (the general variants also with per-trajectory linear cost terms / constraint parameters: only they read them)
  if (with_plants) return forward_mode(false, P.n_cons > 0, P.integrator == INTEG_RK4, true, false, h->traits.forward_plants);
  return forward_mode(forward_simple(P.simple_stage, P.gw != nullptr), P.n_cons > 0, P.integrator == INTEG_RK4,
                      forward_general(P.expand_variant, P.gl != nullptr, P.cp != nullptr, P.cl != nullptr, P.gw != nullptr), P.unit_soc, h->traits.forward);
}
// forward pass: ONE launch runs the whole line search (CW step sizes per round, concurrently, inside each wave) and the
// per-trajectory state machine (k_forward.h), in the kernel variant forward_variant picks
int launch_forward(to_handle* h, bool accept = true, bool two_wave = false) {
  const int mode = forward_variant(h, plants(h) != 0);
  if (plants(h)) {  // one plant per trajectory: as one-wave workgroups
    if (mode < 0) return fail(TO_ERR_UNSUPPORTED, "forward-pass variant with per-trajectory model parameters not compiled for this model");
    TRY(h->ops->forward[1][mode](h));
  } else {
    if (mode < 0) return fail(TO_ERR_UNSUPPORTED, "forward-pass variant not compiled for this model");
    if ((two_wave || h->plan.fwd2 == 1) && h->ops->forward2[mode]) TRY(h->ops->forward2[mode](h));
    else TRY(h->ops->forward[0][mode](h));
  }
  if (accept) TRY(launch_accept(h));  // inside a solve the next expansion writes the accepted step through instead
  return TO_OK;
}
int launch_outer(to_handle* h) { return h->ops->outer(h); }
// stream compaction (k_generic.h; grid: path_plan.h compact_grid): the list of the trajectories that go on, for the next step's kernels ...
int launch_compact(to_handle* h) {
  const KArgs& a = h->a;
  int per, nb;
  if (a.P.Bp <= COMPACT_ONE_LAUNCH) enqueue(k_compact, dim3(1), dim3(1024), 0, h->stream, a);
  else if (!compact_grid(a.P.Bp, &per, &nb)) return fail(TO_ERR_UNSUPPORTED, "batch too large for the compaction kernels (16 777 216 trajectories)");
  else {
    enqueue(k_compact_count, dim3(nb), dim3(1024), 0, h->stream, a, per);
    enqueue(k_compact_write, dim3(nb), dim3(1024), 0, h->stream, a, per);
  }
  TRY(launched());
  return TO_OK;
}
// ... and, in the two-launch line search, of the trajectories whose `pending` flag launch A left set (-> plist / pcount)
int launch_flag_list(to_handle* h) {
  const KArgs& a = h->a;
  int per, nb;
  if (!compact_grid(a.P.Bp, &per, &nb)) return fail(TO_ERR_UNSUPPORTED, "batch too large for the compaction kernels (16 777 216 trajectories)");
  enqueue(k_flags_count, dim3(nb), dim3(1024), 0, h->stream, a.pending, a.P.Bp, per, a.ccount);
  return launch(k_flags_write, dim3(nb), dim3(1024), 0, h->stream, a.pending, a.P.Bp, per, a.ccount, a.plist, a.pcount);
}
// the two-launch line search: launch A — one round for everybody; flags -> list; launch B — the rest of the search for the flagged ones; the accept
int launch_forward_two(to_handle* h) {
  KArgs& a = h->a;
  const PathPlan& pl = h->plan;
  const int cw0 = a.CW, tw0 = a.TW, dump0 = a.dump_wave;
  a.dump_wave = pl.ls2_dump;
  a.CW = pl.ls2_cwa; a.TW = 64 / pl.ls2_cwa; a.ls_phase = 1; a.blk0 = 0;
  TRY(launch_forward(h, false, false));
  TRY(launch_flag_list(h));
  a.CW = pl.ls2_cwb; a.TW = 64 / pl.ls2_cwb; a.ls_phase = 2; a.ls_c0 = pl.ls2_cwa; a.blk0 = pl.ls2_blkA;
  TRY(launch_forward(h, false, false));
  a.ls_phase = 0; a.blk0 = 0; a.CW = cw0; a.TW = tw0; a.dump_wave = dump0;
  return launch_accept(h);
}
int launch_violation(to_handle* h, double* out) { return h->ops->violation(h, out); }

// stats of the last solve; with_defect: c_max also counts the dynamics / initial-condition defects (a polished trajectory is
// not an exact rollout)
int fill_stats(to_handle* h, to_solve_stats* st, bool with_defect) {
  KArgs& a = h->a;
  const DevProblem& P = a.P;
  const int B = P.B;
  std::vector<int32_t> its(B);
  TRY(download_int(h, its.data(), a.iterations));
  int64_t tot = 0;
  for (int b = 0; b < B; ++b) tot += its[b];
  if (st->iterations) std::memcpy(st->iterations, its.data(), sizeof(int32_t) * B);
  TRY(download_int(h, st->iterations_outer, a.outer));
  TRY(download_int(h, st->status, a.status));
  TRY(download_int(h, st->iterations_pn, a.it_pn));
  if (st->cost) { TRY(launch_cost(h, 0, h->d_tmp, nullptr)); TRY(download_scalar(h, st->cost, h->d_tmp)); }
  TRY(download_scalar(h, st->dJ, a.dJ));
  TRY(download_scalar(h, st->gradient, a.grad));
  if (st->c_max) {
    if (P.n_cons > 0) { TRY(launch_violation(h, h->d_tmp)); TRY(download_scalar(h, st->c_max, h->d_tmp)); }
    else std::memset(st->c_max, 0, sizeof(double) * B);
    if (with_defect) {
      std::vector<double> df(B);
      TRY(launch_defect(h, h->d_tmp));
      TRY(download_scalar(h, df.data(), h->d_tmp));
      for (int b = 0; b < B; ++b) if (df[b] > st->c_max[b] || df[b] != df[b]) st->c_max[b] = df[b];
    }
  }
  if (st->penalty_max) {
    TRY(launch(k_penalty_max, grid_b(h), dim3(BLOCK), 0, h->stream, a, h->d_tmp));
    TRY(download_scalar(h, st->penalty_max, h->d_tmp));
  }
  st->total_iterations = tot;
  st->batch_steps = h->last_steps;
  st->solve_ms = h->last_ms;
  return TO_OK;
}

// ---- repacked working set (k_generic.h k_repack_*) ------------------------------------------------------------------------
void*& rp_field(to_handle* h, size_t off) { return *reinterpret_cast<void**>(reinterpret_cast<char*>(&h->a) + off); }
int rp_setup(to_handle* h) {
  if (!h->rp_arr.empty()) return TO_OK;
  KArgs& a = h->a;
  const DevProblem& P = a.P;
  auto add = [&](void* field_addr, int kind, int L) {
    h->rp_arr.push_back({(size_t)(reinterpret_cast<char*>(field_addr) - reinterpret_cast<char*>(&a)), kind, L});
  };
  add(&a.Xs, 0, P.N * P.n); add(&a.Us, 0, (P.N - 1) * P.m); add(&a.x0, 0, P.n);
  if (a.P.gl) add(&a.P.gl, 0, P.n_costs * (P.n + P.m));
  // duals and penalties: an iLQR solve (the only kind that repacks) never writes them, but its expansion, forward pass and cost read
  // them through the tile of the WORKING position whenever the problem has constraints (a hand-built AL loop, to_set_duals, an iLQR
  // re-solve behind an AL solve: per-trajectory values) — moved along, never copied home
  if (P.n_cons > 0) { add(&a.lam, 3, (int)P.n_duals); add(&a.mu, 3, P.n_cons); }
  if (a.P.cp) add(&a.P.cp, 3, P.n_cp);
  if (a.P.cl) add(&a.P.cl, 3, P.n_cl);  // per-trajectory constraint limits travel with their trajectories, like cp
  if (a.P.gw) add(&a.P.gw, 4, P.n_costs * (P.n + P.m));  // ... and so do per-trajectory cost weights (rp_plan.h: a kind of their own for the re-use rule)
  for (double** f : {&a.J, &a.dJ, &a.grad, &a.rho, &a.drho, &a.cmax}) add(f, 1, 1);
  for (int** f : {&a.status, &a.iterations, &a.it_inner, &a.outer, &a.dJzero, &a.ls_index, &a.active, &a.budget, &a.bpfail, &a.acc, &a.accp}) add(f, 2, 1);
  if ((int)h->rp_arr.size() > RP_MAX) return fail(TO_ERR_UNSUPPORTED, "repack table too long");
  return TO_OK;
}
size_t rp_bytes(const to_handle::RpArr& r, int Bp) { return rp_slot_bytes({r.kind, r.L}, Bp); }
// move the `count` active trajectories (list of the NEXT step, built by k_compact) into the other working set and go on there
int rp_move(to_handle* h, int count) {
  KArgs& a = h->a;
  TRY(rp_setup(h));
  const int lvl = h->rp_level, w = lvl & 1;          // target working set: 0, 1, 0, ...
  const int Bp_new = (count + 63) / 64 * 64;
  if (lvl == 0) {
    h->rp_home.clear();
    for (const auto& r : h->rp_arr) h->rp_home.push_back(rp_field(h, r.off));
    h->rp_B = a.P.B; h->rp_Bp = a.P.Bp;
  }
  std::vector<RpSlot> need;
  for (const auto& r : h->rp_arr) need.push_back({r.kind, r.L});
  if (!rp_reusable(h->rp_sized[w], need, Bp_new)) {  // (rp_plan.h; as a rule sized once per configuration: the first move of a solve is the largest for this working set)
    for (void* q : h->rp_work[w]) if (q) g_free(h, q);
    h->rp_work[w].assign(h->rp_arr.size(), nullptr);
    if (h->rp_map[w]) g_free(h, h->rp_map[w]);
    h->rp_map[w] = nullptr; h->rp_sized[w] = RpSized();
    // (+ one spare tile, like the home arrays: k_accept_roll's lanes without an accepted step store into the tile behind the batch)
    bool ok = true;
    for (size_t i = 0; ok && i < h->rp_arr.size(); ++i) ok = g_malloc(h, &h->rp_work[w][i], rp_bytes(h->rp_arr[i], Bp_new + 64), "repacked working set") == TO_OK;
    ok = ok && g_malloc(h, (void**)&h->rp_map[w], rp_map_bytes(Bp_new), "repack map") == TO_OK;
    if (!ok) {  // no memory for a working set: the repack is an optimisation — the solve goes on where it is (return value 1: declined)
      (void)hipGetLastError();
      for (void*& q : h->rp_work[w]) { if (q) g_free(h, q); q = nullptr; }
      if (h->rp_map[w]) { g_free(h, h->rp_map[w]); h->rp_map[w] = nullptr; }
      return 1;
    }
    h->rp_sized[w].slots = need; h->rp_sized[w].cap = Bp_new;
  }
  RpArgs mv, hm;
  mv.n = hm.n = (int)h->rp_arr.size();
  for (int i = 0; i < mv.n; ++i) {
    mv.kind[i] = hm.kind[i] = rp_device_kind(h->rp_arr[i].kind); mv.L[i] = hm.L[i] = h->rp_arr[i].L;
    mv.src[i] = rp_field(h, h->rp_arr[i].off); mv.dst[i] = h->rp_work[w][i];
    hm.src[i] = rp_field(h, h->rp_arr[i].off); hm.dst[i] = h->rp_home[i];
    HIPCHECK(hipMemsetAsync(h->rp_work[w][i], 0, rp_bytes(h->rp_arr[i], Bp_new), h->stream));  // the padding lanes hold valid (zero) data, active = 0
  }
  const int* omap_old = lvl == 0 ? nullptr : h->rp_map[(lvl - 1) & 1];
  const int next = (a.step + 1) & 1;
  const int* list = a.alist + (size_t)next * a.P.Bp;
  const bool dbg = std::getenv("TRAJOPT_SYNC_DEBUG") != nullptr;
  auto dbg_sync = [&](const char* what) {
    if (!dbg) return;
    const hipError_t e = hipStreamSynchronize(h->stream);
    std::fprintf(stderr, "[sync-debug] rp_move level %d -> %d count %d (B %d Bp %d, cap %d / %d) after %s: %s\n", lvl, lvl + 1, count, a.P.B, a.P.Bp, h->rp_sized[0].cap, h->rp_sized[1].cap, what, hipGetErrorString(e));
  };
  dbg_sync("memsets");
  if (lvl > 0)  // what has finished in the set we leave goes home first (level 0 IS home)
    enqueue(k_repack_home, dim3((a.P.B + 63) / 64, hm.n), dim3(64), 0, h->stream, hm, a.active, a.P.B, omap_old, 0);
  dbg_sync("k_repack_home");
  TRY(launch(k_repack_move, dim3((count + 63) / 64, mv.n), dim3(64), 0, h->stream, mv, list, count, omap_old, h->rp_map[w]));
  dbg_sync("k_repack_move");
  for (int i = 0; i < mv.n; ++i) rp_field(h, h->rp_arr[i].off) = h->rp_work[w][i];
  a.P.B = count; a.P.Bp = Bp_new;
  TRY(launch(k_repack_list, dim3((count + 255) / 256), dim3(256), 0, h->stream, a.alist + (size_t)next * a.P.Bp, a.acount + next, count));
  h->rp_level = lvl + 1;
  return TO_OK;
}
// end of a solve: everything in the working set goes home; the handle works on its home arrays again
int rp_finish(to_handle* h, bool copy) {
  if (h->rp_level == 0) return TO_OK;
  KArgs& a = h->a;
  const int w = (h->rp_level - 1) & 1;
  int rc = TO_OK;
  if (copy) {
    RpArgs hm;
    hm.n = (int)h->rp_arr.size();
    for (int i = 0; i < hm.n; ++i) { hm.kind[i] = rp_device_kind(h->rp_arr[i].kind); hm.L[i] = h->rp_arr[i].L; hm.src[i] = rp_field(h, h->rp_arr[i].off); hm.dst[i] = h->rp_home[i]; }
    if (launch(k_repack_home, dim3((a.P.B + 63) / 64, hm.n), dim3(64), 0, h->stream, hm, a.active, a.P.B, h->rp_map[w], 1) != TO_OK)
      rc = fail(TO_ERR_HIP, "k_repack_home launch failed");
  }
  for (size_t i = 0; i < h->rp_arr.size(); ++i) rp_field(h, h->rp_arr[i].off) = h->rp_home[i];
  a.P.B = h->rp_B; a.P.Bp = h->rp_Bp;
  h->rp_level = 0;
  return rc;
}

// what the solve loop knows about its batch, published for to_solve_progress / to_solve_wait_below
// TRAJOPT_TRACE=<file>: every progress report of every solve loop as one line "<handle> <seconds> <batch steps> <active> <tag>" (host clock,
// CLOCK_MONOTONIC) — the timeline of pipelined solves over several handles (tools/ab/pipeline_timeline.py)
void trace_line(to_handle* h, int active, int steps, const char* tag) {
  static const char* path = std::getenv("TRAJOPT_TRACE");
  if (!path) return;
  static std::mutex mu;
  static FILE* f = std::fopen(path, "a");
  if (!f) return;
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  std::lock_guard<std::mutex> lk(mu);
  std::fprintf(f, "%p %.6f %d %d %s\n", (void*)h, ts.tv_sec + 1e-9 * ts.tv_nsec, steps, active, tag);
  std::fflush(f);
}
void publish_progress(to_handle* h, int active, int steps) {
  trace_line(h, active, steps, "step");
  const int before = h->prog_active.exchange(active);
  h->prog_steps = steps;
  if (active < before) { std::lock_guard<std::mutex> lk(h->prog_mu); h->prog_cv.notify_all(); }
}
int solve_impl(to_handle* h, to_solve_stats* st, int al_mode);
SolveKnobs solve_knobs() { return read_solve_knobs([](const char* name) -> const char* { return std::getenv(name); }); }  // (solve_loop.h; per solve)
int solve(to_handle* h, to_solve_stats* st, int al_mode) {
  int rc = solve_impl(h, st, al_mode);
  if (rc == TO_OK && h->guard) rc = check_guards(h, "the end of a solve (final accept, working set home, statistics)");
  publish_progress(h, 0, h->prog_steps);  // on every exit path: nobody may wait for a count that will not come
  rp_finish(h, false);   // (an error path may leave the handle on a working set: back to the home arrays, without the copy)
  h->a.control = 0;  // on every exit path: the phase API must never find the state machine armed
  h->a.compact = 0;  // ... nor take its trajectories from a solve's active list
  h->a.fwd_list = 0; // (either kind)
  h->a.CW = h->plan.cw_base; h->a.TW = h->plan.tw_base;
  h->a.store_x = 1;      // ... and stores whole candidates
  return rc;
}
// Altro solve!(::ProjectedNewtonSolver) on the trajectories of `list` (k_pn.h), with the options `opts`, on the handle's stream;
// device time is added to h->last_ms.  The list goes through the workspace in chunks of h->pn_cap trajectories.
int pn_run(to_handle* h, const std::vector<int>& list, const to_solver_opts& opts) {
  if (list.empty()) return TO_OK;
  if (!h->ops->pn_launch[0]) return fail(TO_ERR_UNSUPPORTED, "projected Newton not compiled for this model");
  const int count = (int)list.size();
  TRY(h->ops->pn_prepare(h, count));
  hipEvent_t e0 = h->sev[0], e1 = h->sev[1];
  HIPCHECK(hipEventRecord(e0, h->stream));
  std::memcpy(h->pn_list_host, list.data(), sizeof(int) * count);
  for (int base = 0; base < count; base += h->pn_cap) {
    const int cnt = std::min(h->pn_cap, count - base);
    HIPCHECK(hipMemcpyAsync(h->pn_list, h->pn_list_host + base, sizeof(int) * cnt, hipMemcpyHostToDevice, h->stream));
    TRY(launch_pn(h, 0, cnt, h->stream, &opts));
  }
  HIPCHECK(hipEventRecord(e1, h->stream));
  HIPCHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
  h->last_ms += ms;
  if (h->profile) { h->prof_ms[3] += ms; h->prof_launches[3] += 1; }  // slot 3: the polish (all its launches of one solve)
  if (h->guard) TRY(check_guards(h, "the projected-Newton polish"));
  return TO_OK;
}
int ensure_solve_events(to_handle* h) {
  if (!h->sev[0]) {
    HIPCHECK(hipEventCreate(&h->sev[0]));
    HIPCHECK(hipEventCreate(&h->sev[1]));
    HIPCHECK(hipEventCreateWithFlags(&h->sev[2], hipEventDisableTiming));
    HIPCHECK(hipEventCreateWithFlags(&h->sev[3], hipEventDisableTiming));
  }
  return TO_OK;
}

// ---- early polish: inside an ALTRO solve, trajectories whose AL stage has ended are polished on a second stream while the
// rest of the batch is still iterating.  The last third of an AL solve's batch steps works on a drained batch (C5: 85 of 275
// steps hold under a quarter of the trajectories: latency-bound kernels on a mostly idle chip), and the polish of a trajectory
// depends on nothing but its own (X, U): the same result, partly hidden behind that tail.  When the active count has fallen
// to B / 4 the AL loop takes a snapshot of the per-trajectory state, the host lists the trajectories that are finished,
// converged and above constraint_tolerance, and their polish goes to a low-priority stream, into workspace slots of its own; the
// rest is polished after the AL stage.  Finished trajectories are never touched again by the AL kernels; the polish writes
// (X, U), status and its own statistics of ITS trajectories only — results are equal to the one-polish path
// (tests/test_gpu_pn.py::test_early_polish_matches_polish_after_the_al_stage).
// Measured on C5 (B = 8192, 3 solves each, M trajectory-iterations/s): no hand-over 1.060; one at B/2 1.072, at B/4 1.088-1.094, at
// B/8 1.078, at B/16 1.067, at B/32 1.074; two from B/8 1.043, three from B/2 1.032, five 0.976 — the polish waves live for
// milliseconds and k_expand needs whole SIMDs (256 VGPR + AGPR), so a polish that starts while the AL stage still fills
// the chip costs it more than it hides; restricting the polish stream to half or a quarter of the compute units
// (hipExtStreamCreateWithCUMask) changed nothing (1.092-1.100).  TRAJOPT_PN_EARLY=0 switches the hand-over off, =n allows n of them
// (halving the threshold each time), TRAJOPT_PN_EARLY_AT=d starts at B / d.
int early_polish_setup(to_handle* h) {
  if (!h->pn_stream) {
    int lo = 0, hi = 0;
    HIPCHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));  // lo: the numerically largest = lowest priority
    HIPCHECK(hipStreamCreateWithPriority(&h->pn_stream, hipStreamNonBlocking, lo));
    HIPCHECK(hipEventCreateWithFlags(&h->pn_ev[0], hipEventDisableTiming));
    HIPCHECK(hipEventCreate(&h->pn_ev[1]));
    HIPCHECK(hipEventCreate(&h->pn_ev[2]));
    const size_t Bp = h->a.P.Bp;
    HIPCHECK(hipHostMalloc((void**)&h->snap_status, sizeof(int32_t) * Bp));
    HIPCHECK(hipHostMalloc((void**)&h->snap_active, sizeof(int32_t) * Bp));
    HIPCHECK(hipHostMalloc((void**)&h->snap_cmax, sizeof(double) * Bp));
  }
  return TO_OK;
}
// AL loop: the state of every trajectory as of this point of the handle's stream -> pinned host arrays; pn_ev[0] marks it
int early_polish_snapshot(to_handle* h) {
  const KArgs& a = h->a;
  const size_t B = a.P.B;
  HIPCHECK(hipMemcpyAsync(h->snap_status, a.status, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipMemcpyAsync(h->snap_active, a.active, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipMemcpyAsync(h->snap_cmax, a.cmax, sizeof(double) * B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipEventRecord(h->pn_ev[0], h->stream));
  return TO_OK;
}
// ... and, once it has arrived, the polish of what it shows finished (enqueued on pn_stream behind the snapshot)
int early_polish_launch(to_handle* h) {
  HIPCHECK(hipEventSynchronize(h->pn_ev[0]));
  const int B = h->a.P.B, s0 = h->pn_early_slots;
  int cnt = 0;
  for (int b = 0; b < B; ++b)
    if (!h->pn_done_early[b] && h->snap_active[b] == 0 && h->snap_status[b] == TO_SOLVE_SUCCEEDED && h->snap_cmax[b] > h->pn_opts.constraint_tolerance) {
      h->pn_list_host[s0 + cnt++] = b;
      h->pn_done_early[b] = 1;
    }
  if (cnt == 0) return TO_OK;
  HIPCHECK(hipStreamWaitEvent(h->pn_stream, h->pn_ev[0], 0));
  if (s0 == 0) HIPCHECK(hipEventRecord(h->pn_ev[2], h->pn_stream));
  HIPCHECK(hipMemcpyAsync(h->pn_list + s0, h->pn_list_host + s0, sizeof(int) * cnt, hipMemcpyHostToDevice, h->pn_stream));
  TRY(launch_pn(h, s0, cnt, h->pn_stream, &h->pn_opts));
  HIPCHECK(hipEventRecord(h->pn_ev[1], h->pn_stream));
  h->pn_early_slots += cnt;
  return TO_OK;
}
int pn_solve(to_handle* h, to_solve_stats* st) {
  TRY(use_device(h));
  TRY(ensure_solve_events(h));
  KArgs& a = h->a;
  const int Bp = a.P.Bp, B = a.P.B;
  HIPCHECK(hipMemsetAsync(a.iterations, 0, sizeof(int) * Bp, h->stream));
  HIPCHECK(hipMemsetAsync(a.outer, 0, sizeof(int) * Bp, h->stream));
  HIPCHECK(hipMemsetAsync(a.it_pn, 0, sizeof(int) * Bp, h->stream));
  std::vector<int> list(B);
  for (int b = 0; b < B; ++b) list[b] = b;
  h->last_steps = 0; h->last_ms = 0.0;
  TRY(pn_run(h, list, a.P.opts));
  if (st) TRY(fill_stats(h, st, true));
  return TO_OK;
}
// Altro solve!(::ALTROSolver): AL stage down to projected_newton_tolerance, polish of what it left SOLVE_SUCCEEDED above
// constraint_tolerance — as the trajectories finish (early polish, above) and, for the rest, after the AL stage
int altro_solve(to_handle* h, to_solve_stats* st) {
  const to_solver_opts user = h->a.P.opts;
  const bool pn = user.projected_newton && h->a.P.n_cons > 0;
  if (!pn) return solve(h, st, 1);
  TRY(use_device(h));
  const int B = h->a.P.B;
  const int early = solve_knobs().pn_early;
  h->pn_early = 0; h->pn_early_slots = 0;
  if (early > 0 && h->ops->pn_launch[0] && !h->ops->write_through) {  // (write-through models keep accepted steps in candidate slots until the solve ends)
    // (a problem the polish cannot take — too many rows on a knot, no memory for the workspace — still gets its AL stage)
    if (h->ops->pn_prepare(h, B) == TO_OK && h->pn_cap >= B) {  // every trajectory has a workspace slot of its own
      TRY(early_polish_setup(h));
      h->pn_done_early.assign(B, 0);
      h->pn_opts = user;
      h->pn_early = early;
    }
  }
  const bool had_early = h->pn_early > 0;
  h->a.P.opts.constraint_tolerance = user.projected_newton_tolerance;
  const int rc = solve(h, nullptr, 1);
  h->a.P.opts = user;
  h->pn_early = 0;
  if (had_early && h->pn_early_slots > 0) {  // on every path: nothing of this solve may still be running when it returns
    const hipError_t e = hipEventSynchronize(h->pn_ev[1]);
    if (rc == TO_OK) HIPCHECK(e);
  }
  if (rc != TO_OK) return rc;
  if (had_early && h->pn_early_slots > 0) {
    float ms = 0.f, tail = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, h->pn_ev[2], h->pn_ev[1]));  // first launch .. end of the last: the span on the second stream
    if (h->profile) { h->prof_ms[3] += ms; h->prof_launches[3] += 1; }
    HIPCHECK(hipEventElapsedTime(&tail, h->sev[1], h->pn_ev[1]));   // what of it outlasted the AL stage
    if (tail > 0.f) h->last_ms += tail;
  }
  std::vector<int32_t> status(B);
  std::vector<double> cmax(B);
  TRY(download_int(h, status.data(), h->a.status));
  TRY(download_scalar(h, cmax.data(), h->a.cmax));
  std::vector<int> list;
  for (int b = 0; b < B; ++b)
    if (status[b] == TO_SOLVE_SUCCEEDED && cmax[b] > user.constraint_tolerance && !(had_early && h->pn_done_early[b])) list.push_back(b);
  // A problem outside the polish's limits (PN_NB_LIMIT rows on one knot) keeps the result of its AL stage: the call succeeds, the
  // trajectories keep their AL status / violation and to_last_error() says why nothing was polished
  trace_line(h, (int)list.size(), h->last_steps, "polish");
  const int prc = pn_run(h, list, user);
  trace_line(h, 0, h->last_steps, "polish_done");
  if (prc != TO_OK && prc != TO_ERR_UNSUPPORTED) return prc;
  if (st) { const std::string note = prc == TO_OK ? std::string() : g_err; TRY(fill_stats(h, st, true)); if (!note.empty()) g_err = "polish skipped: " + note; }
  return TO_OK;
}

// one batch step of a solve: the launches `sp` names (path_plan.h plan_step), with the step's profile events, guard check and sync-debug line
int batch_step(to_handle* h, int step, const StepPlan& sp) {
  KArgs& a = h->a;
  const DevProblem& P = a.P;
  a.step = step;
  if (h->profile) HIPCHECK(hipEventRecord(h->ev[4 * step + 0], h->stream));
  if (sp.kind == STEP_SPLIT) TRY(launch_expand(h));
  if (h->profile) HIPCHECK(hipEventRecord(h->ev[4 * step + 1], h->stream));
  switch (sp.kind) {
    case STEP_FUSED_LANE: TRY(h->ops->expand_backward(h)); break;
    case STEP_SCAN: TRY(h->ops->expand_backward_scan(h)); break;
    case STEP_FUSED_COOP: TRY(h->ops->expand_backward_coop(h)); break;
    case STEP_SPLIT: TRY(launch_backward(h)); break;
  }
  if (h->profile) HIPCHECK(hipEventRecord(h->ev[4 * step + 2], h->stream));
  a.CW = sp.CW; a.TW = sp.TW; a.store_x = sp.store_x;
  if (sp.two_launch) TRY(launch_forward_two(h));
  else TRY(launch_forward(h, !h->ops->write_through || !a.store_x, sp.two_wave));
  a.store_x = 1;
  if (a.al_mode) TRY(launch_outer(h));
  if (a.compact) TRY(launch_compact(h));
  if (h->profile) HIPCHECK(hipEventRecord(h->ev[4 * step + 3], h->stream));
  if (h->guard) {
    if (step == 0) if (const char* env = std::getenv("TRAJOPT_GUARD_SELFTEST")) if (std::atoi(env))  // one double behind the nominal states
      enqueue(k_guard_poke, dim3(1), dim3(1), 0, h->stream, a.Xs, (long long)P.N * P.n * (P.Bp + 64) + 3);
    TRY(check_guards(h, ("batch step " + std::to_string(step) + " of a solve").c_str()));
  }
  if (h->sync_debug) {  // TRAJOPT_SYNC_DEBUG=1: localise a device fault to a batch step
    const hipError_t e = hipStreamSynchronize(h->stream);
    std::fprintf(stderr, "[sync-debug] step %d B=%d Bp=%d level=%d store_x-path=%d: %s\n", step, a.P.B, a.P.Bp, h->rp_level, h->list_active, hipGetErrorString(e));
    if (e != hipSuccess) return fail(TO_ERR_HIP, "device fault (sync debug)");
  }
  return TO_OK;
}

int solve_impl(to_handle* h, to_solve_stats* st, int al_mode) {
  TRY(use_device(h));
  KArgs& a = h->a;
  const DevProblem& P = a.P;
  a.al_mode = al_mode;
  a.control = 1;
  h->rp_arr.clear();  // the table of carried arrays is rebuilt per solve (per-trajectory cost terms may have appeared)
  a.compact = solve_compact(h->plan, plants(h) != 0);
  const int max_steps = (al_mode ? P.opts.iterations_total : P.opts.iterations) + 1;
  if (h->counter_len < max_steps) {
    int* c = nullptr;
    TRY(g_malloc(h, (void**)&c, sizeof(int) * (max_steps + 1), "step counters"));
    h->allocs.push_back(c);
    a.counter = c + 1;  // counter[-1]: the trajectories active when step 0 begins (list mode, below)
    if (h->counter_host) HIPCHECK(hipHostFree(h->counter_host));
    HIPCHECK(hipHostMalloc((void**)&h->counter_host, sizeof(int) * max_steps));
    h->counter_len = max_steps;
  }
  HIPCHECK(hipMemsetAsync(a.counter - 1, 0, sizeof(int) * (max_steps + 1), h->stream));
  const SolveKnobs knobs = solve_knobs();
  h->sync_debug = knobs.sync_debug != 0;
  {  // list mode (path_plan.h solve_forward_list), for this whole solve or not at all; TRAJOPT_FWD_LIST=0 keeps the forward pass's fixed map
    const int mode = forward_variant(h, false);
    a.fwd_list = solve_forward_list(h->plan, h->traits, a.h_diag, P.expand_variant, a.compact, al_mode, P.B, P.Bp, plants(h) != 0, P.gl != nullptr,
                                    mode >= 0 && h->ops->forward2[mode] != nullptr && h->ops->expand_backward_scan != nullptr,
                                    knobs.fwd_list != 0, FWD_LIST_MAX_BP, P.gw != nullptr) ? 1 : 0;
  }
  TRY(ensure_solve_events(h));
  const hipEvent_t e0 = h->sev[0], e1 = h->sev[1];
  HIPCHECK(hipEventRecord(e0, h->stream));
  HIPCHECK(hipMemsetAsync(a.it_pn, 0, sizeof(int) * P.Bp, h->stream));
  TRY(launch(k_solve_init, grid_b(h), dim3(BLOCK), 0, h->stream, a, al_mode));
  TRY(launch_rollout(h));
  TRY(launch_cost(h, 1, a.J, nullptr));
  if (a.compact) {  // the initial rollout may have ended trajectories (TO_STATE_LIMIT / TO_CONTROL_LIMIT): the list of step 0 without them
    a.step = -1;
    TRY(launch_compact(h));
  }
  if (h->profile) {
    while ((int)h->ev.size() < 4 * max_steps) { hipEvent_t e; HIPCHECK(hipEventCreate(&e)); h->ev.push_back(e); }
  }
  h->prog_active = P.B; h->prog_steps = 0;
  // the driver loop: every decision is SolveLoop's (solve_loop.h); here each operation it names is performed and its outcome reported back
  const hipEvent_t cev[QUEUE_EVENTS] = {h->sev[2], h->sev[3]};
  SolveLoopConfig cfg;
  cfg.max_steps = max_steps; cfg.B = P.B; cfg.al_mode = al_mode;
  // repacked working set (above): iLQR solves of the small models on the fused lane path with compaction
  cfg.repack = a.compact && working_set_repack(h->plan, h->traits, plants(h) != 0);
  cfg.rp_at = h->plan.rp_at; cfg.rp_min = h->plan.rp_min;
  cfg.early = h->pn_early; cfg.early_div = knobs.pn_early_at;  // early polish (ALTRO solves)
  SolveLoop lp(cfg);
  for (LoopOp op = lp.next(); op.kind != OP_FINISH; op = lp.next()) switch (op.kind) {
    case OP_CHUNK:
      h->list_active = op.last_active;  // (list mode: the forward pass's grid)
      for (int step = op.step; step < op.step + op.n; ++step)  // what each step launches, from the last active count the host has seen (results do not depend on it)
        TRY(batch_step(h, step, plan_step(h->plan, h->traits, a.h_diag, P.expand_variant, a.compact, op.last_active, op.B, plants(h) != 0)));
      break;
    case OP_COPY:
      HIPCHECK(hipMemcpyAsync(&h->counter_host[op.step], &a.counter[op.step], sizeof(int) * op.n, hipMemcpyDeviceToHost, h->stream));
      HIPCHECK(hipEventRecord(cev[op.event], h->stream));
      break;
    case OP_WAIT: HIPCHECK(hipEventSynchronize(cev[op.event])); break;
    case OP_DRAIN: HIPCHECK(hipStreamSynchronize(h->stream)); break;
    case OP_CONSUME:
      lp.consume(h->counter_host, op);
      publish_progress(h, lp.last_active, lp.steps);
      break;
    case OP_MOVE: {
      a.step = op.step;   // (k_compact of that step built the list the move reads)
      const int mrc = rp_move(h, op.n);
      if (mrc <= 0) TRY(mrc);
      lp.moved(mrc == 0);  // (> 0: declined, out of memory)
      if (h->guard) TRY(check_guards(h, "a move into a repacked working set"));
      break;
    }
    case OP_SNAPSHOT: TRY(early_polish_snapshot(h)); break;
    case OP_POLISH: TRY(early_polish_launch(h)); break;
    case OP_FINISH: break;
  }
  const int steps = lp.steps;
  TRY(launch_accept(h));  // trajectories keep the slot of their last accepted step until here
  a.CW = h->plan.cw_base; a.TW = h->plan.tw_base;
  TRY(rp_finish(h, true));  // a repacked working set goes home
  HIPCHECK(hipEventRecord(e1, h->stream));
  HIPCHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
  if (h->profile) {
    for (int step = 0; step < steps; ++step)
      for (int s = 0; s < 3; ++s) {
        float t = 0.f;
        HIPCHECK(hipEventElapsedTime(&t, h->ev[4 * step + s], h->ev[4 * step + s + 1]));
        h->prof_ms[s] += t;
        h->prof_launches[s] += 1;
      }
  }
  h->last_steps = steps; h->last_ms = ms;
  if (st) TRY(fill_stats(h, st, false));
  return TO_OK;
}

}  // namespace

namespace {
struct Rccl {
  struct Id { char b[128]; };  // ncclUniqueId (NCCL_UNIQUE_ID_BYTES), passed by value
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, Id, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
std::once_flag g_rccl_once;
int load_rccl() {
  std::call_once(g_rccl_once, [] {
    // TRAJOPT_RCCL_LIB names the collective library outright (any library exporting these eight nccl* entry points: a site build of
    // RCCL, or the shared-memory stand-in of tests/rccl_stub that lets several ranks share one GPU); nothing else is tried then
    if (const char* env = std::getenv("TRAJOPT_RCCL_LIB")) g_rccl.lib = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
    else
      for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        g_rccl.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (g_rccl.lib) break;
      }
    if (!g_rccl.lib) return;
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(g_rccl.lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(g_rccl.lib, "ncclCommInitRank");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(g_rccl.lib, "ncclAllGather");
    g_rccl.Broadcast = (decltype(g_rccl.Broadcast))dlsym(g_rccl.lib, "ncclBroadcast");
    g_rccl.GroupStart = (decltype(g_rccl.GroupStart))dlsym(g_rccl.lib, "ncclGroupStart");
    g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))dlsym(g_rccl.lib, "ncclGroupEnd");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(g_rccl.lib, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(g_rccl.lib, "ncclGetErrorString");
  });
  if (!g_rccl.lib || !g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy || !g_rccl.Broadcast ||
      !g_rccl.GroupStart || !g_rccl.GroupEnd)
    return fail(TO_ERR_HIP, "librccl.so not found (or incomplete): the multi-GPU entry points need RCCL");
  return TO_OK;
}
#define RCCLCHECK(expr)                                                                                          \
  do {                                                                                                           \
    int r_ = (expr);                                                                                             \
    if (r_ != 0) return fail(TO_ERR_HIP, std::string(#expr) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "rccl error")); \
  } while (0)
constexpr int kNcclDouble = 8;  // ncclFloat64 (rccl.h)
constexpr int kNcclInt32 = 2;   // ncclInt32
}  // namespace


extern "C" {

int to_abi_version(void) { return TO_ABI_VERSION; }
int to_abi_minor(void) { return TO_ABI_MINOR; }
#ifndef TO_BUILD_ID
#define TO_BUILD_ID "unstamped"
#endif
static const char g_build_stamp[] = "TO_BUILD_ID=" TO_BUILD_ID;  // also found by scanning the file (build.py)
const char* to_build_id(void) { return g_build_stamp + 12; }
const char* to_last_error(void) { return g_err.c_str(); }
int to_device_count(int* count) {
  CHECK_P(count);
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return fail(TO_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
  *count = n;
  return TO_OK;
}
int to_default_options(to_solver_opts* o) { CHECK_P(o); default_opts(o); return TO_OK; }

int to_create(const to_problem_desc* desc, const to_solver_opts* opts, int device, to_handle** out) {
  CHECK_P(out);
  LoweredProblem lp;
  TRY(lower_problem(desc, opts, &lp));  // every refusal of the descriptor and the options, and the host tables (desc_lower.h)
  const int n = lp.n, m = lp.m, ne = lp.ne, key = lp.key, N = desc->N, B = desc->B;
  const std::vector<double>& dt = lp.dt;
  const std::vector<int>& cost_index = lp.cost_index;
  const std::vector<DevCon>& cons = lp.cons;
  const long long n_duals = lp.n_duals;
  int ndev = 0;
  {
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) return fail(TO_ERR_HIP, "no usable HIP device (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(TO_ERR_ARGUMENT, "device ordinal out of range");
  }
  to_handle* h = new to_handle();
  h->device = device;
  h->model_key = key;
  if (const char* env = std::getenv("TRAJOPT_GUARD")) h->guard = std::atoi(env) != 0;
  h->R = coop_lanes(ne, m);
  h->G = 64 / h->R;
  h->ops = model_ops(key);
  if (!h->ops || !h->ops->rollout[0] || !h->ops->expand[0] || !h->ops->backward) { delete h; return fail(TO_ERR_UNSUPPORTED, "model kernels not linked"); }
  h->traits = path_traits(*h->ops);
  h->costs.assign(desc->costs, desc->costs + desc->n_costs);
  h->cons = cons; h->dt = dt; h->cost_index = cost_index; h->step_table = lp.step_table;
  auto bail = [&](int rc) { std::string e = g_err; to_destroy(h); g_err = e; return rc; };
#define TRYB(expr) do { int r_ = (expr); if (r_ != TO_OK) return bail(r_); } while (0)
#define HIPB(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return bail(fail(TO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_))); } while (0)
  HIPB(hipSetDevice(device));
  HIPB(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  KArgs& a = h->a;
  std::memset(&a, 0, sizeof(a));
  DevProblem& P = a.P;
  P.n = n; P.m = m; P.ne = ne; P.N = N; P.B = B; P.Bp = ((B + BLOCK - 1) / BLOCK) * BLOCK;
  P.integrator = desc->integrator; P.n_costs = desc->n_costs; P.n_cons = (int)cons.size(); P.n_duals = n_duals;
  std::memcpy(P.mp, desc->model_params, sizeof(P.mp));
  if (opts) P.opts = *opts; else default_opts(&P.opts);
  const size_t Bp = P.Bp;
  TRYB(dev_alloc(h, &h->d_costs, h->costs.size()));
  TRYB(dev_alloc(h, &h->d_cons, cons.size()));
  TRYB(dev_alloc(h, &h->d_dt, (size_t)N - 1));
  TRYB(dev_alloc(h, &h->d_cost_index, (size_t)N));
  HIPB(hipMemcpyAsync(h->d_dt, dt.data(), sizeof(double) * (N - 1), hipMemcpyHostToDevice, h->stream));
  HIPB(hipMemcpyAsync(h->d_cost_index, cost_index.data(), sizeof(int) * N, hipMemcpyHostToDevice, h->stream));
  if (!h->step_table.empty()) {  // model vector: the table's device address travels in model_params[0] (bit pattern; models.h)
    double* d_tab = nullptr;
    TRYB(dev_alloc(h, &d_tab, h->step_table.size()));
    HIPB(hipMemcpyAsync(d_tab, h->step_table.data(), sizeof(double) * h->step_table.size(), hipMemcpyHostToDevice, h->stream));
    const unsigned long long bits = (unsigned long long)reinterpret_cast<uintptr_t>(d_tab);
    std::memset(P.mp, 0, sizeof(P.mp));
    std::memcpy(&P.mp[0], &bits, sizeof(bits));
  }
  P.dt = (DoubleC*)h->d_dt; P.cost_index = (IntC*)h->d_cost_index; P.costs = (CostC*)h->d_costs; P.cons = (ConC*)h->d_cons;
  {  // the kernel path of this handle (path_plan.h), from the model's traits, the problem's shape and the TRAJOPT_* knobs as they are now
    PathShape sh{B, P.Bp, N, ne, m, P.n_cons, P.opts.iterations_linesearch, diagonal_cost_blocks(h), 256};
    HIPB(hipDeviceGetAttribute(&sh.cus, hipDeviceAttributeMultiprocessorCount, device));
    h->plan = plan_paths(h->traits, sh, read_path_knobs([](const char* name) -> const char* { return std::getenv(name); }));
  }
  const PathPlan& pl = h->plan;
  a.bwd_mfma = pl.bwd_mfma; a.bwd_lane = pl.bwd_lane; a.coop_merge = pl.coop_merge; a.CW = pl.cw_base; a.TW = pl.tw_base;
  a.store_x = 1; a.dump_wave = pl.dump_wave; a.repack_block0 = pl.repack_block0;
  TRYB(upload_tables(h));  // (behind the plan: h_compact / h_diag depend on the backward-pass flavour)
  h->accept_chunks = std::max(1, std::min(128, (N * n + (N - 1) * P.m + 31) / 32));
  TRYB(dev_alloc(h, &a.Xs, (size_t)N * n * (Bp + 64)));  // (+ one spare tile: where k_accept_roll's lanes without an accepted step store)
  TRYB(dev_alloc(h, &a.Us, (size_t)(N - 1) * m * Bp));
  TRYB(dev_alloc(h, &a.Xc, (size_t)N * n * pl.x_blocks * 64));  // candidates, forward-wave-major (common.h)
  TRYB(dev_alloc(h, &a.Uc, (size_t)(N - 1) * m * pl.u_blocks * 64));
  if (pl.ls2_cwa) { TRYB(dev_alloc(h, &a.pending, Bp)); TRYB(dev_alloc(h, &a.plist, Bp)); TRYB(dev_alloc(h, &a.pcount, 1)); }
  TRYB(dev_alloc(h, &a.x0, (size_t)n * Bp));
  TRYB(dev_alloc(h, &a.acc, Bp));
  TRYB(dev_alloc(h, &a.accp, Bp));
  TRYB(dev_alloc(h, &a.alist, 2 * (size_t)Bp)); TRYB(dev_alloc(h, &a.acount, 2)); TRYB(dev_alloc(h, &a.ccount, 256));
  TRYB(dev_alloc(h, &a.oflag, Bp)); TRYB(dev_alloc(h, &a.ost, Bp));
  TRYB(dev_alloc(h, &a.olist, 2 * (size_t)Bp)); TRYB(dev_alloc(h, &a.ocount, 2));
  TRYB(dev_alloc(h, &a.knotbuf, (size_t)N * Bp));
  TRYB(dev_alloc(h, &a.mu_next, (size_t)std::max<size_t>(1, cons.size()) * Bp));
  if (a.bwd_mfma) {  // tangent-matrix layout (k_backward.h): RS rows of 64 per knot for [A B], up to RS+1 for the cost block
    const int rs = h->ops->rs;
    TRYB(dev_alloc(h, &a.Mt, (size_t)Bp * (N - 1) * rs * 64));
    TRYB(dev_alloc(h, &a.Ht, (size_t)Bp * N * (rs + 1) * 64));
    TRYB(dev_alloc(h, &a.gt, (size_t)Bp * N * 16));
    TRYB(dev_alloc(h, &h->d_crow, 64));
    HIPB(hipMemcpyAsync(h->d_crow, h->ops->crow, sizeof(int) * 64, hipMemcpyHostToDevice, h->stream));
  } else if (a.bwd_lane) {  // lane layout (k_backward.h LaneLay), in the column-layout pointers
    const size_t tiles = (size_t)Bp / 64, nc = (size_t)ne + m;
    TRYB(dev_alloc(h, &a.Mc, tiles * (size_t)(N - 1) * ne * nc * 64));
    TRYB(dev_alloc(h, &a.Hc, tiles * (size_t)N * (nc * (nc + 1) / 2) * 64));
    TRYB(dev_alloc(h, &a.gc, tiles * (size_t)N * nc * 64));
  } else {
    const size_t gtiles = ((size_t)B + h->G - 1) / h->G;  // waves of the column-layout kernels
    TRYB(dev_alloc(h, &a.Mc, gtiles * (size_t)(N - 1) * ne * 64));
    TRYB(dev_alloc(h, &a.Hc, gtiles * (size_t)N * (ne + m) * 64));
    TRYB(dev_alloc(h, &a.gc, gtiles * (size_t)N * 64));
  }
  TRYB(dev_alloc(h, &a.Kt, (size_t)Bp * (N - 1) * m * (ne + 1)));  // gains rows, trajectory-major
  TRYB(dev_alloc(h, &a.lam, (size_t)n_duals * Bp));
  TRYB(dev_alloc(h, &a.mu, cons.size() * Bp));
  TRYB(dev_alloc(h, &a.J, Bp)); TRYB(dev_alloc(h, &a.dJ, Bp)); TRYB(dev_alloc(h, &a.grad, Bp));
  TRYB(dev_alloc(h, &a.rho, Bp)); TRYB(dev_alloc(h, &a.drho, Bp)); TRYB(dev_alloc(h, &a.dV, 2 * Bp));
  TRYB(dev_alloc(h, &a.cmax, Bp)); TRYB(dev_alloc(h, &a.Jout, Bp));
  TRYB(dev_alloc(h, &a.it_pn, Bp)); TRYB(dev_alloc(h, &a.pn_cmax, Bp));
  TRYB(dev_alloc(h, &a.status, Bp)); TRYB(dev_alloc(h, &a.iterations, Bp)); TRYB(dev_alloc(h, &a.it_inner, Bp));
  TRYB(dev_alloc(h, &a.outer, Bp)); TRYB(dev_alloc(h, &a.dJzero, Bp)); TRYB(dev_alloc(h, &a.ls_index, Bp));
  TRYB(dev_alloc(h, &a.active, Bp)); TRYB(dev_alloc(h, &a.budget, Bp)); TRYB(dev_alloc(h, &a.bpfail, Bp));
  TRYB(dev_alloc(h, &h->d_tmp, Bp)); TRYB(dev_alloc(h, &h->d_tmp2, Bp));
  // reference defaults: X0 = NaN, U0 = 0 (src/problem.jl:83-84); duals 0, penalties penalty_initial
  {
    std::vector<double> nanv((size_t)N * n * Bp, std::nan(""));
    HIPB(hipMemcpyAsync(a.Xs, nanv.data(), nanv.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPB(hipStreamSynchronize(h->stream));
    {  // the regularisation a phase-API backward pass starts from (a solve resets it the same way: k_solve_init)
      std::vector<double> rho0((size_t)Bp, P.opts.bp_reg_initial);
      HIPB(hipMemcpyAsync(a.rho, rho0.data(), rho0.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIPB(hipStreamSynchronize(h->stream));
    }
    if (!cons.empty()) {
      std::vector<double> mu(cons.size() * Bp, P.opts.penalty_initial);
      HIPB(hipMemcpyAsync(a.mu, mu.data(), mu.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIPB(hipStreamSynchronize(h->stream));
    }
  }
  if (a.Mt && a.h_compact && h->plan.expand_pack && h->ops->expand_const) TRYB(h->ops->expand_const(h));
  HIPB(hipStreamSynchronize(h->stream));
#undef TRYB
#undef HIPB
  *out = h;
  return TO_OK;
}

int to_destroy(to_handle* h) {
  if (!h) return TO_OK;
  if (h->inflight) { h->worker.join(); h->inflight = false; }
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
  for (void* p : h->allocs) g_free(h, p);
  g_free(h, h->stage);
  g_free(h, h->pn_ws);
  g_free(h, h->pn_pak);
  g_free(h, h->pn_koff);
  g_free(h, h->pn_list);
  if (h->guard_tab) hipFree(h->guard_tab);
  if (h->guard_bad) hipFree(h->guard_bad);
  if (h->pn_list_host) hipHostFree(h->pn_list_host);
  if (h->snap_status) hipHostFree(h->snap_status);
  if (h->snap_active) hipHostFree(h->snap_active);
  if (h->snap_cmax) hipHostFree(h->snap_cmax);
  for (hipEvent_t e : h->pn_ev) if (e) hipEventDestroy(e);
  if (h->pn_stream) hipStreamDestroy(h->pn_stream);
  for (int w = 0; w < 2; ++w) { for (void* q : h->rp_work[w]) g_free(h, q); g_free(h, h->rp_map[w]); }
  if (h->counter_host) hipHostFree(h->counter_host);
  for (hipEvent_t e : h->ev) hipEventDestroy(e);
  for (hipEvent_t e : h->sev) if (e) hipEventDestroy(e);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return TO_OK;
}

int to_set_options(to_handle* h, const to_solver_opts* o) { CHECK_H(h); CHECK_IDLE(h); CHECK_P(o); TRY(validate_opts(*o)); h->a.P.opts = *o; return TO_OK; }
int to_get_options(const to_handle* h, to_solver_opts* o) { CHECK_H(h); CHECK_P(o); *o = h->a.P.opts; return TO_OK; }
int to_sync(to_handle* h) { CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h)); HIPCHECK(hipStreamSynchronize(h->stream)); return TO_OK; }
void* to_stream(to_handle* h) { return h ? (void*)h->stream : nullptr; }

int to_solver_path(const to_handle* h, int32_t* info) {
  CHECK_H(h); CHECK_P(info);
  path_report(h->plan, h->traits, h->a.h_diag, h->a.P.expand_variant, h->a.P.B, info, plants(h) != 0);
  return TO_OK;
}
int to_knot_dims(const to_handle* h, int32_t* nx, int32_t* nu) {
  CHECK_H(h); CHECK_P(nx); CHECK_P(nu);
  const DevProblem& P = h->a.P;
  for (int k = 0; k < P.N; ++k) {
    int a = P.n, b = P.m;
    if (h->model_key == 7) HybridDoubleIntegratorModel::knot_dims(P.mp, P.N, k, &a, &b);
    if (h->model_key == 8) {  // the host copy of the table (P.mp[0] holds the DEVICE address)
      const unsigned long long bits = (unsigned long long)reinterpret_cast<uintptr_t>(h->step_table.data());
      double hp[1];
      std::memcpy(&hp[0], &bits, sizeof(bits));
      ModelVectorModel::knot_dims(hp, P.N, k, &a, &b);
    }
    nx[k] = a; nu[k] = b;
  }
  return TO_OK;
}
int to_set_profiling(to_handle* h, int enable) { CHECK_H(h); CHECK_IDLE(h); h->profile = enable != 0; return TO_OK; }
int to_reset_profile(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h);
  for (int i = 0; i < TO_PROFILE_SLOTS; ++i) { h->prof_ms[i] = 0; h->prof_launches[i] = 0; }
  return TO_OK;
}
int to_get_profile(to_handle* h, double* ms, int64_t* launches) {
  CHECK_H(h);
  for (int i = 0; i < TO_PROFILE_SLOTS; ++i) { if (ms) ms[i] = h->prof_ms[i]; if (launches) launches[i] = h->prof_launches[i]; }
  return TO_OK;
}

int to_dims(const to_handle* h, int32_t* n, int32_t* m, int32_t* ne, int32_t* N, int32_t* B) {
  CHECK_H(h);
  const DevProblem& P = h->a.P;
  if (n) *n = P.n; if (m) *m = P.m; if (ne) *ne = P.ne; if (N) *N = P.N; if (B) *B = P.B;
  return TO_OK;
}
int to_num_constraints(const to_handle* h, int32_t* p) {
  CHECK_H(h); CHECK_P(p);
  for (int k = 0; k < h->a.P.N; ++k) p[k] = 0;
  for (const DevCon& ci : h->cons) for (int k = ci.k1; k <= ci.k2; ++k) p[k] += ci.p;
  return TO_OK;
}

int to_set_initial_state(to_handle* h, const double* x0) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(x0); TRY(use_device(h));
  return upload_vec(h, x0, h->a.x0, h->a.P.n);
}
int to_get_initial_state(to_handle* h, double* x0) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(x0); TRY(use_device(h));
  return download_vec(h, x0, h->a.x0, h->a.P.n);
}
int to_set_controls(to_handle* h, const double* U) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(U); TRY(use_device(h));
  return upload_vec(h, U, h->a.Us, h->a.P.m * (h->a.P.N - 1));
}
int to_set_states(to_handle* h, const double* X) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(X); TRY(use_device(h));
  return upload_vec(h, X, h->a.Xs, h->a.P.n * h->a.P.N);
}
int to_infeasible_controls(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  if (!h->ops->infeasible_controls) return fail(TO_ERR_ARGUMENT, "to_infeasible_controls: the handle's model is not TO_MODEL_INFEASIBLE");
  TRY(h->ops->infeasible_controls(h));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
int to_set_controls_uniform(to_handle* h, const double* u) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(u); TRY(use_device(h));
  const DevProblem& P = h->a.P;
  TRY(ensure_stage(h, sizeof(double) * P.m));
  HIPCHECK(hipMemcpyAsync(h->stage, u, sizeof(double) * P.m, hipMemcpyHostToDevice, h->stream));
  TRY(launch(k_fill_uniform, grid_b(h, P.m * (P.N - 1)), dim3(BLOCK), 0, h->stream, h->a.Us, h->stage, P.m, P.m * (P.N - 1), P.B));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
int to_get_states(to_handle* h, double* X) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(X); TRY(use_device(h));
  return download_nominal(h, X, h->a.Xs, h->a.P.n * h->a.P.N);
}
int to_get_controls(to_handle* h, double* U) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(U); TRY(use_device(h));
  return download_nominal(h, U, h->a.Us, h->a.P.m * (h->a.P.N - 1));
}
int to_get_states_device(to_handle* h, void* dX) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(dX); TRY(use_device(h));
  return download_nominal(h, nullptr, h->a.Xs, h->a.P.n * h->a.P.N, dX);
}
int to_get_controls_device(to_handle* h, void* dU) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(dU); TRY(use_device(h));
  return download_nominal(h, nullptr, h->a.Us, h->a.P.m * (h->a.P.N - 1), dU);
}
// the host copy of the per-trajectory cost weights (to_handle::gw_host) -> DevProblem::gw, tiled on the host, in one copy
static int upload_cost_weights(to_handle* h) {
  std::vector<double> shared;
  cost_weights_shared(h->a.P.n, h->a.P.m, h->costs.data(), (int)h->costs.size(), &shared);
  return upload_tiled(h, &h->d_gw, shared.size(), h->gw_host.data(), shared.data());
}
// DevProblem::ga from every cost's descriptor, tiled on the host, in one copy (first use; the clears that keep the handle routed).  From then on the
// device array is the truth — k_track_lower writes it — and one cost's four rows move at a time (restart_cost_attitude, the setter, the getter).
static int upload_cost_attitudes(to_handle* h) {
  std::vector<double> shared;
  cost_attitude_shared(h->costs.data(), (int)h->costs.size(), &shared);
  return upload_tiled(h, &h->d_ga, shared.size(), nullptr, shared.data());
}
static int restart_cost_attitude(to_handle* h, int id) {
  std::vector<double> rows;
  cost_attitude_rows(h->a.P.B, h->costs[id], &rows);
  return upload_vec(h, rows.data(), h->d_ga, 4, 4 * (int)h->costs.size(), 4 * id);
}
// what a transition of to_handle::lane (path_plan.h cost_lane_step) asks of gw / ga; leaves both pointers as the state says
static int cost_lane_apply(to_handle* h, const CostLaneAction& act) {
  DevProblem& P = h->a.P;
  if (act.release || !h->lane.routed()) { P.gw = nullptr; P.ga = nullptr; h->gw_host.clear(); return TO_OK; }
  if (act.fill_gw) {
    cost_weights_fill(P.n, P.m, P.B, h->costs.data(), (int)h->costs.size(), &h->gw_host);
    TRY(upload_cost_weights(h));
  }
  if (act.fill_ga) TRY(upload_cost_attitudes(h));
  P.gw = h->d_gw; P.ga = h->d_ga;
  return TO_OK;
}
// the array behind DevProblem::gl on first use: zero-filled — every cost starts with its descriptor's terms — with gl_set sized next to it
// (to_set_cost indexes gl_set whenever d_gl exists, also behind a failed upload of the caller's)
static int ensure_gl(to_handle* h) {
  if (h->d_gl) return TO_OK;
  TRY(dev_alloc(h, &h->d_gl, h->costs.size() * (size_t)(h->a.P.n + h->a.P.m) * h->a.P.Bp));
  h->gl_set.assign(h->costs.size(), 0);
  return TO_OK;
}
int to_set_cost(to_handle* h, int32_t id, const to_cost_desc* c) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(c); TRY(use_device(h));
  if (id < 0 || id >= (int)h->costs.size()) return fail(TO_ERR_ARGUMENT, "cost id out of range");
  TRY(validate_cost(h->a.P.n, (h->model_key >= 4 && h->model_key <= 6) ? (int)h->a.P.mp[10] : -1, *c));  // rigid bodies only (key 7: hybrid double integrator)
  h->costs[id] = *c;
  if (h->d_gl) {  // the cost's per-trajectory linear terms start over (they were relative to the old descriptor)
    const int nz = h->a.P.n + h->a.P.m, L = (int)h->costs.size() * nz;
    std::vector<double> zero;
    cost_linear_zero(h->a.P.n, h->a.P.m, h->a.P.B, &zero);
    TRY(upload_vec(h, zero.data(), h->d_gl, nz, L, id * nz));
    h->gl_set[id] = 0;
    null_unless_any(&h->a.P.gl, h->gl_set, [](char f) { return f != 0; });  // every cost is back on its shared descriptor: the default forward variants again
  }
  if (h->a.P.gw) {  // ... and so do its per-trajectory weights: the new descriptor's diagonal for every trajectory (the other costs keep theirs)
    cost_weights_restart(h->a.P.n, h->a.P.m, h->a.P.B, h->costs.data(), (int)h->costs.size(), id, &h->gw_host);
    TRY(upload_cost_weights(h));
    TRY(restart_cost_attitude(h, id));  // ... and its per-trajectory q_ref (DevProblem::ga is set whenever gw is)
  }
  return upload_tables(h);
}
int to_set_cost_linear_batch(to_handle* h, int32_t id, const double* q, const double* r) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  if (id < 0 || id >= (int)h->costs.size()) return fail(TO_ERR_ARGUMENT, "cost id out of range");
  DevProblem& P = h->a.P;
  const int n = P.n, m = P.m, nz = n + m, L = (int)h->costs.size() * nz;
  std::vector<double> dq, dr;  // the differences from the descriptor's q / r (desc_lower.h)
  TRY(cost_linear_delta(h->costs[id], n, m, P.B, q, r, &dq, &dr));
  TRY(ensure_gl(h));
  if (q) TRY(upload_vec(h, dq.data(), h->d_gl, n, L, id * nz));
  if (r) TRY(upload_vec(h, dr.data(), h->d_gl, m, L, id * nz + n));
  P.gl = h->d_gl;
  h->gl_set[id] = 1;
  return TO_OK;
}
int to_clear_cost_linear_batch(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  if (h->d_gl) {
    HIPCHECK(hipMemsetAsync(h->d_gl, 0, sizeof(double) * h->costs.size() * (h->a.P.n + h->a.P.m) * h->a.P.Bp, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  h->a.P.gl = nullptr;
  h->gl_set.assign(h->costs.size(), 0);
  return TO_OK;
}
int to_set_constraint(to_handle* h, int32_t id, const to_constraint_desc* c) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(c); TRY(use_device(h));
  if (id < 0 || id >= (int)h->cons.size()) return fail(TO_ERR_ARGUMENT, "constraint id out of range");
  DevCon ci;
  TRY(validate_constraint(h->a.P.n, h->a.P.m, h->a.P.N, *c, &ci));
  const DevCon& old = h->cons[id];
  if (ci.p != old.p || ci.k1 != old.k1 || ci.k2 != old.k2) return fail(TO_ERR_DIMENSION_MISMATCH, "replacement constraint must keep p and the knot range");
  ci.dual_off = old.dual_off;
  h->cons[id] = ci;  // (cp_off = cl_off = -1: the replaced constraint starts on shared parameters and limits again)
  null_unless_any(&h->a.P.cp, h->cons, [](const DevCon& c) { return c.cp_off >= 0; });
  if (!h->cl_host.empty()) h->cl_host[id].clear();
  null_unless_any(&h->a.P.cl, h->cons, [](const DevCon& c) { return c.cl_off >= 0; });
  return upload_tables(h);
}
// One parameter set per TRAJECTORY for constraint con_id.  GOAL: params[p, B] = xf_b[inds]; LINEAR: params[p, B] = b_b.  Stored as the shift of
// z = [x; u] the constraint sees (DevProblem::cp): the GoalConstraint with target xf + d is the shared one evaluated at x - d, the
// LinearConstraint with b + db the shared one at z - A^+ db.
int to_set_constraint_params_batch(to_handle* h, int32_t id, const double* params) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(params); TRY(use_device(h));
  if (id < 0 || id >= (int)h->cons.size()) return fail(TO_ERR_ARGUMENT, "constraint id out of range");
  DevCon& ci = h->cons[id];
  DevProblem& P = h->a.P;
  const int nz = P.n + P.m, L = nz * (int)h->cons.size();
  std::vector<double> shift;
  TRY(lower_constraint_params(ci, nz, P.B, params, &shift));  // the kind refusal, the GOAL scatter, the LINEAR minimum-norm shift (desc_lower.h)
  if (!h->d_cp) TRY(dev_alloc(h, &h->d_cp, (size_t)L * P.Bp));  // zero-filled
  TRY(upload_vec(h, shift.data(), h->d_cp, nz, L, id * nz));
  ci.cp_off = id * nz;
  P.cp = h->d_cp; P.n_cp = L;
  return upload_tables(h);
}
int to_clear_constraint_params_batch(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  for (DevCon& c : h->cons) c.cp_off = -1;
  h->a.P.cp = nullptr;
  return upload_tables(h);
}

// One set of limits per TRAJECTORY for the selector constraint con_id (DevProblem::cl; desc_lower.h lower_constraint_limits has the layouts and
// the checks, constraint_limits_values the rows).  The whole table is rebuilt on the host from what every flagged constraint was given and the
// descriptors of the others, and goes up in one copy.
static int upload_constraint_limits(to_handle* h) {
  std::vector<double> shared, values;
  constraint_limits_shared(h->cons, h->cl_base, h->a.P.n_cl, &shared);
  TRY(constraint_limits_values(h->cons, h->cl_host, h->cl_base, shared, h->a.P.B, &values));
  return upload_tiled(h, &h->d_cl, shared.size(), values.data(), shared.data());
}
int to_set_constraint_limits_batch(to_handle* h, int32_t id, const double* limits) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(limits); TRY(use_device(h));
  if (id < 0 || id >= (int)h->cons.size()) return fail(TO_ERR_ARGUMENT, "constraint id out of range");
  DevCon& ci = h->cons[id];
  DevProblem& P = h->a.P;
  std::vector<double> rows;
  TRY(lower_constraint_limits(ci, P.B, limits, &rows));  // every refusal, before anything changes
  int q = 0;
  TRY(constraint_limits_q(ci, &q));
  if (h->cl_host.empty()) {
    h->cl_host.assign(h->cons.size(), std::vector<double>());
    P.n_cl = constraint_limits_bases(h->cons, &h->cl_base);
  }
  h->cl_host[id].assign(limits, limits + (size_t)q * P.B);
  TRY(upload_constraint_limits(h));
  ci.cl_off = h->cl_base[id];
  P.cl = h->d_cl;
  TRY(upload_tables(h));  // (expand_variant bit 2, unit_soc and the compact cost block follow the flags)
  return check_guards(h, "to_set_constraint_limits_batch");
}
int to_get_constraint_limits_batch(to_handle* h, int32_t id, double* limits) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(limits);
  if (id < 0 || id >= (int)h->cons.size()) return fail(TO_ERR_ARGUMENT, "constraint id out of range");
  const DevCon& ci = h->cons[id];
  int q = 0;
  TRY(constraint_limits_q(ci, &q));
  const int B = h->a.P.B;
  if (ci.cl_off >= 0) std::memcpy(limits, h->cl_host[id].data(), sizeof(double) * q * B);
  else for (int b = 0; b < B; ++b) shared_constraint_limits(ci, q, limits + (size_t)q * b);
  return TO_OK;
}
int to_clear_constraint_limits_batch(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  for (DevCon& c : h->cons) c.cl_off = -1;
  for (auto& v : h->cl_host) v.clear();
  h->a.P.cl = nullptr;
  return upload_tables(h);
}

// One set of model parameters per TRAJECTORY (DevProblem::pm): params[16, B], 16 fastest.  Every column is checked like
// to_policy_opts::plant_params (finite; the entries that select dimensions or the attitude representation equal the problem's).  The solves
// then run the flagged instances of the general kernel variants (path_plan.h `plants`); X, U, duals and gains are left as they are.
static const char* model_key_name(int key) {
  static const char* names[N_MODEL_KEYS] = {"double integrator (D = 1)", "double integrator (D = 2)", "double integrator (D = 3)", "Cartpole", "Quadrotor",
                                            "Quadrotor{MRP}", "Quadrotor{RodriguesParam}", "hybrid double integrator", "model vector",
                                            "InfeasibleModel (double integrator, D = 1)", "InfeasibleModel (double integrator, D = 2)", "InfeasibleModel (Cartpole)"};
  return (key >= 0 && key < N_MODEL_KEYS) ? names[key] : "unknown model";
}
// the models with flagged instances (one plant per trajectory; the time steps ride on them); what: "model parameters" / "time steps"
static int plants_supported(const to_handle* h, const char* who, const char* what) {
  if (h->model_key > 4 || !h->ops->plants(h->a.bwd_lane != 0))
    return fail(TO_ERR_UNSUPPORTED, std::string(who) + ": per-trajectory " + what + " are not available for the " + model_key_name(h->model_key) +
                                        " (double integrator, Cartpole and quaternion Quadrotor only)");
  return TO_OK;
}
// params[16, B] (NULL: the shared parameters for every trajectory) -> DevProblem::pm and its host copy
static int upload_plants(to_handle* h, const double* params) {
  DevProblem& P = h->a.P;
  const int B = P.B;
  TRY(upload_tiled(h, &h->d_pm, 16, params, P.mp));
  if (params) h->pm_host.assign(params, params + (size_t)16 * B);
  else {
    h->pm_host.resize((size_t)16 * B);
    for (int b = 0; b < B; ++b) std::memcpy(&h->pm_host[(size_t)16 * b], P.mp, sizeof(double) * 16);
  }
  P.pm = h->d_pm;
  return TO_OK;
}
int to_set_model_params_batch(to_handle* h, const double* params) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(params); TRY(use_device(h));
  TRY(plants_supported(h, "to_set_model_params_batch", "model parameters"));
  DevProblem& P = h->a.P;
  for (int b = 0; b < P.B; ++b) {
    const double* pp = params + (size_t)16 * b;
    if (!all_finite(pp, 16) || !plant_params_compatible(h->model_key, P.mp, pp))
      return validate_plant_params("to_set_model_params_batch", h->model_key, P.mp, pp, true, " of trajectory " + std::to_string(b));
  }
  TRY(upload_plants(h, params));
  h->pm_own = true;
  TRY(upload_tables(h));  // (expand_variant bit 2, and with it the compact cost block, follow pm)
  return check_guards(h, "to_set_model_params_batch");
}
int to_get_model_params_batch(to_handle* h, double* params) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(params);
  TRY(plants_supported(h, "to_get_model_params_batch", "model parameters"));
  const DevProblem& P = h->a.P;
  if (P.pm) std::memcpy(params, h->pm_host.data(), sizeof(double) * 16 * P.B);
  else for (int b = 0; b < P.B; ++b) std::memcpy(params + (size_t)16 * b, P.mp, sizeof(double) * 16);
  return TO_OK;
}
int to_clear_model_params_batch(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  TRY(plants_supported(h, "to_clear_model_params_batch", "model parameters"));
  h->pm_own = false;
  if (h->a.P.dtb) TRY(upload_plants(h, nullptr));  // per-trajectory time steps ride on the flagged instances: pm stays, on the shared plant
  else { h->a.P.pm = nullptr; h->pm_host.clear(); }
  return upload_tables(h);
}

// One diagonal Q / R per TRAJECTORY for the cost cost_id (DevProblem::gw; desc_lower.h has every refusal, the host copy and the shared row).  The
// array holds the weights of EVERY cost — the descriptors' values where nothing was set — and the whole of it goes up again with every call.
// The handle is then routed like one with per-trajectory constraint limits (path_plan.h TableFlags::cost_weights) and launches the GW
// instances of the kernels that read a cost's diagonal; X, U, duals and gains are left as they are.
static CostWeightFacts cost_weight_facts(const to_handle* h) {
  const DevProblem& P = h->a.P;
  return CostWeightFacts{h->model_key, model_key_name(h->model_key), P.n, P.m, P.B, h->costs.data(), (int)h->costs.size(), h->inflight.load(), h->track_Nref};
}
int to_set_cost_weights_batch(to_handle* h, int32_t cost_id, const double* Q, const double* R) {
  TRY(validate_cost_weights(FactsOf(h, cost_weight_facts), cost_id, Q, R));  // every refusal, before any device call and before anything changes
  TRY(use_device(h));
  DevProblem& P = h->a.P;
  TRY(cost_lane_apply(h, cost_lane_step(&h->lane, LANE_SET_WEIGHTS)));  // first use: gw and ga from the descriptors (gw may already stand, behind attitude references)
  cost_weights_store(P.n, P.m, P.B, (int)h->costs.size(), cost_id, Q, R, &h->gw_host);
  TRY(upload_cost_weights(h));
  TRY(upload_tables(h));  // (expand_variant bit 2, and with it the compact cost block, follow gw)
  return check_guards(h, "to_set_cost_weights_batch");
}
int to_get_cost_weights_batch(to_handle* h, int32_t cost_id, double* Q, double* R) {
  TRY(validate_cost_weights_get(FactsOf(h, cost_weight_facts), cost_id, Q, R));
  const DevProblem& P = h->a.P;
  const int n = P.n, m = P.m, nz = n + m, B = P.B;
  const size_t L = h->costs.size() * (size_t)nz;
  const to_cost_desc& c = h->costs[cost_id];
  for (int b = 0; b < B; ++b) {  // what every trajectory is evaluated with: the stored values, or the descriptor's diagonal repeated
    const double* v = P.gw ? h->gw_host.data() + L * b + (size_t)cost_id * nz : nullptr;
    for (int i = 0; Q && i < n; ++i) Q[i + (size_t)n * b] = v ? v[i] : c.Q[i];
    for (int j = 0; R && j < m; ++j) R[j + (size_t)m * b] = v ? v[n + j] : c.R[j];
  }
  return TO_OK;
}
int to_clear_cost_weights_batch(to_handle* h) {
  TRY(validate_cost_weights_target("to_clear_cost_weights_batch", FactsOf(h, cost_weight_facts), -1, true));
  TRY(use_device(h));
  // every cost on its descriptor's weights; the kernel variants the handle ran before unless attitude references keep it routed (gw then holds the
  // descriptors' diagonals again)
  TRY(cost_lane_apply(h, cost_lane_step(&h->lane, LANE_CLEAR_WEIGHTS)));
  return upload_tables(h);
}

// One reference quaternion per TRAJECTORY for the DiagonalQuatCost cost_id (DevProblem::ga; desc_lower.h has every refusal and the image of the
// array, path_plan.h cost_lane_step the rules by which ga rides on gw).  The setter moves the four rows of its cost and nothing else.
int to_set_cost_attitude_batch(to_handle* h, int32_t cost_id, const double* q_ref) {
  TRY(validate_cost_attitude(FactsOf(h, cost_weight_facts), cost_id, q_ref));  // every refusal, before any device call and before anything changes
  TRY(use_device(h));
  TRY(cost_lane_apply(h, cost_lane_step(&h->lane, LANE_SET_ATTITUDE)));
  TRY(upload_vec(h, q_ref, h->d_ga, 4, 4 * (int)h->costs.size(), 4 * cost_id));
  TRY(upload_tables(h));  // (routed as a handle with weights)
  return check_guards(h, "to_set_cost_attitude_batch");
}
int to_get_cost_attitude_batch(to_handle* h, int32_t cost_id, double* q_ref) {
  TRY(validate_cost_attitude_get(FactsOf(h, cost_weight_facts), cost_id, q_ref));
  if (h->a.P.ga) {  // what every trajectory is evaluated with: the device rows (the setter's, or a tracking window's) ...
    TRY(use_device(h));
    return download_vec(h, q_ref, h->d_ga, 4, 4 * (int)h->costs.size(), 4 * cost_id);
  }
  for (int b = 0; b < h->a.P.B; ++b)  // ... or the descriptor's q_ref repeated
    for (int i = 0; i < 4; ++i) q_ref[i + (size_t)4 * b] = h->costs[cost_id].q_ref[i];
  return TO_OK;
}
int to_clear_cost_attitude_batch(to_handle* h) {
  TRY(validate_cost_weights_target("to_clear_cost_attitude_batch", FactsOf(h, cost_weight_facts), -1, true));
  TRY(use_device(h));
  TRY(cost_lane_apply(h, cost_lane_step(&h->lane, LANE_CLEAR_ATTITUDE)));  // (attitude tracking, while on, writes its rows again with the next lowering)
  return upload_tables(h);
}

// One set of time steps per TRAJECTORY (DevProblem::dtb): dt[(N-1), B], knot fastest.  Validation and tiling are host-only code
// (desc_lower.h validate_time_steps, tile_rows).  The time step rides on the flagged instances that load one plant per trajectory: while
// dtb is set pm is set too — the shared plant repeated unless to_set_model_params_batch gave each trajectory its own — so the handle is
// routed exactly as one with `plants` (path_plan.h) and every launcher picks entry [1]; X, U, duals and gains are left as they are.
int to_set_time_steps_batch(to_handle* h, const double* dt) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(dt); TRY(use_device(h));
  TRY(plants_supported(h, "to_set_time_steps_batch", "time steps"));
  DevProblem& P = h->a.P;
  TRY(validate_time_steps(P.N, P.B, dt));
  TRY(upload_tiled(h, &h->d_dtb, (size_t)P.N - 1, dt, h->dt.data()));
  if (!P.pm) TRY(upload_plants(h, nullptr));
  h->dtb_host.assign(dt, dt + (size_t)(P.N - 1) * P.B);
  P.dtb = h->d_dtb;
  TRY(upload_tables(h));
  return check_guards(h, "to_set_time_steps_batch");
}
int to_get_time_steps_batch(to_handle* h, double* dt) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(dt);
  TRY(plants_supported(h, "to_get_time_steps_batch", "time steps"));
  const DevProblem& P = h->a.P;
  const size_t L = (size_t)P.N - 1;
  if (P.dtb) std::memcpy(dt, h->dtb_host.data(), sizeof(double) * L * P.B);
  else for (int b = 0; b < P.B; ++b) std::memcpy(dt + L * b, h->dt.data(), sizeof(double) * L);
  return TO_OK;
}
int to_clear_time_steps_batch(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  TRY(plants_supported(h, "to_clear_time_steps_batch", "time steps"));
  h->a.P.dtb = nullptr;
  h->dtb_host.clear();
  if (!h->pm_own) { h->a.P.pm = nullptr; h->pm_host.clear(); }
  return upload_tables(h);
}

int to_rollout(to_handle* h) { CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h)); TRY(launch_rollout(h)); HIPCHECK(hipStreamSynchronize(h->stream)); return check_guards(h, "to_rollout"); }
int to_cost(to_handle* h, double* J) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(J); TRY(use_device(h));
  TRY(launch_cost(h, 0, h->d_tmp, nullptr));
  return download_scalar(h, J, h->d_tmp);
}
int to_al_cost(to_handle* h, double* J) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(J); TRY(use_device(h));
  TRY(launch_cost(h, 1, h->d_tmp, nullptr));
  return download_scalar(h, J, h->d_tmp);
}
int to_stage_costs(to_handle* h, double* Jk) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(Jk); TRY(use_device(h));
  const DevProblem& P = h->a.P;
  // per-knot values land in a tiled array (L = N) in the upper half of the staging buffer, then transpose to host (N,B)
  const size_t cnt = (size_t)P.N * P.Bp;
  TRY(ensure_stage(h, 2 * cnt * sizeof(double)));
  double* dJk = h->stage + cnt;
  TRY(launch_cost(h, 0, nullptr, dJk));
  TRY(launch(k_to_host, grid_b(h, P.N), dim3(BLOCK), 0, h->stream, dJk, h->stage, P.N, 0, P.N, P.B));
  HIPCHECK(hipMemcpyAsync(Jk, h->stage, sizeof(double) * P.N * P.B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
static int phase_expand(to_handle* h) {
  TRY(launch_set_active(h, 1)); TRY(launch_expand(h));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return check_guards(h, "to_expand");
}
int to_expand(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  return phase_expand(h);
}
static int phase_backward(to_handle* h) {
  TRY(launch_set_active(h, 1));
  const DevProblem& P = h->a.P;
  if (h->plan.scan == 2 && scan_now(h->plan, h->a.h_diag, P.expand_variant, plants(h) != 0)) {
    // TRAJOPT_SCAN=2 (tests): the phase API runs the solve loop's scan kernel so that its gains can be read back and compared
    // (it expands on its own: to_expand's arrays are not used)
    TRY(h->ops->expand_backward_scan(h));
  } else TRY(launch_backward(h));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return check_guards(h, "to_backward");
}
int to_backward(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  return phase_backward(h);
}

// ---- closed-loop policy rollouts (k_policy.h) -------------------------------------------------------------------------------------
// PolicyRun, and everything its entry points check and compute on the host before the first device call: policy_lower.h.
static int policy_launch(to_handle* h, const PolicyRun& r, const PolicyArgs& a, int w) {
  return r.nz ? h->ops->policy_rollout_mc(h, a, w, r.nz) : h->ops->policy_rollout(h, a, w);
}
// The host half of a run — every refusal, the argument block, the lane map, the plan, the per-sample plants — is policy_lower.h
// lower_policy_opts; here: the gain refresh, the per-sample arrays (grown on demand), their pointers and the plants copy.
static int policy_prepare(to_handle* h, int32_t S, const to_policy_opts* opts, const to_policy_noise* noise, bool force_packed, PolicyRun* run) {
  const DevProblem& P = h->a.P;
  const ModelOps& ops = *h->ops;
  const PolicyFacts facts{h->model_key, P.mp, P.n, P.m, P.ne, P.N, P.B, P.pm != nullptr, P.dtb != nullptr, h->pm_host.data(),
                          ops.policy_rollout != nullptr, ops.policy_rollout_mc != nullptr, ops.policy_noise_mask, ops.lds_gains ? ops.gains_lds_pieces : 0,
                          std::getenv("TRAJOPT_POLICY_MAP"), std::getenv("TRAJOPT_POLICY_CHUNK_WAVES")};
  const double* plants_src = nullptr;
  TRY(lower_policy_opts(facts, S, opts, noise, force_packed, run, &plants_src));
  PolicyArgs& pa = run->pa;
  const PolicyPlan& pl = run->plan;
  const int nz = run->nz;
  const size_t SB = run->SB;
  TRY(use_device(h));
  if (run->refresh_gains) { TRY(phase_expand(h)); TRY(phase_backward(h)); }
  if (h->pol_cap < SB) {
    HIPCHECK(hipStreamSynchronize(h->stream));
    dev_release(h, &h->pol_x0s); dev_release(h, &h->pol_J); dev_release(h, &h->pol_cmax); dev_release(h, &h->pol_dxmax);
    dev_release(h, &h->pol_status); dev_release(h, &h->pol_klim);
    h->pol_cap = 0;
    TRY(dev_alloc(h, &h->pol_x0s, pl.x0s_len, false));
    TRY(dev_alloc(h, &h->pol_J, pl.sample_len, false)); TRY(dev_alloc(h, &h->pol_cmax, pl.sample_len, false)); TRY(dev_alloc(h, &h->pol_dxmax, pl.sample_len, false));
    TRY(dev_alloc(h, &h->pol_status, pl.sample_len, false)); TRY(dev_alloc(h, &h->pol_klim, pl.sample_len, false));
    h->pol_cap = SB;
  }
  pa.x0s = h->pol_x0s; pa.J = h->pol_J; pa.cmax = h->pol_cmax; pa.dxmax = h->pol_dxmax; pa.status = h->pol_status; pa.klim = h->pol_klim;
  if (nz & 4) {
    if (h->pol_plants_cap < SB) {
      HIPCHECK(hipStreamSynchronize(h->stream));
      dev_release(h, &h->pol_plants);
      h->pol_plants_cap = 0;
      TRY(dev_alloc(h, &h->pol_plants, pl.plants_len, false));
      h->pol_plants_cap = SB;
    }
    pa.plants = h->pol_plants;
    HIPCHECK(hipMemcpyAsync(h->pol_plants, plants_src, pl.plants_len * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  return TO_OK;
}
// The closed-loop trajectories go through a bounded staging pair, a chunk of waves at a time (path_plan.h plan_policy: chunk, xw_len, uw_len).
// Sets pa.store / Xw / Uw.
static int policy_staging(to_handle* h, PolicyRun* run, long long* chunk_out) {
  const long long chunk = run->plan.chunk;
  if (h->pol_waves < chunk) {
    HIPCHECK(hipStreamSynchronize(h->stream));
    dev_release(h, &h->pol_xw); dev_release(h, &h->pol_uw);
    h->pol_waves = 0;
    TRY(dev_alloc(h, &h->pol_xw, run->plan.xw_len, false)); TRY(dev_alloc(h, &h->pol_uw, run->plan.uw_len, false));
    h->pol_waves = (int)chunk;
  }
  run->pa.store = 1; run->pa.Xw = h->pol_xw; run->pa.Uw = h->pol_uw;
  *chunk_out = chunk;
  return TO_OK;
}
// per-sample results -> the caller's arrays (any may be NULL); the caller synchronises
static int policy_download_summaries(to_handle* h, size_t SB, double* J, double* c_max, double* dx_max, int32_t* status, int32_t* k_limit) {
  if (J) HIPCHECK(hipMemcpyAsync(J, h->pol_J, SB * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (c_max) HIPCHECK(hipMemcpyAsync(c_max, h->pol_cmax, SB * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (dx_max) HIPCHECK(hipMemcpyAsync(dx_max, h->pol_dxmax, SB * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (status) HIPCHECK(hipMemcpyAsync(status, h->pol_status, SB * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (k_limit) HIPCHECK(hipMemcpyAsync(k_limit, h->pol_klim, SB * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  return TO_OK;
}
static int policy_rollout_impl(to_handle* h, int32_t S, const double* x0s, const to_policy_opts* opts, const to_policy_noise* noise,
                               const to_policy_result* out) {
  CHECK_H(h); CHECK_IDLE(h);
  if (!x0s) return fail(TO_ERR_NULL, "to_policy_rollout: x0s is NULL");
  if (!out) return fail(TO_ERR_NULL, "to_policy_rollout: out is NULL");
  PolicyRun run;
  TRY(policy_prepare(h, S, opts, noise, false, &run));
  PolicyArgs& pa = run.pa;
  const int waves = run.waves;
  const size_t SB = run.SB;
  HIPCHECK(hipMemcpyAsync(h->pol_x0s, x0s, run.plan.x0s_len * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (!out->X && !out->U) {
    TRY(policy_launch(h, run, pa, waves));
  } else {
    // trajectories: each chunk of waves is transposed to host layout in the staging buffer and downloaded: only the caller's arrays grow with S * B * N
    const size_t Lx = run.plan.Lx, Lu = run.plan.Lu;
    long long chunk = 0;
    TRY(policy_staging(h, &run, &chunk));
    TRY(ensure_stage(h, run.plan.rollout_stage_len * sizeof(double)));
    auto first_sample = [&](long long g) { return policy_first_sample(run.plan, S, g); };
    for (long long g0 = 0; g0 < waves; g0 += chunk) {
      const int ng = (int)std::min<long long>(chunk, waves - g0);
      pa.g0 = (int)g0;
      TRY(policy_launch(h, run, pa, ng));
      const long long c0 = first_sample(g0), cnt = first_sample(g0 + ng) - c0;
      double* hx = h->stage;
      double* hu = h->stage + (size_t)cnt * Lx;
      const unsigned gx = (unsigned)((cnt + 63) / 64);
      if (out->X) enqueue(k_policy_to_host, dim3(gx, (unsigned)std::min<size_t>(Lx, 65535)), dim3(BLOCK), 0, h->stream, h->pol_xw, hx, (int)Lx, S, pa.TPW, pa.WPT, pa.g0, c0, cnt);
      if (out->U) enqueue(k_policy_to_host, dim3(gx, (unsigned)std::min<size_t>(Lu, 65535)), dim3(BLOCK), 0, h->stream, h->pol_uw, hu, (int)Lu, S, pa.TPW, pa.WPT, pa.g0, c0, cnt);
      TRY(launched());
      if (out->X) HIPCHECK(hipMemcpyAsync(out->X + (size_t)c0 * Lx, hx, (size_t)cnt * Lx * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      if (out->U) HIPCHECK(hipMemcpyAsync(out->U + (size_t)c0 * Lu, hu, (size_t)cnt * Lu * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCHECK(hipStreamSynchronize(h->stream));  // the staging pair is re-used by the next chunk
    }
  }
  TRY(policy_download_summaries(h, SB, out->J, out->c_max, out->dx_max, out->status, out->k_limit));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return check_guards(h, "to_policy_rollout");
}
int to_policy_rollout(to_handle* h, int32_t S, const double* x0s, const to_policy_opts* opts, const to_policy_result* out) {
  return policy_rollout_impl(h, S, x0s, opts, nullptr, out);
}
int to_policy_rollout_mc(to_handle* h, int32_t S, const double* x0s, const to_policy_opts* opts, const to_policy_noise* noise,
                         const to_policy_result* out) {
  return policy_rollout_impl(h, S, x0s, opts, noise, out);
}

// ---- the receding-horizon step (k_mpc.h) ---------------------------------------------------------------------------------
// to_policy_rollout_mc at S = 1 from x_meas, whose closed-loop trajectory stays on the device: per chunk of tiles the policy kernel, then
// k_mpc_writeback (x0 <- x_cl[s]; the closed-loop guess; the host-layout gather of what was applied) and, for the nominal guess, the
// in-place shift — all on the handle's stream, no synchronisation between chunks (the staging pair is re-used in stream order).  Then the
// handle's ordinary rollout of the new (x0, U).  Duals, penalties, per-trajectory arrays and gains are not touched.
int to_mpc_advance(to_handle* h, const double* x_meas, const to_mpc_opts* mpc, const to_policy_opts* popts, const to_policy_noise* noise,
                   const to_mpc_result* out) {
  static_assert(MPC_MAX_M == TO_MAX_M, "MpcArgs::u_fill holds one control");
  CHECK_H(h); CHECK_IDLE(h);
  const DevProblem& P = h->a.P;
  const int n = P.n, m = P.m, N = P.N, B = P.B;
  MpcArgs ma;
  std::memset(&ma, 0, sizeof(ma));
  TRY(lower_mpc_opts(MpcFacts{h->model_key, model_key_name(h->model_key), N, m}, mpc, ma.u_fill));  // every refusal of to_mpc_opts (policy_lower.h)
  PolicyRun run;
  TRY(policy_prepare(h, 1, popts, noise, true, &run));  // (S = 1, packed: wave g = tile g, lane = b & 63)
  PolicyArgs& pa = run.pa;
  const int s = mpc->shift, waves = run.waves;
  long long chunk = 0;
  TRY(policy_staging(h, &run, &chunk));
  // host-layout gather of the call: [x_next n B][X_applied n (s+1) B][U_applied m s B], the parts the caller asked for
  const MpcPlan mp = plan_mpc(n, m, N, B, s);
  const size_t cx = mp.cx, cX = mp.cX, cU = mp.cU;
  TRY(ensure_stage(h, mp.stage_len * sizeof(double)));
  ma.n = n; ma.m = m; ma.N = N; ma.B = B; ma.s = s; ma.guess = mpc->guess; ma.tail = mpc->tail;
  ma.Xw = h->pol_xw; ma.Uw = h->pol_uw; ma.status = h->pol_status; ma.x0 = h->a.x0; ma.Us = h->a.Us;
  ma.x_next = (out && out->x_next) ? h->stage : nullptr;
  ma.X_applied = (out && out->X_applied) ? h->stage + cx : nullptr;
  ma.U_applied = (out && out->U_applied) ? h->stage + cx + cX : nullptr;
  if (x_meas) HIPCHECK(hipMemcpyAsync(h->pol_x0s, x_meas, cx * sizeof(double), hipMemcpyHostToDevice, h->stream));
  else enqueue(k_mpc_x0_in, dim3((unsigned)waves), dim3(BLOCK), 0, h->stream, (const double*)h->a.x0, h->pol_x0s, n, B);
  for (long long g0 = 0; g0 < waves; g0 += chunk) {
    const int ng = (int)std::min<long long>(chunk, waves - g0);
    pa.g0 = ma.g0 = (int)g0;
    TRY(policy_launch(h, run, pa, ng));
    enqueue(k_mpc_writeback, dim3((unsigned)ng, (unsigned)mp.row_groups), dim3(BLOCK), 0, h->stream, ma);
    if (ma.guess == TO_MPC_GUESS_NOMINAL) enqueue(k_mpc_shift_nominal, dim3((unsigned)ng), dim3(BLOCK), 0, h->stream, ma);
    TRY(launched());
  }
  if (ma.x_next) HIPCHECK(hipMemcpyAsync(out->x_next, ma.x_next, cx * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (ma.X_applied) HIPCHECK(hipMemcpyAsync(out->X_applied, ma.X_applied, cX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (ma.U_applied) HIPCHECK(hipMemcpyAsync(out->U_applied, ma.U_applied, cU * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out) TRY(policy_download_summaries(h, run.SB, out->J, out->c_max, out->dx_max, out->status, out->k_limit));
  TRY(launch_rollout(h));  // the state to_set_initial_state + to_set_controls + to_rollout would have left
  HIPCHECK(hipStreamSynchronize(h->stream));
  return check_guards(h, "to_mpc_advance");
}
// ---- the dual shift of the receding-horizon loop (k_mpc.h k_mpc_shift_duals) -----------------------------------------------
// One launch over (tiles, constraints) after the 4 B bytes of the actions; every refusal before any device call (desc_lower.h).
int to_mpc_shift_duals(to_handle* h, int32_t shift, int32_t tail, const int32_t* action) {
  CHECK_H(h);
  const DevProblem& P = h->a.P;
  TRY(validate_mpc_shift_duals(MpcDualFacts{h->model_key, model_key_name(h->model_key), P.N, P.B, h->inflight.load()}, shift, tail, action));
  if (P.n_cons == 0) return TO_OK;
  TRY(use_device(h));
  std::vector<MpcDualCon> table;  // (lives until the synchronisation below)
  if (!h->d_dual_cons) {
    for (const DevCon& c : h->cons) table.push_back(MpcDualCon{c.dual_off, c.p, c.k2 - c.k1 + 1});
    TRY(dev_alloc(h, &h->d_dual_cons, table.size(), false));
    HIPCHECK(hipMemcpyAsync(h->d_dual_cons, table.data(), table.size() * sizeof(MpcDualCon), hipMemcpyHostToDevice, h->stream));
  }
  if (action) {
    if (!h->d_dual_action) TRY(dev_alloc(h, &h->d_dual_action, (size_t)P.Bp));
    HIPCHECK(hipMemcpyAsync(h->d_dual_action, action, sizeof(int32_t) * P.B, hipMemcpyHostToDevice, h->stream));
  }
  MpcDualArgs da;
  da.B = P.B; da.n_cons = P.n_cons; da.s = shift; da.tail = tail; da.n_duals = P.n_duals; da.mu_reset = P.opts.penalty_initial;
  da.cons = h->d_dual_cons; da.action = action ? h->d_dual_action : nullptr; da.lam = h->a.lam; da.mu = h->a.mu;
  TRY(launch(k_mpc_shift_duals, dim3((unsigned)(P.Bp / 64), (unsigned)P.n_cons), dim3(BLOCK), 0, h->stream, da));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return check_guards(h, "to_mpc_shift_duals");
}
// ---- one tracking reference per trajectory, windowed on the device (k_track.h) --------------------------------------------------------
static TrackFacts track_facts(const to_handle* h) {
  const DevProblem& P = h->a.P;
  return TrackFacts{h->model_key, model_key_name(h->model_key), P.n, P.m, P.N, P.B, h->costs.data(), (int)h->costs.size(), h->cost_index.data(),
                    h->inflight.load(), h->track_Nref, h->track_end, h->lane.weights};
}
// the stored starts -> the device, then all N knots of every trajectory into d_gl from the current descriptors (one launch)
static int track_lower(to_handle* h, const char* who) {
  DevProblem& P = h->a.P;
  const int nz = P.n + P.m;
  TRY(ensure_gl(h));
  HIPCHECK(hipMemcpyAsync(h->d_track_start, h->track_start.data(), sizeof(int32_t) * P.B, hipMemcpyHostToDevice, h->stream));
  TrackArgs ta;
  ta.n = P.n; ta.m = P.m; ta.N = P.N; ta.B = P.B; ta.Nref = h->track_Nref; ta.with_u = h->track_u ? 1 : 0; ta.n_costs = (int)h->costs.size();
  ta.ref = h->d_track_ref; ta.start = h->d_track_start; ta.cost_index = P.cost_index; ta.costs = P.costs; ta.gl = h->d_gl;
  ta.ga = h->lane.track_attitude ? h->d_ga : nullptr;  // attitude tracking: the same launch writes the q_ref rows of the DiagonalQuatCost knots
  const int rows = P.N * (h->track_u ? nz : P.n) + (ta.ga ? P.N * 4 : 0);
  TRY(launch(k_track_lower, dim3((unsigned)(P.Bp / 64), (unsigned)std::min(rows, 32)), dim3(BLOCK), 0, h->stream, ta));
  HIPCHECK(hipStreamSynchronize(h->stream));
  P.gl = h->d_gl;
  for (int k = 0; k < P.N; ++k) h->gl_set[h->cost_index[k]] = 1;
  return check_guards(h, who);
}
int to_set_tracking_reference_batch(to_handle* h, int32_t Nref, const double* Xref, const double* Uref, const int32_t* start, int32_t end_mode) {
  CHECK_H(h);
  TRY(validate_tracking_reference(track_facts(h), Nref, Xref, Uref, start, end_mode));  // every refusal, before any device call
  TRY(use_device(h));
  const DevProblem& P = h->a.P;
  const int nz = P.n + P.m, B = P.B;
  std::vector<double> packed;
  pack_tracking_reference(P.n, P.m, B, Nref, Xref, Uref, &packed);
  dev_release(h, &h->d_track_ref);  // (a reference of another length replaces the stored one)
  h->track_Nref = 0;
  TRY(dev_alloc(h, &h->d_track_ref, (size_t)Nref * nz * P.Bp));
  if (!h->d_track_start) TRY(dev_alloc(h, &h->d_track_start, (size_t)P.Bp));
  TRY(upload_vec(h, packed.data(), h->d_track_ref, Nref * nz));
  h->track_start.assign(B, 1);
  if (start) std::copy(start, start + B, h->track_start.begin());
  h->track_Nref = Nref; h->track_end = end_mode; h->track_u = Uref != nullptr;
  return track_lower(h, "to_set_tracking_reference_batch");
}
int to_set_tracking_window(to_handle* h, const int32_t* start) {
  CHECK_H(h);
  TRY(validate_tracking_window(track_facts(h), start));
  TRY(use_device(h));
  std::copy(start, start + h->a.P.B, h->track_start.begin());
  return track_lower(h, "to_set_tracking_window");
}
int to_get_tracking_window(to_handle* h, int32_t* Nref, int32_t* end_mode, int32_t* start) {
  CHECK_H(h);
  if (Nref) *Nref = h->track_Nref;
  if (end_mode) *end_mode = h->track_Nref ? h->track_end : TO_TRACK_END_REFUSE;
  if (start) for (int b = 0; b < h->a.P.B; ++b) start[b] = h->track_Nref ? h->track_start[b] : 1;
  return TO_OK;
}
// attitude tracking off: the tracked costs' q_ref back on their descriptors.  Without setter calls of the caller's the whole array is filled again
// in one copy (a tracking objective has a cost per knot: every cost in use is a tracked one); next to them only the tracked DiagonalQuatCosts
// restart, four rows at a time, and a cost outside the window keeps what the caller gave it
static int tracking_attitude_off(to_handle* h) {
  if (!h->lane.track_attitude) return TO_OK;
  if (!h->lane.attitude) TRY(upload_cost_attitudes(h));
  else for (int k = 0; k < h->a.P.N; ++k) if (h->costs[h->cost_index[k]].kind == TO_COST_DIAGONAL_QUAT) TRY(restart_cost_attitude(h, h->cost_index[k]));
  TRY(cost_lane_apply(h, cost_lane_step(&h->lane, LANE_TRACK_OFF)));
  return upload_tables(h);
}
int to_set_tracking_attitude(to_handle* h, int32_t on) {
  TRY(validate_tracking_attitude(FactsOf(h, track_facts), on));
  TRY(use_device(h));
  if (!on) return tracking_attitude_off(h);
  TRY(cost_lane_apply(h, cost_lane_step(&h->lane, LANE_TRACK_ON)));
  TRY(upload_tables(h));
  return track_lower(h, "to_set_tracking_attitude");
}
int to_get_tracking_attitude(to_handle* h, int32_t* on) {
  CHECK_H(h); CHECK_P(on);
  *on = h->lane.track_attitude ? 1 : 0;
  return TO_OK;
}
int to_clear_tracking_reference_batch(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  TRY(tracking_attitude_off(h));
  dev_release(h, &h->d_track_ref);
  dev_release(h, &h->d_track_start);
  h->track_start.clear();
  h->track_Nref = 0; h->track_end = 0; h->track_u = false;
  return to_clear_cost_linear_batch(h);
}
int to_get_cost_linear_batch(to_handle* h, int32_t id, double* q, double* r) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  if (id < 0 || id >= (int)h->costs.size()) return fail(TO_ERR_ARGUMENT, "cost id out of range");
  if (!q && !r) return fail(TO_ERR_NULL, "null pointer");
  const to_cost_desc& c = h->costs[id];
  const DevProblem& P = h->a.P;
  const int n = P.n, m = P.m, nz = n + m, L = (int)h->costs.size() * nz, B = P.B;
  // what the kernels evaluate: the descriptor's term plus the stored difference (zero while nothing is set)
  if (q) {
    if (h->d_gl) TRY(download_vec(h, q, h->d_gl, n, L, id * nz));
    for (int b = 0; b < B; ++b) for (int i = 0; i < n; ++i) q[i + (size_t)n * b] = h->d_gl ? c.q[i] + q[i + (size_t)n * b] : c.q[i];
  }
  if (r) {
    if (h->d_gl) TRY(download_vec(h, r, h->d_gl, m, L, id * nz + n));
    for (int b = 0; b < B; ++b) for (int j = 0; j < m; ++j) r[j + (size_t)m * b] = h->d_gl ? c.r[j] + r[j + (size_t)m * b] : c.r[j];
  }
  return TO_OK;
}
// the generator alone (k_policy_noise_draws), so that a parity failure of the stochastic rollout can be localised to it or to the loop
int to_policy_noise_draws(int device, uint64_t seed, uint32_t traj, uint32_t sample, uint32_t k, uint32_t kind, int32_t pairs, double* z) {
  CHECK_P(z);
  if (pairs < 1 || pairs > 256) return fail(TO_ERR_ARGUMENT, "to_policy_noise_draws: pairs must be in 1 .. 256 (the counter holds kind * 256 + pair)");
  if (kind > 1) return fail(TO_ERR_ARGUMENT, "to_policy_noise_draws: kind must be 0 (process noise) or 1 (measurement noise)");
  HIPCHECK(hipSetDevice(device));
  struct DevBuf {  // freed on every exit path
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
  } bz;
  HIPCHECK(hipMalloc(&bz.p, (size_t)2 * pairs * sizeof(double)));
  TRY(launch(k_policy_noise_draws, dim3(1), dim3(64), 0, 0, (unsigned long long)seed, traj, sample, k, kind, (int)pairs, (double*)bz.p));
  HIPCHECK(hipMemcpy(z, bz.p, (size_t)2 * pairs * sizeof(double), hipMemcpyDeviceToHost));
  return TO_OK;
}
int to_forward(to_handle* h, int32_t* ls_index, double* J_new) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  h->a.control = 0;
  // keep bpfail from a preceding to_backward: set active without clearing it
  TRY(launch_cost(h, 1, h->a.J, nullptr));
  TRY(launch_set_active(h, 1, 2));
  h->a.step = 0;
  TRY(launch_forward(h));
  TRY(download_int(h, ls_index, h->a.ls_index));
  TRY(download_scalar(h, J_new, h->a.Jout));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return check_guards(h, "to_forward");
}
int to_ilqr_solve(to_handle* h, to_solve_stats* st) { CHECK_H(h); CHECK_IDLE(h); return solve(h, st, 0); }
int to_al_solve(to_handle* h, to_solve_stats* st) { CHECK_H(h); CHECK_IDLE(h); return solve(h, st, 1); }
int to_pn_solve(to_handle* h, to_solve_stats* st) { CHECK_H(h); CHECK_IDLE(h); return pn_solve(h, st); }
int to_altro_solve(to_handle* h, to_solve_stats* st) { CHECK_H(h); CHECK_IDLE(h); return altro_solve(h, st); }
// Asynchronous solves: the solve loop — enqueue chunks of batch steps, read the activity counters back — runs on
// a worker thread owned by the handle; the handle's stream carries the kernels as before.  Two handles (two streams) solved this
// way overlap on the device: the drained tail of one batch leaves most of the chip to the other.
static int solve_async(to_handle* h, to_solve_stats* st, int kind) {
  CHECK_H(h);
  if (h->inflight) return fail(TO_ERR_ARGUMENT, "a solve is already in flight on this handle (call to_solve_wait first)");
  h->inflight = true;
  h->async_rc = TO_OK;
  h->prog_active = h->a.P.B; h->prog_steps = 0;  // (before the worker exists: a to_solve_wait_below right behind this call must block)
  try {  // no exception may cross the C ABI (std::system_error: out of threads)
    h->worker = std::thread([h, st, kind] {
      h->async_rc = kind == 0 ? solve(h, st, 0) : kind == 1 ? solve(h, st, 1) : altro_solve(h, st);
      h->async_err = g_err;
    });
  } catch (const std::exception& e) {
    h->inflight = false;
    h->prog_active = 0;
    return fail(TO_ERR_HIP, std::string("could not start the solve thread: ") + e.what());
  }
  return TO_OK;
}
int to_ilqr_solve_async(to_handle* h, to_solve_stats* st) { return solve_async(h, st, 0); }
int to_al_solve_async(to_handle* h, to_solve_stats* st) { return solve_async(h, st, 1); }
int to_altro_solve_async(to_handle* h, to_solve_stats* st) { return solve_async(h, st, 2); }
int to_solve_wait(to_handle* h) {
  CHECK_H(h);
  if (!h->inflight) return TO_OK;
  h->worker.join();
  h->inflight = false;
  if (h->async_rc != TO_OK) g_err = h->async_err;
  return h->async_rc;
}
int to_solve_progress(to_handle* h, int32_t* active, int32_t* batch_steps, int32_t* in_flight) {
  CHECK_H(h);
  if (active) *active = h->prog_active.load();
  if (batch_steps) *batch_steps = h->prog_steps.load();
  if (in_flight) *in_flight = h->inflight ? 1 : 0;
  return TO_OK;
}
int to_solve_wait_below(to_handle* h, int32_t active_max) {
  CHECK_H(h);
  if (active_max < 0) return fail(TO_ERR_ARGUMENT, "to_solve_wait_below: the threshold must be >= 0");
  std::unique_lock<std::mutex> lk(h->prog_mu);
  h->prog_cv.wait(lk, [&] { return h->prog_active.load() <= active_max; });
  return TO_OK;
}
int to_dynamics_defect(to_handle* h, double* defect) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(defect);
  TRY(use_device(h));
  TRY(launch_defect(h, h->d_tmp));
  return download_scalar(h, defect, h->d_tmp);
}

// expansion blocks -> host column-major blocks: h[r + Rr*(c + Cc*(k + K*b))] = X_k[row0+r][col0+c], rows / columns counted
// in error-state directions followed by control directions (whichever layout the backward pass uses)
enum { BLK_M = 0, BLK_H = 1 };
static int download_block(to_handle* h, double* host, int which, int row0, int Rr, int col0, int Cc, double* dev_out = nullptr) {
  if (!host && !dev_out) return TO_OK;
  const DevProblem& P = h->a.P;
  const int K = which == BLK_M ? P.N - 1 : P.N;
  const size_t cnt = (size_t)Rr * Cc * K * P.B;
  if (!dev_out) TRY(ensure_stage(h, cnt * sizeof(double)));
  double* const out = dev_out ? dev_out : h->stage;  // (dev_out: a caller-owned device buffer, no host copy)
  if (h->a.bwd_lane) {
    const int nc = P.ne + P.m;
    if (which == BLK_M)
      enqueue(k_lane_to_host, grid_b(h, K * Rr * Cc), dim3(BLOCK), 0, h->stream, h->a.Mc, out, P.ne * nc, 0, nc, row0, Rr, col0, Cc, K, P.B);
    else
      enqueue(k_lane_to_host, grid_b(h, K * Rr * Cc), dim3(BLOCK), 0, h->stream, h->a.Hc, out, nc * (nc + 1) / 2, 1, nc, row0, Rr, col0, Cc, K, P.B);
  } else if (h->a.bwd_mfma) {
    const int nep = h->ops->nep, rs = h->ops->rs;
    auto tix = [&](int i) { return i < P.ne ? i : nep + (i - P.ne); };  // tangent index (control directions start at NEP)
    const bool compact = which == BLK_H && h->a.h_compact;
    enqueue(k_tm_to_host, grid_b(h, K * Rr * Cc), dim3(BLOCK), 0, h->stream, which == BLK_M ? h->a.Mt : h->a.Ht, out,
                       which == BLK_M ? rs : rs + 1, tix(row0), Rr, tix(col0), Cc, K, P.B, compact ? h->d_crow : nullptr);
  } else {
    const int nc = P.ne + P.m;
    const int diag = (which == BLK_H && h->a.h_diag) ? 1 : 0;
    enqueue(k_col_to_host, grid_b(h, K * Rr * Cc), dim3(BLOCK), 0, h->stream, which == BLK_M ? h->a.Mc : h->a.Hc, out,
                       which == BLK_M ? (P.N - 1) * P.ne : (diag ? P.N : P.N * nc), which == BLK_M ? P.ne : nc, row0, Rr, col0, Cc, K, P.B,
                       h->R, h->G, diag);
  }
  TRY(launched());
  if (dev_out) return TO_OK;
  HIPCHECK(hipMemcpyAsync(host, h->stage, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
static int download_gradient(to_handle* h, double* host, int col0, int Cc, double* dev_out = nullptr) {
  if (!host && !dev_out) return TO_OK;
  const DevProblem& P = h->a.P;
  const size_t cnt = (size_t)Cc * P.N * P.B;
  if (!dev_out) TRY(ensure_stage(h, cnt * sizeof(double)));
  double* const out = dev_out ? dev_out : h->stage;
  if (h->a.bwd_lane) {
    const int nc = P.ne + P.m;
    enqueue(k_lane_to_host, grid_b(h, P.N * Cc), dim3(BLOCK), 0, h->stream, h->a.gc, out, nc, 0, nc, 0, 1, col0, Cc, P.N, P.B);
  } else if (h->a.bwd_mfma) {
    const int tcol = col0 < P.ne ? col0 : h->ops->nep + (col0 - P.ne);
    enqueue(k_tmvec_to_host, grid_b(h, P.N * Cc), dim3(BLOCK), 0, h->stream, h->a.gt, out, tcol, Cc, P.N, P.B);
  } else {
    enqueue(k_col_to_host, grid_b(h, P.N * Cc), dim3(BLOCK), 0, h->stream, h->a.gc, out, P.N, 1, 0, 1, col0, Cc, P.N, P.B, h->R, h->G, 0);
  }
  TRY(launched());
  if (dev_out) return TO_OK;
  HIPCHECK(hipMemcpyAsync(host, h->stage, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
int to_get_dynamics_jacobians(to_handle* h, double* A, double* Bm) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  const DevProblem& P = h->a.P;
  TRY(download_block(h, A, BLK_M, 0, P.ne, 0, P.ne));
  TRY(download_block(h, Bm, BLK_M, 0, P.ne, P.ne, P.m));
  return TO_OK;
}
int to_get_cost_expansion(to_handle* h, double* Qxx, double* Quu, double* Qux, double* qx, double* qu) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  const DevProblem& P = h->a.P;
  TRY(download_block(h, Qxx, BLK_H, 0, P.ne, 0, P.ne));
  TRY(download_block(h, Quu, BLK_H, P.ne, P.m, P.ne, P.m));
  TRY(download_block(h, Qux, BLK_H, P.ne, P.m, 0, P.ne));
  TRY(download_gradient(h, qx, 0, P.ne));
  TRY(download_gradient(h, qu, P.ne, P.m));
  return TO_OK;
}
int to_get_gains(to_handle* h, double* K, double* d, double* dV, double* rho) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  const DevProblem& P = h->a.P;
  if (K || d) {
    const size_t nK = (size_t)P.m * P.ne * (P.N - 1) * P.B, nd = (size_t)P.m * (P.N - 1) * P.B;
    TRY(ensure_stage(h, (nK + nd) * sizeof(double)));
    double *dK = h->stage, *dd = h->stage + nK;
    TRY(launch(k_gains_to_host, grid_b(h, (P.N - 1) * P.m * (P.ne + 1)), dim3(BLOCK), 0, h->stream, h->a.Kt, dK, dd, P.m, P.ne, P.N - 1, P.B));
    if (K) HIPCHECK(hipMemcpyAsync(K, dK, nK * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (d) HIPCHECK(hipMemcpyAsync(d, dd, nd * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  if (dV) {  // plain [2][Bp] -> host (2, B)
    std::vector<double> tmp(2 * (size_t)P.Bp);
    HIPCHECK(hipMemcpyAsync(tmp.data(), h->a.dV, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    for (int b = 0; b < P.B; ++b) { dV[2 * b] = tmp[b]; dV[2 * b + 1] = tmp[(size_t)P.Bp + b]; }
  }
  TRY(download_scalar(h, rho, h->a.rho));
  return TO_OK;
}
int to_get_cost_to_go(to_handle* h, double* S, double* s) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  if (!S && !s) return fail(TO_ERR_NULL, "null pointer");
  const DevProblem& P = h->a.P;
  const size_t ne = P.ne, m = P.m, N = P.N, B = P.B;
  // every block in its getter layout, side by side in one device buffer, then the recursion (k_generic.h k_cost_to_go)
  const size_t nA = ne * ne * (N - 1) * B, nB = ne * m * (N - 1) * B, nxx = ne * ne * N * B, nuu = m * m * N * B, nux = m * ne * N * B,
               nx = ne * N * B, nu = m * N * B, nK = m * ne * (N - 1) * B, nd = m * (N - 1) * B;
  struct DevBuf { void* p = nullptr; ~DevBuf() { if (p) hipFree(p); } } buf;
  HIPCHECK(hipMalloc(&buf.p, (nA + nB + nxx + nuu + nux + nx + nu + nK + nd + nxx + nx) * sizeof(double)));
  double* dA = (double*)buf.p; double* dB = dA + nA; double* dxx = dB + nB; double* duu = dxx + nxx; double* dux = duu + nuu;
  double* dx = dux + nux; double* du = dx + nx; double* dK = du + nu; double* dd = dK + nK; double* dS = dd + nd; double* ds = dS + nxx;
  TRY(download_block(h, nullptr, BLK_M, 0, P.ne, 0, P.ne, dA));
  TRY(download_block(h, nullptr, BLK_M, 0, P.ne, P.ne, P.m, dB));
  TRY(download_block(h, nullptr, BLK_H, 0, P.ne, 0, P.ne, dxx));
  TRY(download_block(h, nullptr, BLK_H, P.ne, P.m, P.ne, P.m, duu));
  TRY(download_block(h, nullptr, BLK_H, P.ne, P.m, 0, P.ne, dux));
  TRY(download_gradient(h, nullptr, 0, P.ne, dx));
  TRY(download_gradient(h, nullptr, P.ne, P.m, du));
  enqueue(k_gains_to_host, grid_b(h, (P.N - 1) * P.m * (P.ne + 1)), dim3(BLOCK), 0, h->stream, h->a.Kt, dK, dd, P.m, P.ne, P.N - 1, P.B);
  TRY(launch(k_cost_to_go, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, dA, dB, dxx, duu, dux, dx, du, dK, dd, dS, ds, P.ne, P.m, P.N, P.B));
  if (S) HIPCHECK(hipMemcpyAsync(S, dS, nxx * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (s) HIPCHECK(hipMemcpyAsync(s, ds, nx * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
int to_cost_expansion(to_handle* h, double* grad, double* hess) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  const DevProblem& P = h->a.P;
  const size_t nz = P.n + P.m, ng = nz * P.N * P.B, nh = nz * nz * P.N * P.B;
  TRY(ensure_stage(h, (ng + nh) * sizeof(double)));
  double* dg = h->stage; double* dh = h->stage + ng;
  TRY(h->ops->cost_derivs(h, dg, dh));
  if (grad) HIPCHECK(hipMemcpyAsync(grad, dg, ng * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (hess) HIPCHECK(hipMemcpyAsync(hess, dh, nh * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
int to_discrete_jacobian(to_handle* h, double* F) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(F); TRY(use_device(h));
  const DevProblem& P = h->a.P;
  const size_t cnt = (size_t)P.n * (P.n + P.m) * (P.N - 1) * P.B;
  TRY(ensure_stage(h, cnt * sizeof(double)));
  TRY(launch_discrete_jacobian(h, h->stage));
  HIPCHECK(hipMemcpyAsync(F, h->stage, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}

int to_constraint_info(const to_handle* h, int32_t id, int32_t* p, int32_t* width, int32_t* nk, int32_t* sense) {
  CHECK_H(h);
  if (id < 0 || id >= (int)h->cons.size()) return fail(TO_ERR_ARGUMENT, "constraint id out of range");
  const DevCon& ci = h->cons[id];
  if (p) *p = ci.p; if (width) *width = ci.width; if (nk) *nk = ci.k2 - ci.k1 + 1; if (sense) *sense = ci.d.sense;
  return TO_OK;
}
static int constraint_eval(to_handle* h, int32_t id, double* vals, double* jac) {
  TRY(use_device(h));
  if (id < 0 || id >= (int)h->cons.size()) return fail(TO_ERR_ARGUMENT, "constraint id out of range");
  const DevCon& ci = h->cons[id];
  const DevProblem& P = h->a.P;
  const int nk = ci.k2 - ci.k1 + 1;
  const size_t nv = (size_t)ci.p * nk * P.B, nj = (size_t)ci.p * ci.width * nk * P.B;
  TRY(ensure_stage(h, (nv + nj) * sizeof(double)));
  double* dv = h->stage; double* dj = h->stage + nv;
  TRY(h->ops->constraint_eval(h, (int)id, vals ? dv : nullptr, jac ? dj : nullptr));
  if (vals) HIPCHECK(hipMemcpyAsync(vals, dv, nv * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (jac) HIPCHECK(hipMemcpyAsync(jac, dj, nj * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
int to_evaluate_constraints(to_handle* h, int32_t id, double* vals) { CHECK_H(h); CHECK_IDLE(h); CHECK_P(vals); return constraint_eval(h, id, vals, nullptr); }
int to_constraint_jacobians(to_handle* h, int32_t id, double* jac) { CHECK_H(h); CHECK_IDLE(h); CHECK_P(jac); return constraint_eval(h, id, nullptr, jac); }
int to_constraint_hessians(to_handle* h, int32_t id, const double* lambda, double* H) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(lambda); CHECK_P(H); TRY(use_device(h));
  if (id < 0 || id >= (int)h->cons.size()) return fail(TO_ERR_ARGUMENT, "constraint id out of range");
  const DevCon& ci = h->cons[id];
  const DevProblem& P = h->a.P;
  const int nk = ci.k2 - ci.k1 + 1;
  const size_t nl = (size_t)ci.p * nk * P.B, nh = (size_t)ci.width * ci.width * nk * P.B;
  TRY(ensure_stage(h, (nl + nh) * sizeof(double)));
  double* dl = h->stage; double* dh = h->stage + nl;
  HIPCHECK(hipMemcpyAsync(dl, lambda, nl * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(dh, H, nh * sizeof(double), hipMemcpyHostToDevice, h->stream));  // the operator ADDS (src/abstract_constraint.jl:255-266)
  TRY(h->ops->constraint_hessian(h, (int)id, dl, dh));
  HIPCHECK(hipMemcpyAsync(H, dh, nh * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
int to_max_violation(to_handle* h, double* c_max) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(c_max); TRY(use_device(h));
  if (h->a.P.n_cons == 0) { std::memset(c_max, 0, sizeof(double) * h->a.P.B); return TO_OK; }
  TRY(launch_violation(h, h->d_tmp));
  return download_scalar(h, c_max, h->d_tmp);
}
int to_get_duals(to_handle* h, int32_t id, double* lambda, double* mu) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  if (id < 0 || id >= (int)h->cons.size()) return fail(TO_ERR_ARGUMENT, "constraint id out of range");
  const DevCon& ci = h->cons[id];
  const DevProblem& P = h->a.P;
  if (lambda) TRY(download_vec(h, lambda, h->a.lam, ci.p * (ci.k2 - ci.k1 + 1), (int)P.n_duals, (int)ci.dual_off));
  if (mu) TRY(download_vec(h, mu, h->a.mu, 1, P.n_cons, id));
  return TO_OK;
}
int to_set_duals(to_handle* h, int32_t id, const double* lambda, const double* mu) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  if (id < 0 || id >= (int)h->cons.size()) return fail(TO_ERR_ARGUMENT, "constraint id out of range");
  const DevCon& ci = h->cons[id];
  const DevProblem& P = h->a.P;
  if (lambda) TRY(upload_vec(h, lambda, h->a.lam, ci.p * (ci.k2 - ci.k1 + 1), (int)P.n_duals, (int)ci.dual_off));
  if (mu) TRY(upload_vec(h, mu, h->a.mu, 1, P.n_cons, id));
  return TO_OK;
}
int to_reset_duals(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  const DevProblem& P = h->a.P;
  if (P.n_cons == 0) return TO_OK;
  HIPCHECK(hipMemsetAsync(h->a.lam, 0, sizeof(double) * (size_t)P.n_duals * P.Bp, h->stream));
  std::vector<double> mu((size_t)P.n_cons * P.Bp, P.opts.penalty_initial);
  HIPCHECK(hipMemcpyAsync(h->a.mu, mu.data(), mu.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
int to_dual_update(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h); TRY(use_device(h));
  if (h->a.P.n_cons == 0) return TO_OK;
  TRY(h->ops->dual_update(h));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}

// ---- multi-GPU: the batch shards across ranks as independent units; the only collective is one RCCL
// all-gather of the converged trajectories per solve.  librccl.so is loaded on first use (dlopen), so single-GPU hosts
// need no RCCL at all; a host in ANY language (Julia ccall, Python ctypes) exchanges the 128-byte id out of band
// (MPI / a file / torch.distributed) exactly as with ncclGetUniqueId.
int to_comm_unique_id(void* id128) {
  CHECK_P(id128);
  TRY(load_rccl());
  RCCLCHECK(g_rccl.GetUniqueId(id128));
  return TO_OK;
}
int to_comm_init_rank(to_handle* h, int32_t nranks, int32_t rank, const void* id128) {
  CHECK_H(h); CHECK_IDLE(h); CHECK_P(id128);
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(TO_ERR_ARGUMENT, "rank outside 0..nranks-1");
  if (h->comm) return fail(TO_ERR_ARGUMENT, "communicator already initialised (to_comm_destroy first)");
  TRY(load_rccl());
  TRY(use_device(h));
  Rccl::Id id;
  std::memcpy(id.b, id128, sizeof(id.b));
  RCCLCHECK(g_rccl.CommInitRank(&h->comm, nranks, id, rank));
  h->comm_rank = rank; h->comm_size = nranks;
  // every error from here on leaves the handle without a communicator (a half-initialised one would let a later to_allgather
  // run against peers that have already given up)
  auto abandon = [&](int code, const char* msg) {
    g_rccl.CommDestroy(h->comm);
    h->comm = nullptr; h->comm_rank = 0; h->comm_size = 1; h->comm_counts.clear();
    h->comm_offset = 0; h->comm_total = 0; h->comm_equal = true;
    return fail(code, msg);
  };
  // shard sizes of every rank (they may differ: a batch that does not divide by the number of GPUs)
  int32_t* dcnt = nullptr;
  if (hipMalloc((void**)&dcnt, sizeof(int32_t) * nranks) != hipSuccess) return abandon(TO_ERR_HIP, "to_comm_init_rank: hipMalloc failed");
  const int32_t mine = h->a.P.B;
  hipError_t e1 = hipMemcpyAsync(dcnt + rank, &mine, sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
  int rc = e1 == hipSuccess ? g_rccl.AllGather(dcnt + rank, dcnt, 1, kNcclInt32, h->comm, h->stream) : 0;
  h->comm_counts.assign(nranks, 0);
  hipError_t e2 = hipMemcpyAsync(h->comm_counts.data(), dcnt, sizeof(int32_t) * nranks, hipMemcpyDeviceToHost, h->stream);
  hipError_t e3 = hipStreamSynchronize(h->stream);
  hipFree(dcnt);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || rc != 0)
    return abandon(TO_ERR_HIP, "to_comm_init_rank: exchanging the shard sizes failed");
  h->comm_offset = 0; h->comm_total = 0; h->comm_equal = true;
  for (int r = 0; r < nranks; ++r) {
    if (h->comm_counts[r] < 1) return abandon(TO_ERR_ARGUMENT, "to_comm_init_rank: a rank reported an empty shard");
    if (r < rank) h->comm_offset += h->comm_counts[r];
    h->comm_total += h->comm_counts[r];
    h->comm_equal = h->comm_equal && h->comm_counts[r] == h->comm_counts[0];
  }
  return TO_OK;
}
int to_comm_shards(const to_handle* h, int32_t* nranks, int32_t* rank, int64_t* B_total, int32_t* counts) {
  CHECK_H(h);
  if (!h->comm) return fail(TO_ERR_ARGUMENT, "to_comm_init_rank first");
  if (nranks) *nranks = h->comm_size;
  if (rank) *rank = h->comm_rank;
  if (B_total) *B_total = h->comm_total;
  if (counts) for (int r = 0; r < h->comm_size; ++r) counts[r] = h->comm_counts[r];
  return TO_OK;
}
int to_comm_destroy(to_handle* h) {
  CHECK_H(h); CHECK_IDLE(h);
  if (!h->comm) return TO_OK;
  TRY(use_device(h));
  HIPCHECK(hipStreamSynchronize(h->stream));
  RCCLCHECK(g_rccl.CommDestroy(h->comm));
  h->comm = nullptr; h->comm_rank = 0; h->comm_size = 1; h->comm_counts.clear();
  return TO_OK;
}
// Every rank's block, gathered in rank order into `all` (count[r] * per doubles / int32 from rank r at offset[r] * per):
// one in-place ncclAllGather when the shards are equal, else one grouped ncclBroadcast per rank (same bytes on the wire).
static int gather_blocks(to_handle* h, void* all, size_t per, int dtype, size_t elt) {
  char* base = (char*)all;
  char* mine = base + (size_t)h->comm_offset * per * elt;
  if (h->comm_equal) {
    RCCLCHECK(g_rccl.AllGather(mine, all, (size_t)h->a.P.B * per, dtype, h->comm, h->stream));
    return TO_OK;
  }
  RCCLCHECK(g_rccl.GroupStart());
  size_t off = 0;
  for (int r = 0; r < h->comm_size; ++r) {
    char* blk = base + off * per * elt;
    const int rc = g_rccl.Broadcast(blk, blk, (size_t)h->comm_counts[r] * per, dtype, r, h->comm, h->stream);
    if (rc != 0) { g_rccl.GroupEnd(); return fail(TO_ERR_HIP, std::string("ncclBroadcast: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "rccl error")); }
    off += (size_t)h->comm_counts[r];
  }
  RCCLCHECK(g_rccl.GroupEnd());
  return TO_OK;
}
// dX_all / dU_all: caller-owned DEVICE buffers of n*N*B_total and m*(N-1)*B_total doubles (B_total = sum of the ranks' shard
// sizes, to_comm_shards); on return (the call synchronises the handle's stream) they hold every rank's trajectories in host
// layout (n, N, B_total), rank-major = global trajectory order.  Shards may differ in size.
int to_allgather(to_handle* h, void* dX_all, void* dU_all) {
  CHECK_H(h); CHECK_IDLE(h);
  if (!dX_all && !dU_all) return fail(TO_ERR_NULL, "null pointer");
  if (!h->comm) return fail(TO_ERR_ARGUMENT, "to_comm_init_rank first");
  TRY(use_device(h));
  const DevProblem& P = h->a.P;
  const size_t px = (size_t)P.n * P.N, pu = (size_t)P.m * (P.N - 1);
  if (dX_all) {  // own shard written in place, then one in-place gather on the handle's stream
    double* mine = (double*)dX_all + px * (size_t)h->comm_offset;
    TRY(launch(k_to_host, grid_b(h, P.n * P.N), dim3(BLOCK), 0, h->stream, h->a.Xs, mine, P.n * P.N, 0, P.n * P.N, P.B));
    TRY(gather_blocks(h, dX_all, px, kNcclDouble, sizeof(double)));
  }
  if (dU_all) {
    double* mine = (double*)dU_all + pu * (size_t)h->comm_offset;
    TRY(launch(k_to_host, grid_b(h, P.m * (P.N - 1)), dim3(BLOCK), 0, h->stream, h->a.Us, mine, P.m * (P.N - 1), 0, P.m * (P.N - 1), P.B));
    TRY(gather_blocks(h, dU_all, pu, kNcclDouble, sizeof(double)));
  }
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TO_OK;
}
// The small gather SURVEY.md §8e names next to the trajectories: iterations[B_total], status[B_total] (int32) and the
// objective cost J[B_total] of every rank's CURRENT trajectories, rank-major, into caller-owned HOST arrays (any may be
// NULL).  Staged through a device buffer of the library (a few bytes per trajectory), gathered over the same communicator.
int to_allgather_stats(to_handle* h, int32_t* iterations_all, int32_t* status_all, double* J_all) {
  CHECK_H(h); CHECK_IDLE(h);
  if (!h->comm) return fail(TO_ERR_ARGUMENT, "to_comm_init_rank first");
  if (!iterations_all && !status_all && !J_all) return fail(TO_ERR_NULL, "null pointer");
  TRY(use_device(h));
  const DevProblem& P = h->a.P;
  const size_t T = (size_t)h->comm_total, off = (size_t)h->comm_offset, B = (size_t)P.B;
  struct DevBuf { void* p = nullptr; ~DevBuf() { if (p) hipFree(p); } } buf;
  HIPCHECK(hipMalloc(&buf.p, T * sizeof(double)));
  auto gather_int = [&](const int* src, int32_t* host) -> int {
    if (!host) return TO_OK;
    int32_t* all = (int32_t*)buf.p;
    HIPCHECK(hipMemcpyAsync(all + off, src, B * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    TRY(gather_blocks(h, all, 1, kNcclInt32, sizeof(int32_t)));
    HIPCHECK(hipMemcpyAsync(host, all, T * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return TO_OK;
  };
  TRY(gather_int(h->a.iterations, iterations_all));
  TRY(gather_int(h->a.status, status_all));
  if (J_all) {
    double* all = (double*)buf.p;
    TRY(launch_cost(h, 0, h->d_tmp, nullptr));
    HIPCHECK(hipMemcpyAsync(all + off, h->d_tmp, B * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    TRY(gather_blocks(h, all, 1, kNcclDouble, sizeof(double)));
    HIPCHECK(hipMemcpyAsync(J_all, all, T * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  return TO_OK;
}

// ---- cones: stateless batched ops on `device` ------------------------------------------------------
static int cone_op(int device, int which, int32_t cone, int32_t dim, int64_t count, const double* x, const double* b, double* out, int32_t* status) {
  CHECK_P(x); CHECK_P(out);
  if (dim < 1 || dim > TO_MAX_P) return fail(TO_ERR_ARGUMENT, "cone dimension out of range");
  if (cone < TO_CONE_ZERO || cone > TO_CONE_IDENTITY) return fail(TO_ERR_ARGUMENT, "unknown cone");
  if (count <= 0) return TO_OK;
  HIPCHECK(hipSetDevice(device));
  const size_t nx = (size_t)dim * count, no = which == 0 ? nx : nx * dim;
  struct DevBuf {  // freed on every exit path
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
  } bx, bb, bo, bs;
  HIPCHECK(hipMalloc(&bx.p, nx * sizeof(double)));
  HIPCHECK(hipMalloc(&bo.p, no * sizeof(double)));
  HIPCHECK(hipMalloc(&bs.p, count * sizeof(int)));
  double *dx = (double*)bx.p, *dout = (double*)bo.p, *db = nullptr;
  int* dst = (int*)bs.p;
  HIPCHECK(hipMemcpy(dx, x, nx * sizeof(double), hipMemcpyHostToDevice));
  if (which == 2) { HIPCHECK(hipMalloc(&bb.p, nx * sizeof(double))); db = (double*)bb.p; HIPCHECK(hipMemcpy(db, b, nx * sizeof(double), hipMemcpyHostToDevice)); }
  const unsigned blocks = (unsigned)((count + 255) / 256);
  if (which == 0) enqueue(k_cone_projection, dim3(blocks), dim3(256), 0, 0, cone, dim, (long long)count, dx, dout, dst);
  else if (which == 1) enqueue(k_cone_jacobian, dim3(blocks), dim3(256), 0, 0, cone, dim, (long long)count, dx, dout, dst);
  else enqueue(k_cone_hessian, dim3(blocks), dim3(256), 0, 0, cone, dim, (long long)count, dx, db, dout, dst);
  TRY(launched());
  HIPCHECK(hipMemcpy(out, dout, no * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<int> st(count);
  HIPCHECK(hipMemcpy(st.data(), dst, count * sizeof(int), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < count; ++i) {
    if (st[i] < 0) return fail(TO_ERR_CONE, "Invalid second-order cone projection");
    if (status) status[i] = st[i];
  }
  return TO_OK;
}
int to_cone_projection(int device, int32_t cone, int32_t dim, int64_t count, const double* x, double* px, int32_t* status) {
  return cone_op(device, 0, cone, dim, count, x, nullptr, px, status);
}
int to_cone_projection_jacobian(int device, int32_t cone, int32_t dim, int64_t count, const double* x, double* jac) {
  return cone_op(device, 1, cone, dim, count, x, nullptr, jac, nullptr);
}
int to_cone_projection_hessian(int device, int32_t cone, int32_t dim, int64_t count, const double* x, const double* b, double* hess) {
  CHECK_P(b);
  return cone_op(device, 2, cone, dim, count, x, b, hess, nullptr);
}

}  // extern "C"
