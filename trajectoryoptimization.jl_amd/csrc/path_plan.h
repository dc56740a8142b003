// path_plan.h — which kernels a handle's solves launch, decided in one place.  Plain host logic, no HIP types: to_create calls plan_paths
// once, the solve loop plan_step per batch step, to_solver_path path_report, launch_forward forward_mode; tests/test_path_plan_host.py
// compiles the same functions with g++ and checks them without a GPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace to {

// What the launch table of a model (handle.h ModelOps) tells the host: the trait flags, and which optional launchers exist.
struct PathTraits {
  bool write_through = false, mfma_backward = false, coop_backward = true, lane_backward = false;
  int ls_first_round = 16;
  bool expand_backward = false, expand_backward_coop = false, expand_backward_scan = false, accept_roll = false, expand_lane_k = false, expand_const = false;
  uint32_t forward = 0, forward2 = 0;  // bit i: forward[0][i] / forward2[i] is compiled
  uint32_t forward_plants = 0;         // bit i: forward[1][i], the variant that loads one plant per trajectory, is compiled
};
struct PathShape {
  int B = 1, Bp = 64, N = 2, ne = 1, m = 1, n_cons = 0, iterations_linesearch = 20;
  bool diagonal_cost_blocks = false;  // every knot's cost block diagonal at creation (trajopt_hip.hip diagonal_cost_blocks)
  int cus = 256;                      // compute units of the device
};
// The TRAJOPT_* knobs a handle's path depends on, read afresh by every to_create; a knob that is unset has the value given here.
struct PathKnobs {
  int ls_candidates = 0, ls_deep = 1, scan = 1, backward = 0, expand_lane = 1, fused_coop = 1, fused_lane = 1, accept_roll_min = -1, repack = 16384,
      expand_pack = 1, fwd2 = 2, coop_merge = 1, scan_max = 1 << 30, ls_repack = 1, ls_two_a = 2, ls_two_b = 2, compact = 1;
  double accept_roll_frac = 0.25, repack_at = 0.7;
};
inline PathKnobs read_path_knobs(const char* (*get)(const char*)) {  // THE list of these knobs, with the clamping each has
  PathKnobs k;
  auto num = [&](const char* name, int& o) { const char* s = get(name); if (s) o = std::atoi(s); return s != nullptr; };
  auto flag = [&](const char* name, int& o) { if (num(name, o)) o = o != 0; };
  if (num("TRAJOPT_LS_CANDIDATES", k.ls_candidates)) k.ls_candidates = std::max(1, std::min(16, k.ls_candidates));  // step sizes per round, 1..16 (0: the model's)
  num("TRAJOPT_LS_DEEP", k.ls_deep);                // 0: never switch to the deep forward-wave shape
  num("TRAJOPT_SCAN", k.scan);                      // 0: no scan backward pass (the lane path then takes over earlier); 2: the phase API runs it too
  if (const char* s = get("TRAJOPT_BACKWARD")) k.backward = !std::strcmp(s, "coop") ? 1 : !std::strcmp(s, "mfma") ? 2 : !std::strcmp(s, "lane") ? 3 : 0;  // where the model has it
  flag("TRAJOPT_EXPAND_LANE", k.expand_lane);      // 0: column-per-lane expansion kernel on the lane layout
  num("TRAJOPT_FUSED_COOP", k.fused_coop);          // 0: expansion and cooperative backward pass as two launches
  num("TRAJOPT_FUSED_LANE", k.fused_lane);          // 0: ... and lane backward pass
  num("TRAJOPT_ACCEPT_ROLL_MIN", k.accept_roll_min);  // active trajectories from which candidate controls only are stored (0: never, < 0: the model's default)
  if (const char* s = get("TRAJOPT_ACCEPT_ROLL_FRAC")) k.accept_roll_frac = std::atof(s);  // ... and the fraction of the batch that has to be active
  num("TRAJOPT_REPACK", k.repack);                  // repacked working set while it holds >= n trajectories (0: never)
  if (const char* s = get("TRAJOPT_REPACK_AT")) k.repack_at = std::min(0.95, std::max(0.05, std::atof(s)));  // ... once this fraction of it is left, 0.05..0.95
  flag("TRAJOPT_EXPAND_PACK", k.expand_pack);      // 0: the 4 x 16 tangent-matrix expansion instead of the packed one
  if (num("TRAJOPT_FWD2", k.fwd2)) if (k.fwd2 < 0 || k.fwd2 > 2) k.fwd2 = 2;  // two-wave forward pass: 0 never, 1 always, 2 per batch step
  flag("TRAJOPT_COOP_MERGE", k.coop_merge);
  num("TRAJOPT_SCAN_MAX", k.scan_max);              // scan backward pass up to this many active trajectories
  num("TRAJOPT_LS_REPACK", k.ls_repack);            // 0: no repacked last line-search round
  if (const char* s = get("TRAJOPT_LS_TWO")) { k.ls_two_a = std::atoi(s); const char* c2 = std::strchr(s, ','); k.ls_two_b = c2 ? std::atoi(c2 + 1) : 2; }  // a[,b]; a = 0: off
  num("TRAJOPT_COMPACT", k.compact);                // 0: no active-list compaction
  return k;
}

// Everything to_create decides about a handle's kernel path, and the candidate-buffer sizes that follow from it.
struct PathPlan {
  int bwd_mfma = 0, bwd_lane = 0;      // backward-pass flavour (neither: cooperative)
  int fused_coop = 0, fused_lane = 0;  // solve loop: one k_expand_backward_coop (cooperative path, diagonal cost blocks) / k_expand_backward_lane launch
  int scan = 0, scan_max_active = 0;   // solve loop: scan backward pass (k_scan.h) ahead of the fused cooperative kernel up to that many active trajectories
  int compact = 0;                     // solves run with active-list compaction (KArgs::compact, armed only inside a solve)
  int fwd2 = 2;                        // forward pass as two-wave workgroups (roller + accountant, k_forward2): 0 never, 1 always (phase API included), 2 per batch step
  int coop_merge = 1, expand_pack = 1, expand_lane = 1;  // KArgs::coop_merge; packed tangent-matrix expansion (k_expand.h PACK); expansion by k_expand_lane
  int cw_base = 1, tw_base = 64, cw_deep = 0, tw_deep = 0, deep_max_active = 0;  // forward-wave shape: base, and the deep one (0: none) used once the active trajectories fit
  int simds = 1024;                    // SIMDs of the device (4 per CU)
  int roll_min_active = -1;            // batch steps with at least this many active trajectories store candidate controls only and accept by k_accept_roll (< 0: the
  double roll_min_frac = 0.25;         // measured default per model, 0: never); small models: with at least this fraction of the batch active
  int rp_min = 16384;                  // repacked working set: once the active count has fallen to rp_at of the set, while it holds at least this many (0: never)
  double rp_at = 0.7;
  int ls2_cwa = 0, ls2_cwb = 2, ls2_blkA = 0, ls2_dump = 0;  // two-launch line search (common.h ls_phase): step sizes per round of launch A (0: off) / B; blocks of A; the dump block behind B's
  // candidate buffers in blocks of 64 lanes (forward-wave-major, common.h): `waves` forward waves in the widest launch, one spare block (dump_wave: the store target of
  // lanes that hold no candidate, k_forward.h), the repacked last line-search round from repack_block0 on (k_forward.h LsRound; 0: off); Xc holds x_blocks, Uc u_blocks
  long long waves = 0, x_blocks = 0, u_blocks = 0;
  int dump_wave = 0, repack_block0 = 0;
};
inline int coop_lanes(int ne, int m) { return (ne + m) <= 4 ? 4 : (ne + m) <= 8 ? 8 : 16; }  // lanes per trajectory of the column-layout kernels
inline long long wave_blocks(long long Bp, int TW) { return (Bp + TW - 1) / TW; }             // forward waves of TW trajectories each

inline PathPlan plan_paths(const PathTraits& t, const PathShape& s, const PathKnobs& k) {
  PathPlan p;
  const long long Bp = s.Bp;
  p.simds = 4 * s.cus;
  // Line-search candidates evaluated concurrently per trajectory, CW (a power of two): a forward wave holds CW candidates x 64/CW trajectories, so
  // the launch has Bp*CW/64 waves — enough to cover the 1024 SIMDs of the chip for small batches, at most the model's ls_first_round (4 for the small
  // models, 16 for the Quadrotor; the default search depth is 20: further in-kernel rounds cover the rest).
  int cw = std::max(1, std::min(t.ls_first_round, 1024 / (s.Bp / 64)));  // one forward wave per SIMD (measured: C5 0.71 M it/s with 8, 0.68 M with 16)
  // ... the models that search narrowly anyway (the small ones: 4 step sizes) keep their full first round at every batch size: a trajectory that
  // rejects everything offered costs its wave a second full pass, which is worse than the extra lanes — measured at B = 131 072 (fused lane path):
  // 25.4 / 29.6 / 37.4 M trajectory-iterations/s with 1 / 2 / 4 step sizes per round (forward pass 959 -> 582 us per batch step from 2 to 4), and
  // 18.7 -> 21.8 M at B = 32 768
  if (t.ls_first_round <= 4) cw = t.ls_first_round;
  if (k.ls_candidates) cw = k.ls_candidates;  // tuning knob
  int lg = 0; while ((2 << lg) <= cw) ++lg;
  p.cw_base = 1 << lg;
  // The small (write-through) models take any width: their lane map is the static one in every round (k_forward.h) and nothing in it needs a power of
  // two — lanes CW*TW .. 63 ride along without a candidate.  THREE step sizes x 21 trajectories per wave: the C2-shaped Cartpole solves accept within
  // the first three step sizes in 99.5 % of their line searches (alpha = 1 / 0.5 / 0.25: 18 / 40 / 42 %, measured on the oracle), so a wave serves 21
  // trajectories instead of 16 per pass for one extra pass in ~10 % of the waves.
  if (t.write_through && cw >= 1 && cw <= 16) p.cw_base = cw;
  p.tw_base = 64 / p.cw_base;
  // Deep shape: the WHOLE search depth in one round (20 step sizes x 3 trajectories per wave by default).  A trajectory that rejects the first CW
  // step sizes otherwise costs the batch a second full rollout pass (the Quadrotor solves do so in half of their steps: forward 1.0 ms instead of
  // 0.55 ms).  It needs 64/TW = 21 waves per 64 trajectories instead of 16, so the solve loop switches to it once the active trajectories fit the
  // chip that way (one wave per SIMD).
  // Only while a wave still holds >= 2 trajectories that way (total <= 32): with 33..64 step sizes a deep wave would carry ONE trajectory and the
  // candidate arrays 64x the nominal storage (several GB on C5) — those depths run as further rounds of the base shape instead.
  const int total = s.iterations_linesearch;
  if (!t.write_through && total > p.cw_base && total <= 32 && k.ls_deep) { p.cw_deep = total; p.tw_deep = 64 / total; p.deep_max_active = p.simds * p.tw_deep; }
  // backward-pass flavour: one wave per trajectory on the matrix cores (tangent-matrix expansion) where the model has it, else the cooperative LDS
  // kernel on the column layout.  TRAJOPT_BACKWARD=coop|mfma|lane overrides (A/B measurements).  Models that have the cooperative kernel as well
  // (small ones: several trajectories per wave) default to it: measured on the Cartpole at B = 1024, 78 us cooperative vs 90 us MFMA per backward
  // pass (the 5x5 blocks fill 2 % of a 16x16 tile).
  p.bwd_mfma = (t.mfma_backward && !t.coop_backward) ? 1 : 0;
  // Small models: the cooperative kernel (R lanes per trajectory, LDS exchanges) has the shorter critical path — 78 vs 111 us per pass on the
  // Cartpole at B = 1024, a single lane issues every FMA of a knot itself — and the lane kernel the fewer instructions: it takes over once the
  // cooperative waves would stack three deep on every SIMD (measured at B = 32 768: 12.0 vs 9.8 M trajectory-iterations/s).
  {
    const int G = 64 / coop_lanes(s.ne, s.m);
    const long coop_waves = ((long)s.B + G - 1) / G;
    // (with the expansions fused into both kernels the crossover sits at ~12 000 Cartpole trajectories: measured fused lane vs fused cooperative 10.8
    // vs 9.9 M it/s at B = 12 288, 7.9 vs 9.3 M at B = 8 192)
    // (and where the scan kernel runs ahead of the cooperative one — unconstrained problems with diagonal cost blocks — at ~20 000: scan +
    // cooperative vs fused lane 15.2 vs 11.2 M it/s at B = 12 288, 17.1 vs 14.4 at 16 384, 19.4 vs 20.4 at 24 576)
    const bool scan_path = t.expand_backward_scan && s.n_cons == 0 && s.N <= 126 && s.diagonal_cost_blocks && k.scan;
    const long lane_from = scan_path ? 10L : (t.expand_backward ? 6L : 12L);
    p.bwd_lane = (t.lane_backward && coop_waves >= lane_from * s.cus) ? 1 : 0;
  }
  if (k.backward == 1 && t.coop_backward) { p.bwd_mfma = 0; p.bwd_lane = 0; }
  if (k.backward == 2 && t.mfma_backward) { p.bwd_mfma = 1; p.bwd_lane = 0; }
  if (k.backward == 3 && t.lane_backward) { p.bwd_mfma = 0; p.bwd_lane = 1; }
  p.fused_coop = (!p.bwd_lane && !p.bwd_mfma && t.expand_backward_coop && k.fused_coop) ? 1 : 0;  // used while the cost blocks are diagonal (KArgs::h_diag)
  p.expand_lane = k.expand_lane; p.expand_pack = k.expand_pack; p.fwd2 = k.fwd2; p.coop_merge = k.coop_merge; p.scan_max_active = k.scan_max;
  p.roll_min_active = k.accept_roll_min; p.roll_min_frac = k.accept_roll_frac; p.rp_min = k.repack; p.rp_at = k.repack_at;
  // scan (parallel-in-time) backward pass ahead of the fused cooperative kernel, over the whole range of batches the cooperative path serves
  // (measured, Cartpole: 40.7 vs 95.2 us per step at B = 1024, 76 vs 103 at 4096, 119 vs 164 at 8192)
  p.scan = (p.fused_coop && t.expand_backward_scan && s.N <= 126 && k.scan) ? (k.scan == 2 ? 2 : 1) : 0;
  p.fused_lane = (p.bwd_lane && t.expand_backward && k.fused_lane) ? 1 : 0;
  // active-list compaction: the fused lane path (large batches of the small models) and the MFMA path (Quadrotor: its expansion waves hold four
  // trajectories each and the solves end with long straggler tails — 141 batch steps for a mean of 52 iterations on C3); the cooperative small-batch
  // path is latency-bound and keeps its fixed mapping
  p.compact = ((p.fused_lane || p.bwd_mfma) && k.compact) ? 1 : 0;
  // candidates, forward-wave-major (common.h): 64 lanes per wave in either shape
  p.waves = wave_blocks(Bp, p.tw_base);
  if (p.cw_deep) p.waves = std::max(p.waves, wave_blocks(Bp, p.tw_deep));
  p.dump_wave = (int)p.waves;
  // ... and, for the models whose search goes through several rounds of the base shape, a second block per wave for the repacked last round (as many
  // as either wave shape launches: a search deeper than the deep shape — options changed after creation — repacks there too)
  long long extra = 0;
  if (!t.write_through && k.ls_repack) { extra = p.waves; p.repack_block0 = (int)p.waves + 1; }
  p.x_blocks = p.u_blocks = p.waves + 1 + extra;
  // two-launch line search (small models, dense large batches: the steps that store candidate controls only): launch A's blocks, launch B's behind
  // them, one dump block — control candidates only, so only Uc grows
  if (t.write_through && t.accept_roll && Bp >= 32768) {
    // measured default (r05, Cartpole at B = 1 048 576: 74.1 M it/s with 2 + 2, 71.5 with 1 + 2, 70.9 with one launch)
    const int ca = k.ls_two_a, cb = k.ls_two_b;
    if (ca >= 1 && ca <= 16 && cb >= 1 && cb <= 16 && ca < s.iterations_linesearch) {
      const long long nA = wave_blocks(Bp, 64 / ca), nB = wave_blocks(Bp, 64 / cb);
      p.ls2_cwa = ca; p.ls2_cwb = cb; p.ls2_blkA = (int)nA; p.ls2_dump = (int)(nA + nB);
      p.u_blocks = std::max(p.u_blocks, nA + nB + 1);
    }
  }
  return p;
}
// `plants` (the trailing argument of the predicates below): the handle carries one set of model parameters per trajectory
// (DevProblem::pm, to_set_model_params_batch).  Only the general kernel variants have instances that read them, so such a handle is routed
// the way one with per-trajectory constraint parameters is — its expand_variant has bit 2 forced, which already rules out the scan and the
// fused cooperative kernel — and, beyond that, never takes the fused lane kernel, the two-wave forward pass, the control-only candidate
// stores with their re-roll (k_accept_roll), the two-launch line search or the repacked working set.
// the fused cooperative kernel serves the diagonal cost blocks of the expansion variants 0 / 2; the scan kernel variant 0 only
inline bool fused_coop_now(const PathPlan& p, int h_diag, int expand_variant, bool plants = false) {
  return !plants && p.fused_coop && h_diag && (expand_variant == 0 || expand_variant == 2);
}
inline bool scan_now(const PathPlan& p, int h_diag, int expand_variant, bool plants = false) {
  return p.scan && fused_coop_now(p, h_diag, expand_variant, plants) && expand_variant == 0;
}
// active-list compaction of a solve: the plan's, except on the lane layout with `plants` — there compaction belongs to the fused lane kernel
// (the separate lane kernels address the batch by position, as they do with TRAJOPT_FUSED_LANE=0)
inline int solve_compact(const PathPlan& p, bool plants = false) { return (plants && !p.bwd_mfma) ? 0 : p.compact; }
inline int roll_min(const PathPlan& p, const PathTraits& t) { return p.roll_min_active >= 0 ? p.roll_min_active : t.write_through ? 32768 : 2048; }
// repacked working set (trajopt_hip.hip rp_move): iLQR solves of the small models on the fused lane path with compaction
inline bool working_set_repack(const PathPlan& p, const PathTraits& t, bool plants = false) {
  return !plants && p.fused_lane && p.compact && t.write_through && p.rp_min > 0;
}
enum StepKind { STEP_SPLIT, STEP_FUSED_LANE, STEP_FUSED_COOP, STEP_SCAN };  // expansion + backward pass of one batch step
struct StepPlan { StepKind kind; int CW, TW; bool two_wave; int store_x; bool two_launch; };  // + forward-wave shape, two-wave workgroups, KArgs::store_x, two-launch search
// What one batch step launches, from the last active count the host has seen (results do not depend on it) and the batch B it works on.
inline StepPlan plan_step(const PathPlan& p, const PathTraits& t, int h_diag, int expand_variant, int compact_armed, int last_active, int B,
                          bool plants = false) {
  StepPlan s;
  s.kind = (p.fused_lane && !plants) ? STEP_FUSED_LANE          // expansion in the registers of the lane that runs the recursion
           : scan_now(p, h_diag, expand_variant, plants) && last_active <= p.scan_max_active ? STEP_SCAN  // the recursion as a scan over the horizon (k_scan.h)
           : fused_coop_now(p, h_diag, expand_variant, plants) ? STEP_FUSED_COOP  // expansion by a second wave of the workgroup, through an LDS ring
           : STEP_SPLIT;
  const bool deep = p.cw_deep && last_active <= p.deep_max_active;
  s.CW = deep ? p.cw_deep : p.cw_base; s.TW = deep ? p.tw_deep : p.tw_base;
  // workgroup shape: two waves per candidate group (roller + accountant, k_forward2) shorten the rollout's latency chain by a third, but need twice
  // the wave slots — taken once both waves of every workgroup get a SIMD of their own
  // (C3: 610 vs 812 us per step with the chip full, 480 vs 320 us once the batch has drained)
  s.two_wave = !plants && p.fwd2 == 2 && 2 * wave_blocks(last_active, s.TW) <= (long long)p.simds;
  // ... and what it stores per candidate: with the chip full the pass is bound by its stores, 3/4 of them candidate states that are read once (the
  // accepted one) or never — from roll_min active trajectories on only the controls go out and the accepted candidates are rolled out again
  // (k_accept_roll: bit-identical states, one more latency chain of N-1 steps)
  // (measured, always vs never, whole solve: C5 +0.9 / +4.6 / +7.7 / +7.3 % at B = 2048 / 4096 / 8192 / 16384, C3 -3 / -1 / +1.9 / +4.4 %: the copy
  // by k_accept grows with the accepted trajectories — 93 us at 4096, 227 us at 8192 — the second rollout does not, and an AL line search goes
  // through more rounds, each of which stores its candidates, than an unconstrained one)
  // Small models (write-through; 4 step sizes x 16 trajectories per wave): at the large-batch plateau the forward pass wrote 19 KB per active
  // trajectory for 4 KB of result and the next expansion gathered the accepted candidate through 4x-amplified sectors; with the controls only and the
  // re-roll both kernels stream the nominal (TRAJOPT_ACCEPT_ROLL_MIN overrides every default)
  // (round 6: 2048 for iLQR solves too — alone, C3 at B = 4096 runs 1.12 M it/s with either threshold, and next to other solves on the device
  // (pipelined handles) the candidate-state stores and k_accept's copy cost the others bandwidth: 1.57 -> 1.70 M it/s over three handles; the forward
  // phase's counter traffic drops with it)
  const int rmin = roll_min(p, t);
  // ... and, for those models, only while the batch is still DENSE: the active list is in index order, so once half of the batch has converged a
  // wave's 64 trajectories sit in several tiles and every store of the re-roll becomes scattered 8-byte writes (r05 trace, Cartpole at B = 1 048 576:
  // the re-roll takes 0.9 ms with every trajectory active and 1.8 ms with a quarter of them); the write-through of the next expansion makes the same
  // scattered stores, but behind 2 000 instructions per knot
  const bool dense = !t.write_through || (double)last_active >= p.roll_min_frac * (double)B;
  s.store_x = (!plants && rmin > 0 && t.accept_roll && !s.two_wave && last_active >= rmin && dense) ? 0 : 1;
  // two-launch line search (common.h ls_phase): launch A — one round for everybody; flags -> list; launch B — the rest of the search for the flagged
  // trajectories only; then the accept.  Same candidates, same first accepted step size: bit-identical.
  s.two_launch = !s.store_x && p.ls2_cwa && compact_armed && p.fwd2 != 1;
  return s;
}
// List mode of a solve (fwd_list.h): the scan kernel of every batch step lists the active trajectories and the two-wave forward pass takes
// its trajectories from that list — workgroups only for trajectories still active, no k_compact launch.  A finished trajectory's accepted
// candidate is copied onto the nominal by its own, otherwise idle, wave of the NEXT scan launch, before the forward pass hands the block to
// other trajectories; a step without the list leaves it in its slot until the final accept, where a later step with the list would overwrite
// it.  So the mode is decided once per solve: on only when EVERY step plans the scan kernel and the two-wave forward pass whatever active
// count the host has seen (last_active <= B), on an iLQR solve without the k_compact list.
//   forward2_compiled: the forward variant of this solve has a two-wave instance (launch_forward falls back to k_forward otherwise);
//   linear_terms: DevProblem::gl is set (cp / cl / plants rule the scan out through expand_variant); enabled: the TRAJOPT_FWD_LIST switch;
//   cost_weights: DevProblem::gw is set (its expand_variant has bit 2 forced as well; stated here so that the mode does not hang on that alone).
inline bool solve_forward_list(const PathPlan& p, const PathTraits& t, int h_diag, int expand_variant, int compact_armed, int al_mode, int B, int Bp,
                               bool plants, bool linear_terms, bool forward2_compiled, bool enabled, int max_bp, bool cost_weights = false) {
  if (!enabled || al_mode || compact_armed || plants || linear_terms || cost_weights || !forward2_compiled || !t.write_through || Bp > max_bp) return false;
  const StepPlan full = plan_step(p, t, h_diag, expand_variant, compact_armed, B, B, plants);  // the plan is monotone in last_active: the full batch is its worst case
  if (full.kind != STEP_SCAN || !full.store_x || full.two_launch) return false;
  return full.two_wave || p.fwd2 == 1;
}
// to_solver_path: what a handle's solves run, from the predicates plan_step uses
inline void path_report(const PathPlan& p, const PathTraits& t, int h_diag, int expand_variant, int B, int32_t info[8], bool plants = false) {
  info[0] = p.bwd_mfma ? 1 : p.bwd_lane ? 2 : 0;
  info[1] = ((p.fused_lane && !plants) || fused_coop_now(p, h_diag, expand_variant, plants)) ? 1 : 0;
  info[2] = solve_compact(p, plants);
  info[3] = p.cw_base;
  info[4] = (!plants && p.fwd2 && t.forward2) ? 2 : 1;  // (two-wave workgroups are used while the active trajectories leave room for them)
  info[5] = scan_now(p, h_diag, expand_variant, plants) ? 1 : 0;
  info[6] = (!plants && t.accept_roll && p.roll_min_active != 0) ? 1 : 0;  // full-chip batch steps store candidate controls only (k_accept_roll)
  info[7] = p.repack_block0 != 0 ? 1 : 0;                        // repacked last line-search round
  if (working_set_repack(p, t, plants) && B >= p.rp_min) info[7] |= 2;   // repacked working set (iLQR solves)
}
// What the cost and constraint tables of a handle say about the kernel variants it needs (trajopt_hip.hip upload_tables fills it whenever a cost, a
// constraint or a per-trajectory array changes): DevProblem::expand_variant — bit0: a QuadraticCost / ErrorQuadratic exists; bit1: constraints exist;
// bit2: the general variant — and whether the forward pass takes a general variant (forward_mode's `general`).  Per-trajectory constraint LIMITS
// (con_limits: some constraint reads DevProblem::cl, to_set_constraint_limits_batch) route a handle exactly as per-trajectory constraint
// PARAMETERS (con_params: DevProblem::cp) do: bit 2 forced — expansion variant 7, forward `mode | 8` — which rules out the scan kernel, the fused
// cooperative kernel and the packed Quadrotor expansion; compaction, the fused lane kernel and the repacked working set stay as the plan has them
// (the repacked set carries cl the way it carries cp, trajopt_hip.hip rp_setup).
// Per-trajectory TIME STEPS (time_steps: DevProblem::dtb set, to_set_time_steps_batch) ride on the flagged instances that load one plant per
// trajectory — only they read the step per trajectory — so such a handle IS a `plants` handle to every predicate above (routed_as_plants),
// whether or not the caller also gave each trajectory its own plant.
// Per-trajectory COST WEIGHTS (cost_weights: DevProblem::gw set, to_set_cost_weights_batch) route a handle exactly as con_limits does — bit 2
// forced, forward `mode | 8` — and, beyond that, keep the forward pass off the variants that preload ONE stage cost for the whole wave
// (forward_simple): a trajectory's weights are its own.
struct TableFlags {
  bool dense_costs = false, cons = false, non_selector = false;  // from the descriptors
  bool con_params = false, con_limits = false, plants = false;   // a constraint flagged for cp / for cl; DevProblem::pm set
  bool time_steps = false;                                       // DevProblem::dtb set
  bool cost_weights = false;                                     // DevProblem::gw set
};
// How ga rides on gw.  Three reasons keep the pair of arrays set: the CALLER set weights (to_set_cost_weights_batch), the caller
// set attitudes (to_set_cost_attitude_batch), attitude tracking is on (to_set_tracking_attitude).  While any holds, DevProblem::gw AND ga are
// set — gw on the descriptors' diagonals unless the caller gave weights, ga on the descriptors' q_ref unless attitudes were given — and the
// handle is routed as one with weights; when the last one goes, both pointers return to null and the handle to the kernel variants it ran before.
// The tracking / weights refusals look at `weights` alone: attitude references with gw on the descriptors refuse neither.
struct CostLaneState {
  bool weights = false, attitude = false, track_attitude = false;
  bool routed() const { return weights || attitude || track_attitude; }  // DevProblem::gw / ga are set
};
// what a transition asks of the device arrays
struct CostLaneAction {
  bool fill_gw = false;   // gw (host copy and device) starts from every cost's descriptor
  bool fill_ga = false;   // ga likewise
  bool release = false;   // both pointers back to null
};
enum CostLaneEvent { LANE_SET_WEIGHTS, LANE_CLEAR_WEIGHTS, LANE_SET_ATTITUDE, LANE_CLEAR_ATTITUDE, LANE_TRACK_ON, LANE_TRACK_OFF };
inline CostLaneAction cost_lane_step(CostLaneState* s, CostLaneEvent e) {
  CostLaneAction a;
  const bool was = s->routed();
  switch (e) {
    case LANE_SET_WEIGHTS: s->weights = true; break;
    case LANE_SET_ATTITUDE: s->attitude = true; break;
    case LANE_TRACK_ON: s->track_attitude = true; break;
    case LANE_CLEAR_WEIGHTS: a.fill_gw = s->weights; s->weights = false; break;          // (what stays routed runs on the descriptors' diagonals)
    case LANE_CLEAR_ATTITUDE: a.fill_ga = s->attitude || s->track_attitude; s->attitude = false; break;  // every cost's q_ref; a tracking lowering follows while that mode is on
    case LANE_TRACK_OFF: s->track_attitude = false; break;                              // (the caller restarts the tracked costs' rows)
  }
  if (!was && s->routed()) a.fill_gw = a.fill_ga = true;   // first use: both arrays from the descriptors
  if (was && !s->routed()) { a = CostLaneAction{}; a.release = true; }
  return a;
}
inline bool routed_as_plants(bool plants /* pm */, bool time_steps /* dtb */) { return plants || time_steps; }
inline bool routed_as_plants(const TableFlags& f) { return routed_as_plants(f.plants, f.time_steps); }
inline int expand_variant_of(const TableFlags& f) {
  return (f.dense_costs ? 1 : 0) | (f.cons ? 2 : 0) | ((f.non_selector || f.con_params || f.con_limits || f.cost_weights || routed_as_plants(f)) ? 4 : 0);
}
inline bool forward_general(int expand_variant, bool cost_terms /* gl */, bool con_params /* cp */, bool con_limits /* cl */, bool cost_weights /* gw */ = false) {
  return (expand_variant & 5) != 0 || cost_terms || con_params || con_limits || cost_weights;
}
// forward_mode's `simple_stage`: DevProblem::simple_stage, except with per-trajectory cost weights (no preloaded shared stage cost)
inline bool forward_simple(bool simple_stage, bool cost_weights /* gw */ = false) { return simple_stage && !cost_weights; }
// Forward-pass kernel variant (k_forward.h MODE bits): bit0 simple stage cost, bit1 constraints, bit2 compile-time RK4 (models that
// pin it), bit3 dense costs / generic constraints / per-trajectory terms, bit4 unit-SOC; `mask` holds the compiled ones.  -1: none fits.
inline int forward_mode(bool simple_stage, bool has_cons, bool rk4, bool general, bool unit_soc, uint32_t mask) {
  auto has = [&](int mode) { return (mask >> mode) & 1u; };
  int mode = (simple_stage ? 1 : 0) | (has_cons ? 2 : 0) | (rk4 ? 4 : 0) | (general ? 8 : 0);
  if (!has(mode)) mode &= ~4;  // the model does not pin RK4
  if (unit_soc && has(mode | 16)) mode |= 16;
  if (!has(mode)) mode = (mode | 8) & ~1 & ~16;  // the general variant (any cost kind, stage cost read per knot): a superset
  return has(mode) ? mode : -1;
}
// ---- closed-loop policy rollouts and the receding-horizon step (k_policy.h, k_mpc.h): every size their entry points give a buffer --------
// One routine for to_policy_rollout, to_policy_rollout_mc and to_mpc_advance (trajopt_hip.hip policy_prepare / policy_staging) and for the
// launcher (ops.h op_policy_rollout: the LDS bytes); tests/host_shim/policy_harness.cpp allocates every array of the host build of the kernels
// with exactly these lengths, so a length that is too short here is a heap overflow there.  Lengths are in elements, not bytes.
// LDS of one policy wave: two gains buffers of whole DMA instructions (k_forward.h gains_lds_doubles; pieces = 16-byte pieces of one gains
// row, 0 for the models whose gains travel in registers), TW rows each.
inline size_t policy_lds_bytes(int gains_pieces, int TW) {
  return gains_pieces ? sizeof(double) * 2 * (size_t)(((TW * gains_pieces + 63) / 64) * 64 * 2) : 0;
}
struct PolicyPlan {
  bool packed = true;         // lane map: packed (a wave = TPW trajectories x S samples) or uniform (a wave = 64 samples of one trajectory)
  int TPW = 0, WPT = 1;       // PolicyArgs::TPW (0: uniform), WPT
  long long waves = 0;        // waves over the whole batch
  size_t SB = 0;              // samples
  size_t x0s_len = 0;         // pol_x0s: [n, S, B]
  size_t sample_len = 0;      // pol_J, pol_cmax, pol_dxmax, pol_status, pol_klim: one entry per sample
  size_t plants_len = 0;      // pol_plants: [16, S*B]
  size_t Lx = 0, Lu = 0;      // elements of one trajectory's states / controls
  long long chunk = 0;        // waves of one staging chunk
  size_t xw_len = 0, uw_len = 0;  // the staging pair of one chunk: [chunk][Lx][64], [chunk][Lu][64]
  size_t rollout_stage_len = 0;   // to_policy_rollout with trajectories: host-layout staging of one chunk (h->stage)
  size_t lds_bytes = 0;       // dynamic LDS of one wave
};
// map_env / chunk_env: TRAJOPT_POLICY_MAP (null where the caller forces the packed map: to_mpc_advance) and TRAJOPT_POLICY_CHUNK_WAVES as the
// environment has them (null: unset)
inline PolicyPlan plan_policy(int n, int m, int N, int B, int S, const char* map_env, const char* chunk_env, int gains_pieces) {
  PolicyPlan p;
  // lane map: packed while a wave holds at least two trajectories, one trajectory per wave beyond (TRAJOPT_POLICY_MAP=packed forces the
  // per-lane body up to S = 64: the A/B of tools/policy_rollout_probe.py)
  p.packed = S <= 32;
  if (map_env) {
    if (!std::strcmp(map_env, "packed") && S <= 64) p.packed = true;
    if (!std::strcmp(map_env, "uniform")) p.packed = false;
  }
  p.TPW = p.packed ? 64 / S : 0; p.WPT = (S + 63) / 64;
  p.waves = p.packed ? ((long long)B + p.TPW - 1) / p.TPW : (long long)B * p.WPT;
  p.SB = (size_t)S * B;
  p.x0s_len = p.SB * n; p.sample_len = p.SB; p.plants_len = p.SB * 16;
  p.Lx = (size_t)N * n; p.Lu = (size_t)(N - 1) * m;
  // The closed-loop trajectories go through a bounded staging pair, a chunk of waves at a time (sample-fastest blocks [wave - g0][e][64]):
  // 32 MiB, whatever S * B * N is.  TRAJOPT_POLICY_CHUNK_WAVES overrides the chunk (tests of the chunked path).
  p.chunk = std::max<long long>(1, (32ll << 20) / (long long)(64 * (p.Lx + p.Lu) * sizeof(double)));
  if (chunk_env) p.chunk = std::max(1, std::atoi(chunk_env));
  p.chunk = std::min<long long>(p.chunk, p.waves);
  p.xw_len = (size_t)p.chunk * p.Lx * 64; p.uw_len = (size_t)p.chunk * p.Lu * 64;
  p.rollout_stage_len = (size_t)p.chunk * 64 * (p.Lx + p.Lu);
  p.lds_bytes = policy_lds_bytes(gains_pieces, p.packed ? p.TPW : 1);
  return p;
}
// sample index of lane 0 of wave g (the waves enumerate the samples in order): what a chunk of waves [g0, g0 + ng) hands to the caller
inline long long policy_first_sample(const PolicyPlan& p, int S, long long g) {
  if (g >= p.waves) return (long long)p.SB;
  if (p.packed) return std::min<long long>((long long)p.SB, g * p.TPW * (long long)S);
  const long long b = g / p.WPT, w = g - b * p.WPT;
  return b * S + w * 64;
}
// to_mpc_advance: the host-layout gather of one call, [x_next n B][X_applied n (s+1) B][U_applied m s B] in h->stage, and the row groups
// (grid.y) of k_mpc_writeback
struct MpcPlan {
  size_t cx = 0, cX = 0, cU = 0;  // lengths, and with them the offsets 0, cx, cx + cX
  size_t stage_len = 0;
  int row_groups = 1;
};
inline MpcPlan plan_mpc(int n, int m, int N, int B, int s) {
  MpcPlan p;
  p.cx = (size_t)n * B; p.cX = (size_t)n * (s + 1) * B; p.cU = (size_t)m * s * B;
  p.stage_len = p.cx + p.cX + p.cU;
  p.row_groups = std::min(std::max((N - 1) * m, (s + 1) * n), 32);
  return p;
}

// Stream compaction of Bp flags (k_generic.h): one workgroup up to COMPACT_ONE_LAUNCH, else count + write launches of nb <= 256
// workgroups, each owning `per` flags (a multiple of 1024, at most 64 slices of 1024).  false: the batch is too large (> 16 777 216).
constexpr int COMPACT_ONE_LAUNCH = 16384;
inline bool compact_grid(int Bp, int* per, int* nb) {
  *per = std::min(65536, ((Bp + 255) / 256 + 1023) / 1024 * 1024);
  *nb = (Bp + *per - 1) / *per;
  return *nb <= 256;
}

}  // namespace to
