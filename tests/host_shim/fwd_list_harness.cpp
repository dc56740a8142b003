// Compiles csrc/fwd_list.h for the host and checks the rank a scan wave computes for its trajectory (the passes of 64 flags, in chunks,
// exactly as k_scan.h walks them) against a plain loop, and the list that all the waves of a batch write together against the plain
// compaction (test infrastructure; tests/test_fwd_list_host.py).  A wave is simulated lane by lane: the ballot of a pass is built from the
// flags its lanes would load.
#include <hip/hip_runtime.h>
#include "fwd_list.h"
#include "path_plan.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
using namespace to;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

// what the scan wave of trajectory b does (k_scan.h): flags is the batch's `active` array, Bp ints — every load is checked to stay inside it
static int wave_rank(const std::vector<int>& flags, int Bp, int b, long long* loads) {
  const int np = fwd_list_passes(b);
  int rank = 0;
  for (int p0 = 0; p0 < np; p0 += FWD_LIST_CHUNK) {
    unsigned long long mask[FWD_LIST_CHUNK];
    for (int i = 0; i < FWD_LIST_CHUNK; ++i) {
      const int p = p0 + i < np ? p0 + i : np - 1;
      mask[i] = 0;
      for (int l = 0; l < 64; ++l) {
        const size_t idx = (size_t)p * 64 + l;
        CHECK(idx < (size_t)Bp, "load past the flags: b %d pass %d lane %d", b, p, l);
        if (idx < (size_t)Bp && flags[idx] != 0) mask[i] |= 1ull << l;
        ++*loads;
      }
    }
    for (int i = 0; i < FWD_LIST_CHUNK; ++i) rank += fwd_list_rank_add(mask[i], p0 + i, b);
  }
  return rank;
}

static void check_batch(const std::vector<int>& flags, int B, int Bp, const std::string& what, long long* ranks, long long* loads) {
  std::vector<int> want;  // the plain compaction
  for (int b = 0; b < B; ++b) if (flags[b]) want.push_back(b);
  for (int step = 0; step < 2; ++step) {
    std::vector<int> alist(2 * (size_t)Bp, -1);
    int below = 0;
    for (int b = 0; b < B; ++b) {
      if (flags[b]) {  // (an inactive wave leaves before it looks at the flags)
        const int rank = wave_rank(flags, Bp, b, loads);
        ++*ranks;
        CHECK(rank == below, "%s Bp %d b %d: rank %d, plain loop %d", what.c_str(), Bp, b, rank, below);
        const long long slot = fwd_list_slot(step, Bp, rank);
        CHECK(slot >= (long long)(step & 1) * Bp && slot < (long long)((step & 1) + 1) * Bp, "slot outside this step's list");
        if (slot >= 0 && slot < 2LL * Bp) { CHECK(alist[slot] == -1, "two trajectories in one slot"); alist[slot] = b; }
      }
      below += flags[b] ? 1 : 0;
    }
    for (size_t i = 0; i < want.size(); ++i) CHECK(alist[(size_t)(step & 1) * Bp + i] == want[i], "%s: list entry %zu", what.c_str(), i);
    for (int i = 0; i < Bp; ++i) CHECK(alist[(size_t)((step + 1) & 1) * Bp + i] == -1, "the other parity's list was written");
  }
  // the forward pass's grid covers the list for every count the host may hold (it only ever over-counts) and every wave shape
  for (int TW : {64, 32, 21, 16, 3, 1})
    for (int seen : {(int)want.size(), (int)want.size() + 1, B}) {
      const int g = fwd_list_groups(seen, TW);
      CHECK(g >= 1 && (long long)g * TW >= (long long)want.size() && (long long)(g - 1) * TW < (seen < 1 ? 1 : seen), "groups %d for %d seen, TW %d", g, seen, TW);
    }
}

int main() {
  long long ranks = 0, loads = 0, batches = 0;
  srand(12345);
  for (int Bp : {64, 128, 1024, 2048}) {
    CHECK(Bp <= FWD_LIST_MAX_BP, "Bp beyond the mode's range");
    std::vector<int> sizes = {Bp, Bp - 1, Bp - 63 > 0 ? Bp - 63 : 1};
    for (int B : {1, 17, 65, 200}) if (B <= Bp) sizes.push_back(B);  // ragged batches
    for (int B : sizes) {
      if (((B + 63) / 64) * 64 > Bp) continue;
      for (int pat = 0; pat < 7; ++pat) {
        std::vector<int> flags(Bp, 0);  // (the entries B .. Bp-1 are never set: k_solve_init)
        for (int b = 0; b < B; ++b) {
          switch (pat) {
            case 0: flags[b] = 1; break;                         // all active
            case 1: flags[b] = 0; break;                         // none
            case 2: flags[b] = (b == (B * 7) / 11) ? 1 : 0; break;  // one
            case 3: flags[b] = b & 1; break;                     // alternating
            case 4: flags[b] = (b & 1) ^ 1; break;
            case 5: flags[b] = (rand() % 3 == 0) ? 1 : 0; break;  // a random third
            default: flags[b] = (rand() % 3 != 0) ? 5 : 0; break; // two thirds, a flag value other than 1
          }
        }
        check_batch(flags, B, Bp, "pattern " + std::to_string(pat) + " B " + std::to_string(B), &ranks, &loads);
        ++batches;
      }
    }
  }
  // the pieces on their own
  CHECK(fwd_list_passes(0) == 0 && fwd_list_passes(1) == 1 && fwd_list_passes(64) == 1 && fwd_list_passes(65) == 2 && fwd_list_passes(2047) == 32, "passes");
  CHECK(fwd_list_rank_add(~0ull, 0, 64) == 64 && fwd_list_rank_add(~0ull, 0, 63) == 63 && fwd_list_rank_add(~0ull, 1, 64) == 0 &&
        fwd_list_rank_add(~0ull, 1, 65) == 1 && fwd_list_rank_add(~0ull, 3, 5) == 0 && fwd_list_rank_add(1ull << 63, 0, 64) == 1 &&
        fwd_list_rank_add(1ull << 63, 0, 63) == 0, "rank_add edges");
  CHECK(fwd_list_groups(0, 21) == 1 && fwd_list_groups(21, 21) == 1 && fwd_list_groups(22, 21) == 2 && fwd_list_groups(1024, 21) == 49, "groups");
  // when a solve runs in list mode (path_plan.h solve_forward_list): a small write-through model with the scan kernel and two-wave instances
  {
    PathTraits t;
    t.write_through = true; t.lane_backward = true; t.ls_first_round = 4;
    t.expand_backward = t.expand_backward_coop = t.expand_backward_scan = true;
    t.forward = t.forward2 = 0xffffu;
    PathShape s;
    s.B = 1024; s.Bp = 1024; s.N = 101; s.ne = 4; s.m = 1; s.diagonal_cost_blocks = true;
    const PathKnobs k0;
    const PathPlan p = plan_paths(t, s, k0);
    auto on = [&](const PathPlan& pl, int h_diag, int ev, int compact, int al, int B, int Bp, bool plants, bool gl, bool f2, bool en) {
      return solve_forward_list(pl, t, h_diag, ev, compact, al, B, Bp, plants, gl, f2, en, FWD_LIST_MAX_BP);
    };
    CHECK(p.scan && !p.compact && on(p, 1, 0, 0, 0, 1024, 1024, false, false, true, true), "the headline shape runs in list mode");
    CHECK(on(p, 1, 0, 0, 0, 1, 64, false, false, true, true) && on(p, 1, 0, 0, 0, 2048, 2048, false, false, true, true), "B = 1 and Bp = 2048");
    CHECK(!on(p, 1, 0, 0, 0, 1024, 1024, false, false, true, false), "the switch");
    CHECK(!on(p, 1, 0, 0, 1, 1024, 1024, false, false, true, true), "AL solves");
    CHECK(!on(p, 1, 0, 1, 0, 1024, 1024, false, false, true, true), "k_compact's list armed");
    CHECK(!on(p, 1, 0, 0, 0, 1024, 1024, true, false, true, true), "plants");
    CHECK(!on(p, 1, 0, 0, 0, 1024, 1024, false, true, true, true), "per-trajectory linear cost terms");
    CHECK(!on(p, 1, 0, 0, 0, 1024, 1024, false, false, false, true), "no two-wave instance");
    CHECK(!on(p, 0, 0, 0, 0, 1024, 1024, false, false, true, true) && !on(p, 1, 2, 0, 0, 1024, 1024, false, false, true, true) &&
          !on(p, 1, 4, 0, 0, 1024, 1024, false, false, true, true), "steps that do not plan the scan kernel");
    CHECK(!on(p, 1, 0, 0, 0, 2049, 2112, false, false, true, true), "Bp > 2048");
    PathKnobs k = k0;
    k.scan_max = 512;  // the first steps of a batch of 1024 would run the fused cooperative kernel: not every step is a scan step
    CHECK(!on(plan_paths(t, s, k), 1, 0, 0, 0, 1024, 1024, false, false, true, true) && on(plan_paths(t, s, k), 1, 0, 0, 0, 512, 512, false, false, true, true), "scan_max");
    k = k0; k.scan = 0;
    CHECK(!on(plan_paths(t, s, k), 1, 0, 0, 0, 1024, 1024, false, false, true, true), "TRAJOPT_SCAN=0");
    k = k0; k.fwd2 = 0;
    CHECK(!on(plan_paths(t, s, k), 1, 0, 0, 0, 1024, 1024, false, false, true, true), "TRAJOPT_FWD2=0");
    k = k0; k.fwd2 = 1;
    CHECK(on(plan_paths(t, s, k), 1, 0, 0, 0, 1024, 1024, false, false, true, true), "TRAJOPT_FWD2=1");
    // every step of such a solve then plans what the mode relies on, whatever count the host has seen
    for (int seen = 0; seen <= 1024; ++seen) {
      const StepPlan sp = plan_step(p, t, 1, 0, 0, seen, 1024, false);
      CHECK(sp.kind == STEP_SCAN && sp.two_wave && sp.store_x == 1 && !sp.two_launch, "step plan at %d active", seen);
    }
    PathTraits q = t;  // a model without write-through never runs in list mode
    q.write_through = false;
    CHECK(!solve_forward_list(plan_paths(q, s, k0), q, 1, 0, 0, 0, 1024, 1024, false, false, true, true, FWD_LIST_MAX_BP), "write-through");
  }
  printf("batches %lld ranks %lld loads %lld fails %d\n", batches, ranks, loads, fails);
  return fails ? 1 : 0;
}
