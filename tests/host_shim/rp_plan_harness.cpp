// Compiles csrc/rp_plan.h for the host and replays the allocation logic of rp_move (csrc/trajopt_hip.hip) over every sequence of one,
// two and three differently configured solves on ONE handle (test infrastructure; tests/test_rp_plan_host.py).  The harness keeps a
// ledger of its own — bytes actually allocated per buffer, computed without rp_plan.h's helpers — and requires for every move that each
// carried array and the map fit what they are given, and that a buffer is never re-used for an array of another kind or row length.
#include "rp_plan.h"

#include <cstdio>
#include <vector>
using namespace to;

static long long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

// (n, m, N, n_costs, n_duals, n_cons) of real problems; n_cp = (n + m) * n_cons (to_set_constraint_params_batch)
struct Dims { const char* name; int n, m, N, n_costs, n_duals, n_cons; };
static const Dims DIMS[] = {
    {"cartpole N=41 bound+goal", 4, 1, 41, 2, 2 * 40 + 4, 2},        // configs.cartpole_problem(N=41, constrained=True)
    {"cartpole N=101 bound+goal", 4, 1, 101, 2, 2 * 100 + 4, 2},     // C2 with the notebook's constraints
    {"double integrator linear+goal", 4, 2, 31, 2, 2 * 30 + 4, 2},   // test_goal_batch.linear_problem
    {"hybrid double integrator", 4, 2, 11, 11, 4 * 5 + 3 * 4 + 2, 3},  // test_hybrid_dims.hybrid_problem(constrained=True): a cost per knot
    {"rows of gl == rows of lam", 4, 1, 3, 2, 10, 1},                // same row length, another kind: still another array
};

// the table of one solve, as rp_setup builds it: [Xs, Us, x0, (gl), (lam, mu), (cp), 6 scalars, 11 ints]
static std::vector<RpSlot> table(const Dims& d, bool gl, bool cons, bool cp) {
  std::vector<RpSlot> t;
  t.push_back({0, d.N * d.n}); t.push_back({0, (d.N - 1) * d.m}); t.push_back({0, d.n});
  if (gl) t.push_back({0, d.n_costs * (d.n + d.m)});
  if (cons) { t.push_back({3, d.n_duals}); t.push_back({3, d.n_cons}); }
  if (cp) t.push_back({3, (d.n + d.m) * d.n_cons});
  for (int i = 0; i < 6; ++i) t.push_back({1, 1});
  for (int i = 0; i < 11; ++i) t.push_back({2, 1});
  return t;
}

// the ledger's own arithmetic
static size_t own_bytes(const RpSlot& s, long long Bp) {
  switch (s.kind) {
    case 0: case 3: return (size_t)(8ll * s.L * Bp);
    case 1: return (size_t)(8ll * Bp);
    default: return (size_t)(4ll * Bp);
  }
}

struct Buf { size_t bytes; int kind, L; };
struct Set { RpSized sized; std::vector<Buf> buf; size_t map_bytes = 0; };

static long long n_reuse = 0, n_realloc = 0, n_moves = 0;

// one move into working set w: the branch structure of rp_move
static void move(Set& s, const std::vector<RpSlot>& need, int count, const char* what) {
  const int Bp_new = (count + 63) / 64 * 64;
  ++n_moves;
  if (!rp_reusable(s.sized, need, Bp_new)) {
    ++n_realloc;
    s.buf.clear();
    for (const RpSlot& r : need) s.buf.push_back({rp_slot_bytes(r, Bp_new + 64), r.kind, r.L});   // what rp_move passes to g_malloc
    s.map_bytes = rp_map_bytes(Bp_new);
    s.sized.slots = need; s.sized.cap = Bp_new;
  } else {
    ++n_reuse;
    CHECK(s.buf.size() == need.size(), "%s: re-use with %zu buffers for %zu arrays", what, s.buf.size(), need.size());
    for (size_t i = 0; i < need.size() && i < s.buf.size(); ++i)
      CHECK(s.buf[i].kind == need[i].kind && s.buf[i].L == need[i].L, "%s: buffer %zu sized for (kind %d, L %d) re-used for (kind %d, L %d)", what, i,
            s.buf[i].kind, s.buf[i].L, need[i].kind, need[i].L);
  }
  // the memsets and k_repack_move write Bp_new trajectories of every array, k_accept_roll one spare tile behind them; the map Bp_new ints
  CHECK(s.buf.size() >= need.size(), "%s: %zu buffers for %zu arrays", what, s.buf.size(), need.size());
  for (size_t i = 0; i < need.size() && i < s.buf.size(); ++i) {
    const size_t want = own_bytes(need[i], (long long)Bp_new + 64);
    CHECK(want <= s.buf[i].bytes, "%s: array %zu (kind %d, L %d) needs %zu bytes at Bp %d, its buffer has %zu", what, i, need[i].kind, need[i].L, want, Bp_new, s.buf[i].bytes);
  }
  CHECK(4ull * (size_t)Bp_new <= s.map_bytes, "%s: map needs %zu bytes, has %zu", what, 4 * (size_t)Bp_new, s.map_bytes);
}

// one solve: moves at first, first/2, first/4 ... while the set holds at least rp_min trajectories, into working sets 0, 1, 0, ...
static void solve(Set* sets, const std::vector<RpSlot>& need, int first, int rp_min, const char* what) {
  int lvl = 0;
  for (int count = first; count >= 1; count = count * 2 / 5, ++lvl) {
    move(sets[lvl & 1], need, count, what);
    if (count < rp_min) break;
  }
}

int main() {
  const int firsts[] = {1500, 2049, 12000, 12001, 27000, 49000};   // first-move sizes: shrink, stay and grow between the solves of a sequence
  const int nf = sizeof(firsts) / sizeof(firsts[0]);
  long long seqs = 0;
  char what[256];
  for (const Dims& d : DIMS) {
    std::vector<std::vector<RpSlot>> tabs;
    std::vector<int> tag;
    for (int gl = 0; gl < 2; ++gl)
      for (int cons = 0; cons < 2; ++cons)
        for (int cp = 0; cp <= cons; ++cp) { tabs.push_back(table(d, gl, cons, cp)); tag.push_back(gl * 100 + cons * 10 + cp); }
    const int nt = (int)tabs.size();
    for (int len = 1; len <= 3; ++len) {
      int idx[3] = {0, 0, 0};
      const int total_t = len == 1 ? nt : len == 2 ? nt * nt : nt * nt * nt;
      const int total_f = len == 1 ? nf : len == 2 ? nf * nf : nf * nf * nf;
      for (int ti = 0; ti < total_t; ++ti)
        for (int fi = 0; fi < total_f; ++fi) {
          Set sets[2];
          int t = ti, f = fi;
          for (int s = 0; s < len; ++s) { idx[s] = t % nt; t /= nt; }
          ++seqs;
          for (int s = 0; s < len; ++s) {
            const int first = firsts[f % nf]; f /= nf;
            std::snprintf(what, sizeof what, "%s, solve %d of %d, tables (gl cons cp) %03d %03d %03d, first move %d", d.name, s + 1, len, tag[idx[0]],
                          len > 1 ? tag[idx[1]] : -1, len > 2 ? tag[idx[2]] : -1, first);
            solve(sets, tabs[idx[s]], first, 2048, what);
          }
        }
    }
  }
  printf("sequences %lld moves %lld reuse %lld realloc %lld fails %lld\n", seqs, n_moves, n_reuse, n_realloc, fails);
  return fails ? 1 : 0;
}
