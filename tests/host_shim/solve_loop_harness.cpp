// Compiles csrc/solve_loop.h for the host and plays the device (test infrastructure; tests/test_solve_loop_host.py).  A case is a
// configuration, the per-step active counts a device would write (from per-trajectory iteration counts, as tests/repack_cases.py
// active_counts derives them) and the move attempt that finds no memory (none: every move is accepted).
//   (a) `before` below is the loop of solve_impl as it was before the driver existed, kept verbatim; every HIP call and launcher call is
//       replaced by a trace record.  The driver, performed the way solve_impl performs it, must leave the same trace: operation for
//       operation, argument for argument.
//   (c) invariants of the driver's trace alone (check_invariants).
//   (d) what the randomized cases reached, printed as "name value" words for the Python test to assert.
// With a file argument: one case per line (max_steps B al_mode repack rp_at rp_min early early_div decline_at n it_0 .. it_n-1); prints the
// accepted moves of each as "moves level count level count ...".
#include "solve_loop.h"

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>
using namespace to;

enum RecKind { R_STEP, R_COPY, R_WAIT, R_DRAIN, R_CONSUME, R_PUBLISH, R_MOVE, R_MOVED, R_SNAPSHOT, R_POLISH, R_END, R_KINDS };
static const char* const REC_NAMES[R_KINDS] = {"step", "copy", "wait", "drain", "consume", "publish", "move", "moved", "snapshot", "polish", "end"};
struct Rec {
  int kind, a, b, c;
  bool operator==(const Rec& o) const { return kind == o.kind && a == o.a && b == o.b && c == o.c; }
};
typedef std::vector<Rec> Trace;

struct Case {
  SolveLoopConfig cfg;
  std::vector<int> counter;  // [max_steps]
  int decline_at = -1;       // the move attempt (0, 1, ...) that is declined
};

// ---- the parent's loop -----------------------------------------------------------------------------------------------------------------
namespace before {
enum { TO_OK = 0 };
#define TRY(expr) do { int r_ = (expr); if (r_ != TO_OK) return r_; } while (0)
#define HIPCHECK(expr) (expr)
struct Handle {  // what the loop read from the handle, and the device behind it
  struct { struct { int B; } P; int compact, step; } a;
  struct { double rp_at; int rp_min; } plan;
  int pn_early = 0, rp_level = 0, attempts = 0, decline_at = -1;
  bool repack_path = false;
  const int* counter_host = nullptr;
  Trace* t = nullptr;
  void rec(int kind, int x = 0, int y = 0, int z = 0) { t->push_back({kind, x, y, z}); }
};
static int rp_move(Handle* h, int count) {
  h->rec(R_MOVE, h->a.step, count);
  const bool declined = h->attempts++ == h->decline_at;
  h->rec(R_MOVED, declined ? 0 : 1);
  if (declined) return 1;
  h->a.P.B = count; ++h->rp_level;
  return TO_OK;
}
static void publish_progress(Handle* h, int active, int steps) { h->rec(R_PUBLISH, active, steps); }
static int early_polish_snapshot(Handle* h) { h->rec(R_SNAPSHOT); return TO_OK; }
static int early_polish_launch(Handle* h) { h->rec(R_POLISH); return TO_OK; }

static int loop(Handle* h, int al_mode, int max_steps, int early_div) {
  auto& a = h->a;
  const auto& P = a.P;
  int steps = 0;
  constexpr int CHECK_EVERY = 4;
  const int cev[2] = {0, 1};
  int launched = 0, checked = 0, nchunks = 0, last_active = P.B;
  bool done = false;
  auto enqueue_chunk = [&]() -> int {
    const int chunk = std::min(CHECK_EVERY, max_steps - launched);
    for (int c = 0; c < chunk; ++c) {
      const int step = launched + c;
      a.step = step;
      h->rec(R_STEP, step, last_active, P.B);  // (plan_step's arguments; the launches of the step)
    }
    h->rec(R_COPY, launched, chunk, cev[nchunks & 1]);  // (hipMemcpyAsync of counter[launched .. launched + chunk), hipEventRecord)
    launched += chunk;
    ++nchunks;
    return TO_OK;
  };
  int waited = 0;  // chunks whose counters have been inspected
  // early polish (ALTRO solves): the next active count at which the finished trajectories are handed over
  int early_thr = (al_mode && h->pn_early > 0) ? P.B / early_div : -1, early_left = h->pn_early;
  bool snapshot_pending = false;
  // repacked working set (above): iLQR solves of the small models on the fused lane path with compaction
  bool repack = !al_mode && a.compact && h->repack_path;
  if (max_steps > 0) TRY(enqueue_chunk());
  while (!done && waited < nchunks) {
    if (repack && last_active >= 1 && (double)last_active <= h->plan.rp_at * (double)a.P.B && a.P.B >= h->plan.rp_min) {
      // the exact count is needed on the host (B of every later launch): drain the queue once — a handful of times per solve
      HIPCHECK(h->rec(R_DRAIN));
      h->rec(R_CONSUME, checked, launched);
      for (; checked < launched; ++checked) {
        ++steps;
        last_active = h->counter_host[checked];
        if (last_active == 0) { done = true; break; }
      }
      waited = nchunks;
      publish_progress(h, last_active, steps);
      if (done) break;
      a.step = launched - 1;   // (k_compact of that step built the list the move reads)
      {
        const int mrc = rp_move(h, last_active);
        if (mrc > 0) repack = false;  // declined (out of memory): no further attempts in this solve
        else TRY(mrc);
      }
      if (launched < max_steps) TRY(enqueue_chunk());
      continue;
    }
    if (launched < max_steps) TRY(enqueue_chunk());  // keep the queue one chunk ahead
    if (snapshot_pending) {  // taken before that chunk: the device keeps working while the host lists and launches
      TRY(early_polish_launch(h));
      snapshot_pending = false;
    }
    HIPCHECK(h->rec(R_WAIT, cev[waited & 1]));
    const int upto = std::min(launched, (waited + 1) * CHECK_EVERY);
    h->rec(R_CONSUME, checked, upto);
    for (; checked < upto; ++checked) {
      ++steps;
      last_active = h->counter_host[checked];
      if (h->counter_host[checked] == 0) { done = true; break; }
    }
    ++waited;
    publish_progress(h, last_active, steps);
    if (!done && early_left > 0 && last_active <= early_thr) {
      TRY(early_polish_snapshot(h));
      snapshot_pending = true;
      --early_left;
      while (early_thr > 0 && last_active <= early_thr) early_thr /= 2;
    }
  }
  h->rec(R_END, steps, a.P.B, h->rp_level);
  return TO_OK;
}
#undef TRY
#undef HIPCHECK

static void run(const Case& k, Trace* t) {
  Handle h;
  h.a.P.B = k.cfg.B; h.a.compact = 1; h.a.step = 0;
  h.plan.rp_at = k.cfg.rp_at; h.plan.rp_min = k.cfg.rp_min;
  h.repack_path = k.cfg.repack; h.pn_early = k.cfg.early; h.decline_at = k.decline_at;
  h.counter_host = k.counter.data(); h.t = t;
  loop(&h, k.cfg.al_mode, k.cfg.max_steps, k.cfg.early_div);
}
}  // namespace before

// ---- the driver, performed as solve_impl performs it ------------------------------------------------------------------------------------
struct Outcome { int steps, drain_finish, moves, declined; };
static Outcome run_driver(const Case& k, Trace* t, std::vector<int>* accepted = nullptr) {
  SolveLoop lp(k.cfg);
  int attempts = 0, level = 0, B = k.cfg.B;
  Outcome out = {0, 0, 0, 0};
  bool drained = false;
  for (LoopOp op = lp.next(); op.kind != OP_FINISH; op = lp.next()) switch (op.kind) {
    case OP_CHUNK: for (int s = op.step; s < op.step + op.n; ++s) t->push_back({R_STEP, s, op.last_active, op.B}); break;
    case OP_COPY: t->push_back({R_COPY, op.step, op.n, op.event}); break;
    case OP_WAIT: t->push_back({R_WAIT, op.event, 0, 0}); drained = false; break;
    case OP_DRAIN: t->push_back({R_DRAIN, 0, 0, 0}); drained = true; break;
    case OP_CONSUME:
      t->push_back({R_CONSUME, op.step, op.step + op.n, 0});
      lp.consume(k.counter.data(), op);
      t->push_back({R_PUBLISH, lp.last_active, lp.steps, 0});
      if (lp.done && drained) out.drain_finish = 1;
      break;
    case OP_MOVE: {
      t->push_back({R_MOVE, op.step, op.n, 0});
      const bool declined = attempts++ == k.decline_at;
      t->push_back({R_MOVED, declined ? 0 : 1, 0, 0});
      if (!declined) { if (accepted) { accepted->push_back(level); accepted->push_back(op.n); } B = op.n; ++level; ++out.moves; } else out.declined = 1;
      lp.moved(!declined);
      break;
    }
    case OP_SNAPSHOT: t->push_back({R_SNAPSHOT, 0, 0, 0}); break;
    case OP_POLISH: t->push_back({R_POLISH, 0, 0, 0}); break;
    case OP_FINISH: break;
  }
  t->push_back({R_END, lp.steps, B, level});
  out.steps = lp.steps;
  return out;
}

static long long fails = 0, checks = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static std::string describe(const Case& k) {
  char s[240];
  snprintf(s, sizeof s, "max_steps %d B %d al %d repack %d at %.2f min %d early %d / %d decline_at %d", k.cfg.max_steps, k.cfg.B, k.cfg.al_mode, (int)k.cfg.repack,
           k.cfg.rp_at, k.cfg.rp_min, k.cfg.early, k.cfg.early_div, k.decline_at);
  return s;
}

// (c) what must hold of any trace of the driver, whatever the parent did.  (Between a snapshot and its hand-over exactly one chunk is
// enqueued while steps are left to launch; with all max_steps launched the hand-over follows with none in between, as in the parent's loop.
// A snapshot taken on the last inspection of a solve has no hand-over: the polish behind the AL stage takes those trajectories.)
static void check_invariants(const Case& k, const Trace& t) {
  const std::string what = describe(k);
  const char* w = what.c_str();
  int copied = 0, synced = 0, cover[QUEUE_EVENTS] = {0, 0}, outstanding = 0, launched = 0, B = k.cfg.B, consumed = 0, steps = 0;
  int snapshots = 0, polishes = 0, chunks_since_snapshot = -1, room_at_snapshot = 0, moving = 0;
  bool declined = false, step_open = false;
  for (const Rec& r : t) switch (r.kind) {
    case R_STEP:
      CHECK(r.a == launched, "%s: step %d enqueued as number %d", w, r.a, launched);
      CHECK(r.c == B, "%s: step %d planned with B %d, the set holds %d", w, r.a, r.c, B);
      if (!step_open) { ++outstanding; step_open = true; if (chunks_since_snapshot >= 0) ++chunks_since_snapshot; }
      ++launched;
      CHECK(launched <= k.cfg.max_steps, "%s: %d steps launched", w, launched);
      CHECK(outstanding <= QUEUE_EVENTS, "%s: %d chunks outstanding", w, outstanding);
      break;
    case R_COPY:
      CHECK(step_open && r.a == copied && r.a + r.b == launched && r.b >= 1 && r.b <= CHECK_EVERY, "%s: copy of [%d, %d) with %d launched, %d copied", w, r.a, r.a + r.b, launched, copied);
      CHECK(r.c >= 0 && r.c < QUEUE_EVENTS, "%s: event %d", w, r.c);
      copied = r.a + r.b; cover[r.c % QUEUE_EVENTS] = copied; step_open = false;
      break;
    case R_WAIT: CHECK(outstanding > 0 && cover[r.a] > synced, "%s: wait for event %d: nothing new behind it", w, r.a); synced = std::max(synced, cover[r.a]); --outstanding; break;
    case R_DRAIN: synced = copied; outstanding = 0; break;
    case R_CONSUME:
      CHECK(r.a == consumed && r.b >= r.a && r.b <= synced, "%s: counters [%d, %d) consumed, %d read before, %d copied and waited for", w, r.a, r.b, consumed, synced);
      break;
    case R_PUBLISH:  // (the counters read: one per batch step counted)
      consumed += r.b - steps; steps = r.b;
      CHECK(consumed <= synced, "%s: counter %d read, %d waited for", w, consumed - 1, synced);
      CHECK(r.a == k.counter[steps - 1], "%s: active count %d published after step %d, the device wrote %d", w, r.a, steps - 1, k.counter[steps - 1]);
      break;
    case R_MOVE:
      CHECK(!declined, "%s: a move attempted after one was declined", w);
      CHECK(r.b >= 1 && r.b < B && r.a == launched - 1 && outstanding == 0, "%s: move of %d from a set of %d behind step %d, %d chunks outstanding", w, r.b, B, r.a, outstanding);
      moving = r.b;
      break;
    case R_MOVED: if (r.a) B = moving; else declined = true; break;
    case R_SNAPSHOT: ++snapshots; CHECK(chunks_since_snapshot < 0, "%s: a snapshot while one is pending", w); chunks_since_snapshot = 0; room_at_snapshot = launched < k.cfg.max_steps; break;
    case R_POLISH:
      ++polishes;
      CHECK(chunks_since_snapshot == room_at_snapshot, "%s: %d chunks between snapshot and hand-over (steps left to launch: %d)", w, chunks_since_snapshot, room_at_snapshot);
      chunks_since_snapshot = -1;
      break;
    case R_END: {
      int first0 = k.cfg.max_steps;
      for (int i = 0; i < k.cfg.max_steps; ++i) if (k.counter[i] == 0) { first0 = i + 1; break; }
      CHECK(r.a == first0 && r.a == steps, "%s: %d batch steps, first zero counter + 1 = %d", w, r.a, first0);
      break;
    }
  }
  CHECK(snapshots <= k.cfg.early && polishes <= snapshots && polishes >= snapshots - 1, "%s: %d snapshots, %d hand-overs, allowance %d", w, snapshots, polishes, k.cfg.early);
  CHECK(k.cfg.al_mode || snapshots == 0, "%s: early polish in an iLQR solve", w);
}

// ---- cases -----------------------------------------------------------------------------------------------------------------------------
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 16); }
static int pick(std::initializer_list<int> l) { return l.begin()[rnd() % l.size()]; }

// counter[k]: trajectories still iterating after batch step k (a trajectory that takes i iterations is active in steps 0 .. i-1)
static void active_counts(const std::vector<int>& it, int steps, std::vector<int>* counter) {
  std::vector<int> hist(steps + 2, 0);
  for (int i : it) ++hist[std::min(std::max(i, 0), steps + 1)];
  counter->assign(steps, 0);
  int above = 0;  // trajectories with more than k + 1 iterations
  for (int k = steps - 1; k >= 0; --k) { above += hist[k + 2]; (*counter)[k] = above; }
}

static std::map<std::string, long long> cov;
static std::set<int> seen_max_steps, seen_B, seen_at, seen_early, seen_div;

static void run_case(const Case& k, Trace* was, Trace* now) {
  was->clear(); now->clear();
  before::run(k, was);
  const Outcome o = run_driver(k, now);
  ++checks;
  if (!(*was == *now)) {
    ++fails;
    if (fails < 10) {
      size_t i = 0;
      while (i < was->size() && i < now->size() && (*was)[i] == (*now)[i]) ++i;
      printf("FAIL %s: traces differ at record %zu of %zu / %zu", describe(k).c_str(), i, was->size(), now->size());
      if (i < was->size()) printf("; parent: %s %d %d %d", REC_NAMES[(*was)[i].kind], (*was)[i].a, (*was)[i].b, (*was)[i].c);
      if (i < now->size()) printf("; driver: %s %d %d %d", REC_NAMES[(*now)[i].kind], (*now)[i].a, (*now)[i].b, (*now)[i].c);
      printf("\n");
    }
  }
  check_invariants(k, *now);
  for (const Rec& r : *now) ++cov[std::string("op_") + REC_NAMES[r.kind]];
  const bool finished = o.steps < k.cfg.max_steps || k.counter[k.cfg.max_steps - 1] == 0;
  if (!finished) ++cov["end_max_steps"];
  else if (o.steps == 1) ++cov["end_first_step"];
  else if (o.steps % CHECK_EVERY == 0 || o.steps == k.cfg.max_steps) ++cov["end_chunk_edge"];
  else ++cov["end_mid_chunk"];
  if (o.drain_finish) ++cov["end_in_drain"];
  ++cov[k.cfg.al_mode ? "mode_al" : "mode_ilqr"];
  ++cov[k.cfg.repack ? "repack_on" : "repack_off"];
  if (o.moves) ++cov["solves_that_moved"];
  seen_max_steps.insert(k.cfg.max_steps); seen_B.insert(k.cfg.B);
  if (k.cfg.repack && !k.cfg.al_mode) seen_at.insert((int)(k.cfg.rp_at * 100 + 0.5));
  if (k.cfg.al_mode) { seen_early.insert(k.cfg.early); if (k.cfg.early) seen_div.insert(k.cfg.early_div); }
}

static void random_cases(int count) {
  Case k;
  Trace was, now, probe;
  std::vector<int> it;
  for (int n = 0; n < count; ++n) {
    SolveLoopConfig& c = k.cfg;
    c.max_steps = pick({1, 2, 3, 4, 5, 8, 9, 81, 301});
    c.B = pick({1, 63, 64, 65, 200, 2, 7, 130, 1 + (int)(rnd() % 300)});
    c.al_mode = rnd() % 3 == 0;
    c.repack = rnd() % 4 != 0;
    c.rp_at = 0.05 * (1 + rnd() % 19);
    c.rp_min = pick({1, 1, 1, 2, 16, 64, 100});
    c.early = c.al_mode ? pick({0, 1, 4, 8, (int)(rnd() % 9)}) : 0;
    c.early_div = pick({1, 2, 4, 4, 1 + (int)(rnd() % 6)});
    // iteration counts: everybody together, spread evenly over a span, or most early and a tail
    const int span = std::max(1, pick({1, 2, 3, 4, 5, 8, 9, c.max_steps / 2, c.max_steps - 1, c.max_steps, c.max_steps + 3, 12, 40}));
    const int shape = rnd() % 4;
    it.resize(c.B);
    for (int& i : it) {
      if (shape == 0) i = span;
      else if (shape == 1) i = 1 + rnd() % span;
      else { i = 1; while (i < span && rnd() % 8 != 0) ++i; if (shape == 3 && rnd() % 16 == 0) i = span + 2; }
    }
    active_counts(it, c.max_steps, &k.counter);
    // the move that finds no memory: none, the first, a middle one, the last of those the solve makes when every move is accepted
    k.decline_at = -1;
    probe.clear();
    const int moves = run_driver(k, &probe).moves;
    const int choice = rnd() % 4;
    if (moves > 0 && choice == 1) { k.decline_at = 0; ++cov["declined_first"]; }
    if (moves > 2 && choice == 2) { k.decline_at = 1 + rnd() % (moves - 2); ++cov["declined_middle"]; }
    if (moves > 0 && choice == 3) { k.decline_at = moves - 1; ++cov["declined_last"]; }
    run_case(k, &was, &now);
  }
}

static int file_cases(const char* path) {
  std::ifstream f(path);
  std::string line;
  Trace was, now;
  while (std::getline(f, line)) {
    std::istringstream s(line);
    Case k;
    int repack = 0, n = 0;
    if (!(s >> k.cfg.max_steps >> k.cfg.B >> k.cfg.al_mode >> repack >> k.cfg.rp_at >> k.cfg.rp_min >> k.cfg.early >> k.cfg.early_div >> k.decline_at >> n)) continue;
    k.cfg.repack = repack != 0;
    std::vector<int> it(n);
    for (int& i : it) s >> i;
    if (!s || k.cfg.max_steps < 1) { printf("bad case: %s\n", line.c_str()); return 2; }
    active_counts(it, k.cfg.max_steps, &k.counter);
    run_case(k, &was, &now);
    std::vector<int> accepted;
    now.clear();
    run_driver(k, &now, &accepted);
    printf("moves");
    for (int v : accepted) printf(" %d", v);
    printf("\n");
  }
  printf("checks %lld fails %lld\n", checks, fails);
  return fails ? 1 : 0;
}

// the switches of a solve: defaults, clamping, and that nothing else is read
static std::map<std::string, std::string> g_env;
static std::set<std::string> g_asked;
static const char* lookup(const char* name) { g_asked.insert(name); auto it = g_env.find(name); return it == g_env.end() ? nullptr : it->second.c_str(); }
static void knob_cases() {
  g_env.clear();
  SolveKnobs k = read_solve_knobs(lookup);
  CHECK(k.fwd_list == 1 && k.pn_early == 1 && k.pn_early_at == 4 && k.sync_debug == 0, "defaults: %d %d %d %d", k.fwd_list, k.pn_early, k.pn_early_at, k.sync_debug);
  CHECK(g_asked == (std::set<std::string>{"TRAJOPT_FWD_LIST", "TRAJOPT_PN_EARLY", "TRAJOPT_PN_EARLY_AT", "TRAJOPT_SYNC_DEBUG"}), "%zu names asked for", g_asked.size());
  g_env = {{"TRAJOPT_FWD_LIST", "0"}, {"TRAJOPT_PN_EARLY", "12"}, {"TRAJOPT_PN_EARLY_AT", "0"}, {"TRAJOPT_SYNC_DEBUG", "0"}};
  k = read_solve_knobs(lookup);
  CHECK(k.fwd_list == 0 && k.pn_early == 8 && k.pn_early_at == 1 && k.sync_debug == 1, "clamped above / below: %d %d %d %d", k.fwd_list, k.pn_early, k.pn_early_at, k.sync_debug);
  g_env = {{"TRAJOPT_FWD_LIST", "1"}, {"TRAJOPT_PN_EARLY", "-3"}, {"TRAJOPT_PN_EARLY_AT", "2"}};
  k = read_solve_knobs(lookup);
  CHECK(k.fwd_list == 1 && k.pn_early == 0 && k.pn_early_at == 2 && k.sync_debug == 0, "set: %d %d %d %d", k.fwd_list, k.pn_early, k.pn_early_at, k.sync_debug);
  g_env = {{"TRAJOPT_FWD_LIST", "x"}, {"TRAJOPT_PN_EARLY", "4"}};  // (atoi: anything that is not a number counts as 0, as before)
  k = read_solve_knobs(lookup);
  CHECK(k.fwd_list == 0 && k.pn_early == 4, "text: %d %d", k.fwd_list, k.pn_early);
}

int main(int argc, char** argv) {
  if (argc > 1) return file_cases(argv[1]);
  knob_cases();
  random_cases(120000);
  for (const auto& kv : cov) printf("%s %lld\n", kv.first.c_str(), kv.second);
  auto show = [](const char* name, const std::set<int>& s) { printf("%s", name); for (int v : s) printf(" %d", v); printf(" ;\n"); };
  show("max_steps_seen", seen_max_steps); show("batches_seen", seen_B); show("rp_at_percent_seen", seen_at); show("early_seen", seen_early); show("early_div_seen", seen_div);
  printf("cases 120000 checks %lld fails %lld\n", checks, fails);
  return fails ? 1 : 0;
}
