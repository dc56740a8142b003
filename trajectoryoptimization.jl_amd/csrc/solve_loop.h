// solve_loop.h — what the host decides while a solve runs, in one place.  Plain host logic, no HIP types: solve_impl (trajopt_hip.hip) asks
// SolveLoop::next() for the next operation, performs it with HIP calls and reports back (consume, moved);
// tests/host_shim/solve_loop_harness.cpp compiles the same driver with g++ and plays the device (tests/test_solve_loop_host.py).
//
// The host only needs to know WHEN every trajectory has finished: it enqueues CHECK_EVERY batch steps back to back and reads the per-step
// "still active" counters once per chunk.  The read-back is pipelined: chunk g+1 is already enqueued when the host waits for the counters
// of chunk g, so the GPU never idles on the round trip; the price is at most one chunk of launches whose kernels find nothing to do
// (kernels of finished trajectories exit at once).
#pragma once

#include <algorithm>
#include <cstdlib>

namespace to {

constexpr int CHECK_EVERY = 4;  // batch steps per chunk
constexpr int QUEUE_EVENTS = 2; // the queue runs one chunk ahead: the chunk the host waits for and the one behind it, an event each

// The TRAJOPT_* switches of a solve, read afresh at the start of every solve; a switch that is unset has the value given here.
struct SolveKnobs { int fwd_list = 1, pn_early = 1, pn_early_at = 4, sync_debug = 0; };
inline SolveKnobs read_solve_knobs(const char* (*get)(const char*)) {  // THE list of these switches, with the clamping each has
  SolveKnobs k;
  if (const char* s = get("TRAJOPT_FWD_LIST")) k.fwd_list = std::atoi(s) != 0;                            // 0: the forward pass keeps its fixed map
  if (const char* s = get("TRAJOPT_PN_EARLY")) k.pn_early = std::max(0, std::min(8, std::atoi(s)));       // hand-overs to the early polish per ALTRO solve, 0..8
  if (const char* s = get("TRAJOPT_PN_EARLY_AT")) k.pn_early_at = std::max(1, std::atoi(s));              // the first when 1 / this of the batch is left
  k.sync_debug = get("TRAJOPT_SYNC_DEBUG") != nullptr;                                                    // set: a stream synchronisation and a line on stderr per batch step
  return k;
}

struct SolveLoopConfig {
  int max_steps = 1, B = 1, al_mode = 0;
  bool repack = false;  // the handle's path has the repacked working set (iLQR solves only: the driver sees to that) ...
  double rp_at = 0.7;   // ... a move is due once this fraction of the current set is left ...
  int rp_min = 0;       // ... while the set holds at least this many trajectories
  int early = 0;        // AL solves: hand-overs of finished trajectories to the early polish ...
  int early_div = 4;    // ... the first when B / early_div trajectories are left, every later one at half the previous count
};

enum LoopOpKind {
  OP_CHUNK,     // enqueue batch steps step .. step + n - 1, each planned with last_active and B
  OP_COPY,      // copy the counters of those steps to the host, record event `event` behind the copy
  OP_WAIT,      // wait for event `event`
  OP_DRAIN,     // wait for everything on the stream (a move needs the exact count on the host: B of every later launch)
  OP_CONSUME,   // SolveLoop::consume on counters step .. step + n - 1, then publish last_active and steps
  OP_MOVE,      // move the n active trajectories (the list k_compact built in batch step `step`) into the other working set; report moved()
  OP_SNAPSHOT,  // early polish: snapshot of what has finished (before the next chunk: the device keeps working while the host lists) ...
  OP_POLISH,    // ... and its launch, behind that chunk
  OP_FINISH
};
struct LoopOp { LoopOpKind kind; int step, n, event, last_active, B; };

struct SolveLoop {
  const SolveLoopConfig c;
  int launched = 0, checked = 0, waited = 0, nchunks = 0, steps = 0;  // steps enqueued, counters read; chunks inspected, enqueued; batch steps of the solve
  int last_active, B;  // the last active count the host has seen; the size of the set the kernels work on
  bool done = false, repack, snapshot_pending = false;
  int early_left, early_thr;
  explicit SolveLoop(const SolveLoopConfig& cfg)
      : c(cfg), last_active(cfg.B), B(cfg.B), repack(!cfg.al_mode && cfg.repack), early_left(cfg.early),
        early_thr(cfg.al_mode && cfg.early > 0 ? cfg.B / cfg.early_div : -1) {}

  LoopOp next() {
    for (;;) switch (at) {
      case START: at = TOP; if (c.max_steps > 0) return chunk(); continue;
      case COPY: {
        const LoopOp o = op(OP_COPY, launched, pending, nchunks % QUEUE_EVENTS);
        launched += pending; ++nchunks; at = after_copy;
        return o;
      }
      case TOP:
        if (done || waited >= nchunks) return op(OP_FINISH);
        if (repack && last_active >= 1 && (double)last_active <= c.rp_at * (double)B && B >= c.rp_min) { at = DRAINED; return op(OP_DRAIN); }
        at = AHEAD;
        if (launched < c.max_steps) return chunk();  // keep the queue one chunk ahead
        continue;
      case AHEAD: at = WAIT; if (snapshot_pending) { snapshot_pending = false; return op(OP_POLISH); } continue;
      case WAIT: at = READ; return op(OP_WAIT, 0, 0, waited % QUEUE_EVENTS);
      case READ: at = EARLY; ++waited; return op(OP_CONSUME, checked, std::min(launched, waited * CHECK_EVERY) - checked);
      case EARLY:
        at = TOP;
        if (done || early_left <= 0 || last_active > early_thr) continue;
        snapshot_pending = true; --early_left;
        while (early_thr > 0 && last_active <= early_thr) early_thr /= 2;
        return op(OP_SNAPSHOT);
      case DRAINED: at = MOVE; waited = nchunks; return op(OP_CONSUME, checked, launched - checked);
      case MOVE: if (done) return op(OP_FINISH); at = MOVED; return op(OP_MOVE, launched - 1, last_active);
      case MOVED: at = TOP; if (launched < c.max_steps) return chunk(); continue;
    }
  }
  // the counters an OP_CONSUME names: every one a batch step of the solve, up to the first that says nobody is left
  void consume(const int* counter, const LoopOp& o) {
    for (const int upto = o.step + o.n; checked < upto; ++checked) {
      ++steps;
      last_active = counter[checked];
      if (last_active == 0) { done = true; break; }
    }
  }
  // the outcome of an OP_MOVE: the kernels work on the moved set from here on, or (no memory for it) the solve goes on where it is, for good
  void moved(bool accepted) { if (accepted) B = last_active; else repack = false; }

 private:
  enum At { START, COPY, TOP, AHEAD, WAIT, READ, EARLY, DRAINED, MOVE, MOVED } at = START, after_copy = TOP;
  int pending = 0;  // steps of the chunk whose OP_COPY is due
  LoopOp op(LoopOpKind k, int step = 0, int n = 0, int event = 0) const { return {k, step, n, event, last_active, B}; }
  LoopOp chunk() {  // (called with `at` already set to what follows the chunk)
    pending = std::min(CHECK_EVERY, c.max_steps - launched);
    after_copy = at; at = COPY;
    return op(OP_CHUNK, launched, pending);
  }
};

}  // namespace to
