// rp_plan.h — sizing and re-use of a repacked working set (trajopt_hip.hip rp_move).  Plain host logic, no HIP types:
// tests/test_rp_plan_host.py compiles it with g++ and replays every sequence of carried-array tables a handle can produce against an
// independent ledger of allocated bytes.
#pragma once

#include <cstddef>
#include <vector>

namespace to {

// One carried array: kind 0 / 3 / 4 a tiled double array with L rows per trajectory (3, 4: never copied home; 4: the per-trajectory cost
// weights, DevProblem::gw — a kind of their own because their row length is that of the per-trajectory cost terms, so that a set sized
// with them is told from one sized without), 1 a double and 2 an int per trajectory.
struct RpSlot { int kind; int L; };
inline bool rp_tiled(int kind) { return kind == 0 || kind == 3 || kind == 4; }
inline int rp_device_kind(int kind) { return kind == 4 ? 3 : kind; }  // what the repack kernels see (k_generic.h RpArgs::kind)

// What the buffers of one working set were sized for (cap = 0: nothing allocated).
struct RpSized {
  std::vector<RpSlot> slots;
  int cap = 0;  // trajectories (a multiple of 64); every buffer also holds one spare tile behind them, the map holds exactly cap
};

inline size_t rp_slot_bytes(const RpSlot& s, int Bp) {
  return rp_tiled(s.kind) ? sizeof(double) * (size_t)s.L * (size_t)Bp : (s.kind == 1 ? sizeof(double) : sizeof(int)) * (size_t)Bp;
}
inline size_t rp_map_bytes(int Bp) { return sizeof(int) * (size_t)Bp; }

// Can the working set sized as `have` take the table `need` at Bp_new trajectories as it is?  The table is rebuilt per solve and
// its optional entries (per-trajectory cost terms, duals and penalties, per-trajectory constraint parameters) come and go with the
// configuration of the handle: two tables of the same length need not hold the same arrays.  Buffer i of the set serves entry i of
// the table, so every entry must be the array the buffer was sized for — same kind, same row length — and the capacity must cover the
// move (the map follows the capacity).  Anything else: the caller frees the whole set and allocates it for `need`.
inline bool rp_reusable(const RpSized& have, const std::vector<RpSlot>& need, int Bp_new) {
  if (have.cap < Bp_new || have.slots.size() != need.size()) return false;
  for (size_t i = 0; i < need.size(); ++i)
    if (have.slots[i].kind != need[i].kind || have.slots[i].L != need[i].L) return false;
  return true;
}

}  // namespace to
