// fwd_list.h — the list of active trajectories the two-wave forward pass takes its trajectories from ("list mode", k_forward.h), built by
// the scan backward pass of the same batch step (k_scan.h) without a launch of its own.  Plain integer logic: tests/test_fwd_list_host.py
// compiles it for the host and checks the rank against a plain loop.
//
// Every scan workgroup is one wave and one trajectory b.  An active wave reads the batch's `active` flags in passes of 64 (lane l of pass p
// holds flag 64 p + l; a ballot makes the pass a 64-bit mask), counts the set flags below b — its rank among the active trajectories — and
// writes b at that position: the list comes out in index order, as k_compact builds it, with no exchange between the waves.  The list's
// length is the previous step's count of trajectories that go on (KArgs::counter), which the forward pass accumulates anyway.
// The wave of a trajectory that has just finished on an accepted candidate copies it onto the nominal before it leaves (k_scan.h): the
// forward pass of this step gives the candidate block to other trajectories.
#pragma once

namespace to {

constexpr int FWD_LIST_MAX_BP = 2048;  // list mode serves padded batches up to here: at most 32 passes per wave
constexpr int FWD_LIST_CHUNK = 16;     // passes whose loads a scan wave has in flight at once (k_scan.h)

// passes that hold a flag below b: the flags 0 .. b-1 sit in the passes 0 .. fwd_list_passes(b) - 1
__host__ __device__ __forceinline__ int fwd_list_passes(int b) { return (b + 63) >> 6; }
// what pass p (mask: bit l = flag 64 p + l is set) adds to the rank of b: its set flags with an index below b
__host__ __device__ __forceinline__ int fwd_list_rank_add(unsigned long long mask, int p, int b) {
  const int d = b - 64 * p, below = d < 0 ? 0 : d;  // flags of this pass that lie below b (selects, no branch: 16 passes sit back to back)
  const unsigned long long keep = below >= 64 ? ~0ull : (1ull << below) - 1ull;
  return __builtin_popcountll(mask & keep);
}
// where the trajectory of that rank goes: the list of batch step `step` (two lists, by the parity of the step, as KArgs::alist is laid out)
__host__ __device__ __forceinline__ long long fwd_list_slot(int step, int Bp, int rank) { return (long long)(step & 1) * Bp + rank; }
// workgroups of TW trajectories the forward pass launches for a list of at most `count` entries (at least one: the kernel reads the count itself)
__host__ __device__ __forceinline__ int fwd_list_groups(int count, int TW) { return count < 1 ? 1 : (count + TW - 1) / TW; }

}  // namespace to
