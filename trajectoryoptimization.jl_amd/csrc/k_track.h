// k_track.h — one tracking reference per trajectory, windowed on the device (to_set_tracking_reference_batch / to_set_tracking_window):
// the knot with 0-based index k of trajectory b tracks knot j = start_b - 1 + k of ITS reference (held at the last knot once the window runs
// past the end), and k_track_lower turns that window into the per-trajectory linear cost terms of DevProblem::gl — what N calls of
// to_set_cost_linear_batch with q_b = -Q x_ref[j], r_b = -R u_ref[j] store, bit for bit, in one launch and without the reference leaving
// the device.
//
// Layouts (common.h): the reference is tiled like every per-trajectory array, L = Nref (n + m), row j (n + m) + i = entry i of [x_ref[j];
// u_ref[j]]:  ref[((b >> 6) L + e) 64 + (b & 63)];  gl is tiled with L = n_costs (n + m), row cost (n + m) + i.  Lane = trajectory, one wave
// per workgroup, grid (tiles, row groups) as in k_mpc_writeback; no LDS, no atomics.  A row of gl is stored whole (512 bytes); the read is
// a whole row when the tile's starts agree and a gather inside the tile's block otherwise.  The only lane-divergent region is the exit of
// the lanes behind the batch; everything that selects code — the knot, the row, the cost's kind — is the same in every lane, and the cost
// descriptor is read through the constant address space (scalar loads).
//
// Arithmetic: every product, sum and difference is rounded on its own (contraction is switched off inside the kernel: a fused
// multiply-add would differ from the host recipe in the last bit; the translation unit keeps hipcc's default elsewhere).
//   diagonal kinds:  delta = (-(Q_i x_i)) - c.q[i]
//   QUADRATIC:       acc = Q[i,0] x_0;  acc = acc + Q[i,j] x_j  for ascending j;  delta = (-acc) - c.q[i]
// and the same with R, u, c.r for the control rows, which are not written at all while the reference has no controls.
//
// Attitude rows (to_set_tracking_attitude; TrackArgs::ga set): behind the linear rows the same launch takes N * 4 more rows, (knot k, entry i of
// q_ref).  Where the knot's cost is a DiagonalQuatCost, row 4 ci + i of DevProblem::ga gets x_ref[j][q_ind[i] - 1] — an exact copy, j the
// reference knot of the linear rows (the clamp included), the row stored whole like a row of gl; costs of other kinds are not touched.  With
// ga null the kernel has the rows it always had.
// Non-template: included from trajopt_hip.hip only (and, through the host shim, from tests/host_shim/track_lower_harness.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "models.h"  // (problem_dev.h uses its rcp_fast)
#include "problem_dev.h"

namespace to {

struct TrackArgs {
  int n, m, N, B;
  int Nref;     // knots of the stored reference
  int with_u;   // the reference carries controls: the r rows are lowered too
  int n_costs;
  const double* ref;   // tiled, L = Nref (n + m)
  const int* start;    // [B] 1-based first reference knot of trajectory b's window
  IntC* cost_index;    // [N]
  CostC* costs;        // [n_costs]
  double* gl;          // tiled, L = n_costs (n + m)
  double* ga;          // tiled, L = 4 n_costs: DevProblem::ga while attitude tracking is on, else null (no attitude rows)
};

// grid (tiles, row groups): workgroup (x, y) takes the rows y, y + gridDim.y, ... of tile x, a row being (knot k, entry i of [q; r] — of q alone
// without controls), followed by the attitude rows (knot k, entry i of q_ref) while a.ga is set.  Lanes behind the batch store nothing.
__global__ void __launch_bounds__(64) k_track_lower(TrackArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, tile = blockIdx.x, b = tile * 64 + lane;
  if (b >= a.B) return;
  const int n = a.n, m = a.m, nz = n + m, per = a.with_u ? nz : n, rows = a.N * per, last = a.Nref - 1;
  const int all = rows + (a.ga != nullptr ? a.N * 4 : 0);
  const int j0 = a.start[b] - 1;
  const double* ref = a.ref + ((size_t)tile * (size_t)(a.Nref * nz)) * 64 + lane;
  double* gl = a.gl + ((size_t)tile * (size_t)(a.n_costs * nz)) * 64 + lane;
  for (int e = blockIdx.y; e < all; e += gridDim.y) {
    if (e >= rows) {  // an attitude row (wave-uniform: e is)
      const int k = (e - rows) >> 2, i = (e - rows) & 3;
      int j = j0 + k;
      j = j < last ? j : last;
      j = j > 0 ? j : 0;
      const int ci = a.cost_index[k];
      CostC& c = a.costs[ci];
      if (c.kind != TO_COST_DIAGONAL_QUAT) continue;
      const int src = c.q_ind[i] - 1;  // (1 <= q_ind <= n: desc_lower.h validate_cost)
      (a.ga + ((size_t)tile * (size_t)(a.n_costs * 4)) * 64 + lane)[(size_t)(ci * 4 + i) * 64] = ref[((size_t)j * nz + src) * 64];
      continue;
    }
    const int k = e / per, i = e - k * per;
    int j = j0 + k;          // this lane's reference knot; the host has checked the window, the clamp keeps every read inside the block
    j = j < last ? j : last;
    j = j > 0 ? j : 0;
    const int ci = a.cost_index[k];
    CostC& c = a.costs[ci];
    const bool state = i < n;
    const int d = state ? n : m, r = state ? i : i - n;         // dimension and row of the block this row belongs to
    DoubleC* W = state ? c.Q : c.R;
    const double* z = ref + ((size_t)j * nz + (state ? 0 : n)) * 64;  // x_ref[j] or u_ref[j] of this lane
    double acc;
    if (c.kind == TO_COST_QUADRATIC) {  // dense, column-major (ld = d): ascending columns
      acc = W[r] * z[0];
      for (int col = 1; col < d; ++col) {
        const double p = W[r + d * col] * z[(size_t)col * 64];
        acc = acc + p;
      }
    } else {
      acc = W[r] * z[(size_t)r * 64];
    }
    const double lin = state ? c.q[r] : c.r[r];
    gl[(size_t)(ci * nz + i) * 64] = (-acc) - lin;
  }
}

}  // namespace to
