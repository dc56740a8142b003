// scan_combine.h — the element of the scan backward pass (k_scan.h) and its associative combination: plain per-lane arithmetic, no
// lane exchange, so that the host shim compiles it too (tests/host_shim/scan_combine_harness.cpp).
#pragma once
#include "models.h"

namespace to {

template <int n>
struct ScanEl {
  static constexpr int NSY = n * (n + 1) / 2;
  static constexpr int NV = n * n + 2 * n + 2 * NSY;  // doubles per element
  double A[n * n], b[n], C[NSY], eta[n], J[NSY];
  __device__ __forceinline__ static constexpr int sy(int i, int j) { return i <= j ? j * (j + 1) / 2 + i : i * (i + 1) / 2 + j; }
  __device__ __forceinline__ void identity() {
#pragma unroll
    for (int i = 0; i < n; ++i) {
#pragma unroll
      for (int j = 0; j < n; ++j) A[i * n + j] = (i == j) ? 1.0 : 0.0;
      b[i] = 0.0; eta[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < NSY; ++i) { C[i] = 0.0; J[i] = 0.0; }
  }
};

// in-place solve M X = R (M n x n general, R n x r), no pivoting: M = I + (PSD)(PSD) has eigenvalues >= 1
template <int n, int r>
__device__ __forceinline__ void scan_lu_solve(double (&Mx)[n][n], double (&R)[n][r]) {
  double piv[n];
#pragma unroll
  for (int c = 0; c < n; ++c) {
    piv[c] = rcp_fast(Mx[c][c]);
#pragma unroll
    for (int i = c + 1; i < n; ++i) {
      const double f = Mx[i][c] * piv[c];
#pragma unroll
      for (int j = c + 1; j < n; ++j) Mx[i][j] -= f * Mx[c][j];
#pragma unroll
      for (int j = 0; j < r; ++j) R[i][j] -= f * R[c][j];
    }
  }
#pragma unroll
  for (int c = n - 1; c >= 0; --c) {
#pragma unroll
    for (int j = 0; j < r; ++j) {
      double v = R[c][j];
#pragma unroll
      for (int i = c + 1; i < n; ++i) v -= Mx[c][i] * R[i][j];
      R[c][j] = v * piv[c];
    }
  }
}

// o = e1 (earlier span) combined with e2 (the span right after it).
// VALUE_ONLY: the value part (eta, J) alone — the very expressions of the full form, which depend on e1 and on e2.J, e2.eta only:
// e2.A, e2.b, e2.C are not read and o.A, o.b, o.C are not written (the last round of the scan: nobody reads them).
template <int n, bool VALUE_ONLY = false>
__device__ __forceinline__ void scan_combine(const ScanEl<n>& e1, const ScanEl<n>& e2, ScanEl<n>& o) {
  using E = ScanEl<n>;
  double Mm[n][n], Mt[n][n];
#pragma unroll
  for (int i = 0; i < n; ++i)
#pragma unroll
    for (int j = 0; j < n; ++j) {
      double v = (i == j) ? 1.0 : 0.0;
#pragma unroll
      for (int t = 0; t < n; ++t) v += e1.C[E::sy(i, t)] * e2.J[E::sy(t, j)];
      Mm[i][j] = v;
      Mt[j][i] = v;
    }
  if constexpr (!VALUE_ONLY) {
    double R[n][2 * n + 1];
#pragma unroll
    for (int i = 0; i < n; ++i) {
#pragma unroll
      for (int j = 0; j < n; ++j) R[i][j] = e1.A[i * n + j];
      double v = e1.b[i];
#pragma unroll
      for (int t = 0; t < n; ++t) v -= e1.C[E::sy(i, t)] * e2.eta[t];
      R[i][n] = v;
#pragma unroll
      for (int j = 0; j < n; ++j) R[i][n + 1 + j] = e1.C[E::sy(i, j)];
    }
    scan_lu_solve<n, 2 * n + 1>(Mm, R);
    double XC[n][n];
#pragma unroll
    for (int i = 0; i < n; ++i) {
#pragma unroll
      for (int j = 0; j < n; ++j) {
        double v = 0.0, w = 0.0;
#pragma unroll
        for (int t = 0; t < n; ++t) { v += e2.A[i * n + t] * R[t][j]; w += e2.A[i * n + t] * R[t][n + 1 + j]; }
        o.A[i * n + j] = v;
        XC[i][j] = w;
      }
      double v = e2.b[i];
#pragma unroll
      for (int t = 0; t < n; ++t) v += e2.A[i * n + t] * R[t][n];
      o.b[i] = v;
    }
#pragma unroll
    for (int j = 0; j < n; ++j)
#pragma unroll
      for (int i = 0; i <= j; ++i) {
        double cij = e2.C[E::sy(i, j)], cji = cij;
#pragma unroll
        for (int t = 0; t < n; ++t) { cij += XC[i][t] * e2.A[j * n + t]; cji += XC[j][t] * e2.A[i * n + t]; }
        o.C[E::sy(i, j)] = 0.5 * (cij + cji);
      }
  }
  double Y[n][n + 1];
#pragma unroll
  for (int i = 0; i < n; ++i) {
    double v = e2.eta[i];
#pragma unroll
    for (int t = 0; t < n; ++t) v += e2.J[E::sy(i, t)] * e1.b[t];
    Y[i][0] = v;
#pragma unroll
    for (int j = 0; j < n; ++j) {
      double w = 0.0;
#pragma unroll
      for (int t = 0; t < n; ++t) w += e2.J[E::sy(i, t)] * e1.A[t * n + j];
      Y[i][1 + j] = w;
    }
  }
  scan_lu_solve<n, n + 1>(Mt, Y);
#pragma unroll
  for (int i = 0; i < n; ++i) {
    double v = e1.eta[i];
#pragma unroll
    for (int t = 0; t < n; ++t) v += e1.A[t * n + i] * Y[t][0];
    o.eta[i] = v;
  }
#pragma unroll
  for (int j = 0; j < n; ++j)
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      double a = e1.J[E::sy(i, j)], c = a;
#pragma unroll
      for (int t = 0; t < n; ++t) { a += e1.A[t * n + i] * Y[t][1 + j]; c += e1.A[t * n + j] * Y[t][1 + i]; }
      o.J[E::sy(i, j)] = 0.5 * (a + c);
    }
}

}  // namespace to
