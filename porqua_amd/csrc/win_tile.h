// Window staging shared by the tile kernels that read the panel through a row table
// (cov.hip, pca_cov.hip): the lower-tile enumeration and the 16-row chunk of a window as a
// K-major LDS image.
#pragma once
#include "common.h"

namespace pq {

__device__ __forceinline__ void tri_index(int t, int& I, int& J) {
  // t enumerates lower tiles row by row: (0,0),(1,0),(1,1),(2,0),...
  I = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  J = t - I * (I + 1) / 2;
}

// stage one 16-row chunk of window columns [c0, c0+64) into image S[k][i] (centred)
__device__ __forceinline__ void load_win(double (&v)[4], const double* panel, int64_t ldp, int n,
                                         const int32_t* rw, int T, int k0, int c0,
                                         const double* mu) {
  const int t = threadIdx.x;
  const int k = t >> 4, i = (t & 15) * 4;
  const int kk = k0 + k;
  const int64_t row = kk < T ? (int64_t)rw[kk] : -1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = c0 + i + e;
    double x = 0.0;
    if (row >= 0 && c < n) {
      x = panel[row * ldp + c];
      if (mu) x -= mu[c];
    }
    v[e] = x;
  }
}
__device__ __forceinline__ void store_win(const double (&v)[4], double* S) {
  const int t = threadIdx.x;
  const int k = t >> 4, i = (t & 15) * 4;
  double2* p = reinterpret_cast<double2*>(S + k * LDW + i);
  p[0] = double2{v[0], v[1]};
  p[1] = double2{v[2], v[3]};
}

}  // namespace pq
