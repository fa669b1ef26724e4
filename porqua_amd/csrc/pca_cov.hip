// PCA factor covariance (probabilistic PCA, Tipping & Bishop 1999): the two window kernels
// around the batched eigensolver.
//
// With Xc the date's centred T x n window and G = Xc Xc' = V diag(g) V' its T x T Gram, the
// nonzero eigenvalues of S = Xc'Xc / (T-1) are l_j = g_j / (T-1) and its eigenvectors are
// Xc' v_j / sqrt(g_j), so the k-factor covariance with one noise level sigma2 for the rest of
// the spectrum is
//     Sigma = Z'Z + sigma2 I,    Z_j = sqrt((1 - sigma2 / l_j) / (T-1)) v_j' Xc    (k x n)
// -- the uncentred window form (a = 1, c = sigma2) of a factor panel with k rows per date.
// pq_window_gram_batched forms G (contraction over the n assets, centred while staging, lower
// 64 x 64 tiles and their mirrors as k_syrk writes Sigma); pq_window_project_batched writes the
// rows Z_j, a (k x T)(T x n) product per date with the window read once through the row table.
// The eigenvalue map between them (sort, sigma2, the factor count) is a few O(T) device ops
// per date in engine.pca_window_form.
#include "common.h"
#include "capi_util.h"
#include "win_tile.h"

namespace pq {

// 16 columns [c0 + k] of the window row this thread stages (i = t >> 2 of the tile's 64 rows;
// row < 0: past the window) for the image S[k][i] that store_ik writes: the contraction runs
// over the assets
__device__ __forceinline__ void load_row_chunk(Stage4& s, const double* panel, int64_t ldp, int n, int64_t row,
                                               int c0, const double* mu) {
  const int k = (threadIdx.x & 3) * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = c0 + k + e;
    double x = 0.0;
    if (row >= 0 && c < n) {
      x = panel[row * ldp + c];
      if (mu) x -= mu[c];
    }
    s.v[e] = x;
  }
}

__global__ __launch_bounds__(256) void k_window_gram(const double* panel, int64_t ldp, int n, const int32_t* rows,
                                                     const int32_t* tlen, int tmax, const double* mu,
                                                     int64_t mu_stride, double* out, int ldg, int64_t out_stride) {
  __shared__ __attribute__((aligned(16))) double smem[4 * STAGE];
  const int b = blockIdx.y;
  int I, J;
  tri_index(blockIdx.x, I, J);
  const int T = min(max(tlen[b], 0), tmax);
  const int32_t* rw = rows + (int64_t)b * tmax;
  const double* m = mu ? mu + (int64_t)b * mu_stride : nullptr;
  Acc acc;
  acc.zero();
  if (I * TB < T) {   // (else the tile lies in the padding: rows >= T, written as zeros)
    const int i = threadIdx.x >> 2;
    const int64_t ra = I * TB + i < T ? (int64_t)rw[I * TB + i] : -1;
    const int64_t rb = J * TB + i < T ? (int64_t)rw[J * TB + i] : -1;
    Stage4 sa, sb;
    load_row_chunk(sa, panel, ldp, n, ra, 0, m);
    load_row_chunk(sb, panel, ldp, n, rb, 0, m);
    store_ik(sa, smem);
    store_ik(sb, smem + STAGE);
    __syncthreads();
    int buf = 0;
    for (int c0 = 0; c0 < n; c0 += KC) {
      const bool more = (c0 + KC) < n;
      if (more) {
        load_row_chunk(sa, panel, ldp, n, ra, c0 + KC, m);
        load_row_chunk(sb, panel, ldp, n, rb, c0 + KC, m);
      }
      mma_lds(acc, smem + buf * 2 * STAGE, smem + buf * 2 * STAGE + STAGE, KC);
      if (more) {
        store_ik(sa, smem + (buf ^ 1) * 2 * STAGE);
        store_ik(sb, smem + (buf ^ 1) * 2 * STAGE + STAGE);
      }
      __syncthreads();
      buf ^= 1;
    }
  }
  double* o = out + (int64_t)b * out_stride;
  acc_store(acc, o, ldg, I * TB, J * TB);
  if (I != J) acc_store_T(acc, o, ldg, J * TB, I * TB);
}

// acc[q] += the 16 x 16 block (factors [16 q, 16 q + 16)) x (this wave's 16 columns) of one staged
// chunk, q < MT: SA[k][factor], SB[k][column] with pitch LDW (the operand lane maps of common.h)
template <int MT>
__device__ __forceinline__ void mma_factor_rows(f64x4 (&acc)[4], const double* SA, const double* SB) {
  const int l = lane_id(), w = wave_id();
#pragma unroll
  for (int kk = 0; kk < KC; kk += 4) {
    const double* ra = SA + (kk + (l >> 4)) * LDW + (l & 15);
    const double bv = SB[(kk + (l >> 4)) * LDW + w * 16 + (l & 15)];
#pragma unroll
    for (int q = 0; q < MT; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[q * 16], bv, acc[q], 0, 0, 0);
  }
}

// One workgroup per 64 columns and date:acc(j, c) = sum_t V[t][col_j] Xc[t][c0 + c].  Wave w
// owns columns [16 w, 16 w + 16) and the ceil(kcnt / 16) row tiles that hold factors, so the
// MFMA work follows the factor count, not PQ_PCA_KMAX.
__global__ __launch_bounds__(256) void k_window_project(const double* panel, int64_t ldp, int n,
                                                        const int32_t* rows, const int32_t* tlen, int tmax,
                                                        const double* mu, int64_t mu_stride, const double* V,
                                                        int ldv, int64_t v_stride, const int32_t* col,
                                                        const double* s, const int32_t* kcnt, int kmax,
                                                        const int32_t* frow, double* F, int64_t ldf) {
  __shared__ __attribute__((aligned(16))) double smem[4 * STAGE];
  const int b = blockIdx.y;
  const int kc = min(max(kcnt[b], 0), kmax);
  if (kc == 0) return;
  const int c0 = blockIdx.x * TB;
  const int T = min(max(tlen[b], 0), tmax);
  const int32_t* rw = rows + (int64_t)b * tmax;
  const double* m = mu ? mu + (int64_t)b * mu_stride : nullptr;
  const double* Vb = V + (int64_t)b * v_stride;
  const int t = threadIdx.x, l = lane_id(), w = wave_id();
  const int mt = (kc + 15) >> 4;
  f64x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
  if (c0 < n) {   // (else a tile of the row padding [n, ldf): zeros)
    // the eigenvector columns of this thread's four factors (image S[k = t][i = factor])
    const int k = t >> 4, j0 = (t & 15) * 4;
    int cj[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      cj[e] = j0 + e < kc ? min(max(col[(int64_t)b * kmax + j0 + e], 0), ldv - 1) : -1;
    auto load_vec = [&](double (&v)[4], int k0) {
      const int kk = k0 + k;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (kk < T && cj[e] >= 0) ? Vb[(int64_t)kk * ldv + cj[e]] : 0.0;
    };
    double va[4], vb[4];
    load_vec(va, 0);
    load_win(vb, panel, ldp, n, rw, T, 0, c0, m);
    store_win(va, smem);
    store_win(vb, smem + STAGE);
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < T; k0 += KC) {
      const bool more = (k0 + KC) < T;
      if (more) {
        load_vec(va, k0 + KC);
        load_win(vb, panel, ldp, n, rw, T, k0 + KC, c0, m);
      }
      const double* SA = smem + buf * 2 * STAGE;
      switch (mt) {   // (uniform)
        case 1: mma_factor_rows<1>(acc, SA, SA + STAGE); break;
        case 2: mma_factor_rows<2>(acc, SA, SA + STAGE); break;
        case 3: mma_factor_rows<3>(acc, SA, SA + STAGE); break;
        default: mma_factor_rows<4>(acc, SA, SA + STAGE); break;
      }
      if (more) {
        store_win(va, smem + (buf ^ 1) * 2 * STAGE);
        store_win(vb, smem + (buf ^ 1) * 2 * STAGE + STAGE);
      }
      __syncthreads();
      buf ^= 1;
    }
  }
  const int c = c0 + w * 16 + (l & 15);
  if (c >= ldf) return;
  double* Fb = F + (int64_t)frow[b] * ldf;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = q * 16 + (l >> 4) + 4 * r;
      if (j < kc) Fb[(int64_t)j * ldf + c] = c < n ? s[(int64_t)b * kmax + j] * acc[q][r] : 0.0;
    }
}

}  // namespace pq

static const int32_t kGridY = 65535;

extern "C" int pq_window_gram_batched(const double* panel, int64_t ldp, int32_t n, const int32_t* rows,
                                      const int32_t* tlen, int32_t tmax, int32_t batch, const double* mu,
                                      int64_t mu_stride, double* G, int32_t ldg, int64_t g_stride, void* stream) {
  PQ_CHECK_ARG(panel && rows && tlen && G, "pq_window_gram_batched: null pointer");
  PQ_CHECK_ARG(n >= 1 && ldp >= n && batch >= 0, "pq_window_gram_batched: bad sizes n=%d ldp=%lld batch=%d", n,
               (long long)ldp, batch);
  PQ_CHECK_ARG(tmax >= 1 && tmax <= PQ_PCA_TMAX, "pq_window_gram_batched: tmax=%d outside 1..%d", tmax, PQ_PCA_TMAX);
  PQ_CHECK_ARG(ldg >= tmax && ldg % 64 == 0 && g_stride >= (int64_t)ldg * ldg,
               "pq_window_gram_batched: ldg must be a multiple of 64 >= tmax, g_stride >= ldg^2");
  PQ_CHECK_ARG(!mu || mu_stride >= n, "pq_window_gram_batched: mu_stride < n");
  const int nb = ldg / 64;
  for (int32_t b0 = 0; b0 < batch; b0 += kGridY) {
    const int32_t nbat = batch - b0 < kGridY ? batch - b0 : kGridY;
    hipLaunchKernelGGL(pq::k_window_gram, dim3(nb * (nb + 1) / 2, nbat), dim3(256), 0, (hipStream_t)stream, panel,
                       ldp, n, rows + (int64_t)b0 * tmax, tlen + b0, tmax, mu ? mu + (int64_t)b0 * mu_stride : nullptr,
                       mu_stride, G + (int64_t)b0 * g_stride, ldg, g_stride);
    PQ_CHECK_LAUNCH("pq_window_gram_batched");
  }
  return 0;
}

extern "C" int pq_window_project_batched(const double* panel, int64_t ldp, int32_t n, const int32_t* rows,
                                         const int32_t* tlen, int32_t tmax, int32_t batch, const double* mu,
                                         int64_t mu_stride, const double* V, int32_t ldv, int64_t v_stride,
                                         const int32_t* col, const double* s, const int32_t* kcnt, int32_t kmax,
                                         const int32_t* frow, double* F, int64_t ldf, void* stream) {
  PQ_CHECK_ARG(panel && rows && tlen && V && col && s && kcnt && frow && F,
               "pq_window_project_batched: null pointer");
  PQ_CHECK_ARG(n >= 1 && ldp >= n && batch >= 0, "pq_window_project_batched: bad sizes n=%d ldp=%lld batch=%d", n,
               (long long)ldp, batch);
  PQ_CHECK_ARG(tmax >= 1 && tmax <= PQ_PCA_TMAX, "pq_window_project_batched: tmax=%d outside 1..%d", tmax,
               PQ_PCA_TMAX);
  PQ_CHECK_ARG(kmax >= 1 && kmax <= PQ_PCA_KMAX, "pq_window_project_batched: kmax=%d outside 1..%d", kmax,
               PQ_PCA_KMAX);
  PQ_CHECK_ARG(ldv >= tmax && v_stride >= (int64_t)ldv * ldv,
               "pq_window_project_batched: ldv must be >= tmax, v_stride >= ldv^2");
  PQ_CHECK_ARG(ldf >= n && ldf <= ((int64_t)1 << 30), "pq_window_project_batched: ldf=%lld must be >= n=%d",
               (long long)ldf, n);
  PQ_CHECK_ARG(!mu || mu_stride >= n, "pq_window_project_batched: mu_stride < n");
  for (int32_t b0 = 0; b0 < batch; b0 += kGridY) {
    const int32_t nbat = batch - b0 < kGridY ? batch - b0 : kGridY;
    hipLaunchKernelGGL(pq::k_window_project, dim3((unsigned)((ldf + 63) / 64), nbat), dim3(256), 0,
                       (hipStream_t)stream, panel, ldp, n, rows + (int64_t)b0 * tmax, tlen + b0, tmax,
                       mu ? mu + (int64_t)b0 * mu_stride : nullptr, mu_stride, V + (int64_t)b0 * v_stride, ldv,
                       v_stride, col + (int64_t)b0 * kmax, s + (int64_t)b0 * kmax, kcnt + b0, kmax, frow + b0, F, ldf);
    PQ_CHECK_LAUNCH("pq_window_project_batched");
  }
  return 0;
}
