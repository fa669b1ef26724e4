// Exponentially weighted covariance (RiskMetrics 1996; np.cov(aweights=), pandas'
// ewm(adjust=True).cov(bias=False)) of every date on FP64 MFMA, direct and sliding.
//
// A window of T rows x_0 .. x_{T-1}, oldest first, weights its rows by their age k = T-1-j with
// a table built on the host, w_j = wage[T-1-j] (the kernels never form a power themselves):
//     W1 = sum w,  W2 = sum w^2,  m = sum w_j x_j / W1,
//     Sigma = sum_j w_j (x_j - m)(x_j - m)' / (W1 - W2 / W1).
// k_ewma_moments computes m, W1 and the denominator once per date (one thread per column, the
// table summed in one fixed order, so every tile of a date scales by the same bits) and the
// date's status.  k_ewma_syrk is k_syrk with weighted rows: one 256-thread workgroup per lower
// 64x64 tile and date.  k_ewma_syrk_slide is k_syrk_slide with a decaying recursion: the anchor
// of a slide group is a full weighted SYRK shifted by its own mean c, a later date whose window
// moved by s rows is
//     A <- wage[s] A + sum_{entering, age k < s} wage[k] (x - c)(x - c)'
//                    - sum_{leaving, old position j < s} wage[s] wage[T-1-j] (x - c)(x - c)'
// as one MFMA pass over the [entering; -leaving] operand, emitted as
//     Sigma_d = (A - W1 (m_d - c)(m_d - c)') / (W1 - W2 / W1)
// through the LDS tile with 16-byte row stores: 2 s n^2 flops per date, 8 n^2 bytes written.
// The decay contracts the rounding error of the recursion.
//
// Symmetry: BOTH MFMA operands carry sqrt(w) (IEEE sqrt of the table entry, correctly rounded,
// taken once per call by k_ewma_sqrt_table; a leaving row carries sqrt(wage[s]) sqrt(w_old)).
// Inside a diagonal tile the A and B images then hold the same numbers, so element (i, j) and
// element (j, i) are the same products summed in the same order; off-diagonal tiles are written
// as the tile and its transpose.  Weighting one operand by w would round (w x_i) x_j and
// (w x_j) x_i differently.  The leaving rows carry -sqrt(w) on the A side only, and the
// correction is W1 * (d_i d_j) with the product formed first, so S == S' bit for bit.
#include "common.h"
#include "capi_util.h"
#include "win_tile.h"

namespace pq {

constexpr int EW_SP = 65;   // pitch of the LDS output tile

__device__ __forceinline__ int ewma_len(const int32_t* tlen, int b, int tmax) { return min(max(tlen[b], 0), tmax); }

// wsqrt[k] = sqrt(wage[k]): what both operands of a staged row are scaled by
__global__ __launch_bounds__(256) void k_ewma_sqrt_table(const double* __restrict__ wage, double* __restrict__ wsqrt,
                                                         int len) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < len) wsqrt[k] = sqrt(wage[k]);
}

// Weighted mean, (W1, W1 - W2 / W1) and the status of every date.  Ages count from the window's
// own end, so a partial window (tlen < tmax) uses the head of the table.
__global__ __launch_bounds__(256) void k_ewma_moments(const double* panel, int64_t ldp, int n, const int32_t* rows,
                                                      const int32_t* tlen, int tmax, const double* wage, double* mean,
                                                      int64_t mean_stride, int ldm, double* wsum, int32_t* status) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ldm) return;
  const int T = ewma_len(tlen, b, tmax);
  const int32_t* rw = rows + (int64_t)b * tmax;
  double W1 = 0.0, W2 = 0.0;
  for (int k = 0; k < T; ++k) {   // the same order in every thread: one value per date
    const double w = wage[k];
    W1 += w;
    W2 = fma(w, w, W2);
  }
  const double den = W1 - W2 / W1;
  bool bad = T < 2 || !(den > 0.0) || !isfinite(den);
  double m = 0.0;
  if (j < n) {
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < T; ++k) {
      const double x = panel[(int64_t)rw[k] * ldp + j];
      if (!isfinite(x)) bad = true;
      s = fma(wage[T - 1 - k], x, s);
    }
    m = s / W1;
  }
  mean[(int64_t)b * mean_stride + j] = m;
  if (j == 0) {
    wsum[2 * (int64_t)b] = W1;
    wsum[2 * (int64_t)b + 1] = den;
  }
  if (bad) status[b] = PQ_EWMA_BAD_INPUT;   // (every writer stores the same value)
}

// acc = sum_j w_j (x_j - c)(x_j - c)' over the window rw[0, T) for the tile (i0, j0): k_syrk's
// double-buffered loop, each staged row scaled by sqrt(w_j) on both sides
__device__ __forceinline__ void ewma_window_syrk(Acc& acc, double* smem, const double* panel, int64_t ldp, int n,
                                                 const int32_t* rw, int T, int i0, int j0, const double* c,
                                                 const double* wsqrt) {
  const int k = threadIdx.x >> 4;
  auto stage = [&](double (&va)[4], double (&vb)[4], int k0) {
    load_win(va, panel, ldp, n, rw, T, k0, i0, c);
    load_win(vb, panel, ldp, n, rw, T, k0, j0, c);
    const int kk = k0 + k;
    const double sw = kk < T ? wsqrt[T - 1 - kk] : 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      va[e] *= sw;
      vb[e] *= sw;
    }
  };
  acc.zero();
  double va[4], vb[4];
  stage(va, vb, 0);
  store_win(va, smem);
  store_win(vb, smem + STAGE);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < T; k0 += KC) {
    const bool more = (k0 + KC) < T;
    if (more) stage(va, vb, k0 + KC);
    mma_lds(acc, smem + buf * 2 * STAGE, smem + buf * 2 * STAGE + STAGE, KC);
    if (more) {
      store_win(va, smem + (buf ^ 1) * 2 * STAGE);
      store_win(vb, smem + (buf ^ 1) * 2 * STAGE + STAGE);
    }
    __syncthreads();
    buf ^= 1;
  }
}

// a bad date's tile: NaN inside [0, n) x [0, n), zero in the padding
__device__ __forceinline__ void ewma_bad_tile(Acc& acc, int n, int i0, int j0) {
  const double qnan = __builtin_nan("");
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc.c[m][nn][r] = (i0 + acc_row(m, r) < n && j0 + acc_col(nn) < n) ? qnan : 0.0;
}

__global__ __launch_bounds__(256) void k_ewma_syrk(const double* __restrict__ panel, int64_t ldp, int n,
                                                   const int32_t* __restrict__ rows, const int32_t* __restrict__ tlen,
                                                   int tmax, const double* __restrict__ wsqrt,
                                                   const double* __restrict__ mean, int64_t mean_stride,
                                                   const double* __restrict__ wsum, const int32_t* __restrict__ status,
                                                   double* __restrict__ out, int ld, int64_t out_stride) {
  __shared__ __attribute__((aligned(16))) double smem[4 * STAGE];
  const int b = blockIdx.y;
  int I, J;
  tri_index(blockIdx.x, I, J);
  Acc acc;
  if (status[b] != PQ_EWMA_OK) {
    ewma_bad_tile(acc, n, I * TB, J * TB);
  } else {
    const int T = ewma_len(tlen, b, tmax);
    ewma_window_syrk(acc, smem, panel, ldp, n, rows + (int64_t)b * tmax, T, I * TB, J * TB,
                     mean + (int64_t)b * mean_stride, wsqrt);
    const double sc = 1.0 / wsum[2 * (int64_t)b + 1];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn) acc.c[m][nn] *= sc;
  }
  double* o = out + (int64_t)b * out_stride;
  acc_store(acc, o, ld, I * TB, J * TB);
  if (I != J) acc_store_T(acc, o, ld, J * TB, I * TB);
}

// one 16-row operand chunk of a slide: rows k < na enter (age s - 1 - (k0 + k), weight
// wage[age]), rows na <= k < 2 na leave (old position k0 + k - na, weight wage[s] times their
// old weight, minus sign on the A side), the rest is zero; wsqrt holds the square roots
__device__ __forceinline__ void ewma_slide_load(double (&va)[4], double (&vb)[4], const double* panel, int64_t ldp,
                                                int n, const int32_t* add, const int32_t* drop, int na, int k0, int s,
                                                int T, int i0, int j0, const double* c, const double* wsqrt) {
  const int t = threadIdx.x;
  const int k = t >> 4, i = (t & 15) * 4;
  int64_t row = -1;
  double wa = 0.0, wb = 0.0;
  if (k < na) {
    row = add[k0 + k];
    wb = wsqrt[s - 1 - (k0 + k)];
    wa = wb;
  } else if (k < 2 * na) {
    row = drop[k0 + k - na];
    wb = wsqrt[s] * wsqrt[T - 1 - (k0 + k - na)];
    wa = -wb;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    double a = 0.0, b = 0.0;
    if (row >= 0) {
      const int ca = i0 + i + e, cb = j0 + i + e;
      if (ca < n) a = wa * (panel[row * ldp + ca] - c[ca]);
      if (cb < n) b = wb * (panel[row * ldp + cb] - c[cb]);
    }
    va[e] = a;
    vb[e] = b;
  }
}

// A date that is bad input (a non-finite row that entered its window) writes its NaN block and
// leaves the recursion: the next good date of the group is formed as a fresh anchor, exactly as
// if a group started there, so no date inherits anything from a bad one.
// What a date needs beside its rows is fetched ahead of the chain of dates: the statuses of 64
// dates at a time as one ballot, W1 and the denominator once per group (they depend on the length
// alone), the shift and decay of the next date while the current one is being written.
__global__ __launch_bounds__(256) void k_ewma_syrk_slide(
    const double* __restrict__ panel, int64_t ldp, int n, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ tlen, int tmax, const double* __restrict__ wage, const double* __restrict__ wsqrt,
    const double* __restrict__ mean, int64_t mean_stride, const double* __restrict__ wsum,
    const int32_t* __restrict__ status, double* __restrict__ out, int ld, int64_t out_stride,
    const int32_t* __restrict__ gstart, const int32_t* __restrict__ shift) {
  __shared__ __attribute__((aligned(16))) double smem[4 * STAGE + TB * EW_SP];
  double* tile = smem + 4 * STAGE;
  int I, J;
  tri_index(blockIdx.x, I, J);
  const int g = blockIdx.y;
  const int d0 = gstart[g], d1 = gstart[g + 1];
  const int T = ewma_len(tlen, d0, tmax);   // one length per group (engine.slide_plan)
  const int t = threadIdx.x;
  const double* c = nullptr;   // the shift: the mean of the last anchor
  const double W1 = wsum[2 * (int64_t)d0];
  const double sc = 1.0 / wsum[2 * (int64_t)d0 + 1];
  Acc acc;
  bool live = false;           // acc holds the shifted weighted Gram of date d - 1
  unsigned long long okmask = 0;
  int mbase = d0 - 64;
  int s_next = 0;
  double lam_next = 0.0;
  auto fetch_shift = [&](int d) {
    if (d < d1) {
      s_next = min(max(shift[d], 0), T);
      lam_next = wage[s_next];
    }
  };
  fetch_shift(d0 + 1);
  for (int d = d0; d < d1; ++d) {
    if (d - mbase >= 64) {
      mbase = d;
      const int dd = d + lane_id();
      okmask = __ballot(dd < d1 && status[dd] == PQ_EWMA_OK);
    }
    const bool ok = (okmask >> (d - mbase)) & 1ull;
    const int s = s_next;
    const double lam = lam_next;
    fetch_shift(d + 1);
    bool fresh = false;
    if (!ok) {
      live = false;
    } else if (!live) {
      // ---- anchor: the full weighted SYRK of this window, shifted by its own mean -------
      c = mean + (int64_t)d * mean_stride;
      ewma_window_syrk(acc, smem, panel, ldp, n, rows + (int64_t)d * tmax, T, I * TB, J * TB, c, wsqrt);
      live = true;
      fresh = true;
    } else {
      // ---- slide: decay, + rows entering the window, - rows leaving it (8 of each a chunk)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) acc.c[m][nn] *= lam;
      const int32_t* add = rows + (int64_t)d * tmax + (T - s);
      const int32_t* drop = rows + (int64_t)(d - 1) * tmax;
      for (int k0 = 0; k0 < s; k0 += KC / 2) {
        const int na = min(KC / 2, s - k0);
        double va[4], vb[4];
        ewma_slide_load(va, vb, panel, ldp, n, add, drop, na, k0, s, T, I * TB, J * TB, c, wsqrt);
        store_win(va, smem);
        store_win(vb, smem + STAGE);
        __syncthreads();
        mma_lds(acc, smem, smem + STAGE, (2 * na + 3) & ~3);
        __syncthreads();
      }
    }
    // ---- emit date d: centre by its own mean, scale, stage through LDS --------------------
    const double* md = mean + (int64_t)d * mean_stride;
    const double qnan = __builtin_nan("");
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = acc_row(m, r), j = acc_col(nn);
          const int gi = I * TB + i, gj = J * TB + j;
          double v;
          if (!ok) {
            v = (gi < n && gj < n) ? qnan : 0.0;
          } else {
            v = acc.c[m][nn][r];
            if (!fresh) {
              const double di = gi < n ? md[gi] - c[gi] : 0.0;
              const double dj = gj < n ? md[gj] - c[gj] : 0.0;
              v -= W1 * (di * dj);   // (di dj) first: bitwise symmetric tiles
            }
            v *= sc;
          }
          tile[i * EW_SP + j] = v;
        }
    __syncthreads();
    double* o = out + (int64_t)d * out_stride;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int idx = t + 256 * e;
      const int r = idx >> 5, c2 = (idx & 31) * 2;
      reinterpret_cast<double2*>(o + (int64_t)(I * TB + r) * ld + J * TB)[c2 >> 1] =
          double2{tile[r * EW_SP + c2], tile[r * EW_SP + c2 + 1]};
      if (I != J)
        reinterpret_cast<double2*>(o + (int64_t)(J * TB + r) * ld + I * TB)[c2 >> 1] =
            double2{tile[c2 * EW_SP + r], tile[(c2 + 1) * EW_SP + r]};
    }
    __syncthreads();
  }
}

}  // namespace pq

static const int32_t kGridY = 65535;

extern "C" int pq_ewma_cov_batched(const double* panel, int64_t ldp, int32_t n, const int32_t* rows,
                                   const int32_t* tlen, int32_t tmax, int32_t batch, const double* wage, double* wsqrt,
                                   double* mean, int64_t mean_stride, double* wsum, double* out, int32_t ld, int64_t out_stride,
                                   int32_t* status, const int32_t* gstart, int32_t ngroups, const int32_t* shift,
                                   void* stream) {
  PQ_CHECK_ARG(panel && rows && tlen && wage && wsqrt && mean && wsum && out && status,
               "pq_ewma_cov_batched: null pointer");
  PQ_CHECK_ARG(n >= 1 && ldp >= n && batch >= 0, "pq_ewma_cov_batched: bad sizes n=%d ldp=%lld batch=%d", n,
               (long long)ldp, batch);
  PQ_CHECK_ARG(tmax >= 1 && tmax <= PQ_EWMA_TMAX, "pq_ewma_cov_batched: tmax=%d outside 1..%d", tmax, PQ_EWMA_TMAX);
  PQ_CHECK_ARG(ld >= n && ld % 64 == 0 && mean_stride >= ld && out_stride >= (int64_t)ld * ld,
               "pq_ewma_cov_batched: ld must be a multiple of 64 >= n=%d, mean_stride >= ld, out_stride >= ld^2", n);
  PQ_CHECK_ARG((gstart == nullptr) == (shift == nullptr) && ngroups >= 0,
               "pq_ewma_cov_batched: a slide plan needs gstart and shift");
  if (batch == 0) return 0;
  hipStream_t strm = (hipStream_t)stream;
  PQ_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)batch * sizeof(int32_t), strm));
  hipLaunchKernelGGL(pq::k_ewma_sqrt_table, dim3((tmax + 1 + 255) / 256), dim3(256), 0, strm, wage, wsqrt, tmax + 1);
  PQ_CHECK_LAUNCH("pq_ewma_cov_batched (table)");
  for (int32_t b0 = 0; b0 < batch; b0 += kGridY) {
    const int32_t nbat = batch - b0 < kGridY ? batch - b0 : kGridY;
    hipLaunchKernelGGL(pq::k_ewma_moments, dim3((ld + 255) / 256, nbat), dim3(256), 0, strm, panel, ldp, n,
                       rows + (int64_t)b0 * tmax, tlen + b0, tmax, wage, mean + (int64_t)b0 * mean_stride, mean_stride,
                       ld, wsum + 2 * (int64_t)b0, status + b0);
    PQ_CHECK_LAUNCH("pq_ewma_cov_batched (moments)");
  }
  const int nb = ld / 64;
  if (gstart) {
    for (int32_t g0 = 0; g0 < ngroups; g0 += kGridY) {
      const int32_t ng = ngroups - g0 < kGridY ? ngroups - g0 : kGridY;
      hipLaunchKernelGGL(pq::k_ewma_syrk_slide, dim3(nb * (nb + 1) / 2, ng), dim3(256), 0, strm, panel, ldp, n, rows,
                         tlen, tmax, wage, (const double*)wsqrt, (const double*)mean, mean_stride,
                         (const double*)wsum, (const int32_t*)status, out, ld, out_stride, gstart + g0, shift);
      PQ_CHECK_LAUNCH("pq_ewma_cov_batched (slide)");
    }
    return 0;
  }
  for (int32_t b0 = 0; b0 < batch; b0 += kGridY) {
    const int32_t nbat = batch - b0 < kGridY ? batch - b0 : kGridY;
    hipLaunchKernelGGL(pq::k_ewma_syrk, dim3(nb * (nb + 1) / 2, nbat), dim3(256), 0, strm, panel, ldp, n,
                       rows + (int64_t)b0 * tmax, tlen + b0, tmax, (const double*)wsqrt,
                       (const double*)(mean + (int64_t)b0 * mean_stride),
                       mean_stride, (const double*)(wsum + 2 * (int64_t)b0), (const int32_t*)(status + b0),
                       out + (int64_t)b0 * out_stride, ld, out_stride);
    PQ_CHECK_LAUNCH("pq_ewma_cov_batched (syrk)");
  }
  return 0;
}
