// Gerber covariance (Gerber, Markowitz, Ernst, Miao, Javid, Sargen 2022): co-movement counts of
// every date on the int8 matrix cores.
//
// With s_tk in {-1, 0, +1} the sign of asset k's move on day t beyond h_k = c sd_k (raw returns
// against the window's own standard deviation), the co-movement matrix N^UU + N^DD - N^UD - N^DU
// is H = S'S, an integer Gram of an int8 panel, and the count of days on which both assets move is
// P = |S|'|S|.  k_gerber_sign thresholds the window and writes the signs asset-major
// (St[b][k][t], pitch Tp = round_up(tmax, 64), zeros past the window: a zero row is neutral in
// both Grams), so that a lane's MFMA fragment is one 16-byte load of 16 consecutive t of one
// asset; k_gerber_gram forms H (variant 1: and P, |s| being byte & 1) per 64 x 64 output tile
// with v_mfma_i32_16x16x64_i8 and applies the FP64 epilogue.  Both operands of a Gram are read
// with the same k mapping inside the instruction, so the order of the 64 k values of a fragment
// does not matter; the C/D map is the 16 x 16 one of the f32 forms (col = lane & 15,
// row = 4 (lane >> 4) + reg).  The counts are exact, and so every tile is computed on its own:
// a_i a_j and sd_i sd_j commute bit for bit, which makes the output symmetric bit for bit without
// a transposed store.
#include "common.h"
#include "capi_util.h"

namespace pq {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int GB_TILE = 64;    // assets per column block of the sign kernel, output tile edge of the Gram
constexpr int GB_PITCH = 68;   // bytes per asset row of the LDS transpose tile (17 words: conflict-free column writes)

__device__ __forceinline__ int gerber_len(const int32_t* tlen, int b, int tmax) { return min(max(tlen[b], 0), tmax); }

// sd_k = sqrt(dg_k / (T - 1)): the one expression both kernels (and the model) use
__device__ __forceinline__ double gerber_sd(double dg, int T) { return sqrt(dg / (double)(T - 1)); }

// One workgroup per (64 assets, date).  Thread t reads column c0 + (t & 63) of the rows
// (t >> 6) + 4 i of a 64-row chunk (coalesced along the assets), the signs go through an LDS tile
// [asset][t], and thread t then stores the 16 bytes (t & 3) of asset t >> 2.
__global__ __launch_bounds__(256) void k_gerber_sign(const double* panel, int64_t ldp, int n, const int32_t* rows,
                                                     const int32_t* tlen, int tmax, const double* dg,
                                                     int64_t dg_stride, double thr, int8_t* St, int ldk, int Tp,
                                                     int32_t* counts, int64_t ldc, int32_t* status) {
  __shared__ __attribute__((aligned(16))) int8_t tile[GB_TILE * GB_PITCH];
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * GB_TILE;
  const int T = gerber_len(tlen, b, tmax);
  const int32_t* rw = rows + (int64_t)b * tmax;
  const int tid = threadIdx.x;
  const int col = tid & 63, rsub = tid >> 6;
  const int c = c0 + col;
  bool bad = T < 2;
  double h = 0.0;
  if (c < n) {
    const double d = dg[(int64_t)b * dg_stride + c];
    if (!(d > 0.0) || !isfinite(d)) bad = true;
    h = thr * gerber_sd(d, T);
  }
  const int k = tid >> 2, seg = tid & 3;
  int8_t* dst = St + ((int64_t)b * ldk + c0 + k) * Tp + 16 * seg;
  int cnt = 0;
  for (int t0 = 0; t0 < Tp; t0 += GB_TILE) {
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int tl = rsub + 4 * i;
      int8_t s = 0;
      if (t0 + tl < T && c < n) {
        const double x = panel[(int64_t)rw[t0 + tl] * ldp + c];
        if (!isfinite(x)) bad = true;
        s = x >= h ? 1 : (x <= -h ? -1 : 0);
      }
      tile[col * GB_PITCH + tl] = s;
    }
    __syncthreads();
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tile + k * GB_PITCH + 16 * seg);
    i32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t wd = src[j];
      cnt += __popc(wd & 0x01010101u);
      v[j] = (int)wd;
    }
    *reinterpret_cast<i32x4*>(dst + t0) = v;
    __syncthreads();
  }
  cnt += __shfl_xor(cnt, 1);
  cnt += __shfl_xor(cnt, 2);
  if (seg == 0 && c0 + k < ldc) counts[(int64_t)b * ldc + c0 + k] = c0 + k < n ? cnt : 0;
  if (c0 + k < n && cnt == 0) bad = true;
  if (bad) status[b] = PQ_GERBER_BAD_INPUT;   // (every writer stores the same value)
}

// One workgroup per (64 x 64 output tile, date); wave w owns the rows [16 w, 16 w + 16) of the
// tile and its four 16-column blocks.  The fragments come straight from St (n Tp bytes per date,
// resident in L2): lane l holds the 16 bytes k0 + 16 (l >> 4) .. of asset (l & 15) of its block.
template <int VARIANT>
__global__ __launch_bounds__(256) void k_gerber_gram(const int8_t* St, int ldk, int Tp, int n, const int32_t* tlen,
                                                     int tmax, const double* dg, int64_t dg_stride,
                                                     const int32_t* counts, int64_t ldc, const int32_t* status,
                                                     int corr, double* out, int ld, int64_t out_stride) {
  const int b = blockIdx.y;
  const int nt = (n + GB_TILE - 1) / GB_TILE;
  const int I = blockIdx.x / nt, J = blockIdx.x % nt;
  const int l = lane_id(), w = wave_id();
  const int i0 = I * GB_TILE + 16 * w + 4 * (l >> 4);   // + reg: this lane's rows
  const int j0 = J * GB_TILE + (l & 15);                // + 16 q: this lane's columns
  double* o = out + (int64_t)b * out_stride;
  if (status[b] != PQ_GERBER_OK) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (i0 + r < n && j0 + 16 * q < n) o[(int64_t)(i0 + r) * ld + j0 + 16 * q] = nan;
    return;
  }
  const int T = gerber_len(tlen, b, tmax);
  const int Tk = (T + 63) & ~63;   // <= Tp; the signs past T are zero
  const int8_t* sb = St + (int64_t)b * ldk * Tp + 16 * (l >> 4);
  const int8_t* pa = sb + (int64_t)(I * GB_TILE + 16 * w + (l & 15)) * Tp;
  const int8_t* pb = sb + (int64_t)(J * GB_TILE + (l & 15)) * Tp;
  const i32x4 zero = {0, 0, 0, 0};
  const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
  i32x4 H[4] = {zero, zero, zero, zero}, P[4] = {zero, zero, zero, zero};
  for (int k0 = 0; k0 < Tk; k0 += 64) {
    const i32x4 a = *reinterpret_cast<const i32x4*>(pa + k0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const i32x4 bv = *reinterpret_cast<const i32x4*>(pb + (int64_t)16 * q * Tp + k0);
      H[q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bv, H[q], 0, 0, 0);
      if (VARIANT == 1) P[q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a & ones, bv & ones, P[q], 0, 0, 0);
    }
  }
  const double* dgb = dg + (int64_t)b * dg_stride;
  const int32_t* ab = counts + (int64_t)b * ldc;
  int ai[4], aj[4];
  double si[4], sj[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool in = i0 + r < n;
    ai[r] = in ? ab[i0 + r] : 1;
    si[r] = in ? gerber_sd(dgb[i0 + r], T) : 0.0;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool in = j0 + 16 * q < n;
    aj[q] = in ? ab[j0 + 16 * q] : 1;
    sj[q] = in ? gerber_sd(dgb[j0 + 16 * q], T) : 0.0;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (i0 + r >= n || j0 + 16 * q >= n) continue;
      double g;
      if (VARIANT == 1)   // T - N^NN = a_i + a_j - P_ij, in integers (>= 1 on a valid date)
        g = (double)H[q][r] / (double)(ai[r] + aj[q] - P[q][r]);
      else
        g = (double)H[q][r] / sqrt((double)ai[r] * (double)aj[q]);
      o[(int64_t)(i0 + r) * ld + j0 + 16 * q] = corr ? g : g * (si[r] * sj[q]);
    }
}

}  // namespace pq

static const int32_t kGridY = 65535;

extern "C" int pq_gerber_cov_batched(const double* panel, int64_t ldp, int32_t n, const int32_t* rows,
                                     const int32_t* tlen, int32_t tmax, int32_t batch, const double* dg,
                                     int64_t dg_stride, double threshold, int32_t variant, int32_t corr,
                                     int32_t stages, int8_t* St, int32_t* counts, int64_t ldc, double* out,
                                     int32_t ld, int64_t out_stride, int32_t* status, void* stream) {
  PQ_CHECK_ARG(panel && rows && tlen && dg && St && counts && out && status, "pq_gerber_cov_batched: null pointer");
  PQ_CHECK_ARG(n >= 1 && ldp >= n && batch >= 0, "pq_gerber_cov_batched: bad sizes n=%d ldp=%lld batch=%d", n,
               (long long)ldp, batch);
  PQ_CHECK_ARG(tmax >= 1 && tmax <= PQ_GERBER_TMAX, "pq_gerber_cov_batched: tmax=%d outside 1..%d", tmax,
               PQ_GERBER_TMAX);
  PQ_CHECK_ARG(variant == 1 || variant == 2, "pq_gerber_cov_batched: variant=%d is not 1 or 2", variant);
  PQ_CHECK_ARG(threshold > 0.0 && threshold <= 1.0, "pq_gerber_cov_batched: threshold=%g outside (0, 1]", threshold);
  PQ_CHECK_ARG(stages >= 1 && stages <= 3, "pq_gerber_cov_batched: stages=%d outside 1..3", stages);
  PQ_CHECK_ARG(dg_stride >= n && ldc >= n && ld >= n && out_stride >= (int64_t)(n - 1) * ld + n,
               "pq_gerber_cov_batched: dg_stride, ldc and ld must be >= n=%d, out_stride >= (n - 1) ld + n", n);
  hipStream_t strm = (hipStream_t)stream;
  const int ldk = (n + 63) / 64 * 64, Tp = (tmax + 63) / 64 * 64;
  const int nt = ldk / 64;
  if (batch == 0) return 0;
  if (stages & 1) PQ_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)batch * sizeof(int32_t), strm));
  for (int32_t b0 = 0; b0 < batch; b0 += kGridY) {
    const int32_t nbat = batch - b0 < kGridY ? batch - b0 : kGridY;
    int8_t* Sb = St + (int64_t)b0 * ldk * Tp;
    if (stages & 1) {
      hipLaunchKernelGGL(pq::k_gerber_sign, dim3(nt, nbat), dim3(256), 0, strm, panel, ldp, n,
                         rows + (int64_t)b0 * tmax, tlen + b0, tmax, dg + (int64_t)b0 * dg_stride, dg_stride, threshold,
                         Sb, ldk, Tp, counts + (int64_t)b0 * ldc, ldc, status + b0);
      PQ_CHECK_LAUNCH("pq_gerber_cov_batched (signs)");
    }
    if (stages & 2) {
      auto kern = variant == 1 ? pq::k_gerber_gram<1> : pq::k_gerber_gram<2>;
      hipLaunchKernelGGL(kern, dim3(nt * nt, nbat), dim3(256), 0, strm, (const int8_t*)Sb, ldk, Tp, n, tlen + b0, tmax,
                         dg + (int64_t)b0 * dg_stride, dg_stride, (const int32_t*)(counts + (int64_t)b0 * ldc), ldc,
                         (const int32_t*)(status + b0), corr, out + (int64_t)b0 * out_stride, ld, out_stride);
      PQ_CHECK_LAUNCH("pq_gerber_cov_batched (gram)");
    }
  }
  return 0;
}
