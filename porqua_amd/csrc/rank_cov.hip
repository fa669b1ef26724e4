// Rank covariance of every date: Spearman's rho and Kendall's tau-b.
//
// k_rank counts, per asset of a window, the doubled mid-ranks d_tk = 2 #{x_u < x_t} + #{x_u == x_t}
// + 1 (O(T^2) compares per column on a strip held in LDS).  For Spearman it writes the centred
// ranks c = d - (T + 1) as doubles into a date-stacked row-major panel (tmax rows per date, zero
// rows past T) whose Gram C = c'c the FP64 tile GEMM of pq_cov_batched (mode 1) forms exactly --
// integers far below 2^53 --, and k_spearman_finish applies the FP64 epilogue in place.  For
// Kendall it writes the ranks as int16, asset-major (Rk[b][k][t], pitch Tp = round_up(tmax, 64),
// zeros past the window and past n).
//
// Kendall's numerator is H = kappa'kappa with kappa_(s,t),k = sgn(x_tk - x_sk) = sgn(d_tk - d_sk),
// one row per pair of days s < t: T (T - 1) / 2 rows, about 32 KB per asset at T = 252, which is
// never stored.  k_kendall_gram keeps the two 64-asset rank strips of an output tile in LDS and
// builds the int8 fragments of v_mfma_i32_16x16x64_i8 in registers.  A k-block of 64 pairs is
// {s0 .. s0 + 15} x {t0 .. t0 + 3}, s0 a multiple of 16 and t0 of 4: the lane (asset l & 15, group
// g = l >> 4) holds the sixteen s of its asset in eight registers for the whole inner loop over t0
// and reads one rank r_t, t = t0 + g, per step; its sixteen bytes are clamp(r_t - r_s, -1, 1) by
// packed 16-bit subtract / max / min and a byte permute.  Pairs with s >= t or t >= T (only in the
// blocks on the diagonal and at the window's end) are masked to zero.  Both operands use this one
// pair-to-k map, the C/D map is the one documented in gerber.hip.  Wave w builds the B fragment
// of column block w and shares it through a double-buffered LDS slot (one barrier per k-block),
// so a k-block costs a wave two fragments for four MFMAs.  The counts are exact, so an
// off-diagonal tile stores its transpose as well and the output is symmetric bit for bit.
#include "common.h"
#include "capi_util.h"

namespace pq {

typedef int rk_i32x4 __attribute__((ext_vector_type(4)));
typedef short rk_s16x2 __attribute__((ext_vector_type(2)));

constexpr int RK_COLS = 16;   // assets per workgroup of the ranking kernel
constexpr int RK_TILE = 64;   // output tile edge of the Kendall Gram
constexpr int RK_PAD = 8;     // int16 of padding per LDS rank row: consecutive assets 4 banks apart

__device__ __forceinline__ int rank_len(const int32_t* tlen, int b, int tmax) { return min(max(tlen[b], 0), tmax); }

// sd_k = sqrt(dg_k / (T - 1)): the expression of gerber_sd
__device__ __forceinline__ double rank_sd(double dg, int T) { return sqrt(dg / (double)(T - 1)); }

__device__ __forceinline__ double rank_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// One workgroup per (16 assets, date): thread (col = tid & 15, sub = tid >> 4) ranks the days
// sub, sub + 16, ... of its column, two at a time against every day of the window.
// Dynamic LDS: tmax x 16 doubles, and for Kendall 16 x (Tp + RK_PAD) int16.
__global__ __launch_bounds__(256) void k_rank(const double* panel, int64_t ldp, int n, const int32_t* rows,
                                              const int32_t* tlen, int tmax, int kind, int16_t* Rk, int ldk, int Tp,
                                              double* Cp, int64_t ldr, double* diag, int64_t ldd, int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) double rk_lds[];
  __shared__ int sums[RK_COLS];
  double* xs = rk_lds;
  int16_t* rks = reinterpret_cast<int16_t*>(rk_lds + (size_t)tmax * RK_COLS);
  const int RP = Tp + RK_PAD;
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * RK_COLS;
  const int T = rank_len(tlen, b, tmax);
  const int32_t* rw = rows + (int64_t)b * tmax;
  const int tid = threadIdx.x;
  const int col = tid & 15, sub = tid >> 4;
  const int c = c0 + col;
  const bool in = c < n;
  bool bad = T < 2;
  for (int t = sub; t < T; t += 16) {
    const double x = in ? panel[(int64_t)rw[t] * ldp + c] : 0.0;
    if (!isfinite(x)) bad = true;
    xs[t * RK_COLS + col] = x;
  }
  if (tid < RK_COLS) sums[tid] = 0;
  __syncthreads();
  int acc = 0;   // Spearman: sum c^2 (<= (T^3 - T) / 3 < 2^26); Kendall: sum (eq - 1) (<= T (T - 1))
  auto emit = [&](int t, int lt, int le) {
    const int d = lt + le + 1;   // 2 lt + eq + 1
    if (kind == PQ_RANK_SPEARMAN) {
      const int cc = d - (T + 1);
      if (in) Cp[((int64_t)b * tmax + t) * ldr + c] = (double)cc;
      acc += cc * cc;
    } else {
      rks[col * RP + t] = in ? (int16_t)d : (int16_t)0;
      acc += le - lt - 1;
    }
  };
  for (int t = sub; t < T; t += 32) {
    const bool two = t + 16 < T;
    const double x0 = xs[t * RK_COLS + col];
    const double x1 = two ? xs[(t + 16) * RK_COLS + col] : x0;
    int lt0 = 0, le0 = 0, lt1 = 0, le1 = 0;
#pragma unroll 4
    for (int u = 0; u < T; ++u) {
      const double xu = xs[u * RK_COLS + col];
      lt0 += xu < x0;
      le0 += xu <= x0;
      lt1 += xu < x1;
      le1 += xu <= x1;
    }
    emit(t, lt0, le0);
    if (two) emit(t + 16, lt1, le1);
  }
  if (kind == PQ_RANK_SPEARMAN) {
    if (in)
      for (int t = T + sub; t < tmax; t += 16) Cp[((int64_t)b * tmax + t) * ldr + c] = 0.0;
  } else {
    for (int t = T + sub; t < Tp; t += 16) rks[col * RP + t] = 0;
  }
  atomicAdd(&sums[col], acc);   // integers: any order gives the same sum
  __syncthreads();
  if (kind == PQ_RANK_KENDALL) {
    const int vec = Tp / 8;   // 16-byte pieces per asset row
    for (int i = tid; i < RK_COLS * vec; i += 256) {
      const int a = i / vec, v = i % vec;
      *reinterpret_cast<rk_i32x4*>(Rk + ((int64_t)b * ldk + c0 + a) * Tp + 8 * v) =
          *reinterpret_cast<const rk_i32x4*>(rks + a * RP + 8 * v);
    }
  }
  if (tid < RK_COLS && c < ldd) {
    const int s = sums[tid];
    const int64_t v = kind == PQ_RANK_SPEARMAN ? (int64_t)s : ((int64_t)T * (T - 1) - s) / 2;
    diag[(int64_t)b * ldd + c] = in ? (double)v : 0.0;
    if (in && v == 0) bad = true;   // a constant column: C_kk = 0 and H_kk = 0 alike
  }
  if (bad) status[b] = PQ_RANK_BAD_INPUT;   // (every writer stores the same value)
}

// out_ij for an integer count h_ij: the count itself, g = h / sqrt(d_i d_j), or g (sd_i sd_j)
__device__ __forceinline__ double rank_entry(double h, double di, double dj, double si, double sj, int mode) {
  if (mode == PQ_RANK_COUNTS) return h;
  const double g = h / sqrt(di * dj);
  return mode == PQ_RANK_CORR ? g : g * (si * sj);
}

// Spearman's epilogue, in place on the Gram C that pq_cov_batched left in out: one workgroup per
// row of a date's block.  Rows and columns in [n, ldk) are set to zero.
__global__ __launch_bounds__(256) void k_spearman_finish(int n, int ldk, const int32_t* tlen, int tmax, const double* dg,
                                                         int64_t dg_stride, const double* diag, int64_t ldd,
                                                         const int32_t* status, int mode, double* out, int ld,
                                                         int64_t out_stride) {
  const int b = blockIdx.y, i = blockIdx.x;
  double* o = out + (int64_t)b * out_stride + (int64_t)i * ld;
  const bool ok = status[b] == PQ_RANK_OK;
  const int T = rank_len(tlen, b, tmax);
  const double* dgb = dg + (int64_t)b * dg_stride;
  const double* db = diag + (int64_t)b * ldd;
  const double di = i < n ? db[i] : 1.0;
  const double si = i < n && ok ? rank_sd(dgb[i], T) : 0.0;
  for (int j = threadIdx.x; j < ldk; j += 256) {
    if (i >= n || j >= n) {
      o[j] = 0.0;
    } else if (!ok) {
      o[j] = rank_nan();
    } else {
      o[j] = rank_entry(o[j], di, db[j], si, rank_sd(dgb[j], T), mode);
    }
  }
}

// sixteen signs clamp(r_t - r_s, -1, 1) of one asset as the bytes of a fragment, s ascending
__device__ __forceinline__ rk_i32x4 kendall_signs(int rt, const rk_i32x4& lo, const rk_i32x4& hi) {
  const int rt2i = (rt & 0xffff) | (rt << 16);
  const rk_s16x2 rt2 = __builtin_bit_cast(rk_s16x2, rt2i);
  const int one = 0x00010001, mone = -1;   // {1, 1} and {-1, -1}
  int x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int rs = j < 4 ? lo[j] : hi[j - 4];
    const int d = __builtin_bit_cast(int, rt2 - __builtin_bit_cast(rk_s16x2, rs));
    // (written out: from elementwise min / max the compiler makes compares and selects per half)
    int y;
    asm("v_pk_max_i16 %0, %1, %2\n\tv_pk_min_i16 %0, %0, %3" : "=&v"(y) : "v"(d), "v"(mone), "v"(one));
    x[j] = y;
  }
  rk_i32x4 f;
#pragma unroll
  for (int q = 0; q < 4; ++q) f[q] = (int)__builtin_amdgcn_perm((unsigned)x[2 * q + 1], (unsigned)x[2 * q], 0x06040200u);
  return f;
}

// keeps the first cnt (0..16) bytes of a fragment
__device__ __forceinline__ rk_i32x4 kendall_mask(rk_i32x4 f, int cnt) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int m = min(max(cnt - 4 * q, 0), 4);
    const unsigned mk = m >= 4 ? 0xffffffffu : ((1u << (8 * m)) - 1u);
    f[q] &= (int)mk;
  }
  return f;
}

// One workgroup per (pair of 64-asset blocks I <= J, date); wave w owns the rows [16 w, 16 w + 16)
// of the tile and its four 16-column blocks.  Dynamic LDS: the rank strips of I and J,
// 64 x (Tp + RK_PAD) int16 each, and 2 x 4 x 64 sixteen-byte B fragments (double-buffered).
__global__ __launch_bounds__(256) void k_kendall_gram(const int16_t* Rk, int ldk, int Tp, int n, const int32_t* tlen,
                                                      int tmax, const double* dg, int64_t dg_stride, const double* diag,
                                                      int64_t ldd, const int32_t* status, int mode, double* out, int ld,
                                                      int64_t out_stride) {
  extern __shared__ __attribute__((aligned(16))) double rk_lds[];
  const int b = blockIdx.y;
  const int nt = ldk / RK_TILE;
  int I = 0, J = blockIdx.x;   // the blockIdx.x-th pair of the upper triangle, row by row
  while (J >= nt - I) {
    J -= nt - I;
    ++I;
  }
  J += I;
  const int tid = threadIdx.x, l = lane_id(), w = wave_id();
  const int i0 = I * RK_TILE + 16 * w + 4 * (l >> 4);   // + reg: this lane's rows
  const int j0 = J * RK_TILE + (l & 15);                // + 16 q: this lane's columns
  double* o = out + (int64_t)b * out_stride;
  const bool ok = status[b] == PQ_RANK_OK;
  const int T = rank_len(tlen, b, tmax);
  const rk_i32x4 zero = {0, 0, 0, 0};
  rk_i32x4 H[4] = {zero, zero, zero, zero};
  if (ok) {
    const int SP = Tp + RK_PAD;
    int16_t* sA = reinterpret_cast<int16_t*>(rk_lds);
    int16_t* sB = I == J ? sA : sA + RK_TILE * SP;
    rk_i32x4* fb = reinterpret_cast<rk_i32x4*>(sA + 2 * RK_TILE * SP);
    const int vec = Tp / 8;
    const int16_t* gA = Rk + ((int64_t)b * ldk + I * RK_TILE) * Tp;
    const int16_t* gB = Rk + ((int64_t)b * ldk + J * RK_TILE) * Tp;
    for (int i = tid; i < RK_TILE * vec; i += 256) {
      const int a = i / vec, v = i % vec;
      *reinterpret_cast<rk_i32x4*>(sA + a * SP + 8 * v) = *reinterpret_cast<const rk_i32x4*>(gA + (int64_t)a * Tp + 8 * v);
      if (I != J)
        *reinterpret_cast<rk_i32x4*>(sB + a * SP + 8 * v) = *reinterpret_cast<const rk_i32x4*>(gB + (int64_t)a * Tp + 8 * v);
    }
    __syncthreads();
    const int g = l >> 4;
    const int16_t* ra = sA + (16 * w + (l & 15)) * SP;
    const int16_t* rb = sB + (16 * w + (l & 15)) * SP;
    int step = 0;
    for (int s0 = 0; s0 + 1 < T; s0 += 16) {   // (s0 + 16 <= Tp: the strips hold zeros past T)
      const rk_i32x4 alo = *reinterpret_cast<const rk_i32x4*>(ra + s0), ahi = *reinterpret_cast<const rk_i32x4*>(ra + s0 + 8);
      const rk_i32x4 blo = *reinterpret_cast<const rk_i32x4*>(rb + s0), bhi = *reinterpret_cast<const rk_i32x4*>(rb + s0 + 8);
      int rtA = ra[s0 + g], rtB = rb[s0 + g];
      for (int t0 = s0; t0 < T; t0 += 4, ++step) {
        const int t = t0 + g;   // < Tp
        rk_i32x4 fB = kendall_signs(rtB, blo, bhi);
        rk_i32x4 fA = I == J ? fB : kendall_signs(rtA, alo, ahi);
        const int tn = min(t + 4, Tp - 1);   // the next block's ranks, in flight across the barrier
        rtA = ra[tn];
        rtB = rb[tn];
        if (t0 < s0 + 16 || t0 + 4 > T) {   // a block on the diagonal or at the window's end: pairs s < t < T only
          const int cnt = t < T ? min(max(t - s0, 0), 16) : 0;
          fB = kendall_mask(fB, cnt);
          fA = kendall_mask(fA, cnt);
        }
        rk_i32x4* slot = fb + (step & 1) * 256;
        slot[w * 64 + l] = fB;
        __syncthreads();   // the other slot is rewritten only after the next barrier, past every read of it
#pragma unroll
        for (int q = 0; q < 4; ++q) H[q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fA, slot[q * 64 + l], H[q], 0, 0, 0);
      }
    }
  }
  const double* dgb = dg + (int64_t)b * dg_stride;
  const double* db = diag + (int64_t)b * ldd;
  double di[4], dj[4], si[4], sj[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool in = ok && i0 + r < n;
    di[r] = in ? db[i0 + r] : 1.0;
    si[r] = in ? rank_sd(dgb[i0 + r], T) : 0.0;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool in = ok && j0 + 16 * q < n;
    dj[q] = in ? db[j0 + 16 * q] : 1.0;
    sj[q] = in ? rank_sd(dgb[j0 + 16 * q], T) : 0.0;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + r, j = j0 + 16 * q;   // < ldk <= ld
      double v = 0.0;                          // rows and columns in [n, ldk)
      if (i < n && j < n) v = ok ? rank_entry((double)H[q][r], di[r], dj[q], si[r], sj[q], mode) : rank_nan();
      o[(int64_t)i * ld + j] = v;
      if (I != J) o[(int64_t)j * ld + i] = v;
    }
}

constexpr size_t rank_lds_bytes(int kind, int tmax, int Tp) {
  return (size_t)tmax * RK_COLS * sizeof(double) + (kind == PQ_RANK_KENDALL ? (size_t)RK_COLS * (Tp + RK_PAD) * 2 : 0);
}
constexpr size_t kendall_lds_bytes(int Tp) { return (size_t)2 * RK_TILE * (Tp + RK_PAD) * 2 + 2 * 4 * 64 * 16; }
static_assert(rank_lds_bytes(PQ_RANK_KENDALL, PQ_RANK_TMAX, PQ_RANK_TMAX) <= 160 * 1024, "the ranking strip must fit the LDS");
static_assert(kendall_lds_bytes(PQ_RANK_TMAX) <= 160 * 1024, "two rank strips of PQ_RANK_TMAX days must fit the LDS");

}  // namespace pq

static const int32_t kRankGridY = 65535;

extern "C" int pq_rank_cov_batched(const double* panel, int64_t ldp, int32_t n, const int32_t* rows,
                                   const int32_t* tlen, int32_t tmax, int32_t batch, const double* dg,
                                   int64_t dg_stride, int32_t kind, int32_t mode, int32_t stages, void* scratch,
                                   int64_t ldr, double* diag, int64_t ldd, double* out, int32_t ld,
                                   int64_t out_stride, int32_t* status, void* stream) {
  PQ_CHECK_ARG(panel && rows && tlen && dg && scratch && diag && out && status, "pq_rank_cov_batched: null pointer");
  PQ_CHECK_ARG(n >= 1 && ldp >= n && batch >= 0, "pq_rank_cov_batched: bad sizes n=%d ldp=%lld batch=%d", n,
               (long long)ldp, batch);
  PQ_CHECK_ARG(tmax >= 1 && tmax <= PQ_RANK_TMAX, "pq_rank_cov_batched: tmax=%d outside 1..%d", tmax, PQ_RANK_TMAX);
  PQ_CHECK_ARG(kind == PQ_RANK_SPEARMAN || kind == PQ_RANK_KENDALL, "pq_rank_cov_batched: unknown kind %d", kind);
  PQ_CHECK_ARG(mode == PQ_RANK_COV || mode == PQ_RANK_CORR || mode == PQ_RANK_COUNTS,
               "pq_rank_cov_batched: unknown output mode %d", mode);
  PQ_CHECK_ARG(stages >= 1 && stages <= 3, "pq_rank_cov_batched: stages=%d outside 1..3", stages);
  PQ_CHECK_ARG(kind != PQ_RANK_SPEARMAN || stages != 3,
               "pq_rank_cov_batched: Spearman needs the Gram between its stages: call stages 1 and 2 apart");
  const int ldk = (n + 63) / 64 * 64, Tp = (tmax + 63) / 64 * 64;
  PQ_CHECK_ARG(dg_stride >= n && ldd >= n && ld >= n && ld % 64 == 0 && out_stride >= (int64_t)(ldk - 1) * ld + ldk,
               "pq_rank_cov_batched: dg_stride and ldd must be >= n=%d, ld a multiple of 64 >= n, out_stride >= "
               "(round_up(n, 64) - 1) ld + round_up(n, 64)", n);
  PQ_CHECK_ARG(kind != PQ_RANK_SPEARMAN || ldr >= n, "pq_rank_cov_batched: ldr=%lld < n=%d", (long long)ldr, n);
  hipStream_t strm = (hipStream_t)stream;
  if (batch == 0) return 0;
  const int nt = ldk / 64;
  const size_t rank_bytes = pq::rank_lds_bytes(kind, tmax, Tp), gram_bytes = pq::kendall_lds_bytes(Tp);
  if ((stages & PQ_RANK_RANKS) && rank_bytes > 48 * 1024)
    PQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pq::k_rank), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)rank_bytes));
  if ((stages & PQ_RANK_FINISH) && kind == PQ_RANK_KENDALL && gram_bytes > 48 * 1024)
    PQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pq::k_kendall_gram),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)gram_bytes));
  if (stages & PQ_RANK_RANKS) PQ_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)batch * sizeof(int32_t), strm));
  for (int32_t b0 = 0; b0 < batch; b0 += kRankGridY) {
    const int32_t nbat = batch - b0 < kRankGridY ? batch - b0 : kRankGridY;
    int16_t* Rk = kind == PQ_RANK_KENDALL ? (int16_t*)scratch + (int64_t)b0 * ldk * Tp : nullptr;
    double* Cp = kind == PQ_RANK_SPEARMAN ? (double*)scratch + (int64_t)b0 * tmax * ldr : nullptr;
    const double* dgb = dg + (int64_t)b0 * dg_stride;
    double* db = diag + (int64_t)b0 * ldd;
    double* ob = out + (int64_t)b0 * out_stride;
    if (stages & PQ_RANK_RANKS) {
      hipLaunchKernelGGL(pq::k_rank, dim3(ldk / pq::RK_COLS, nbat), dim3(256), rank_bytes, strm, panel, ldp, n,
                         rows + (int64_t)b0 * tmax, tlen + b0, tmax, kind, Rk, ldk, Tp, Cp, ldr, db, ldd, status + b0);
      PQ_CHECK_LAUNCH("pq_rank_cov_batched (ranks)");
    }
    if (!(stages & PQ_RANK_FINISH)) continue;
    if (kind == PQ_RANK_KENDALL) {
      hipLaunchKernelGGL(pq::k_kendall_gram, dim3(nt * (nt + 1) / 2, nbat), dim3(256), gram_bytes, strm,
                         (const int16_t*)Rk, ldk, Tp, n, tlen + b0, tmax, dgb, dg_stride, (const double*)db, ldd,
                         (const int32_t*)(status + b0), mode, ob, ld, out_stride);
      PQ_CHECK_LAUNCH("pq_rank_cov_batched (kendall gram)");
    } else {
      hipLaunchKernelGGL(pq::k_spearman_finish, dim3(ldk, nbat), dim3(256), 0, strm, n, ldk, tlen + b0, tmax, dgb,
                         dg_stride, (const double*)db, ldd, (const int32_t*)(status + b0), mode, ob, ld, out_stride);
      PQ_CHECK_LAUNCH("pq_rank_cov_batched (spearman epilogue)");
    }
  }
  return 0;
}
