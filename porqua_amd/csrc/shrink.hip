// Shrinkage intensities (Ledoit-Wolf 2004, OAS: Chen et al. 2010) of every date's window, from
// three sums over the window's T x T Gram K = Xc Xc' (centred) or X X' (uncentred):
//   a = tr K,  f = sum_st K_st^2,  g = sum_t K_tt^2
//   delta_LW  = clip((g - f/T) / (f - a^2/n), 0, 1)          (0 where the denominator is <= 0)
//   delta_OAS = min(1, (f + a^2) / ((T+1) (f - a^2/n)))      (1 where the denominator is <= 0)
// (sklearn's ledoit_wolf_shrinkage / oas through ||Xc'Xc||_F = ||Xc Xc'||_F and
// sum_t ||x_t||^4 = sum_t K_tt^2), target mean(diag S) I.  K is read from the panel's band
// Gram (pq_lr_band_gram: band[r][j] = x_{r0+r} . x_{r0+r-j}), so a date costs two passes
// over the T (T+1) / 2 doubles of its half window, served from L2 / the Infinity Cache,
// instead of T^2 n flops.
//
// One 256-thread workgroup per date.  Lane l of a wave owns the columns t = 64 cb + l; wave w
// walks the rows s = w, w + 4, ... (NR of them in flight) and reads G_st = band[w_s][w_s - w_t]
// for t <= s: along a band row, so the 64 lanes of a load read one contiguous (decreasing-lag)
// piece of it, 8 B per lane (the piece's 16-byte alignment alternates from row to row and
// breaks at every calendar gap, so a wider load per lane has no fixed column to own).
// Every element feeds the row sum of s (a per-lane partial, one wave reduction per row) and
// the column sum of t (a register of the owning lane); the half below the diagonal is never
// walked in the strided direction.  Pass 1: c_s = (1/T) sum_t G_st into LDS; pass 2: a, f, g
// from the centred entries (G_st - c_s - c_t) + cbar themselves (the expanded square
// cancels).  No floating-point atomics and a fixed reduction order: bit-reproducible.
#include "common.h"
#include "capi_util.h"

namespace pq {

constexpr int SHR_TMAX = 1024;
constexpr int SHR_NR = 2;   // rows a wave keeps in flight (4: 0.37 ms against 0.34 at T = 252, 4749 dates)

// what the kernel found wrong with a date's row table (the largest code of a batch is reported)
enum { SHR_OK = 0, SHR_TLEN = 1, SHR_ROW_RANGE = 2, SHR_ROW_ORDER = 3, SHR_SPAN = 4 };

__device__ int g_shrink_flag;

// NCB: column blocks of 64 the lanes hold accumulators for (tmax <= 64 NCB)
template <int NCB>
__global__ __launch_bounds__(256) void k_shrink_stats(const double* __restrict__ band, int64_t ldo, int r0,
                                                      int nrows, int W, const int32_t* __restrict__ rows,
                                                      int64_t ld_rows, const int32_t* __restrict__ tlen,
                                                      int tmax, double n_assets, int centred, int kind,
                                                      double* __restrict__ stats) {
  constexpr int NR = SHR_NR;
  __shared__ int s_w[64 * NCB];          // window rows relative to r0
  __shared__ double s_c[64 * NCB];       // row parts, then the centring terms c_s
  __shared__ double s_col[4][64 * NCB];  // column parts of the four waves
  __shared__ double red[16];
  const int b = xcd_slot(blockIdx.x, gridDim.x);
  const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(wave_id()), l = lane_id();
  const int T = tlen[b];
  double* out = stats + (int64_t)b * 4;

  // ---- the row table: nothing below reads the band unless every index is inside it ------
  int bad = (T < 1 || T > tmax) ? SHR_TLEN : SHR_OK;
  if (!bad) {
    const int32_t* rw = rows + (int64_t)b * ld_rows;
    for (int a = t; a < T; a += 256) {
      const int r = rw[a];
      if (r < r0 || r - r0 >= nrows) bad = max(bad, (int)SHR_ROW_RANGE);
      else if (a > 0 && r <= rw[a - 1]) bad = max(bad, (int)SHR_ROW_ORDER);
      s_w[a] = r - r0;
    }
    if (t == 0 && !bad && (int64_t)rw[T - 1] - rw[0] + 1 > W) bad = SHR_SPAN;
  }
  bad = (int)block_max((double)bad, red);   // (its barriers also publish s_w)
  if (bad) {   // (uniform)
    if (t < 4) out[t] = __builtin_nan("");
    if (t == 0) atomicMax(&g_shrink_flag, bad);
    return;
  }

  // the lane's columns t = 64 cb + l: their window rows (0 past the window: such a lane is
  // masked wherever it would be read)
  int wt[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) wt[cb] = cb * 64 + l < T ? s_w[cb * 64 + l] : 0;

  // The NR rows a wave has in flight, s + 4 i: row s reads G_st = band[w_s][w_s - w_t] of the
  // lane's column in every block up to the diagonal's, db = s / 64 -- a scalar row base plus a
  // 32-bit lane offset; blocks left of db need no lane mask, blocks right of it no work at all
  // (all wave-uniform branches).  v is 0 where nothing is read.
  auto load_rows = [&](int s, double (&v)[NR][NCB]) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int si = s + 4 * i;
      const bool live = si < T;
      const int ws = live ? __builtin_amdgcn_readfirstlane(s_w[si]) : 0;
      const char* rowp = reinterpret_cast<const char*>(band + (int64_t)ws * ldo);
      const int db = si >> 6;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        v[i][cb] = 0.0;
        if (live && cb <= db) {
          const unsigned off = (unsigned)(ws - wt[cb]) * 8u;
          if (cb < db || cb * 64 + l <= si) v[i][cb] = *reinterpret_cast<const double*>(rowp + off);
        }
      }
    }
  };

  // ---- pass 1: row sums ---------------------------------------------------------------
  double cbar = 0.0;
  double ct[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) ct[cb] = 0.0;
  if (centred) {
    double col[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) col[cb] = 0.0;
    for (int s = w; s < T; s += 4 * NR) {
      double v[NR][NCB], r[NR];
      load_rows(s, v);
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const int si = s + 4 * i, db = si >> 6;
        r[i] = 0.0;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          if (cb > db) continue;
          r[i] += v[i][cb];
          // the diagonal element belongs to the row part only
          col[cb] += (cb < db || cb * 64 + l < si) ? v[i][cb] : 0.0;
        }
      }
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        if (s + 4 * i >= T) continue;
        r[i] = wave_sum(r[i]);
        if (l == 0) s_c[s + 4 * i] = r[i];
      }
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) s_col[w][cb * 64 + l] = col[cb];
    __syncthreads();
    double part = 0.0;
    for (int a = t; a < T; a += 256) {   // c_a = (row part + column parts) / T, each slot by one thread
      const double c = (s_c[a] + ((s_col[0][a] + s_col[1][a]) + (s_col[2][a] + s_col[3][a]))) / T;
      s_c[a] = c;
      part += c;
    }
    cbar = block_sum(part, red) / T;   // (its barriers also publish s_c)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) ct[cb] = cb * 64 + l < T ? s_c[cb * 64 + l] : 0.0;
  }

  // ---- pass 2: a, f, g from the centred entries -----------------------------------------
  // (uncentred: c_s = c_t = cbar = 0 and (G - 0 - 0) + 0 is G exactly)
  double tr = 0.0, dsq = 0.0, osq = 0.0;   // sum K_tt, sum K_tt^2, sum_{s > t} K_st^2
  for (int s = w; s < T; s += 4 * NR) {
    double v[NR][NCB];
    load_rows(s, v);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int si = s + 4 * i, db = si >> 6;
      if (si >= T) continue;
      const double cs = centred ? s_c[si] : 0.0;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        if (cb > db) continue;
        const double k = (v[i][cb] - cs - ct[cb]) + cbar;
        if (cb < db) {
          osq += k * k;
        } else {
          const int tc = cb * 64 + l;
          osq += tc < si ? k * k : 0.0;
          tr += tc == si ? k : 0.0;
          dsq += tc == si ? k * k : 0.0;
        }
      }
    }
  }
  const double a = block_sum(tr, red);
  const double g = block_sum(dsq, red);
  const double f = g + 2.0 * block_sum(osq, red);
  if (t == 0) {
    const double Td = (double)T;
    const double den = f - a * a / n_assets;
    double delta;
    if (kind == 0) {
      delta = den > 0.0 ? fmin(fmax((g - f / Td) / den, 0.0), 1.0) : 0.0;
    } else {
      delta = den > 0.0 ? fmin((f + a * a) / ((Td + 1.0) * den), 1.0) : 1.0;
    }
    out[0] = a;
    out[1] = f;
    out[2] = g;
    out[3] = delta;
  }
}

}  // namespace pq

extern "C" int pq_shrink_stats_band(const double* band, int64_t ldo, int32_t r0, int32_t nrows, int32_t W,
                                    const int32_t* rows, int64_t ld_rows, const int32_t* tlen, int32_t tmax,
                                    int32_t batch, int32_t n, int32_t centred, int32_t kind, double* stats,
                                    void* stream) {
  PQ_CHECK_ARG(band && rows && tlen && stats, "pq_shrink_stats_band: null argument");
  PQ_CHECK_ARG(tmax >= 1 && tmax <= pq::SHR_TMAX, "pq_shrink_stats_band: tmax outside [1, 1024]");
  PQ_CHECK_ARG(r0 >= 0 && nrows > 0 && W > 0 && ldo >= W && ld_rows >= tmax && n > 0 && batch >= 0,
               "pq_shrink_stats_band: bad arguments");
  PQ_CHECK_ARG(kind == 0 || kind == 1, "pq_shrink_stats_band: kind must be 0 (Ledoit-Wolf) or 1 (OAS)");
  if (batch == 0) return 0;
  hipStream_t str = (hipStream_t)stream;
  int* flag = nullptr;
  PQ_CHECK_HIP(hipGetSymbolAddress(reinterpret_cast<void**>(&flag), HIP_SYMBOL(pq::g_shrink_flag)));
  PQ_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int), str));
#define PQ_SHRINK(NCB)                                                                                       \
  hipLaunchKernelGGL((pq::k_shrink_stats<NCB>), dim3(batch), dim3(256), 0, str, band, ldo, r0, nrows, W, rows, \
                     ld_rows, tlen, tmax, (double)n, centred, kind, stats)
  if (tmax <= 64) PQ_SHRINK(1);
  else if (tmax <= 128) PQ_SHRINK(2);
  else if (tmax <= 256) PQ_SHRINK(4);
  else if (tmax <= 512) PQ_SHRINK(8);
  else PQ_SHRINK(16);
#undef PQ_SHRINK
  PQ_CHECK_LAUNCH("pq_shrink_stats_band");
  // the row table lives on the device: what the kernel refused comes back as one flag
  int h = 0;
  PQ_CHECK_HIP(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, str));
  PQ_CHECK_HIP(hipStreamSynchronize(str));
  static const char* const why[] = {"", "a window length outside [1, tmax]", "a window row outside [r0, r0 + nrows)",
                                    "window rows not strictly increasing", "a window spans more than W panel rows"};
  PQ_CHECK_ARG(h >= 0 && h <= 4, "pq_shrink_stats_band: bad flag");
  PQ_CHECK_ARG(h == 0, "pq_shrink_stats_band: %s (the stats of such dates are NaN)", why[h]);
  return 0;
}
