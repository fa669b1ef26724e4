// Risk-parity (risk-budgeting) portfolios of every date at once: Spinu's convex form
//   y* = argmin_{y > 0} 1/2 y' Sigma y - sum_i b_i log y_i,    x = scale y* / sum(y*)
// by cyclical coordinate descent (Griveau-Billion, Richard, Roncalli 2013) on the window form
// Sigma = a Xc'Xc + c I (Xc: the date's centred T x n window; nothing n x n is formed).  With
// d_i = a dg_i + c and s_i = (Sigma y)_i - d_i y_i each coordinate has the closed-form minimiser
//   y_i <- (-s_i + sqrt(s_i^2 + 4 d_i b_i)) / (2 d_i)        (order i = 0..n-1, start sqrt(b_i / d_i))
// and r = Xc y (a T-vector, in LDS) carries (Sigma y)_i = a x_i . r + c y_i along.
//
// One 256-thread workgroup per date.  The assets are walked 16 at a time -- the same ordered
// recurrence in exact arithmetic: the T x 16 tile Xt is staged centred into LDS (a panel row's
// 16 neighbouring assets are contiguous: coalesced row reads; zero past tlen and past n), then
//   G = a Xt'Xt (16 x 16)   FP64 MFMA 16x16x4 over T: lane l of a k-step holds Xt[4 st + (l >> 4)][l & 15],
//                           which is its A fragment and its B fragment at once (one LDS read per
//                           step, 16 lanes per tile row); the four waves split the k-steps
//   g = a Xt'r  (16)        one FMA per lane on the same fragment, folded over the lane groups
//   the serial chain        16 dependent steps on lanes 0..15 of wave 0 (lane i: asset j0 + i, the
//                           column G[.][i] in registers):
//                             s_i = g_i + sum_{k<i} G_ik delta_k - a dg_j y_j      (the ridge c cancels)
//   y[j0 .. j0+16) += delta,  r += Xt delta   (a window row per thread)
// The next tile's global loads are in flight while the current one is worked (two LDS tile
// buffers up to T = 512; a single buffer above: two 128 KiB tiles do not fit the 160 KiB).
// y lives in the date's row of x (global / L2), each entry read and written by the same lane.
//
// Stopping: the chain yields, for free, the residual of every coordinate just before its update
// (at the mixed iterate); once its maximum over a sweep is <= 4 eps, or at max_sweeps, the
// residual of the y AT HAND is evaluated honestly -- r recomputed from y (one pass), then
// max_i |y_i (a x_i . r + c y_i) - b_i| / b_i (a second pass) -- and only that value stops the
// date and is reported.  The sweeps then go on from the recomputed r.  No floating-point
// atomics, fixed reduction orders: the same input gives the same bits, and a date never reads
// or writes another date's data.
#include <type_traits>

#include "common.h"
#include "capi_util.h"

namespace pq {

constexpr int RP_TMAX = 1024;
constexpr int RP_TW = 16;       // assets per tile
constexpr int RP_NT = 256;      // threads

enum { RP_SWEEP = 0, RP_RVEC = 1, RP_RES = 2 };

// LDS row pitch of a tile (doubles): 18 lets a thread read a whole row (ds_read_b128, rows 144 B
// apart: the 8 lanes of a group land on 8 different bank quads) and keeps the MFMA fragment read
// -- 16 lanes per row, 128 contiguous bytes -- conflict-free; at TP = 1024 only 16 fits the LDS
constexpr int rp_pitch(int TP) { return TP > 512 ? 16 : 18; }
// doubles of LDS: the tile buffer(s), r, the four waves' G and g partials, delta, reductions
constexpr int rp_lds_doubles(int TP, int NBUF) {
  return NBUF * TP * rp_pitch(TP) + TP + 4 * 256 + 4 * 16 + 16 + 16;
}
constexpr size_t rp_lds_bytes(int TP, int NBUF) {
  return sizeof(double) * (size_t)rp_lds_doubles(TP, NBUF) + sizeof(int) * (size_t)TP;
}

// TP: the padded window length (tmax <= TP); NBUF: LDS tile buffers
template <int TP, int NBUF>
__global__ __launch_bounds__(RP_NT) void k_risk_parity(
    const double* __restrict__ panel, int64_t ldp, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ tlen, int tmax, const double* __restrict__ mu, int64_t mu_stride,
    const double* __restrict__ dg, int64_t dg_stride, int n, const double* __restrict__ av,
    const double* __restrict__ cv, const double* __restrict__ budget, int64_t ldb, double scale, double eps,
    int max_sweeps, double* __restrict__ x, int64_t ldx, double* __restrict__ stats,
    int32_t* __restrict__ status) {
  constexpr int NQ = TP / 16;   // tile rows a thread stages
  constexpr int LP = rp_pitch(TP);
  extern __shared__ double rp_lds[];
  double* s_tile = rp_lds;
  double* s_r = s_tile + NBUF * TP * LP;
  double* s_G = s_r + TP;
  double* s_g = s_G + 4 * 256;
  double* s_dl = s_g + 4 * 16;
  double* red = s_dl + 16;
  int* s_rows = reinterpret_cast<int*>(red + 16);

  const int b = xcd_slot(blockIdx.x, gridDim.x);
  const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(wave_id()), l = lane_id();
  const int col = t & 15, rq = t >> 4;
  const int T = tlen[b];
  const double a = av[b], c = cv[b];
  const double* bud = budget + (int64_t)b * ldb;
  const double* dgb = dg + (int64_t)b * dg_stride;
  const double* mub = mu ? mu + (int64_t)b * mu_stride : nullptr;
  double* y = x + (int64_t)b * ldx;   // y lives in the date's row of x
  double* out = stats + (int64_t)b * 4;

  // ---- the checks: nothing else is read from a date that fails one -----------------------
  int bad = !(a >= 0.0) || !(c >= 0.0) || !isfinite(a) || !isfinite(c) || T < 1 || T > tmax;
  if (!bad) {
    for (int u = t; u < T; u += RP_NT) {
      const int r = rows[(int64_t)b * tmax + u];
      if (r < 0) bad = 1;
      s_rows[u] = r;
    }
    for (int j = t; j < n; j += RP_NT) {
      const double bj = bud[j], dj = fma(a, dgb[j], c);
      // (a NaN or an infinity in the window makes dg_j, hence d_j, non-finite)
      if (!(bj > 0.0) || !isfinite(bj) || !(dj > 0.0) || !isfinite(dj)) bad = 1;
      else y[j] = sqrt(bj / dj);
    }
  }
  bad = (int)block_max((double)bad, red);   // (its barriers also publish s_rows and y)
  if (bad) {   // (uniform)
    const double qnan = __builtin_nan("");
    for (int j = t; j < n; j += RP_NT) y[j] = qnan;
    if (t < 4) out[t] = qnan;
    if (t == 0) status[b] = PQ_RP_BAD_INPUT;
    return;
  }

  const int nst = (T + 3) >> 2;        // MFMA k-steps (4 window rows each)
  const int T4 = nst << 2;
  const int ntiles = (n + RP_TW - 1) / RP_TW;

  // this thread's part of the tile at asset j0: column j0 + col, rows rq + 16 q, centred
  auto load_one = [&](int j0, int q, double m) -> double {
    const int tt = rq + 16 * q, j = j0 + col;
    return (j < n && tt < T) ? panel[(int64_t)s_rows[tt] * ldp + j] - m : 0.0;
  };
  auto col_mean = [&](int j0) -> double { return (mub && j0 + col < n) ? mub[j0 + col] : 0.0; };

  double est_run = 0.0;                      // lanes 0..15 of wave 0: max pre-update residual of a sweep
  double res_run = 0.0, sy = 0.0, syy = 0.0; // the same lanes: the honest pass's residual, sum y, sum y^2

  auto run_pass = [&](auto mode_) {
    constexpr int MODE = decltype(mode_)::value;
    double v[NBUF == 2 ? NQ : 1];
    // tile 0 (the barrier first: the previous pass may still read the buffer)
    __syncthreads();
    {
      const double m = col_mean(0);
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (16 * q < T4) s_tile[(rq + 16 * q) * LP + col] = load_one(0, q, m);
    }
    __syncthreads();
    for (int tile = 0; tile < ntiles; ++tile) {
      const int j0 = tile * RP_TW;
      const bool more = tile + 1 < ntiles;
      const double* Xt = s_tile + (NBUF == 2 ? (tile & 1) * TP * LP : 0);
      // lanes 0..15 of wave 0 own the tile's assets (their loads are issued before the next tile's:
      // loads return in order, and the chain must not wait for the prefetch)
      const int j = j0 + t;
      const bool own = t < 16 && j < n;
      double yj = 1.0, bj = 1.0, dgj = 0.0;
      if (own) {
        yj = y[j];
        if (MODE != RP_RVEC) bj = bud[j];
        if (MODE == RP_SWEEP) dgj = dgb[j];
      }
      if (NBUF == 2 && more) {
        const double m = col_mean(j0 + RP_TW);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          if (16 * q < T4) v[NBUF == 2 ? q : 0] = load_one(j0 + RP_TW, q, m);
      }
      if (MODE == RP_RVEC) {
        if (t < 16) s_dl[t] = own ? yj : 0.0;
      } else {
        // partial G = Xt'Xt (MFMA) and g = Xt'r of this wave's k-steps
        f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
        double gp = 0.0;
        for (int st = w; st < nst; st += 4) {
          const double xv = Xt[(4 * st + (l >> 4)) * LP + (l & 15)];
          const double rv = s_r[4 * st + (l >> 4)];
          if (MODE == RP_SWEEP) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, xv, acc, 0, 0, 0);
          gp = fma(xv, rv, gp);
        }
        gp += __shfl_xor(gp, 16, 64);
        gp += __shfl_xor(gp, 32, 64);
        if (l < 16) s_g[w * 16 + l] = gp;
        if (MODE == RP_SWEEP) {
#pragma unroll
          for (int r = 0; r < 4; ++r) s_G[w * 256 + ((l >> 4) + 4 * r) * 16 + (l & 15)] = acc[r];
        }
        __syncthreads();
        if (t < 16) {   // (wave 0)
          const double g = a * ((s_g[t] + s_g[16 + t]) + (s_g[32 + t] + s_g[48 + t]));
          if (MODE == RP_RES) {
            const double e = fabs(yj * fma(c, yj, g) - bj) / bj;
            if (own) {
              res_run = fmax(res_run, e);
              sy += yj;
              syy = fma(yj, yj, syy);
            }
          } else {
            double Gc[16];   // G[.][t] = G[t][.]
#pragma unroll
            for (int i = 0; i < 16; ++i)
              Gc[i] = a * ((s_G[i * 16 + t] + s_G[256 + i * 16 + t]) + (s_G[512 + i * 16 + t] + s_G[768 + i * 16 + t]));
            const double dj = own ? fma(a, dgj, c) : 1.0;
            double ac = g - a * dgj * yj;
            double yfin = yj, dfin = 0.0, e = 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const double s = ac;
              const double q = sqrt(fma(s, s, 4.0 * dj * bj));
              const double ynew = s > 0.0 ? (2.0 * bj) / (s + q) : (q - s) / (2.0 * dj);
              const double dl = own ? ynew - yj : 0.0;
              const double di = readlane_f64(dl, i);
              if (t == i) {
                yfin = ynew;
                dfin = dl;
                e = fabs(yj * fma(dj, yj, s) - bj) / bj;
              }
              ac = fma(Gc[i], di, ac);
            }
            if (own) {
              y[j] = yfin;
              est_run = fmax(est_run, e);
            }
            s_dl[t] = dfin;
          }
        }
      }
      if (MODE != RP_RES) {
        __syncthreads();
        // r += Xt delta (RP_RVEC: delta = the tile's y): a window row per thread
        double dv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) dv[i] = s_dl[i];
        for (int u = t; u < T; u += RP_NT) {
          const double* xr = Xt + u * LP;
          double p = 0.0;
#pragma unroll
          for (int i = 0; i < 16; ++i) p = fma(xr[i], dv[i], p);
          s_r[u] += p;
        }
      }
      if (more) {
        if (NBUF == 2) {
          double* Xn = s_tile + ((tile + 1) & 1) * TP * LP;
#pragma unroll
          for (int q = 0; q < NQ; ++q)
            if (16 * q < T4) Xn[(rq + 16 * q) * LP + col] = v[NBUF == 2 ? q : 0];
        } else {
          __syncthreads();
          const double m = col_mean(j0 + RP_TW);
#pragma unroll
          for (int q = 0; q < NQ; ++q)
            if (16 * q < T4) s_tile[(rq + 16 * q) * LP + col] = load_one(j0 + RP_TW, q, m);
        }
      }
      __syncthreads();
    }
  };

  auto zero_r = [&]() {
    __syncthreads();
    for (int u = t; u < TP; u += RP_NT) s_r[u] = 0.0;
  };

  zero_r();
  run_pass(std::integral_constant<int, RP_RVEC>{});
  int sweeps = 0;
  double res = 0.0, sumy = 0.0, ysy = 0.0;
  for (;;) {
    bool check = sweeps >= max_sweeps;
    if (!check) {
      est_run = 0.0;
      run_pass(std::integral_constant<int, RP_SWEEP>{});
      ++sweeps;
      const double est = block_max(t < 16 ? est_run : 0.0, red);
      check = est <= 4.0 * eps || sweeps >= max_sweeps;
    }
    if (check) {   // (uniform) the residual of the y at hand, with r recomputed from it
      zero_r();
      run_pass(std::integral_constant<int, RP_RVEC>{});
      res_run = sy = syy = 0.0;
      run_pass(std::integral_constant<int, RP_RES>{});
      res = block_max(t < 16 ? res_run : 0.0, red);
      sumy = block_sum(t < 16 ? sy : 0.0, red);
      const double yy = block_sum(t < 16 ? syy : 0.0, red);
      double rr = 0.0;
      for (int u = t; u < T; u += RP_NT) rr = fma(s_r[u], s_r[u], rr);
      rr = block_sum(rr, red);
      ysy = fma(a, rr, c * yy);   // y' Sigma y
      if (res <= eps || sweeps >= max_sweeps) break;
    }
  }

  // (the barriers of the reductions above order every lane's y stores before these reads)
  const double f = scale / sumy;
  for (int j = t; j < n; j += RP_NT) y[j] *= f;
  if (t == 0) {
    out[0] = res;
    out[1] = (double)sweeps;
    out[2] = f * f * ysy;
    out[3] = sumy;
    status[b] = res <= eps ? PQ_RP_OK : PQ_RP_MAX_SWEEPS;
  }
}

}  // namespace pq

extern "C" int pq_risk_parity_batched(const pq_lowrank* lr, int32_t n, int32_t batch, const double* a,
                                      const double* c, const double* budget, int64_t ldb, double scale,
                                      double eps, int32_t max_sweeps, double* x, int64_t ldx, double* stats,
                                      int32_t* status, void* stream) {
  PQ_CHECK_ARG(lr && a && c && budget && x && stats && status, "pq_risk_parity_batched: null argument");
  PQ_CHECK_ARG(lr->panel && lr->rows && lr->tlen && lr->dg, "pq_risk_parity_batched: needs panel, rows, tlen and dg");
  PQ_CHECK_ARG(lr->tmax >= 1 && lr->tmax <= pq::RP_TMAX, "pq_risk_parity_batched: tmax = %d outside [1, %d]",
               lr->tmax, pq::RP_TMAX);
  PQ_CHECK_ARG(n >= 1 && batch >= 0, "pq_risk_parity_batched: needs n >= 1 and batch >= 0 (n=%d, batch=%d)", n, batch);
  PQ_CHECK_ARG(lr->ldp >= n && lr->dg_stride >= 0 && (!lr->mu || lr->mu_stride >= 0),
               "pq_risk_parity_batched: bad panel / mu / dg strides");
  PQ_CHECK_ARG(ldb == 0 || ldb >= n, "pq_risk_parity_batched: ldb = %lld must be 0 (one shared row) or >= n = %d",
               (long long)ldb, n);
  PQ_CHECK_ARG(ldx >= n, "pq_risk_parity_batched: ldx = %lld < n = %d", (long long)ldx, n);
  PQ_CHECK_ARG(max_sweeps >= 0 && eps >= 0.0 && scale == scale, "pq_risk_parity_batched: needs max_sweeps >= 0, eps >= 0");
  if (batch == 0) return 0;
  hipStream_t str = (hipStream_t)stream;
#define PQ_RP(TP, NBUF)                                                                                          \
  do {                                                                                                           \
    constexpr size_t bytes = pq::rp_lds_bytes(TP, NBUF);                                                         \
    static_assert(bytes <= 160 * 1024, "the tile buffers must fit the LDS");                                     \
    if (bytes > 48 * 1024)                                                                                       \
      PQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pq::k_risk_parity<TP, NBUF>),               \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));                 \
    hipLaunchKernelGGL((pq::k_risk_parity<TP, NBUF>), dim3(batch), dim3(pq::RP_NT), bytes, str, lr->panel,       \
                       lr->ldp, lr->rows, lr->tlen, lr->tmax, lr->mu, lr->mu_stride, lr->dg, lr->dg_stride, n, a, \
                       c, budget, ldb, scale, eps, max_sweeps, x, ldx, stats, status);                           \
  } while (0)
  const int tmax = lr->tmax;
  if (tmax <= 64) PQ_RP(64, 2);
  else if (tmax <= 128) PQ_RP(128, 2);
  else if (tmax <= 256) PQ_RP(256, 2);
  else if (tmax <= 512) PQ_RP(512, 2);
  else PQ_RP(1024, 1);
#undef PQ_RP
  PQ_CHECK_LAUNCH("pq_risk_parity_batched");
  return 0;
}
