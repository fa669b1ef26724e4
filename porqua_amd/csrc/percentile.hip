// Quantile (percentile) portfolios for a whole batch of dates.
//
// Reference: PercentilePortfolios.solve (src/optimization.py:398-417) negates one score per
// asset, takes th = np.percentile(-s, linspace(0, 100, N + 1)), puts asset x into bucket 1
// when x <= th[1] and into bucket i when th[i-1] < x <= th[i], gives every member of bucket
// i the weight 1 / len(bucket i) (w_dict) and builds the long-short weights +1 / len(bucket
// 1) on bucket 1, then -1 / len(bucket N) on bucket N (the second assignment wins, so N = 1
// is all -1 / n).  An empty bucket is a ZeroDivisionError there; here it is a row status.
//
// MI355X mapping: one workgroup per date.  The row is loaded once with the sign applied and
// staged in LDS, padded with +inf to a power of two P >= 64, and sorted by a bitonic network
// (values only: the thresholds need order statistics, not indices).  The compare-exchange
// steps at distance j >= 64 run in LDS: lane t of a step owns the pair (i, i + j) with
// consecutive lanes on consecutive keys, so every ds_read_b64 / ds_write_b64 of a 32-lane
// half covers one 256 B bank row -- the power-of-two stride is between a lane's own two
// keys, never between lanes.  The steps at distance j <= 32 would put the lanes of a half on
// every other group of j keys (a 2-way conflict per access); they run in registers instead,
// each wave holding a 64-key chunk one key per lane and exchanging through __shfl_xor, which
// also removes six barriers per merge stage and all 21 steps of the first six stages.
//
// The N + 1 thresholds are numpy's linear interpolation between two order statistics; the
// index plan (prev, next, gamma) comes from the host, computed with numpy's own arithmetic,
// and the two-branch lerp below is numpy's _lerp without fused multiply-adds, so the
// thresholds are np.percentile's bit for bit (up to the sign of a zero: the order of -0.0
// and +0.0 among equal keys is the sorter's).  A second pass re-reads the row (L2-hot),
// finds the smallest i with x <= th[i] (the reference's mask chain, th being monotone),
// counts members with LDS integer atomics, and after a barrier writes the weights.
//
// LDS: 8 P + 8 (N + 1) + 4 N + 8 bytes, so a 1000-asset universe (P = 1024, 8.3 KiB) runs
// many workgroups per CU and the largest (P = 16384, 128 KiB of keys) one.  HBM traffic is
// 8 n B read and 12 n B written per date (the second read hits L2).
#include <limits>

#include "capi_util.h"
#include "common.h"

// numpy's thresholds and 1 / count are plain IEEE operations: nothing in this file may be
// contracted into a fused multiply-add
#pragma clang fp contract(off)

namespace pq {

// Steps j = j0, j0 / 2, ..., 1 (j0 <= 32) of merge stage k on a wave-resident chunk: lane l
// holds key i = 64 c + l.  The pair (i, i ^ j) sorts ascending where (i & k) == 0; equal keys
// stay where they are (-0.0 and +0.0 are equal), so the multiset is kept exactly.
__device__ __forceinline__ double wave_steps(double v, int i, int k, int j0) {
  const bool up = (i & k) == 0;
  for (int j = j0; j > 0; j >>= 1) {
    const double p = __shfl_xor(v, j, 64);
    const bool keep_min = ((i & j) == 0) == up;
    v = keep_min ? (p < v ? p : v) : (p > v ? p : v);
  }
  return v;
}

template <int NT>
__global__ __launch_bounds__(NT) void k_percentile(
    const double* __restrict__ scores, int64_t lds, int n, double sign, int N,
    const int32_t* __restrict__ prev, const int32_t* __restrict__ next,
    const double* __restrict__ gamma, int P, double* __restrict__ th, int32_t* __restrict__ bucket,
    int32_t* __restrict__ counts, double* __restrict__ w, int32_t* __restrict__ status) {
  extern __shared__ double smem[];
  double* keys = smem;                         // P sorted keys
  double* sth = keys + P;                      // N + 1 thresholds
  int* scnt = reinterpret_cast<int*>(sth + N + 1);   // N member counts
  int* sflag = scnt + N;                       // row verdict (NaN score / empty bucket)
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double* row = scores + b * lds;
  double* thb = th + b * (N + 1);
  int32_t* bkb = bucket + b * n;
  int32_t* cnb = counts + b * N;
  double* wb = w + b * n;
  const double qnan = std::numeric_limits<double>::quiet_NaN();

  // ---- load with the sign applied, pad with +inf, NaN check --------------------------
  if (tid == 0) *sflag = 0;
  for (int t = tid; t < N; t += NT) scnt[t] = 0;
  bool nan = false;
  for (int i = tid; i < P; i += NT) {
    const double v = i < n ? sign * row[i] : std::numeric_limits<double>::infinity();
    nan |= v != v;
    keys[i] = v;
  }
  __syncthreads();
  if (nan) *sflag = 1;
  __syncthreads();
  if (*sflag) {   // np.percentile of such a row is NaN and every mask of the reference empty
    for (int t = tid; t <= N; t += NT) thb[t] = qnan;
    for (int t = tid; t < N; t += NT) cnb[t] = 0;
    for (int i = tid; i < n; i += NT) {
      bkb[i] = 0;
      wb[i] = qnan;
    }
    if (tid == 0) status[b] = PQ_PCT_NAN_SCORE;
    return;
  }

  // ---- bitonic sort of the P keys ----------------------------------------------------
  const int lane = tid & 63, wv = tid >> 6, nchunk = P >> 6;
  for (int c = wv; c < nchunk; c += NT / 64) {   // stages k = 2 .. 64: chunks in registers
    const int i = c * 64 + lane;
    double v = keys[i];
    for (int k = 2; k <= 64; k <<= 1) v = wave_steps(v, i, k, k >> 1);
    keys[i] = v;
  }
  __syncthreads();
  for (int k = 128; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= 64; j >>= 1) {     // distance >= 64: compare-exchange in LDS
      for (int t = tid; t < (P >> 1); t += NT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const double lo = keys[i], hi = keys[i + j];
        const bool up = (i & k) == 0;
        if (up ? lo > hi : lo < hi) {
          keys[i] = hi;
          keys[i + j] = lo;
        }
      }
      __syncthreads();
    }
    for (int c = wv; c < nchunk; c += NT / 64) {   // distance 32 .. 1: in registers
      const int i = c * 64 + lane;
      keys[i] = wave_steps(keys[i], i, k, 32);
    }
    __syncthreads();
  }

  // ---- thresholds: numpy's _lerp between the plan's two order statistics ---------------
  for (int t = tid; t <= N; t += NT) {
    const int ip = min(max(prev[t], 0), n - 1), in = min(max(next[t], 0), n - 1);
    const double a = keys[ip], c = keys[in], g = gamma[t];
    const double d = c - a;
    double r = a + d * g;
    if (g >= 0.5) r = c - d * (1.0 - g);
    sth[t] = r;
    thb[t] = r;
  }
  __syncthreads();

  // ---- buckets: smallest i with x <= th[i]; th[N] is the row maximum -------------------
  for (int i = tid; i < n; i += NT) {
    const double x = sign * row[i];
    int k = 1;
    while (k < N && !(x <= sth[k])) ++k;
    bkb[i] = k;
    atomicAdd(&scnt[k - 1], 1);
  }
  __syncthreads();
  for (int t = tid; t < N; t += NT) {
    const int c = scnt[t];
    cnb[t] = c;
    if (c == 0) *sflag = 1;
  }
  __syncthreads();

  // ---- long-short weights (this thread re-reads the bucket ids it wrote itself) ---------
  const bool empty = *sflag != 0;
  const double wl = 1.0 / (double)scnt[0], ws = -1.0 / (double)scnt[N - 1];
  for (int i = tid; i < n; i += NT) {
    const int k = bkb[i];
    double v = k == 1 ? wl : 0.0;
    if (k == N) v = ws;
    wb[i] = empty ? qnan : v;
  }
  if (tid == 0) status[b] = empty ? PQ_PCT_EMPTY_BUCKET : PQ_PCT_OK;
}

}  // namespace pq

extern "C" int pq_percentile_batched(const double* scores, int64_t lds, int32_t n, int32_t batch,
                                     double sign, int32_t n_percentiles, const int32_t* prev,
                                     const int32_t* next, const double* gamma, double* th,
                                     int32_t* bucket, int32_t* counts, double* w, int32_t* status,
                                     void* stream) {
  PQ_CHECK_ARG(scores && prev && next && gamma && th && bucket && counts && w && status,
               "pq_percentile_batched: null argument");
  PQ_CHECK_ARG(n >= 1 && n <= PQ_PCT_MAX_N, "pq_percentile_batched: n = %d outside 1..%d", n, PQ_PCT_MAX_N);
  PQ_CHECK_ARG(n_percentiles >= 1 && n_percentiles <= PQ_PCT_MAX_BUCKETS,
               "pq_percentile_batched: n_percentiles = %d outside 1..%d", n_percentiles, PQ_PCT_MAX_BUCKETS);
  PQ_CHECK_ARG(lds >= n, "pq_percentile_batched: row stride %lld < n = %d", (long long)lds, n);
  PQ_CHECK_ARG(sign == 1.0 || sign == -1.0, "pq_percentile_batched: sign must be +1 or -1");
  if (batch <= 0) return 0;
  int P = 64;
  while (P < n) P <<= 1;
  const int N = n_percentiles;
  const size_t bytes = sizeof(double) * (size_t)(P + N + 1) + sizeof(int) * (size_t)(N + 2);
  hipStream_t s = (hipStream_t)stream;
#define PQ_PCT(NT)                                                                                  \
  do {                                                                                              \
    if (bytes > 48 * 1024)                                                                          \
      PQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pq::k_percentile<NT>),         \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));    \
    hipLaunchKernelGGL(pq::k_percentile<NT>, dim3(batch), dim3(NT), bytes, s, scores, lds, n, sign, \
                       N, prev, next, gamma, P, th, bucket, counts, w, status);                     \
  } while (0)
  // two to sixteen keys per thread: small universes keep several workgroups on a CU
  if (P <= 256) PQ_PCT(64);
  else if (P <= 2048) PQ_PCT(256);
  else PQ_PCT(1024);
#undef PQ_PCT
  PQ_CHECK_LAUNCH("pq_percentile_batched");
  return 0;
}
