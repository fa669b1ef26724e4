// The steps that the grouped polish's per-date solvers share: pg_solve_date and pg_big_date
// (polish_g.hip) and rt_solve_date (polish_rt.hip).  Each solver keeps its own factorisation of
// P_FF + delta I, its triangular solves and its residual product (they sum in different orders);
// what follows is identical in all of them, and the record the pipeline's other kernels read
// (R_K, R_LAM, R_SOL, fl, xb, Fl, rF, solx) is written here only.  Called by every thread of the
// workgroup with its thread id t (rebuilt from loop_zero() inside the callers' loops); T threads.
#pragma once
#include "polish_dev.h"
#include "pg_record.h"

namespace pq {

// S = U'U + delta I of the active rows (rows of U: L^-1 C_aF', pitch ld), lower triangle into
// Sm (leading dimension lds), one wave sum per entry.  schur_potrf follows a barrier.
template <int T>
PQ_DEVFN void pg_schur(int t, const double* U, int ld, int k, int ma, double delta, double* Sm, int lds) {
  const int l = T > 64 ? t & 63 : t, w = T > 64 ? t >> 6 : 0;   // (one wave: t is the lane)
  for (int e = w; e < ma * ma; e += T / 64) {
    const int ii = e / ma, jj = e % ma;
    if (jj > ii) continue;
    const double* ui = U + (int64_t)ii * ld;
    const double* uj = U + (int64_t)jj * ld;
    double sum = 0.0;
    for (int p = l; p < k; p += 64) sum += ui[p] * uj[p];
    sum = wave_sum(sum);
    if (l == 0) Sm[ii * lds + jj] = sum + (ii == jj ? delta : 0.0);
  }
}

// LDS of the inner primal step: x_F and the K position of each free variable (both rewritten);
// the kept variables' K position, index, value and rhs; the violators' K position, 4 x index +
// bound side and bound value; the active rows and their rhs; a flag for nv
struct PgFixLds {
  double* xF;
  int *s_map, *s_m2, *s_f2;
  double *t1, *t2;
  int *s_vp, *s_vi;
  double* vv;
  const int* s_al;
  double* dAv;
  int* s_flag;
};

// Inner primal step: the nv free variables the solve left outside their box are fixed at the
// bound they cross (box_cross, as the round's checks), the others compacted in order; the
// reduced rhs and the active rows' rhs take the fixed values (the P_FB columns are K's columns).
// Returns nv; with nv = 0 (feasible) or nv = k (nothing left free: the rounds decide) nothing is
// written.  PAD > 0: s_map / xF are kept zero from the new k up to PAD.  Ends with a barrier.
template <int T, int PAD>
PQ_DEVFN int pg_fix_violators(int t, const PgFixLds L, const PGWork& wk, const double* K, int ldk,
                              const double* lb, const double* ub, const double* Cg, int ld, int ma, int k,
                              double* R) {
  const int l = T > 64 ? t & 63 : t, w = T > 64 ? t >> 6 : 0;   // (one wave: t is the lane)
  int nk = 0, nv = 0;
  if (w == 0) {
    for (int p0 = 0; p0 < k; p0 += 64) {
      const int p = p0 + l;
      int f = 0, i = 0;
      double v = 0.0;
      if (p < k) {
        i = wk.Fl[p];
        f = box_cross(L.xF[p], lb[i], ub[i], POLISH_INNER_BOX_TOL);
        if (f) v = f == 1 ? lb[i] : ub[i];
      }
      const unsigned long long mv = __ballot(p < k && f != 0);
      const unsigned long long mk = __ballot(p < k && f == 0);
      const unsigned long long below = (1ull << l) - 1ull;
      if (p < k && f != 0) {
        const int j = nv + __popcll(mv & below);
        L.s_vp[j] = L.s_map[p];
        L.s_vi[j] = 4 * i + f;
        L.vv[j] = v;
      } else if (p < k) {
        const int j = nk + __popcll(mk & below);
        L.s_m2[j] = L.s_map[p];
        L.s_f2[j] = i;
        L.t1[j] = L.xF[p];
        L.t2[j] = wk.rF[p];
      }
      nv += __popcll(mv);
      nk += __popcll(mk);
    }
  }
  if constexpr (T > 64) {   // the other waves learn nv from wave 0
    if (t == 0) *L.s_flag = nv;
    __syncthreads();
    nv = *L.s_flag;
  } else {
    __syncthreads();
  }
  if (nv == 0 || nv == k) return nv;   // uniform
  const int k2 = k - nv;
  for (int p = t; p < (PAD > 0 ? PAD : k2); p += T) {
    if (p < k2) {
      const int mp = L.s_m2[p];
      double r = L.t2[p];
      for (int j = 0; j < nv; ++j)
        if (L.vv[j] != 0.0) r = fma(-K[(int64_t)mp * ldk + L.s_vp[j]], L.vv[j], r);
      wk.rF[p] = r;
      wk.Fl[p] = L.s_f2[p];
      L.s_map[p] = mp;
      L.xF[p] = L.t1[p];
    } else {
      L.s_map[p] = 0;
      L.xF[p] = 0.0;
    }
  }
  for (int j = t; j < nv; j += T) {
    const int i = L.s_vi[j] >> 2;
    wk.fl[i] = L.s_vi[j] & 3;
    wk.xb[i] = L.vv[j];
  }
  for (int a = w; a < ma; a += T / 64) {
    const double* cr = Cg + (int64_t)L.s_al[a] * ld;
    double sum = 0.0;
    for (int j = l; j < nv; j += 64) sum += cr[L.s_vi[j] >> 2] * L.vv[j];
    sum = wave_sum(sum);
    if (l == 0) L.dAv[a] -= sum;
  }
  if (t == 0) R[R_K] = k2;
  __syncthreads();
  return nv;
}

// Expand and write back: xs = x_B off F, x_F on F; solx; the general multipliers by row (the 64
// slots of R_LAM) and by active row (R_SOL)
template <int T>
PQ_DEVFN void pg_expand(int t, const PGWork& wk, int n, int k, const double* xF, int ma, const int* s_al,
                        const double* lamv, double* R) {
  for (int ii = t; ii < n; ii += T) wk.xs[ii] = wk.xb[ii];
  __syncthreads();
  for (int p = t; p < k; p += T) {
    wk.xs[wk.Fl[p]] = xF[p];
    wk.solx[p] = xF[p];
  }
  if (t < 64) R[R_LAM + t] = 0.0;
  __syncthreads();
  if (t < ma) {
    R[R_LAM + s_al[t]] = lamv[t];
    R[R_SOL + t] = lamv[t];
  }
}

}  // namespace pq
