// The active-set polish rules, stated once for the kernels that apply them: the per-date
// kernels (polish.hip, polish_w.hip), the grouped pipeline (polish_g.hip, polish_rt.hip) and
// its wide rounds (polish_gw.hip).  tests/manufactured.py is their model: STOP_REL, ROW_ZERO
// and reduced_kkt_f64 there state the same refinement, so model and kernel read side by side.
// Every kernel must take the same decision from the same numbers (a rule that differs between
// two of them makes the solvers disagree by free-set size), and the operation order below is
// part of the kernels' behaviour.
#pragma once
#include "common.h"

namespace pq {

constexpr double POLISH_STOP_REL = 1e-13;        // the refinement ends at this residual x problem scale
constexpr double POLISH_ROW_ZERO = 1e-14;        // a row residual within this x (1 + |d_a| + |C_aF x_F|) is zero
constexpr double POLISH_INNER_BOX_TOL = 1e-12;   // box tolerance of the grouped solvers' inner primal step

// Starting classification of a variable from the ADMM point (z, y: its box row, x: its value):
// 0 free, 1 at lower, 2 at upper.  fix_thr: a variable this close to its lower bound starts
// fixed there too (k_pg_init; -INFINITY elsewhere: never).
PQ_DEVFN int start_box(double z, double y, double x, double lb, double ub, double fix_thr) {
  int f = 0;
  if (!isinf(lb) && (z - lb < -y || x - lb < fix_thr)) f = 1;
  else if (!isinf(ub) && ub - z < y) f = 2;
  if (lb == ub) f = 1;
  return f;
}
// ... and of a general row: 0 inactive, 1 at lg, 2 at ug (equality rows: 2)
PQ_DEVFN int start_row(double z, double y, double lg, double ug) {
  if (lg == ug) return 2;
  if (!isinf(lg) && z - lg < -y) return 1;
  if (!isinf(ug) && ug - z < y) return 2;
  return 0;
}

// r_a = d_a - C_aF x_F of an active row (sum = C_aF x_F): a rounding-level residual of a row
// with no free support must not move lam
PQ_DEVFN double row_residual(double dA, double sum) {
  const double v = dA - sum;
  return fabs(v) <= POLISH_ROW_ZERO * (1.0 + fabs(dA) + fabs(sum)) ? 0.0 : v;
}
// converged to rounding level (rm: the largest residual): further refinement steps change nothing
PQ_DEVFN bool refine_done(double rm, double sc) { return rm <= POLISH_STOP_REL * sc; }

// A free variable outside its box: 1 below lb, 2 above ub, else 0
PQ_DEVFN int box_cross(double x, double lb, double ub, double tol) {
  if (!isinf(lb) && x < lb - tol * (1.0 + fabs(lb))) return 1;
  if (!isinf(ub) && x > ub + tol * (1.0 + fabs(ub))) return 2;
  return 0;
}
// A variable fixed at a bound (f = 1, 2) whose dual -g has the wrong sign is released
PQ_DEVFN bool bound_release(int f, double lb, double ub, double g, double dtol) {
  return (f == 1 && lb != ub && -g > dtol) || (f == 2 && -g < -dtol);
}
// The activity of an inequality row after a round (sum = C x, lam its multiplier): the new
// one, or a when nothing changed
PQ_DEVFN int row_verdict(int a, double sum, double lg, double ug, double lam, double ptol, double dtol) {
  if (a == 0 && sum > ug + ptol * (1.0 + fabs(ug))) return 2;
  if (a == 0 && sum < lg - ptol * (1.0 + fabs(lg))) return 1;
  if (a == 2 && lam < -dtol) return 0;
  if (a == 1 && lam > dtol) return 0;
  return a;
}

// Cholesky of the active rows' Schur complement S (ma x ma, lower, leading dimension lds), in
// place, by one lane.  Returns 1 when S is not positive definite.
PQ_DEVFN int schur_potrf(double* S, int lds, int ma) {
  for (int c = 0; c < ma; ++c) {
    double d = S[c * lds + c];
    for (int m = 0; m < c; ++m) d -= S[c * lds + m] * S[c * lds + m];
    if (!(d > 0.0) || !isfinite(d)) return 1;
    d = sqrt(d);
    S[c * lds + c] = d;
    for (int r = c + 1; r < ma; ++r) {
      double v = S[r * lds + c];
      for (int m = 0; m < c; ++m) v -= S[r * lds + m] * S[c * lds + m];
      S[r * lds + c] = v / d;
    }
  }
  return 0;
}
// wl <- S^-1 wl with S = Ls Ls' factored as above (or by tile_potrf_lds), by one lane
PQ_DEVFN void schur_solve(const double* S, int lds, int ma, double* wl) {
  for (int i = 0; i < ma; ++i) {            // forward Ls
    double v = wl[i];
    for (int j = 0; j < i; ++j) v -= S[i * lds + j] * wl[j];
    wl[i] = v / S[i * lds + i];
  }
  for (int i = ma - 1; i >= 0; --i) {       // backward Ls'
    double v = wl[i];
    for (int j = i + 1; j < ma; ++j) v -= S[j * lds + i] * wl[j];
    wl[i] = v / S[i * lds + i];
  }
}

}  // namespace pq
