// The ADMM row rules, stated once for the factor kernels (chol_dev.h, lowrank.hip, eigcap.hip)
// and the four iteration kernels (admm.hip, admm_grp.hip, admm_gcap.hip, admm_sweep.hip).
// tests/admm_reference.py is their model: row_rho and _iterate there use the same names, so
// model and kernel read side by side.  The factored KKT matrix and the iterates must agree
// on row_rho bit for bit, and the operation order below is part of the kernels' behaviour.
#pragma once
#include "common.h"
#include "../../include/porqua_hip.h"

namespace pq {

// Per-row rho: rho * eq_scale on equality rows, rho_min on rows without bounds.
__device__ __forceinline__ double row_rho(double l, double u, double rho, double rho_min, double eq_scale) {
  if (l == u) return rho * eq_scale;
  if (isinf(l) && isinf(u)) return rho_min;
  return rho;
}
__device__ __forceinline__ double row_rho(double l, double u, double rho, const pq_settings& s) {
  return row_rho(l, u, rho, s.rho_min, s.eq_scale);
}

// The relaxed update of one constraint row (zt: the row of C x~, r: its rho):
//   zh = alpha zt + (1 - alpha) z;  zn = clip(zh + y / r, l, u);  yn = y + r (zh - zn)
struct RowStep {
  double zh, zn, yn;
};
__device__ __forceinline__ RowStep row_step(double zt, double z, double y, double r, double l, double u,
                                            double alpha) {
  const double zh = alpha * zt + (1.0 - alpha) * z;
  const double zn = fmin(fmax(zh + y / r, l), u);
  const double yn = y + r * (zh - zn);
  return RowStep{zh, zn, yn};
}

// The 7 residual maxima of an iteration, mv:
//   0 |Cx - z|, 1 |Cx|, 2 |z|, 3 |Px + q + C'y|, 4 |Px|, 5 |C'y|, 6 |q|
__device__ __forceinline__ double eps_prim(const double* mv, const pq_settings& s) {
  return s.eps_abs + s.eps_rel * fmax(mv[1], mv[2]);
}
__device__ __forceinline__ double eps_dual(const double* mv, const pq_settings& s) {
  return s.eps_abs + s.eps_rel * fmax(mv[4], fmax(mv[5], mv[6]));
}

// The rho that balances the relative residuals: rho sqrt(rp / rd), kept in [rho_min, rho_max].
__device__ __forceinline__ double rho_request(const double* mv, double rho, const pq_settings& s) {
  const double rp = mv[0] / (fmax(mv[1], mv[2]) + 1e-30);
  const double rd = mv[3] / (fmax(mv[4], fmax(mv[5], mv[6])) + 1e-30);
  return fmin(fmax(rho * sqrt(rp / (rd + 1e-30)), s.rho_min), s.rho_max);
}

// The per-problem decision after iteration `it`: SOLVED, NEED_REFACTOR with the requested rho
// (a request beyond adapt_tol of the current one), MAX_ITER, or UNSOLVED (go on; rho unchanged).
struct Verdict {
  int status;
  double rho;
};
__device__ __forceinline__ Verdict verdict(const double* mv, int it, double rho, const pq_settings& s) {
  Verdict v{PQ_UNSOLVED, rho};
  if (it >= s.min_iter && mv[0] <= eps_prim(mv, s) && mv[3] <= eps_dual(mv, s)) {
    v.status = PQ_SOLVED;
  } else if (s.adapt_interval > 0 && it % s.adapt_interval == 0 && it < s.max_iter) {
    // (not at max_iter itself: the run ends there, and a rho request would cost a
    // refactorisation that no iteration uses)
    // (in the grouped and sweep kernels a problem left NEED_REFACTOR at max_iter was resumed
    // after the refactorisation for one iteration beyond max_iter)
    const double rn = rho_request(mv, rho, s);
    if (rn > rho * s.adapt_tol || rn < rho / s.adapt_tol) {
      v.rho = rn;
      v.status = PQ_NEED_REFACTOR;
    }
  }
  if (v.status == PQ_UNSOLVED && it >= s.max_iter) v.status = PQ_MAX_ITER;
  return v;
}

}  // namespace pq
