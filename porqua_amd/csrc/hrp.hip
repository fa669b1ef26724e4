// Hierarchical risk parity (Lopez de Prado 2016) of every date at once on the dense
// Sigma_b = alpha_b S_b + c_b I: the single-linkage tree of the correlation distance
// D_ij = sqrt((1 - rho_ij) / 2) with SciPy's conventions, its leaves in pre-order, and the
// recursive bisection of that order by inverse-variance cluster variances.  Nothing is inverted
// or factored.  One 256-thread workgroup per date, everything but S in LDS and registers:
//
//   diagonal   d_j = alpha S_jj + c, iv_j = 1 / d_j, isd_j = 1 / sqrt(d_j)           (the checks)
//   Prim       from asset 0; thread t owns the columns 4t .. 4t+3 (best[] in registers).  A step
//              reads row x of the vertex that joined last -- contiguous, once --, forms
//              key = 1 - clip((alpha S_xj)(isd_x isd_j)) (the order of D without its root; the
//              product is symmetric in x and j), updates best on strict <, and takes the argmin
//              with the lowest index: a min by wave shuffle, the lowest lane that holds it (lane
//              order is column order), then the four waves through LDS.  One barrier per step.
//              Edge k joins the vertices that entered k-th and (k+1)-th, as in SciPy: the
//              clusters of a single-linkage tree are runs of Prim's sequence.
//   sort       bitonic on (key, insertion index): a total order, so the result is the stable sort
//   merges     in sorted order on the runs (lane 0): edge k joins the run that ends at position k
//              with the one that starts at k + 1 -- the roots a union-find would return, in O(1)
//   order      top-down output offsets (a parent's id exceeds its children's): no stack at all
//   bisection  over the tree of the ordered positions (heap numbering, the first L / 2 positions
//              left).  Q_c = iv_c' Sigma_cc iv_c bottom-up: Q_c = Q_l + Q_r + 2 alpha X_c with the
//              cross block X_c = sum_{p in l, q in r} iv_p S_pq iv_q, a leaf has Q = iv; the
//              cluster variance is v_c = Q_c / (sum iv_c)^2.  Every level reads its cross blocks
//              by lane groups as wide as the level's right halves (64 .. 1 lanes per row), each
//              entry of S once: n^2 / 2 entries over all levels.  A second pass over the same
//              blocks with the final weights gives x' Sigma x.
//
// The complete, average, weighted and Ward trees (k_hrp_link) replace Prim and the run merges by
// SciPy's nearest-neighbour chain on a distance matrix in a global work slab of the date:
//
//   D          D_ij = sqrt(key_ij / 2) with Prim's key, from the upper triangle of S and mirrored
//              (SciPy's condensed form), four rows of S in flight; every entry of S is checked here,
//              so the chain only ever sees finite numbers
//   chain      thread t owns the columns 4t .. 4t+3 and their cluster sizes (registers; 0: dead).
//              A scan reads row x of the chain's top -- contiguous --, takes Prim's argmin over
//              the live columns but x, and the owners of x and of the previous element y publish
//              their sizes and D_xy with it: one barrier.  Only a strictly smaller minimum
//              replaces y; otherwise x and y merge: rows x and y are read contiguously, the
//              Lance-Williams update in SciPy's operation order (no contraction, correctly rounded
//              division and root) is written to row y contiguously and to column y strided, and a
//              second barrier publishes it together with the lowest live column, where an empty
//              chain restarts.  At most 3n scans; the loop is capped at 4n (the failure path).
//   sort       as above, on (distance, merge index)
//   merges     a union-find with path compression over the recorded slots (lane 0), the smaller
//              root first; the sizes are the union-find's, as in SciPy's label(), not the chain's
//
// LDS: 38 bytes per asset slot (pow2ceil(n) slots), the tree's arrays aliased by the bisection's:
// 39 KiB at n = 1024, four workgroups per CU.  The chain adds nothing to it: the chain and the
// merge slots live in the child arrays the merges fill later, the union-find in the place of
// 1 / sd, the published scalars in the reduction scratch.  No floating-point atomics, fixed
// reduction orders: the same input gives the same bits; a date never reads or writes another
// date's data.
#include <limits.h>
#include <type_traits>

#include "common.h"
#include "capi_util.h"

namespace pq {

constexpr int HRP_NT = 256;
constexpr int HRP_PER = PQ_HRP_NMAX / HRP_NT;   // columns per thread
static_assert(HRP_PER == 4, "a thread owns four neighbouring columns");
typedef unsigned short u16;                     // ids < 2 n <= 2048

// asset slots of the LDS arrays: the sort pads n - 1 edges to a power of two, the bisection
// tree's internal nodes have heap numbers below pow2ceil(n)
__host__ __device__ constexpr int hrp_slots(int n) {
  int s = 8;
  while (s < n) s <<= 1;
  return s;
}
__host__ __device__ constexpr size_t hrp_lds_bytes(int n) {
  return (size_t)hrp_slots(n) * 38 + sizeof(double) * (16 + 8) + sizeof(int) * 8;
}

// the node m of level lvl (its bits, most significant first, pick the halves): [lo, hi)
PQ_DEVFN void hrp_node(int n, int lvl, int m, int& lo, int& hi) {
  lo = 0;
  hi = n;
  for (int bit = lvl - 1; bit >= 0; --bit) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((m >> bit) & 1) lo = mid; else hi = mid;
  }
}

// The Lance-Williams update of the distance of cluster i to the merged x and y, in the operation
// order of SciPy's _hierarchy_distance_update.pxi (sizes as doubles, every product left to right,
// nothing contracted: a fused multiply-add changes bits and eventually trees).
template <int M>
PQ_DEVFN double hrp_lance_williams(double dxi, double dyi, double dxy, int nx, int ny, int ni) {
#pragma clang fp contract(off)
  if constexpr (M == PQ_HRP_COMPLETE) return dxi > dyi ? dxi : dyi;
  else if constexpr (M == PQ_HRP_AVERAGE) return ((double)nx * dxi + (double)ny * dyi) / (double)(nx + ny);
  else if constexpr (M == PQ_HRP_WEIGHTED) return 0.5 * (dxi + dyi);
  else {
    const double tt = 1.0 / (double)(nx + ny + ni);
    return sqrt((double)(ni + nx) * tt * dxi * dxi + (double)(ni + ny) * tt * dyi * dyi -
                (double)ni * tt * dxy * dxy);
  }
}

// One date.  M = PQ_HRP_SINGLE: Prim, and work is not touched.  Otherwise the chain on the
// date's slab of work (read back by other threads after a barrier: not a restrict pointer).
template <int M>
PQ_DEVFN void hrp_date(const double* __restrict__ S, int64_t ld, int n, const double* __restrict__ av,
                       const double* __restrict__ cv, double scale, double* __restrict__ x, int64_t ldx,
                       int32_t* __restrict__ order, int64_t ldo, double* __restrict__ link,
                       double* __restrict__ stats, int32_t* __restrict__ status, double* work, int64_t ldw) {
  extern __shared__ double hrp_lds[];
  const int na = hrp_slots(n);
  // persistent
  double* red = hrp_lds;                        // 16
  double* s_slotv = red + 16;                   // 2 x 4: the waves' minima, double-buffered
  double* s_dinv = s_slotv + 8;                 // iv by asset; later the cross blocks' row sums, the alphas
  double* uni = s_dinv + na;
  // the tree's arrays ...
  double* s_isd = uni;                          // dead after Prim:
  u16* s_idat = reinterpret_cast<u16*>(uni);    //   id of the run that starts here
  u16* s_start = s_idat + na;                   //   start of the run that ends here
  double* s_ekey = uni + na;
  u16* s_sidx = reinterpret_cast<u16*>(uni + 2 * na);
  u16* s_pv = s_sidx + na;                      // Prim's sequence
  u16* s_end = s_pv + na;                       // end of the run that starts here; later the offsets
  u16* s_c0 = s_end + na;
  u16* s_c1 = s_c0 + na;
  u16* s_cs = s_c1 + na;
  // ... aliased by the bisection's
  double* s_wt = uni;                           // iv by position, then the weights
  double* s_Q = uni + na;
  double* s_siv = uni + 2 * na;
  u16* s_order = reinterpret_cast<u16*>(uni + 3 * na + na / 2);   // (after s_cs)
  int* s_sloti = reinterpret_cast<int*>(s_order + na);

  const int b = blockIdx.x;
  const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(wave_id()), l = lane_id();
  const double* Sb = S + (int64_t)b * ld * ld;
  double* xb = x + (int64_t)b * ldx;
  int32_t* ob = order + (int64_t)b * ldo;
  double* lb = link ? link + (int64_t)b * (n - 1) * 4 : nullptr;
  const double a = av[b], c = cv[b];
  const double INF = __builtin_inf();

  // ---- the diagonal and the checks ----------------------------------------------------------
  int bad = !(a >= 0.0) || !(c >= 0.0) || !isfinite(a) || !isfinite(c);
  if (!bad) {
    for (int j = t; j < n; j += HRP_NT) {
      const double d = fma(a, Sb[(int64_t)j * ld + j], c);
      if (!(d > 0.0) || !isfinite(d)) bad = 1;
      else {
        s_dinv[j] = 1.0 / d;
        s_isd[j] = 1.0 / sqrt(d);
      }
    }
  }
  bad = (int)block_max((double)bad, red);   // (its barriers publish s_dinv and s_isd)

  auto fail = [&]() {
    const double qnan = __builtin_nan("");
    for (int j = t; j < n; j += HRP_NT) {
      xb[j] = qnan;
      ob[j] = -1;
    }
    if (lb)
      for (int i = t; i < 4 * (n - 1); i += HRP_NT) lb[i] = qnan;
    if (t < 2) stats[(int64_t)b * 2 + t] = qnan;
    if (t == 0) status[b] = PQ_HRP_BAD_INPUT;
  };
  if (bad) {   // (uniform)
    fail();
    return;
  }
  if (n == 1) {
    if (t == 0) {
      xb[0] = scale;
      ob[0] = 0;
      stats[(int64_t)b * 2] = scale * scale / s_dinv[0];
      stats[(int64_t)b * 2 + 1] = INF;
      status[b] = PQ_HRP_OK;
    }
    return;
  }

  // ---- Prim ---------------------------------------------------------------------------------
  const int j0 = HRP_PER * t;
  const bool vec = (reinterpret_cast<uintptr_t>(Sb) & 15) == 0 && (ld & 1) == 0 && j0 + 3 < n;
  if constexpr (M == PQ_HRP_SINGLE) {
    double best[HRP_PER], isdj[HRP_PER];
    unsigned done = 0;   // bit q: column j0 + q has joined (or lies past n)
#pragma unroll
    for (int q = 0; q < HRP_PER; ++q) {
      best[q] = INF;
      isdj[q] = j0 + q < n ? s_isd[j0 + q] : 0.0;
      if (j0 + q >= n) done |= 1u << q;
    }
    if (t == 0) {
      done |= 1u;
      s_pv[0] = 0;
    }
    int xc = 0;
    auto load_row = [&](int r, double (&sv)[HRP_PER]) {
      const double* row = Sb + (int64_t)r * ld;
      if (vec) {
        const double2 p0 = *reinterpret_cast<const double2*>(row + j0);
        const double2 p1 = *reinterpret_cast<const double2*>(row + j0 + 2);
        sv[0] = p0.x; sv[1] = p0.y; sv[2] = p1.x; sv[3] = p1.y;
      } else {
#pragma unroll
        for (int q = 0; q < HRP_PER; ++q) sv[q] = j0 + q < n ? row[j0 + q] : 0.0;   // never past column n
      }
    };
    for (int k = 0; k < n - 1; ++k) {
      double sv[HRP_PER];
      load_row(xc, sv);
      const double ix = s_isd[xc];
      double bv = INF;
      int bi = INT_MAX;
#pragma unroll
      for (int q = 0; q < HRP_PER; ++q) {
        const int j = j0 + q;
        // NaN never compares <: the explicit check (the diagonal was checked above)
        if (j < n && j != xc && !isfinite(sv[q])) bad = 1;
        const double rho = fmin(fmax((a * sv[q]) * (ix * isdj[q]), -1.0), 1.0);
        const double key = 1.0 - rho;
        if (!((done >> q) & 1u)) {
          if (key < best[q]) best[q] = key;
          if (best[q] < bv || bi == INT_MAX) {
            bv = best[q];
            bi = j;
          }
        }
      }
      // the wave's minimum, then the lowest lane that holds it (lanes are in column order)
      double mv = bv;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mv = fmin(mv, __shfl_xor(mv, o, 64));
      const unsigned long long bal = __ballot(bi != INT_MAX && bv == mv);
      const int src = bal ? __ffsll((long long)bal) - 1 : 0;
      int wi = __shfl(bi, src, 64);
      if (!bal) wi = INT_MAX;
      const int par = (k & 1) * 4;
      if (l == 0) {
        s_slotv[par + w] = mv;
        s_sloti[par + w] = wi;
      }
      __syncthreads();
      double gv = INF;
      int gi = INT_MAX;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double v2 = s_slotv[par + u];
        const int i2 = s_sloti[par + u];
        if (i2 != INT_MAX && (v2 < gv || gi == INT_MAX)) {
          gv = v2;
          gi = i2;
        }
      }
      // (k < n - 1: a vertex is left, so gi is one; the clamp keeps a corrupt date inside its rows)
      gi = min(max(gi, 0), n - 1);
      if ((gi >> 2) == t) done |= 1u << (gi & 3);
      if (t == 0) {
        s_ekey[k] = gv;
        s_pv[k + 1] = (u16)gi;
      }
      xc = gi;
    }
    // the row of the last vertex: read for its check alone, so that every row is checked
    double sv[HRP_PER];
    load_row(xc, sv);
#pragma unroll
    for (int q = 0; q < HRP_PER; ++q)
      if (j0 + q < n && j0 + q != xc && !isfinite(sv[q])) bad = 1;
  } else {
    // ---- the distance matrix: the upper triangle of S, mirrored ------------------------------
    double* Wb = work + (int64_t)b * n * ldw;
    const bool vecw = (reinterpret_cast<uintptr_t>(Wb) & 15) == 0 && (ldw & 1) == 0 && j0 + 3 < n;
    {
      double isdj[HRP_PER];
#pragma unroll
      for (int q = 0; q < HRP_PER; ++q) isdj[q] = j0 + q < n ? s_isd[j0 + q] : 0.0;
      constexpr int RU = 4;   // rows in flight
      for (int r0 = 0; r0 < n; r0 += RU) {
        double sv[RU][HRP_PER];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          const double* row = Sb + (int64_t)min(r0 + u, n - 1) * ld;
          if (vec) {
            const double2 p0 = *reinterpret_cast<const double2*>(row + j0);
            const double2 p1 = *reinterpret_cast<const double2*>(row + j0 + 2);
            sv[u][0] = p0.x; sv[u][1] = p0.y; sv[u][2] = p1.x; sv[u][3] = p1.y;
          } else {
#pragma unroll
            for (int q = 0; q < HRP_PER; ++q) sv[u][q] = j0 + q < n ? row[j0 + q] : 0.0;   // never past column n
          }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          const int r = r0 + u;
          if (r >= n) break;
          const double ix = s_isd[r];
          double* wrow = Wb + (int64_t)r * ldw;
#pragma unroll
          for (int q = 0; q < HRP_PER; ++q) {
            const int j = j0 + q;
            if (j >= n) continue;
            if (j == r) {
              wrow[j] = 0.0;
              continue;
            }
            if (!isfinite(sv[u][q])) bad = 1;   // every entry, though only the upper ones are used
            if (j < r) continue;
            const double rho = fmin(fmax((a * sv[u][q]) * (ix * isdj[q]), -1.0), 1.0);   // Prim's key: ties stay exact
            const double dv = sqrt(0.5 * (1.0 - rho));
            wrow[j] = dv;
            Wb[(int64_t)j * ldw + r] = dv;
          }
        }
      }
    }
    bad = (int)block_max((double)bad, red);   // (its barriers publish D)
    if (bad) {   // (uniform) before the chain: it must only ever see finite numbers
      fail();
      return;
    }

    // ---- the nearest-neighbour chain ------------------------------------------------------------
    u16* s_chain = s_c0;
    u16* s_mx = s_pv;                                  // the slots of merge k, x < y
    u16* s_my = s_end;
    // (past the four doubles the block reductions use: a wave may still be reading those)
    double* s_dxy = red + 4;                           // 2: D_xy of a scan, double-buffered
    int* s_nsz = reinterpret_cast<int*>(red + 6);      // 2 x 2: the sizes of x and y, likewise
    int* s_low = s_nsz + 4;                            // 4: the waves' lowest live columns
    auto load_wrow = [&](int r, double (&dv)[HRP_PER]) {
      const double* row = Wb + (int64_t)r * ldw;
      if (vecw) {
        const double2 p0 = *reinterpret_cast<const double2*>(row + j0);
        const double2 p1 = *reinterpret_cast<const double2*>(row + j0 + 2);
        dv[0] = p0.x; dv[1] = p0.y; dv[2] = p1.x; dv[3] = p1.y;
      } else {
#pragma unroll
        for (int q = 0; q < HRP_PER; ++q) dv[q] = j0 + q < n ? row[j0 + q] : 0.0;
      }
    };
    int sz[HRP_PER];   // the cluster in column j0 + q; 0: dead (or past n)
#pragma unroll
    for (int q = 0; q < HRP_PER; ++q) sz[q] = j0 + q < n ? 1 : 0;
    const int ne = n - 1;
    int len = 1, top = 0, prev = 0, merges = 0;   // an empty chain starts at the lowest live index
    if (t == 0) s_chain[0] = 0;
    for (int step = 0; step < 4 * n && merges < ne; ++step) {
      double rv[HRP_PER];
      load_wrow(top, rv);
      double bv = INF;
      int bi = INT_MAX;
#pragma unroll
      for (int q = 0; q < HRP_PER; ++q)
        if (sz[q] > 0 && j0 + q != top && rv[q] < bv) {   // strict <: the lowest index among the minima
          bv = rv[q];
          bi = j0 + q;
        }
      double mv = bv;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mv = fmin(mv, __shfl_xor(mv, o, 64));
      const unsigned long long bal = __ballot(bi != INT_MAX && bv == mv);
      const int src = bal ? __ffsll((long long)bal) - 1 : 0;
      int wi = __shfl(bi, src, 64);
      if (!bal) wi = INT_MAX;
      const int par = step & 1;
      if (l == 0) {
        s_slotv[par * 4 + w] = mv;
        s_sloti[par * 4 + w] = wi;
      }
      if ((top >> 2) == t) s_nsz[par * 2] = sz[top & 3];
      if (len >= 2 && (prev >> 2) == t) {
        s_nsz[par * 2 + 1] = sz[prev & 3];
        s_dxy[par] = rv[prev & 3];
      }
      __syncthreads();
      double gv = INF;
      int gi = INT_MAX;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double v2 = s_slotv[par * 4 + u];
        const int i2 = s_sloti[par * 4 + u];
        if (i2 != INT_MAX && v2 < gv) {
          gv = v2;
          gi = i2;
        }
      }
      const double dxy = len >= 2 ? s_dxy[par] : INF;
      if (!(len >= 2 && !(gv < dxy))) {
        // a strictly nearer neighbour than the previous element: push it
        if (gi == INT_MAX || len >= n) {   // (uniform; not with finite distances)
          bad = 1;
          break;
        }
        gi = min(max(gi, 0), n - 1);
        if (t == 0) s_chain[len] = (u16)gi;
        prev = top;
        top = gi;
        ++len;
        continue;
      }
      // the previous element is the nearest: merge the two
      const bool topx = top < prev;
      const int mx = topx ? top : prev, my = topx ? prev : top;
      const int nx = s_nsz[par * 2 + (topx ? 0 : 1)], ny = s_nsz[par * 2 + (topx ? 1 : 0)];
      double pv[HRP_PER], nv[HRP_PER];
      load_wrow(prev, pv);
      bool any = false;
#pragma unroll
      for (int q = 0; q < HRP_PER; ++q) {
        const int j = j0 + q;
        const double dxi = topx ? rv[q] : pv[q], dyi = topx ? pv[q] : rv[q];
        const bool upd = sz[q] > 0 && j != mx && j != my;
        nv[q] = upd ? hrp_lance_williams<M>(dxi, dyi, dxy, nx, ny, sz[q]) : dyi;
        if (upd) Wb[(int64_t)j * ldw + my] = nv[q];
        any |= upd;
      }
      double* yrow = Wb + (int64_t)my * ldw;
      if (vecw) {   // (the entries of dead columns are rewritten as they were)
        if (any) {
          *reinterpret_cast<double2*>(yrow + j0) = make_double2(nv[0], nv[1]);
          *reinterpret_cast<double2*>(yrow + j0 + 2) = make_double2(nv[2], nv[3]);
        }
      } else {
#pragma unroll
        for (int q = 0; q < HRP_PER; ++q)
          if (sz[q] > 0 && j0 + q != mx && j0 + q != my) yrow[j0 + q] = nv[q];   // never past column n
      }
      if (t == 0) {
        s_ekey[merges] = dxy;
        s_mx[merges] = (u16)mx;
        s_my[merges] = (u16)my;
      }
      if ((mx >> 2) == t) sz[mx & 3] = 0;
      if ((my >> 2) == t) sz[my & 3] = nx + ny;
      int lj = INT_MAX;
#pragma unroll
      for (int q = HRP_PER - 1; q >= 0; --q)
        if (sz[q] > 0) lj = j0 + q;
      const unsigned long long lbal = __ballot(lj != INT_MAX);
      const int lw = __shfl(lj, lbal ? __ffsll((long long)lbal) - 1 : 0, 64);
      if (l == 0) s_low[w] = lbal ? lw : INT_MAX;
      ++merges;
      len -= 2;
      __syncthreads();   // publishes the new row and column y
      if (len == 0) {
        int low = INT_MAX;
#pragma unroll
        for (int u = 3; u >= 0; --u)
          if (s_low[u] != INT_MAX) low = s_low[u];   // (waves are in column order)
        top = min(max(low, 0), n - 1);
        prev = top;
        len = 1;
        if (t == 0) s_chain[0] = (u16)top;
      } else {
        top = s_chain[len - 1];
        prev = len >= 2 ? s_chain[len - 2] : top;
      }
    }
    if (merges < ne) bad = 1;   // (uniform) the cap: the failure path
  }
  bad = (int)block_max((double)bad, red);
  if (bad) {   // (uniform)
    fail();
    return;
  }

  // ---- the stable sort of the edges: bitonic on (key, insertion index) ----------------------
  const int ne = n - 1;
  int N2 = 1;
  while (N2 < ne) N2 <<= 1;
  for (int i = t; i < N2; i += HRP_NT) {
    if (i >= ne) s_ekey[i] = INF;
    s_sidx[i] = (u16)i;
  }
  for (int kk = 2; kk <= N2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = t; i < N2; i += HRP_NT) {
        const int p = i ^ j;
        if (p > i) {
          const double ki = s_ekey[i], kp = s_ekey[p];
          const u16 ii = s_sidx[i], ip = s_sidx[p];
          const bool gt = ki > kp || (ki == kp && ii > ip);
          if (gt == ((i & kk) == 0)) {
            s_ekey[i] = kp; s_ekey[p] = ki;
            s_sidx[i] = ip; s_sidx[p] = ii;
          }
        }
      }
    }
  }
  __syncthreads();
  // the smallest gap between consecutive merge distances (the isd reads are long done: the
  // run arrays may take their place)
  double gap = INF;
  u16* s_par = s_idat;          // the union-find of the chain's merges: parent and size of the
  u16* s_usz = s_idat + 2 * na;   // ids below 2 n - 1 (the four u16 arrays 1 / sd leaves)
  if constexpr (M == PQ_HRP_SINGLE) {
    for (int i = t; i + 1 < ne; i += HRP_NT) gap = fmin(gap, sqrt(0.5 * s_ekey[i + 1]) - sqrt(0.5 * s_ekey[i]));
    for (int p = t; p < n; p += HRP_NT) {
      s_idat[p] = s_pv[p];
      s_start[p] = (u16)p;
      s_end[p] = (u16)p;
    }
  } else {   // (the chain recorded distances, not keys)
    for (int i = t; i + 1 < ne; i += HRP_NT) gap = fmin(gap, s_ekey[i + 1] - s_ekey[i]);
    for (int i = t; i < 2 * n - 1; i += HRP_NT) {
      s_par[i] = (u16)i;
      s_usz[i] = 1;
    }
  }
  gap = -block_max(-gap, red);

  // ---- the merges, then the leaves' offsets (lane 0; both are serial chains) -----------------
  if (t == 0) {
    for (int m = 0; m < ne; ++m) {
      const int k = s_sidx[m];
      if constexpr (M == PQ_HRP_SINGLE) {
        const int sl = s_start[k], er = s_end[k + 1];
        const int idl = s_idat[sl], idr = s_idat[k + 1];
        s_c0[m] = (u16)min(idl, idr);
        s_c1[m] = (u16)max(idl, idr);
        s_cs[m] = (u16)(er - sl + 1);
        s_idat[sl] = (u16)(n + m);
        s_end[sl] = (u16)er;
        s_start[er] = (u16)sl;
      } else {   // SciPy's label(): the roots of the recorded slots, the sizes the union-find's
        auto find = [&](int v) {
          int r = v;
          while (s_par[r] != r) r = s_par[r];
          while (s_par[v] != r) {   // path compression
            const int up = s_par[v];
            s_par[v] = (u16)r;
            v = up;
          }
          return r;
        };
        const int ra = find(s_pv[k]), rb = find(s_end[k]);
        const int cs = s_usz[ra] + s_usz[rb];
        s_par[ra] = s_par[rb] = (u16)(n + m);
        s_usz[n + m] = (u16)cs;
        s_c0[m] = (u16)min(ra, rb);
        s_c1[m] = (u16)max(ra, rb);
        s_cs[m] = (u16)cs;
      }
    }
    u16* s_off = s_end;   // (the runs are done)
    s_off[ne - 1] = 0;
    for (int m = ne - 1; m >= 0; --m) {
      const int o = s_off[m], a0 = s_c0[m], a1 = s_c1[m];
      const int z0 = a0 < n ? 1 : s_cs[a0 - n];
      if (a0 < n) s_order[o] = (u16)a0; else s_off[a0 - n] = (u16)o;
      if (a1 < n) s_order[o + z0] = (u16)a1; else s_off[a1 - n] = (u16)(o + z0);
    }
  }
  __syncthreads();
  if (lb) {
    for (int m = t; m < ne; m += HRP_NT) {
      double* z = lb + 4 * m;
      z[0] = (double)s_c0[m];
      z[1] = (double)s_c1[m];
      z[2] = M == PQ_HRP_SINGLE ? sqrt(0.5 * s_ekey[m]) : s_ekey[m];
      z[3] = (double)s_cs[m];
    }
  }
  for (int p = t; p < n; p += HRP_NT) ob[p] = s_order[p];
  __syncthreads();   // the tree's arrays are dead from here

  // ---- bisection ------------------------------------------------------------------------------
  for (int p = t; p < n; p += HRP_NT) s_wt[p] = s_dinv[s_order[p]];
  __syncthreads();
  double* s_tmp = s_dinv;   // (iv by asset is dead)
  int maxlvl = 0;           // the deepest level with a node of two or more positions
  while (((n + (2 << maxlvl) - 1) >> (maxlvl + 1)) >= 2) ++maxlvl;

  // the cross blocks of level lvl with the weights s_wt: f(p, wt_p sum_{q in right} S_pq wt_q) for
  // every position p of a left half; lane groups of G lanes per row, RU rows per group and round,
  // and every load of a round issued before the first is used (KU per lane and row: the gathers
  // are latency-bound)
  auto cross = [&](int lvl, auto f) {
    const int maxL = (n + (1 << lvl) - 1) >> lvl;
    const int maxLeft = maxL >> 1, maxRight = maxL - maxLeft;
    int G = 1;
    while (G < maxRight && G < 64) G <<= 1;
    const int R = 64 / G, tasks = maxLeft << lvl;
    const int g = l / G, s = l & (G - 1);
    auto run = [&](auto ku_, auto ru_) {
      constexpr int KU = decltype(ku_)::value, RU = decltype(ru_)::value;
      for (int base = 0; base < tasks; base += 4 * R * RU) {
        double v[RU][KU], wq[RU][KU];
        int pp[RU];
        bool val[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          const int task = base + (u * 4 + w) * R + g;
          const int m = task / maxLeft, r = task - m * maxLeft;
          int lo, hi;
          hrp_node(n, lvl, m, lo, hi);
          const int mid = lo + ((hi - lo) >> 1);
          val[u] = task < tasks && hi - lo >= 2 && r < mid - lo;
          pp[u] = val[u] ? lo + r : 0;
          const double* row = Sb + (int64_t)s_order[pp[u]] * ld;
#pragma unroll
          for (int i = 0; i < KU; ++i) {
            const int q = mid + s + i * G;
            const bool ok = val[u] && q < hi;
            v[u][i] = ok ? row[s_order[q]] : 0.0;
            wq[u][i] = ok ? s_wt[q] : 0.0;
          }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          double acc = 0.0;
#pragma unroll
          for (int i = 0; i < KU; ++i) acc = fma(v[u][i], wq[u][i], acc);
          for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
          if (val[u] && s == 0) f(pp[u], s_wt[pp[u]] * acc);
        }
      }
    };
    // (G = 64 below PQ_HRP_NMAX / 2 = 8 x 64 columns of a right half)
    if (maxRight <= G) run(std::integral_constant<int, 1>{}, std::integral_constant<int, 4>{});
    else run(std::integral_constant<int, 8>{}, std::integral_constant<int, 2>{});
  };

  for (int lvl = 0; lvl <= maxlvl; ++lvl) {
    cross(lvl, [&](int p, double v) { s_tmp[p] = v; });
    __syncthreads();
    for (int m = w; m < (1 << lvl); m += 4) {   // X of node m: the sum over its left half's rows
      int lo, hi;
      hrp_node(n, lvl, m, lo, hi);
      if (hi - lo < 2) continue;
      const int mid = lo + ((hi - lo) >> 1);
      double v = 0.0;
      for (int p = lo + l; p < mid; p += 64) v += s_tmp[p];
      v = wave_sum(v);
      if (l == 0) s_Q[(1 << lvl) + m] = v;
    }
    __syncthreads();
  }
  // Q, sum iv and the split alpha of every node, the deepest level first
  double* s_al = s_tmp;
  for (int lvl = maxlvl; lvl >= 0; --lvl) {
    for (int m = t; m < (1 << lvl); m += HRP_NT) {
      int lo, hi;
      hrp_node(n, lvl, m, lo, hi);
      if (hi - lo < 2) continue;
      const int mid = lo + ((hi - lo) >> 1), h = (1 << lvl) + m;
      const bool ll = mid - lo == 1, rl = hi - mid == 1;
      const double Ql = ll ? s_wt[lo] : s_Q[2 * h], sl = ll ? s_wt[lo] : s_siv[2 * h];
      const double Qr = rl ? s_wt[mid] : s_Q[2 * h + 1], sr = rl ? s_wt[mid] : s_siv[2 * h + 1];
      s_Q[h] = (Ql + Qr) + 2.0 * (a * s_Q[h]);
      s_siv[h] = sl + sr;
      const double vl = Ql / (sl * sl), vr = Qr / (sr * sr);
      s_al[h] = 1.0 - vl / (vl + vr);
    }
    __syncthreads();
  }
  // the weights: the product of the splits on the way down, the root's first
  double wp[HRP_PER], dterm = 0.0;
#pragma unroll
  for (int q = 0; q < HRP_PER; ++q) {
    const int p = t + q * HRP_NT;
    wp[q] = 1.0;
    if (p < n) {
      int h = 1, lo = 0, hi = n;
      double wv = 1.0;
      while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        const double al = s_al[h];
        if (p < mid) {
          wv *= al;
          h = 2 * h;
          hi = mid;
        } else {
          wv *= 1.0 - al;
          h = 2 * h + 1;
          lo = mid;
        }
      }
      wp[q] = wv;
      dterm += wv * wv / s_wt[p];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < HRP_PER; ++q) {
    const int p = t + q * HRP_NT;
    if (p < n) {
      s_wt[p] = wp[q];
      xb[s_order[p]] = scale * wp[q];
    }
  }
  __syncthreads();
  // x' Sigma x = scale^2 (sum w_p^2 d_p + 2 alpha sum of the cross blocks under w)
  double vacc = 0.0;
  for (int lvl = 0; lvl <= maxlvl; ++lvl) cross(lvl, [&](int, double v) { vacc += v; });
  const double var = block_sum(fma(2.0 * a, vacc, dterm), red);
  if (t == 0) {
    stats[(int64_t)b * 2] = scale * scale * var;
    stats[(int64_t)b * 2 + 1] = gap;
    status[b] = PQ_HRP_OK;
  }
}

__global__ __launch_bounds__(HRP_NT) void k_hrp(
    const double* __restrict__ S, int64_t ld, int n, const double* __restrict__ av,
    const double* __restrict__ cv, double scale, double* __restrict__ x, int64_t ldx,
    int32_t* __restrict__ order, int64_t ldo, double* __restrict__ link, double* __restrict__ stats,
    int32_t* __restrict__ status) {
  hrp_date<PQ_HRP_SINGLE>(S, ld, n, av, cv, scale, x, ldx, order, ldo, link, stats, status, nullptr, 0);
}

template <int M>
__global__ __launch_bounds__(HRP_NT) void k_hrp_link(
    const double* __restrict__ S, int64_t ld, int n, const double* __restrict__ av,
    const double* __restrict__ cv, double scale, double* work, int64_t ldw, double* __restrict__ x, int64_t ldx,
    int32_t* __restrict__ order, int64_t ldo, double* __restrict__ link, double* __restrict__ stats,
    int32_t* __restrict__ status) {
  hrp_date<M>(S, ld, n, av, cv, scale, x, ldx, order, ldo, link, stats, status, work, ldw);
}

// the host-checkable arguments the two entry points share
static int hrp_check_args(const char* who, const double* S, int64_t ld, int32_t n, int32_t batch, const double* alpha,
                          const double* c, double scale, const double* x, int64_t ldx, const int32_t* order,
                          int64_t ldo, const double* stats, const int32_t* status) {
  PQ_CHECK_ARG(S && alpha && c && x && order && stats && status, "%s: null argument", who);
  PQ_CHECK_ARG(n >= 1 && n <= PQ_HRP_NMAX, "%s: n = %d outside [1, %d]", who, n, PQ_HRP_NMAX);
  PQ_CHECK_ARG(batch >= 0, "%s: batch = %d < 0", who, batch);
  PQ_CHECK_ARG(ld >= n, "%s: ld = %lld < n = %d", who, (long long)ld, n);
  PQ_CHECK_ARG(ldx >= n && ldo >= n, "%s: ldx = %lld, ldo = %lld must be >= n = %d", who, (long long)ldx,
               (long long)ldo, n);
  PQ_CHECK_ARG(scale == scale, "%s: scale is NaN", who);
  return 0;
}

}  // namespace pq

extern "C" int pq_hrp_batched(const double* S, int64_t ld, int32_t n, int32_t batch, const double* alpha,
                              const double* c, double scale, double* x, int64_t ldx, int32_t* order, int64_t ldo,
                              double* link, double* stats, int32_t* status, void* stream) {
  if (int rc = pq::hrp_check_args("pq_hrp_batched", S, ld, n, batch, alpha, c, scale, x, ldx, order, ldo, stats, status))
    return rc;
  if (batch == 0) return 0;
  static_assert(pq::hrp_lds_bytes(PQ_HRP_NMAX) <= 48 * 1024, "the default dynamic LDS limit");
  hipLaunchKernelGGL(pq::k_hrp, dim3(batch), dim3(pq::HRP_NT), pq::hrp_lds_bytes(n), (hipStream_t)stream, S, ld, n,
                     alpha, c, scale, x, ldx, order, ldo, link, stats, status);
  PQ_CHECK_LAUNCH("pq_hrp_batched");
  return 0;
}

extern "C" int pq_hrp_linkage_batched(const double* S, int64_t ld, int32_t n, int32_t batch, const double* alpha,
                                      const double* c, double scale, int32_t method, double* work, int64_t ldw,
                                      double* x, int64_t ldx, int32_t* order, int64_t ldo, double* link,
                                      double* stats, int32_t* status, void* stream) {
  const char* who = "pq_hrp_linkage_batched";
  PQ_CHECK_ARG(method >= PQ_HRP_SINGLE && method <= PQ_HRP_WARD, "%s: method = %d outside [%d, %d]", who, method,
               PQ_HRP_SINGLE, PQ_HRP_WARD);
  if (method == PQ_HRP_SINGLE)
    return pq_hrp_batched(S, ld, n, batch, alpha, c, scale, x, ldx, order, ldo, link, stats, status, stream);
  if (int rc = pq::hrp_check_args(who, S, ld, n, batch, alpha, c, scale, x, ldx, order, ldo, stats, status)) return rc;
  PQ_CHECK_ARG(work, "%s: work is NULL (only PQ_HRP_SINGLE needs none)", who);
  PQ_CHECK_ARG(ldw >= n, "%s: ldw = %lld < n = %d", who, (long long)ldw, n);
  if (batch == 0) return 0;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(pq::HRP_NT), pq::hrp_lds_bytes(n), (hipStream_t)stream, S, ld, n,
                       alpha, c, scale, work, ldw, x, ldx, order, ldo, link, stats, status);
  };
  switch (method) {
    case PQ_HRP_COMPLETE: launch(pq::k_hrp_link<PQ_HRP_COMPLETE>); break;
    case PQ_HRP_AVERAGE: launch(pq::k_hrp_link<PQ_HRP_AVERAGE>); break;
    case PQ_HRP_WEIGHTED: launch(pq::k_hrp_link<PQ_HRP_WEIGHTED>); break;
    default: launch(pq::k_hrp_link<PQ_HRP_WARD>); break;
  }
  PQ_CHECK_LAUNCH(who);
  return 0;
}
