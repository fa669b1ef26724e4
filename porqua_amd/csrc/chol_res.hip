// K2R: Cholesky + explicit inverse of one small matrix per workgroup with the lower triangle
// RESIDENT in the registers of the workgroup's eight waves (n <= 288: the slide groups' M_U,
// 250 problems of valid size <= 284 at the headline config, one per CU).
//
// Why: k_factor_sk keeps the matrix in global memory and streams every 64 x 64 tile GEMM
// through LDS in 16-deep chunks, so its time is a dependent chain of global round trips
// (569 us for ~75 us of FP64 MFMA work).  Here K is read once (through form_elem, the single
// source of the matrix), potrf / trtri / lauum run on 16 x 16 tiles that never leave the CU,
// and K^-1 is written once.  Only the plain form p_scale P + (p_diag + sigma) I is taken (mg = 0,
// no box: factor_res_supports): with those known at compile time form_elem's general-row loop
// and box term fold away in the 30 unrolled tile loads; the other forms keep k_factor(_sk).
//
// Budget.  The lower triangle of 18 x 18 tiles is 171 tiles = 342 KB; the CU has 512 KB of
// vector registers and 160 KB of LDS.  512 threads = 8 waves, 2 per SIMD, 256 registers
// each.  Tiles are owned by block ROW: wave w holds rows 17 - w (18 - w tiles) and 2 + w
// (3 + w tiles), 21 tiles each, and waves 7 / 6 also rows 0 / 1 (1 / 2 tiles): at most 23
// tiles = 184 VGPRs per lane, which leaves ~70 for operands and the pivot chain.  The long
// row is indexed from the front of the tile array and the short one from its back, so every
// tile's register index is a compile-time function of (slot, block column) although the rows
// differ from wave to wave (no dynamic register indexing).  The compiler ends at 256 VGPRs, 0 AGPRs and
// 32 spilled dwords (132 B of scratch per lane, four tiles parked around trtri's column loop, not
// inside the product loops): profiles/r07_chol_res_resource_usage.txt.  Pairing a long row
// with a short one also balances the waves: potrf's trailing update, trtri's row products
// and lauum's accumulation all cost row I a number of tile products that grows with I.
// (4 waves x 512 registers would need the tiles split over VGPRs and AGPRs by hand; 8 x 256
// stays in plain VGPRs.)  LDS: two panel buffers of 18 tile images (pitch 17: the direct and
// the transposed access are both at most 2-way bank conflicted) = 76.5 KB, two diagonal
// images, 2 ints: ~81 KB.
//
// Tiles are kept in polish_rt.hip's "stored" form S(X): lane l, register q holds
// X[l & 15][(l >> 4) + 4 q], so that  mfma(a = S(P), b = S(Q))  accumulates  S(Q P^T).
// An LDS image of Y answers get -> S(Y) and getT -> S(Y^T); putT(S(Z)) writes the image of
// Z^T.  Per 16-wide block column J (block loops are rolled; the tile a step touches is picked
// by compile-time matching of its register index):
//   potrf  the owner of row J factors and inverts A_JJ in registers (wave_chol_inv16) and
//          publishes L_JJ^-1; after a barrier every wave forms its panel tiles
//          L_IJ = A_IJ L_JJ^-T and publishes them; after a second barrier every wave updates
//          its own trailing tiles A_IJ' -= L_IJ L_J'J^T from the published panel.  Diagonal
//          tiles keep L_JJ^-1.
//   trtri  columns right to left: column J of L is published transposed, then row I forms
//          X_IJ = -(sum_{K=J+1..I} X_IK L_KJ) L_JJ^-1 from its own registers.
//   lauum  rows top to bottom: the owner publishes row K of X transposed, its registers
//          become the accumulators of output row K, and every output tile (I, J), J <= I <= K,
//          adds X_KI^T X_KJ.  No second copy of the triangle.
// Output: K^-1 at pitch ld, lower triangle (and the upper triangle of the diagonal 64 x 64
// blocks) for invert == 1, both triangles for invert == 2 -- the region k_factor_sk defines --
// with the identity in the padding rows / columns; every global store writes 16-double row
// segments.  st.Dt is NOT written: after an inverting factor nothing reads it (the polish
// kernels and chol_large.hip fill Dt themselves before their solves; the ADMM kernels and
// k_gcap_prep read K^-1 only).
// Failure: a non-positive or non-finite pivot ends the problem with info = 1 + the first
// column of its 16-column block and status = PQ_NON_CONVEX (uniform branch).
//
// Replaces, for few small problems: k_factor_sk (chol.hip), i.e. isPD's np.linalg.cholesky
// and the KKT factorisation inside qpsolvers' backends.
#include "chol_dev.h"
#include "chol_res.h"

namespace pq {
namespace {

constexpr int RNB = PQ_RES_NMAX / 16;   // block rows of the resident triangle
constexpr int RNT = 23;                 // tile registers per wave
constexpr int RIMG = 16 * 17;           // doubles per LDS tile image

// slot 0: row 17 - w, tile j at j; slot 1: row 2 + w, tile j at 20 - j; slot 2: row 0 (wave
// 7) or 1 (wave 6), tile j at 21 + j
__device__ constexpr int slot_len(int s) { return s == 0 ? 18 : (s == 1 ? 10 : 2); }
__device__ constexpr int tix(int s, int j) { return s == 0 ? j : (s == 1 ? 20 - j : 21 + j); }

__device__ __forceinline__ f64x4 img_get(const double* img, int od) {
  f64x4 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = img[od + 68 * q];
  return v;
}
__device__ __forceinline__ void img_put(double* img, int od, const f64x4& v) {
#pragma unroll
  for (int q = 0; q < 4; ++q) img[od + 68 * q] = v[q];
}
__device__ __forceinline__ f64x4 img_getT(const double* img, int ot) {
  f64x4 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = img[ot + 4 * q];
  return v;
}
__device__ __forceinline__ void img_putT(double* img, int ot, const f64x4& v) {
#pragma unroll
  for (int q = 0; q < 4; ++q) img[ot + 4 * q] = v[q];
}
// c + S(Q P^T) for a = S(P), b = S(Q)
__device__ __forceinline__ f64x4 mma4(const f64x4& a, const f64x4& b, f64x4 c) {
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s4], b[s4], c, 0, 0, 0);
  return c;
}

#ifdef PQ_PROFILE
// wall-clock ticks (100 MHz) of load / potrf / trtri / lauum / store, per workgroup of the last launch
__device__ long long g_res_prof[PQ_RES_PROF_BLOCKS * 8];
#define RSTAMP(k_)                                                                        \
  do {                                                                                    \
    __syncthreads();                                                                      \
    if (threadIdx.x == 0) { const long long n_ = wall_clock64(); pclk[k_] = n_ - tclk; tclk = n_; } \
  } while (0)
#else
#define RSTAMP(k_) do { } while (0)
#endif

// every (slot, block column) of the tile array, compile-time indices after unrolling
#define RES_TILES(s_, j_)                         \
  _Pragma("unroll") for (int s_ = 0; s_ < 3; ++s_) \
  _Pragma("unroll") for (int j_ = 0; j_ < RNB; ++j_) \
  if (j_ < slot_len(s_))

__global__ __launch_bounds__(512, 1) void k_factor_res(pq_problem pb, pq_state st, const int32_t* idx,
                                                    int nidx, pq_settings s, int invert) {
  __shared__ __attribute__((aligned(16))) double pan[2 * RNB * RIMG];
  __shared__ double dgi[2 * RIMG];
  __shared__ int s_bad[2];
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int l = threadIdx.x & 63, c16 = l & 15, g = l >> 4;
  const int b = idx ? idx[blockIdx.x] : (int)blockIdx.x;
  const int ld = pb.ld, n = pb.n;
  const int nbv = (n + 15) >> 4;   // block rows that hold the matrix (the rest: identity padding)
  double* K = st.K + (int64_t)b * st.K_stride;
  FormCtx f;
  f.P = pb.P + (int64_t)b * pb.P_stride;
  f.ld = ld; f.n = n; f.mg = pb.mg;
  f.ps = pb.p_scale ? pb.p_scale[b] : 1.0;
  f.pd = pb.p_diag ? pb.p_diag[b] : 0.0;
  f.sigma = s.sigma;
  f.Cg = pb.Cg ? pb.Cg + (int64_t)b * pb.Cg_stride : nullptr;
  f.lb = pb.lb ? pb.lb + (int64_t)b * pb.box_stride : nullptr;
  f.ub = pb.ub ? pb.ub + (int64_t)b * pb.box_stride : nullptr;
  f.rho = st.rho[b]; f.rho_min = s.rho_min; f.eq_scale = s.eq_scale;
  f.lg = pb.mg ? pb.lg + (int64_t)b * pb.g_stride : nullptr;
  f.ug = pb.mg ? pb.ug + (int64_t)b * pb.g_stride : nullptr;
#ifdef PQ_PROFILE
  long long pclk[5] = {0, 0, 0, 0, 0};
  long long tclk = wall_clock64();
#endif

#define RES_ROWS(w_) {RNB - 1 - (w_), 2 + (w_), (w_) == 7 ? 0 : ((w_) == 6 ? 1 : -1)}
  const int rows0[3] = RES_ROWS(w);
  const f64x4 zero4 = f64x4{0.0, 0.0, 0.0, 0.0};
  f64x4 T[RNT];
#pragma unroll
  for (int i = 0; i < RNT; ++i) T[i] = zero4;

  // ---- load: each lower tile once, every tile of the wave in one memory round trip; a diagonal
  // tile takes both triangles from the lower one.  (mg = 0 and no box, known at compile time here:
  // form_elem's general-row loop and box term fold away; see factor_res_supports) ----
  {
    FormCtx fp = f;
    fp.mg = 0;
    fp.lb = fp.ub = nullptr;
    RES_TILES(sl, j) {
      const int I = rows0[sl];
      if (I >= 0 && I < nbv && j <= I) {   // uniform
        const int gi = 16 * I + c16;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int gj = 16 * j + g + 4 * q;
          T[tix(sl, j)][q] = form_elem(fp, gi > gj ? gi : gj, gi > gj ? gj : gi);
        }
      }
    }
  }
  RSTAMP(0);

  // ---- potrf ------------------------------------------------------------------------------------
  int info = 0;
#pragma unroll 1
  for (int J = 0; J < nbv; ++J) {
    const int wz = w + loop_zero();   // (the per-tile conditions are not hoisted out of the loop)
    const int rows[3] = RES_ROWS(wz);
    const int lz = l + loop_zero(), od = (lz >> 4) * 17 + (lz & 15), ot = (lz & 15) * 17 + (lz >> 4);
    const double* pn = pan + (J & 1) * (RNB * RIMG);
    double* pnw = pan + (J & 1) * (RNB * RIMG);
    double* dg = dgi + (J & 1) * RIMG;
    bool own = false;   // the owner of the diagonal tile (uniform)
    f64x4 d = zero4;
    RES_TILES(sl, j) {
      if (rows[sl] == J && j == J) {
        d = T[tix(sl, j)];
        own = true;
      }
    }
    if (own) {
      double A[4], Bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        A[q] = d[q];                   // symmetric: stored form = C layout
        Bv[q] = (g + 4 * q == c16) ? 1.0 : 0.0;
      }
      const int bad = wave_chol_inv16(A, Bv, l);
      // Bv = L_JJ^-1 in C layout = S(L_JJ^-T): the image of L_JJ^-1
      img_putT(dg, ot, f64x4{Bv[0], Bv[1], Bv[2], Bv[3]});
      if (l == 0) s_bad[J & 1] = bad;
    }
    __syncthreads();
    if (s_bad[J & 1]) {   // uniform
      info = 16 * J + 1;
      break;
    }
    const f64x4 Li = img_get(dg, od);   // S(L_JJ^-1)
    RES_TILES(sl, j) {
      const int I = rows[sl];
      if (j == J && I >= J && I < nbv) {
        if (I == J) {
          T[tix(sl, j)] = Li;
        } else {   // S(L_IJ) = S(A_IJ L_JJ^-T)
          const f64x4 p = mma4(Li, T[tix(sl, j)], zero4);
          T[tix(sl, j)] = p;
          img_put(pnw + I * RIMG, od, p);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
      const int I = rows[sl];
      if (I > J && I < nbv) {
        const f64x4 bI = img_get(pn + I * RIMG, od);   // S(L_IJ)
#pragma unroll
        for (int jp = 0; jp < RNB; ++jp) {
          if (jp < slot_len(sl)) {
            if (jp > J && jp <= I) {   // S(A_IJ') -= S(L_IJ L_J'J^T)
              const f64x4 a = img_get(pn + jp * RIMG, od);
              T[tix(sl, jp)] = mma4(-a, bI, T[tix(sl, jp)]);
            }
          }
        }
      }
    }
  }
  if (threadIdx.x == 0) {
    st.info[b] = info;
    if (info) st.status[b] = PQ_NON_CONVEX;
  }
  if (info) return;   // uniform
  RSTAMP(1);

  // ---- trtri: X = L^-1 in place, block columns right to left -------------------------------------
  __syncthreads();
#pragma unroll 1
  for (int J = nbv - 2; J >= 0; --J) {
    const int wz = w + loop_zero();   // (the per-tile conditions are not hoisted out of the loop)
    const int rows[3] = RES_ROWS(wz);
    const int lz = l + loop_zero(), od = (lz >> 4) * 17 + (lz & 15), ot = (lz & 15) * 17 + (lz >> 4);
    double* pn = pan + (J & 1) * (RNB * RIMG);
    double* dg = dgi + (J & 1) * RIMG;
    RES_TILES(sl, j) {
      const int I = rows[sl];
      if (j == J && I >= J && I < nbv) {
        if (I == J) img_putT(dg, ot, T[tix(sl, j)]);             // image of L_JJ^-T
        else img_putT(pn + I * RIMG, ot, T[tix(sl, j)]);         // image of L_IJ^T
      }
    }
    __syncthreads();
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
      const int I = rows[sl];
      if (I > J && I < nbv) {
        f64x4 acc = zero4;   // S(sum_K X_IK L_KJ), K = J + 1 .. I
#pragma unroll
        for (int k = 0; k < RNB; ++k) {
          if (k < slot_len(sl)) {
            if (k > J && k <= I) {
              const f64x4 a = img_get(pn + k * RIMG, od);   // S(L_KJ^T)
              acc = mma4(a, T[tix(sl, k)], acc);
            }
          }
        }
        const f64x4 Lt = img_get(dg, od);   // S(L_JJ^-T)
#pragma unroll
        for (int j = 0; j < RNB; ++j)
          if (j < slot_len(sl))
            if (j == J) T[tix(sl, j)] = mma4(-Lt, acc, zero4);   // S(-W L_JJ^-1)
      }
    }
  }
  RSTAMP(2);

  // ---- lauum: K^-1 = X^T X, rows of X top to bottom -----------------------------------------------
  __syncthreads();
#pragma unroll 1
  for (int Kr = 0; Kr < nbv; ++Kr) {
    const int wz = w + loop_zero();   // (the per-tile conditions are not hoisted out of the loop)
    const int rows[3] = RES_ROWS(wz);
    const int lz = l + loop_zero(), od = (lz >> 4) * 17 + (lz & 15), ot = (lz & 15) * 17 + (lz >> 4);
    double* pn = pan + (Kr & 1) * (RNB * RIMG);
    RES_TILES(sl, j) {
      if (rows[sl] == Kr && j <= Kr) img_putT(pn + j * RIMG, ot, T[tix(sl, j)]);   // image of X_Kj^T
    }
    __syncthreads();
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
      const int I = rows[sl];
      if (I >= 0 && I <= Kr) {
        const f64x4 bI = img_get(pn + I * RIMG, od);   // S(X_KI^T)
#pragma unroll
        for (int j = 0; j < RNB; ++j) {
          if (j < slot_len(sl)) {
            if (j <= I) {   // S(O_Ij) += S(X_KI^T X_Kj); row K's registers start their sum here
              const f64x4 a = img_get(pn + j * RIMG, od);
              T[tix(sl, j)] = mma4(a, bI, I == Kr ? zero4 : T[tix(sl, j)]);
            }
          }
        }
      }
    }
  }
  RSTAMP(3);

  // ---- store: the mirrored tile straight from the stored form, the tile itself transposed through
  // a wave-private image; then the identity padding ----------------------------------------------------
  __syncthreads();
  double* scr = pan + w * RIMG;
  const int od = g * 17 + c16, ot = c16 * 17 + g;
  RES_TILES(sl, j) {
    const int I = rows0[sl];
    if (I >= 0 && I < nbv && j <= I) {   // uniform
      f64x4 v = T[tix(sl, j)];
      if (j < I) {
        if (invert == 2 || (I >> 2) == (j >> 2)) {
#pragma unroll
          for (int q = 0; q < 4; ++q) K[(int64_t)(16 * j + g + 4 * q) * ld + 16 * I + c16] = v[q];
        }
        img_put(scr, od, v);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        v = img_getT(scr, ot);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) K[(int64_t)(16 * I + g + 4 * q) * ld + 16 * j + c16] = v[q];
    }
  }
  const int r0 = 16 * nbv, npad = ld - r0;
  if (npad > 0) {   // uniform: rows r0.. (all columns), then columns r0.. of the rows above
    for (int e = threadIdx.x; e < npad * ld; e += 512) {
      const int r = r0 + e / ld, c = e % ld;
      if (invert == 2 || (c >> 6) <= (r >> 6)) K[(int64_t)r * ld + c] = r == c ? 1.0 : 0.0;
    }
    for (int e = threadIdx.x; e < r0 * npad; e += 512) {
      const int r = e / npad, c = r0 + e % npad;
      if (invert == 2 || (c >> 6) <= (r >> 6)) K[(int64_t)r * ld + c] = 0.0;
    }
  }
  RSTAMP(4);
#ifdef PQ_PROFILE
  if (threadIdx.x == 0 && blockIdx.x < PQ_RES_PROF_BLOCKS) {
#pragma unroll
    for (int k = 0; k < 5; ++k) g_res_prof[blockIdx.x * 8 + k] = pclk[k];
  }
#endif
}

#undef RES_TILES
#undef RSTAMP
}  // namespace

void factor_res_launch(int grid, hipStream_t stream, const pq_problem* pb, const pq_state* st, const int32_t* idx,
                       int nidx, const pq_settings* s, int invert) {
  hipLaunchKernelGGL(k_factor_res, dim3(grid), dim3(512), 0, stream, *pb, *st, idx, nidx, *s, invert);
}

}  // namespace pq

// PQ_PROFILE builds: the phase clocks of the last resident launch, 8 slots per workgroup (load,
// potrf, trtri, lauum, store in 100 MHz ticks); other builds report -1
extern "C" int pq_factor_res_prof(long long* out, int32_t nblocks) {
#ifdef PQ_PROFILE
  if (!out || nblocks <= 0 || nblocks > PQ_RES_PROF_BLOCKS) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(pq::g_res_prof), sizeof(long long) * 8 * nblocks) == hipSuccess ? 0 : -2;
#else
  return -1;
#endif
}
