// What the bond-order kernels (orbbond.hip) and the Löwdin kernels (orblowdin.hip) share: operand tiles whose staging orientation is chosen at run time, the
// product loop over them.  (The workgroup -> (molecule, tile) map that reads the layout of the state alone and the host-side check of the grid, which began
// here, are orb_tile_mol<ORB_HDR_DIMS> and orb_check_launch of orbstate.h.)  Shared by orbcomm.hip and orbfrontier.hip too.  Header-only, every function static or __forceinline__ (each file keeps its own copy and its own flags); orbbond.hip's header comment describes the orientation rule.
#pragma once
#include "orbresp_tiles.h"

// ---- operand tiles with the orientation chosen at run time (uniform over the workgroup) --------------------------------------------------------------------
struct BdOperand {
  const void* p;        // m x m block
  int f64;              // element type
  int sym;              // 1: symmetric, only the lower triangle is read; 0: general, read as p[x * m + k] (kfast) or p[k * m + x]
                        // 2 (bd_gemm<TWO, true> alone, orbcomm.hip): antisymmetric, only the STRICT lower triangle is read: the mirrored element is the negated
                        // one, the stored diagonal is ignored and taken as 0
  int kfast;            // general operands only
};

__device__ __forceinline__ bool bd_kfast(const BdOperand& o, int k0, int x0) { return o.sym ? k0 < x0 : o.kfast != 0; }

// SIGNED: the operand may be antisymmetric (sym == 2); krow: k is the element's row in the MATRIX (a B operand), else x is (an A operand)
template <bool SIGNED = false>
__device__ __forceinline__ void bd_fetch(double (&r)[NQ_RS_PER], const BdOperand& o, bool kf, int m, int k0, int x0, bool krow = false) {
#pragma unroll
  for (int q = 0; q < NQ_RS_PER; ++q) {
    const int e = threadIdx.x + q * NQ_RS_NT;
    const int k = k0 + (kf ? (e & (NQ_RS_KT - 1)) : (e >> 6)), x = x0 + (kf ? (e >> 4) : (e & 63));
    double v = 0.0;
    if (k < m && x < m) {
      const bool xrow = o.sym ? k <= x : kf;                   // the element's row in memory is x
      v = nq_load_f64(o.p, xrow ? (long long)x * m + k : (long long)k * m + x, o.f64);
      if (SIGNED && o.sym == 2) v = k == x ? 0.0 : ((krow ? k < x : x < k) ? -v : v);     // above the diagonal of the matrix: the negated mirror image
    }
    r[q] = v;
  }
}
__device__ __forceinline__ void bd_stage(double* t, const double (&r)[NQ_RS_PER], bool kf) {
  if (kf) rs_stage<true>(t, r);
  else rs_stage<false>(t, r);
}
__device__ __forceinline__ double bd_get(const double* t, bool kf, int k, int x) { return kf ? rs_get<true>(t, k, x) : rs_get<false>(t, k, x); }

// acc[s] += sum_k A1(i, k) B1(k, j) (+ A2(i, k) B2(k, j) with TWO) over k in [0, m), i = i0 + 16 wave .., j = j0 + 16 s .., s < nsub.  Every thread of the
// workgroup calls it (barriers inside).  lds: 2 tiles, 4 with TWO.  SIGNED (needs TWO): the second term is SUBTRACTED, by the flipped sign of its A fragment
// (exact), and an operand may be antisymmetric (sym == 2); without it the arithmetic is what it was before the parameter existed.
template <bool TWO, bool SIGNED = false>
__device__ __forceinline__ void bd_gemm(const BdOperand& A1, const BdOperand& B1, const BdOperand& A2, const BdOperand& B2, int m, int i0, int j0, int nsub,
                                        double* lds, orb_f64x4 (&acc)[4]) {
  double* tA1 = lds;
  double* tB1 = lds + NQ_RS_TILE;
  double* tA2 = lds + 2 * NQ_RS_TILE;
  double* tB2 = lds + 3 * NQ_RS_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const bool rows = i0 + wave * 16 < m;                        // uniform over the wavefront
  double ra1[NQ_RS_PER], rb1[NQ_RS_PER], ra2[NQ_RS_PER], rb2[NQ_RS_PER];
  bool fa1 = bd_kfast(A1, 0, i0), fb1 = bd_kfast(B1, 0, j0), fa2 = TWO && bd_kfast(A2, 0, i0), fb2 = TWO && bd_kfast(B2, 0, j0);
  bd_fetch<SIGNED>(ra1, A1, fa1, m, 0, i0, false);
  bd_fetch<SIGNED>(rb1, B1, fb1, m, 0, j0, true);
  if (TWO) {
    bd_fetch<SIGNED>(ra2, A2, fa2, m, 0, i0, false);
    bd_fetch<SIGNED>(rb2, B2, fb2, m, 0, j0, true);
  }
  for (int k0 = 0; k0 < m; k0 += NQ_RS_KT) {
    __syncthreads();                                           // the previous tile has been consumed
    const bool ca1 = fa1, cb1 = fb1, ca2 = fa2, cb2 = fb2;     // the orientation of the tile now staged
    bd_stage(tA1, ra1, ca1);
    bd_stage(tB1, rb1, cb1);
    if (TWO) {
      bd_stage(tA2, ra2, ca2);
      bd_stage(tB2, rb2, cb2);
    }
    __syncthreads();
    const int kn = k0 + NQ_RS_KT;
    if (kn < m) {
      fa1 = bd_kfast(A1, kn, i0);
      fb1 = bd_kfast(B1, kn, j0);
      bd_fetch<SIGNED>(ra1, A1, fa1, m, kn, i0, false);
      bd_fetch<SIGNED>(rb1, B1, fb1, m, kn, j0, true);
      if (TWO) {
        fa2 = bd_kfast(A2, kn, i0);
        fb2 = bd_kfast(B2, kn, j0);
        bd_fetch<SIGNED>(ra2, A2, fa2, m, kn, i0, false);
        bd_fetch<SIGNED>(rb2, B2, fb2, m, kn, j0, true);
      }
    }
    if (rows) {
#pragma unroll
      for (int kk = 0; kk < NQ_RS_KT; kk += 4) {
        if (k0 + kk >= m) break;                               // uniform
        const double a1 = bd_get(tA1, ca1, kk + lk, wave * 16 + lc);
        const double a2p = TWO ? bd_get(tA2, ca2, kk + lk, wave * 16 + lc) : 0.0;
        const double a2 = SIGNED ? -a2p : a2p;
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (s < nsub && j0 + s * 16 < m) {                   // uniform
            acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bd_get(tB1, cb1, kk + lk, s * 16 + lc), acc[s], 0, 0, 0);
            if (TWO) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, bd_get(tB2, cb2, kk + lk, s * 16 + lc), acc[s], 0, 0, 0);
          }
      }
    }
  }
}
