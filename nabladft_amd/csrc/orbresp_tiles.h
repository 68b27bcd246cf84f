// The tile routines of the density-response kernels (orbresp.hip: the closed-shell chain; orbsmear.hip: the chain over all orbital pairs) and of the files
// that came after them (orbpurify.hip, orbsqrt.hip and, through orbbond_tiles.h, orbbond.hip, orblowdin.hip, orbcomm.hip, orbfrontier.hip): staging of operand
// tiles through padded LDS, the product loop on v_mfma_f64_16x16x4_f64, the occupied-layout part of the workgroup -> (molecule, tile) map (the common part is
// orbstate.h's), the symmetrise tile routine behind k_orb_resp_sym, k_orb_low_symmetrize and k_orb_comm_antisymmetrize, and the host-side check of the
// occupied-packed layout.  Header-only, every function static or __forceinline__ (each file keeps its own copy and its own flags); orbresp.hip's header comment describes
// the orientation of the operands and why the tiles are padded as they are.
#pragma once
#include "orbstate.h"

#define NQ_RS_NT 256
#define NQ_RS_KT 16                                        // K tile: four steps of the matrix instruction
#define NQ_RS_LD_SLOW (NQ_ORB_TILE + 16)                   // [k][x]: 80 doubles = 160 dwords = 32 mod 64 banks
#define NQ_RS_LD_FAST (NQ_RS_KT + 2)                       // [x][k]: 18 doubles = 36 dwords: 16 rows x 2 k land on 32 distinct bank pairs
#define NQ_RS_TILE (NQ_RS_KT * NQ_RS_LD_SLOW)              // doubles per staged operand tile (>= 64 * NQ_RS_LD_FAST)
#define NQ_RS_PER (NQ_RS_KT * NQ_ORB_TILE / NQ_RS_NT)      // elements of a tile per thread
typedef double orb_f64x4 __attribute__((ext_vector_type(4)));

// ---- operand tiles: element (k, x), k = contraction index, x = output index; KF: k is the fast index in memory (p[x * ld + k]) ------------------------------
template <bool KF>
__device__ __forceinline__ void rs_fetch(double (&r)[NQ_RS_PER], const double* p, long long ld, int k0, int khi, int x0, int xhi) {
#pragma unroll
  for (int q = 0; q < NQ_RS_PER; ++q) {
    const int e = threadIdx.x + q * NQ_RS_NT;
    const int k = k0 + (KF ? (e & (NQ_RS_KT - 1)) : (e >> 6)), x = x0 + (KF ? (e >> 4) : (e & 63));
    r[q] = (k < khi && x < xhi) ? (KF ? p[(long long)x * ld + k] : p[(long long)k * ld + x]) : 0.0;
  }
}
template <bool KF>
__device__ __forceinline__ void rs_stage(double* t, const double (&r)[NQ_RS_PER]) {
#pragma unroll
  for (int q = 0; q < NQ_RS_PER; ++q) {
    const int e = threadIdx.x + q * NQ_RS_NT;
    const int k = KF ? (e & (NQ_RS_KT - 1)) : (e >> 6), x = KF ? (e >> 4) : (e & 63);
    t[KF ? x * NQ_RS_LD_FAST + k : k * NQ_RS_LD_SLOW + x] = r[q];
  }
}
template <bool KF>
__device__ __forceinline__ double rs_get(const double* t, int k, int x) {
  return t[KF ? x * NQ_RS_LD_FAST + k : k * NQ_RS_LD_SLOW + x];
}

// acc[s] += A(i0 + 16 wave .., k) B(k, j0 + 16 s ..) over k in [klo, khi); with TWO a second A against the same B.  Every thread of the workgroup must call it
// with the same klo / khi (barriers inside).  lds: 3 tiles.
template <bool AKF, bool BKF, bool TWO>
__device__ __forceinline__ void rs_gemm(const double* A0, const double* A1, long long lda, const double* Bp, long long ldb, int klo, int khi, int i0, int ihi,
                                        int j0, int jhi, double* lds, orb_f64x4 (&acc0)[4], orb_f64x4 (&acc1)[4]) {
  double* tA0 = lds;
  double* tA1 = lds + NQ_RS_TILE;
  double* tB = lds + 2 * NQ_RS_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const bool rows = i0 + wave * 16 < ihi;                      // uniform over the wavefront
  double ra0[NQ_RS_PER], ra1[NQ_RS_PER], rb[NQ_RS_PER];
  if (klo < khi) {
    rs_fetch<AKF>(ra0, A0, lda, klo, khi, i0, ihi);
    if (TWO) rs_fetch<AKF>(ra1, A1, lda, klo, khi, i0, ihi);
    rs_fetch<BKF>(rb, Bp, ldb, klo, khi, j0, jhi);
  }
  for (int k0 = klo; k0 < khi; k0 += NQ_RS_KT) {
    __syncthreads();                                           // the previous tile has been consumed
    rs_stage<AKF>(tA0, ra0);
    if (TWO) rs_stage<AKF>(tA1, ra1);
    rs_stage<BKF>(tB, rb);
    __syncthreads();
    if (k0 + NQ_RS_KT < khi) {
      rs_fetch<AKF>(ra0, A0, lda, k0 + NQ_RS_KT, khi, i0, ihi);
      if (TWO) rs_fetch<AKF>(ra1, A1, lda, k0 + NQ_RS_KT, khi, i0, ihi);
      rs_fetch<BKF>(rb, Bp, ldb, k0 + NQ_RS_KT, khi, j0, jhi);
    }
    if (rows) {
#pragma unroll
      for (int kk = 0; kk < NQ_RS_KT; kk += 4) {
        if (k0 + kk >= khi) break;                             // uniform
        const double a0 = rs_get<AKF>(tA0, kk + lk, wave * 16 + lc);
        const double a1 = TWO ? rs_get<AKF>(tA1, kk + lk, wave * 16 + lc) : 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (j0 + s * 16 < jhi) {                             // uniform
            const double bv = rs_get<BKF>(tB, kk + lk, s * 16 + lc);
            acc0[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv, acc0[s], 0, 0, 0);
            if (TWO) acc1[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv, acc1[s], 0, 0, 0);
          }
      }
    }
  }
}

__device__ __forceinline__ void rs_zero(orb_f64x4 (&acc)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = orb_f64x4{0.0, 0.0, 0.0, 0.0};
}

// ---- which molecule and tile a workgroup serves (orb_tile_mol) and where its occupied-packed block lies; false: exit (uniform over the workgroup) -----------------
struct RsMol : OrbTile {
  int no;
  long long obase;
};

__device__ __forceinline__ bool rs_mol(const OrbArgs& a, int nt, const int* n_occ, const long long* occ_ptr, long long O, RsMol& q) {
  if (!orb_tile_mol<ORB_HDR_SOLVE>(a, nt, q)) return false;
  const int no = n_occ[q.b];
  q.no = no < 0 ? 0 : (no > q.m ? q.m : no);
  q.obase = occ_ptr[q.b];
  return q.obase >= 0 && q.obase + (long long)q.no * q.m <= O;
}

// ---- (G + G^T) / 2, or with ANTI (G - G^T) / 2, on the lower-triangle 64 x 64 tile (i0, j0), j0 <= i0, of an m x m block, mirrored ------------------------------------
// The transposed tile comes through LDS, so that both global reads and both stores run along rows.  Every entry below the diagonal is computed once and stored
// twice: the result is exactly symmetric, or exactly antisymmetric with a +0.0 diagonal.  failed: NaN.  Every thread of the workgroup calls it (barriers
// inside); Z must not be Gb.
template <bool ANTI>
__device__ __forceinline__ void orb_symmetrize_tile(const double* Gb, double* Z, int m, int i0, int j0, bool failed, double (&tile)[NQ_ORB_TILE][NQ_ORB_TILE + 1]) {
  const double nan = nq_nan_f64();
  constexpr int PER = NQ_ORB_TILE * NQ_ORB_TILE / NQ_RS_NT;
  for (int e = threadIdx.x; e < NQ_ORB_TILE * NQ_ORB_TILE; e += NQ_RS_NT) {    // tile[r][c] = G[j0 + r][i0 + c]: the mirror image of this workgroup's tile
    const int r = e >> 6, c = e & 63;
    tile[r][c] = (j0 + r < m && i0 + c < m) ? Gb[(long long)(j0 + r) * m + i0 + c] : 0.0;
  }
  __syncthreads();
  double v[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = threadIdx.x + k * NQ_RS_NT, r = e >> 6, c = e & 63;
    const int i = i0 + r, j = j0 + c;
    v[k] = 0.0;
    if (i < m && j <= i) {
      if (ANTI) v[k] = failed ? nan : (i == j ? 0.0 : 0.5 * (Gb[(long long)i * m + j] - tile[c][r]));
      else v[k] = failed ? nan : 0.5 * (Gb[(long long)i * m + j] + tile[c][r]);
      Z[(long long)i * m + j] = v[k];
    }
  }
  __syncthreads();                                             // the mirror image has been consumed
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = threadIdx.x + k * NQ_RS_NT;
    tile[e >> 6][e & 63] = v[k];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < NQ_ORB_TILE * NQ_ORB_TILE; e += NQ_RS_NT) {    // out[j0 + r][i0 + c] from the value of (i0 + c, j0 + r), strictly above the diagonal
    const int r = e >> 6, c = e & 63;
    const int j = j0 + r, i = i0 + c;
    // 0.0 - v is exact; equal entries give +0.0 on both sides, as (G_ji - G_ij) / 2 does
    if (i < m && j < i) Z[(long long)j * m + i] = ANTI ? 0.0 - tile[c][r] : tile[c][r];
  }
}

// One workgroup per (molecule, lower-triangle tile); KEEP_FAILED: a failed molecule's block is averaged like any other (orbresp.hip), else it is NaN.
template <bool ANTI, bool KEEP_FAILED>
__device__ __forceinline__ void orb_symmetrize_kernel(const OrbArgs& a, int nt, const double* G, double* out) {
  __shared__ double tile[NQ_ORB_TILE][NQ_ORB_TILE + 1];
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, nt, q)) return;
  if (q.t >= orb_tile_count(q.m)) return;                       // uniform: the barriers are reached by the whole workgroup or not at all
  int ti, tj;
  orb_tile_decode(q.t, &ti, &tj);
  orb_symmetrize_tile<ANTI>(G + q.base, out + q.base, q.m, ti * NQ_ORB_TILE, tj * NQ_ORB_TILE, KEEP_FAILED ? false : q.failed, tile);
}

// ---- host: the occupied-packed layout, after what every launch of the family checks first (orb_check_launch) --------------------------------------------------------
static int rs_check(const char* who, const void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, int* tr) {
  NQ_TRY(orb_check_launch(who, state, B, M, P, ORB_GRID_LOWER, tr));
  if (!n_occ) return nq_fail(NQ_ERR_ARG, "%s: n_occ is missing", who);
  if (!occ_ptr) return nq_fail(NQ_ERR_ARG, "%s: occ_ptr is missing", who);
  if (O < 0 || O > P) return nq_fail(NQ_ERR_ARG, "%s: O=%lld occupied-packed entries do not fit P=%lld", who, (long long)O, (long long)P);
  return NQ_OK;
}
