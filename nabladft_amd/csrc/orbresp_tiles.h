// The tile routines of the density-response kernels (orbresp.hip: the closed-shell chain; orbsmear.hip: the chain over all orbital pairs): staging of operand
// tiles through padded LDS, the product loop on v_mfma_f64_16x16x4_f64, the workgroup -> (molecule, tile) map and the host-side check of the occupied-packed
// layout.  Header-only, every function static or __forceinline__ (each file keeps its own copy and its own flags); orbresp.hip's header comment describes
// the orientation of the operands and why the tiles are padded as they are.
#pragma once
#include <limits.h>

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

// ---- which molecule and tile a workgroup serves; false: exit (uniform over the workgroup) -----------------------------------------------------------------------
struct RsMol {
  int b, t, m, no, o0;
  long long base, obase;
  bool failed;
};

__device__ __forceinline__ bool rs_mol(const OrbArgs& a, int nt, const int* n_occ, const long long* occ_ptr, long long O, RsMol& q) {
  if (!orb_kind_ok(a, false)) return false;
  q.b = blockIdx.x / nt;
  q.t = blockIdx.x - q.b * nt;
  if (q.b >= a.B) return false;
  q.o0 = a.orb_ptr[q.b];
  q.m = a.orb_ptr[q.b + 1] - q.o0;
  q.base = a.pack_ptr[q.b];
  if (q.m < 1 || q.m > NQ_ORB_MAX_M || q.o0 < 0 || q.o0 + q.m > a.M || q.base < 0 || q.base + (long long)q.m * q.m > a.P) return false;
  int no = n_occ[q.b];
  q.no = no < 0 ? 0 : (no > q.m ? q.m : no);
  q.obase = occ_ptr[q.b];
  if (q.obase < 0 || q.obase + (long long)q.no * q.m > O) return false;
  q.failed = a.status[q.b] != 0;
  return true;
}

// ---- host: the arguments every launch of the family checks first --------------------------------------------------------------------------------------------------
static int rs_check(const char* who, const void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, int* tr) {
  if (!state) return nq_fail(NQ_ERR_ARG, "%s: null argument", who);
  if (!n_occ) return nq_fail(NQ_ERR_ARG, "%s: n_occ is missing", who);
  if (!occ_ptr) return nq_fail(NQ_ERR_ARG, "%s: occ_ptr is missing", who);
  NQ_TRY(orb_check_dims(B, M, P));
  if (O < 0 || O > P) return nq_fail(NQ_ERR_ARG, "%s: O=%lld occupied-packed entries do not fit P=%lld", who, (long long)O, (long long)P);
  *tr = orb_tile_rows(orb_largest_m_bound(B, M, P));
  if ((long long)B * (*tr * (*tr + 1) / 2) > INT_MAX) return nq_fail(NQ_ERR_ARG, "%s: B=%d molecules of up to %d tiles exceed the grid", who, B, *tr * (*tr + 1) / 2);
  return NQ_OK;
}
