// The SCF residual on the device: commutators of packed symmetric matrices, the antisymmetric part of an upstream gradient, and the norms of a residual.
// For a Hamiltonian H, a density D and an overlap S the residual (the DIIS error vector) is R = H D S - S D H; in the Löwdin basis of orblowdin.hip it is
// the plain commutator R^L = [H^L, D^L], which this file computes.  Serves the same empty slots of the reference as the solver
// (phisnet/nn/neural_network.py:969-993).
//
//   C = alpha (X Y - Y X),  Y symmetric (its lower triangle is read)
//     x_anti = 0: X symmetric (lower triangle read), C ANTISYMMETRIC: C_ji = -C_ij from the same number, C_ii = +0.0 exactly
//     x_anti = 1: X antisymmetric (STRICT lower triangle read, the mirrored element is the negated one, the stored diagonal is ignored), C SYMMETRIC
//   reverse of C = X Y - Y X for symmetric X, Y and G_a = (dL/dC - dL/dC^T) / 2:  dL/dX = [G_a, Y] (x_anti = 1, alpha = +1),  dL/dY = [X, G_a] = -[G_a, X]
//     (x_anti = 1, alpha = -1): both symmetric, the same kernel.
//
// k_orb_comm_product        one 256-thread workgroup per (molecule, lower-triangle 64 x 64 tile).  Both contractions of a K tile go into one accumulator set, term
//                           1 (X Y) before term 2 (Y X) in every step of four: the loop of bd_gemm<true> (orbbond_tiles.h) with the sign of the second term's A
//                           fragment flipped, which is exact.  Every entry i > j is computed once and stored twice; a diagonal tile computes the sub-tiles on and
//                           below the diagonal only.
// k_orb_comm_antisymmetrize out = (G - G^T) / 2 on lower-triangle tiles, mirrored through LDS (the shape of k_orb_low_symmetrize); the diagonal is +0.0.
// k_orb_comm_norms          one 512-thread workgroup per molecule: sum R_ij^2 and max |R_ij| over the whole m x m block (the maximum is the DIIS error).  Every
//                           thread adds its entries in four interleaved chains in a fixed order, the chains meet, then the wavefronts, in a fixed order.  A NaN
//                           entry gives NaN in both figures.
//
// Float64 throughout on v_mfma_f64_16x16x4_f64; no atomics, fixed summation orders: bitwise reproducible, independent of the rest of the batch.  status != 0:
// NaN in the molecule's own blocks (own entries of the norms).  The grids are sized from (B, M, P); a surplus workgroup exits.  Other dimensions than
// nq_orb_init: header status -2, nothing touched.  Only the layout of the state is read, so a solver state and a purification state serve alike.
//
// Resources (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage):
//   k_orb_comm_product         252 VGPRs, 0 AGPRs, 66 SGPRs, no scratch, no spills, 40960 B of LDS (four operand tiles), 2 waves per SIMD = two workgroups per CU
//   k_orb_comm_antisymmetrize  58 VGPRs, 26 SGPRs, no scratch, 33280 B of LDS, 4 waves per SIMD (bounded by LDS)
//   k_orb_comm_norms           35 VGPRs, 30 SGPRs, no scratch, 64 B of LDS, 8 waves per SIMD
//
// Compiled with -ffp-contract=off like its neighbours.
#include "orbbond_tiles.h"

// ---- out = alpha (X Y - Y X) ------------------------------------------------------------------------------------------------------------------------------------------
// two workgroups per SIMD and four LDS tiles, the bound of k_orb_low_symprod, whose product loop this is
__global__ __launch_bounds__(NQ_RS_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_orb_comm_product(OrbArgs a, int nt, const double* Xs, int x_anti, const double* Ys,
                                                                                                        double alpha, double* out) {
  __shared__ double lds[4 * NQ_RS_TILE];
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, nt, q)) return;
  const int m = q.m;
  if (q.t >= orb_tile_count(m)) return;                        // uniform
  int ti, tj;
  orb_tile_decode(q.t, &ti, &tj);
  const int i0 = ti * NQ_ORB_TILE, j0 = tj * NQ_ORB_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const int nsub = ti == tj ? wave + 1 : 4;                    // a diagonal tile: the sub-tiles on and below the diagonal
  const bool anti = x_anti != 0;
  double* Z = out + q.base;
  const double nan = nq_nan_f64();
  orb_f64x4 acc[4];
  rs_zero(acc);
  // X[i][k] Y[k][j] - Y[i][k] X[k][j]
  const BdOperand oX = {Xs + q.base, 1, anti ? 2 : 1, 0};
  const BdOperand oY = {Ys + q.base, 1, 1, 0};
  if (!q.failed) bd_gemm<true, true>(oX, oY, oY, oX, m, i0, j0, nsub, lds, acc);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= nsub) continue;
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + lk + 4 * r;
      if (i < m && j <= i) {
        const double v = q.failed ? nan : alpha * acc[s][r];
        if (j != i) {
          Z[(long long)i * m + j] = v;
          Z[(long long)j * m + i] = anti ? v : -v;
        } else {
          Z[(long long)i * m + j] = (anti || q.failed) ? v : 0.0;   // the diagonal of a commutator of symmetric matrices: not the rounded difference of two sums
        }
      }
    }
  }
}

// ---- out = (G - G^T) / 2 ------------------------------------------------------------------------------------------------------------------------------------------------
// one workgroup per (molecule, lower-triangle 64 x 64 tile): the transposed tile comes through LDS, so that both global reads and both stores run along rows
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_comm_antisymmetrize(OrbArgs a, int nt, const double* G, double* out) {
  orb_symmetrize_kernel<true, false>(a, nt, G, out);
}

// ---- sum R_ij^2 and max |R_ij| ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_ORB_NT) void k_orb_comm_norms(OrbArgs a, const double* R, double* out_sumsq, double* out_maxabs) {
  __shared__ double red[NQ_ORB_NW];
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, 1, q)) return;
  const int tid = threadIdx.x;
  const double nan = nq_nan_f64();
  if (q.failed) {
    if (tid == 0) out_sumsq[q.b] = nan, out_maxabs[q.b] = nan;
    return;
  }
  const double* Rb = R + q.base;
  const long long n = (long long)q.m * q.m;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, mx = 0.0;
  for (long long e = tid; e < n; e += 4 * NQ_ORB_NT) {          // four chains per thread, entries e, e + 512, e + 1024, e + 1536
    const long long e1 = e + NQ_ORB_NT, e2 = e + 2 * NQ_ORB_NT, e3 = e + 3 * NQ_ORB_NT;
    const double v0 = Rb[e], v1 = e1 < n ? Rb[e1] : 0.0, v2 = e2 < n ? Rb[e2] : 0.0, v3 = e3 < n ? Rb[e3] : 0.0;
    s0 += v0 * v0;
    s1 += v1 * v1;
    s2 += v2 * v2;
    s3 += v3 * v3;
    mx = fmax(fmax(mx, fmax(fabs(v0), fabs(v1))), fmax(fabs(v2), fabs(v3)));
  }
  const double sum = orb_block_sum((s0 + s1) + (s2 + s3), red);
  const double top = orb_block_max(mx, red);
  if (tid == 0) {
    out_sumsq[q.b] = sum;
    out_maxabs[q.b] = sum != sum ? nan : top;                  // fmax drops a NaN entry, the sum keeps it
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int nq_orb_comm_product(void* state, int32_t B, int32_t M, int64_t P, const double* X, int32_t x_anti, const double* Y, double alpha, double* out, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_comm_product", state, B, M, P, ORB_GRID_LOWER, &tr));
  if (!X || !Y || !out) return nq_fail(NQ_ERR_ARG, "nq_orb_comm_product: null argument");
  if (x_anti != 0 && x_anti != 1) return nq_fail(NQ_ERR_ARG, "nq_orb_comm_product: x_anti=%d is neither 0 (X symmetric) nor 1 (X antisymmetric)", x_anti);
  if (out == X || out == Y) return nq_fail(NQ_ERR_ARG, "nq_orb_comm_product: the output must not be an operand");
  const int nt = tr * (tr + 1) / 2;
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, x_anti ? "orb_comm_product_anti" : "orb_comm_product");
  hipLaunchKernelGGL(k_orb_comm_product, dim3(B * nt), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), nt, X, x_anti, Y, alpha, out);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_comm_antisymmetrize(void* state, int32_t B, int32_t M, int64_t P, const double* G, double* out, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_comm_antisymmetrize", state, B, M, P, ORB_GRID_LOWER, &tr));
  if (!G || !out) return nq_fail(NQ_ERR_ARG, "nq_orb_comm_antisymmetrize: null argument");
  if (out == G) return nq_fail(NQ_ERR_ARG, "nq_orb_comm_antisymmetrize: the output must not be the operand");
  const int nt = tr * (tr + 1) / 2;
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_comm_antisymmetrize");
  hipLaunchKernelGGL(k_orb_comm_antisymmetrize, dim3(B * nt), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), nt, G, out);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_comm_norms(void* state, int32_t B, int32_t M, int64_t P, const double* R, double* out_sumsq, double* out_maxabs, void* stream) {
  NQ_TRY(orb_check_launch("nq_orb_comm_norms", state, B, M, P, ORB_GRID_MOL));
  if (!R || !out_sumsq || !out_maxabs) return nq_fail(NQ_ERR_ARG, "nq_orb_comm_norms: null argument");
  if (out_sumsq == out_maxabs) return nq_fail(NQ_ERR_ARG, "nq_orb_comm_norms: the outputs must be arrays of their own");
  if (out_sumsq == R || out_maxabs == R) return nq_fail(NQ_ERR_ARG, "nq_orb_comm_norms: an output must not be the operand");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_comm_norms");
  hipLaunchKernelGGL(k_orb_comm_norms, dim3(B), dim3(NQ_ORB_NT), 0, st, orb_args(state, B, M, P), R, out_sumsq, out_maxabs);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
