// Löwdin (symmetric) orthogonalisation on the device: the matrix functions A = S^(1/2) and A^- = S^(-1/2) of the overlap, the congruences A D A and A^- H A^-,
// and the reverse of both, after a STANDARD solve of S itself (nq_orb_solve with S = NULL: S = U diag(s) U^T, the state's eps = s, row k of coeff = u_k).
// Serves the same empty slots of the reference as the solver (phisnet/nn/neural_network.py:969-993).
//
//   a_k = sqrt(s_k),  A = U diag(a) U^T,  A^- = U diag(1 / a) U^T          (k_orb_low_weights, then ONE nq_orb_wgram launch with the two weight vectors)
//   congruence of a symmetric M (D or H) with a symmetric X (A or A^-):  Y = M X (kept for the reverse),  M^L = sym(X Y)
//   reverse for a symmetric G = dL/dM^L:  dL/dM = sym(X (G X)),  dL/dX = Y G + G Y^T = 2 sym(Y G)
//   reverse of the matrix function (Daleckii-Krein) for g = sym(dL/dX):  dL/dS = U [K o (U^T g U)] U^T, the diagonal included,
//     K_ij = 1 / (a_i + a_j) for A,  K_ij = -1 / (a_i a_j (a_i + a_j)) for A^-:  no difference of eigenvalues is divided, equal levels of S are harmless.
//     T = g U is nq_orb_resp_project over all orbitals, U (K o W) U^T is nq_orb_smear_back and nq_orb_syr2k over all orbitals (orbresp.hip, orbsmear.hip).
//
// k_orb_low_weights  one 512-thread workgroup per molecule: a_k, 1 / a_k and s_max / s_min.  A failed solve, a non-finite s_k or s_min <= 0: info 1 and NaN in
//                    the molecule's own slices (which nq_orb_wgram turns into NaN blocks of A and A^-).
// k_orb_low_product  Y = M X, the general m x m product from the lower triangles of two symmetric operands: one 256-thread workgroup per (molecule, 64 x 64
//                    output tile), every tile of the square; the product loop and the run-time staging orientation are orbbond.hip's (orbbond_tiles.h).
// k_orb_low_symprod  out = alpha / 2 (A1 B1 + A2 B2) on lower-triangle 64 x 64 tiles, mirrored: side 0: sym(X E) = 1/2 (X E + E^T X), side 1: sym(E X) =
//                    1/2 (E X + X E^T); E general, X symmetric and read from its lower triangle; both contractions of a K tile go into one accumulator set, term
//                    1 before term 2 in every step of four (the loop of k_orb_bond_backward).
// k_orb_low_symmetrize  out = (G + G^T) / 2 on lower-triangle tiles, mirrored through LDS: the upstream gradient of a congruence made exactly symmetric on the
//                    device before the two products read its lower triangle.
// k_orb_low_mo       W[i][j] = sum_mu Ct[i][mu] T[mu][j] and its epilogue A_out[i][j] = K_ij W_ij, the diagonal included; a = sqrt(eps) recomputed from the
//                    state.  The shape of k_orb_smear_mo: a workgroup owns 64 rows and walks the columns itself.  A molecule k_orb_low_weights would flag: NaN.
//
// Float64 throughout on v_mfma_f64_16x16x4_f64 through the tile routines of the response kernels; no atomics, fixed summation orders: bitwise reproducible,
// independent of the rest of the batch.  status != 0: NaN in the molecule's own blocks of every output.  The grids are sized from (B, M, P); a surplus
// workgroup exits.  Other dimensions than nq_orb_init: header status -2, nothing touched.  k_orb_low_weights and k_orb_low_mo read eps and coeff and refuse a
// state that holds a purification (header status -3); the products and the symmetrisation read the layout of the state alone, so a solver state and a
// purification state serve alike.
//
// Compiled with -ffp-contract=off like its neighbours: K is a sum, a product and a division as written.
#include "orbbond_tiles.h"

// a level of S the square roots cannot be taken of: not finite, or not positive (NaN fails the comparison)
__device__ __forceinline__ bool lw_bad_level(double s) { return !(s > 0.0) || !isfinite(s); }

// ---- a = sqrt(s), 1 / a, s_max / s_min -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_ORB_NT) void k_orb_low_weights(OrbArgs a, double* out_half, double* out_inv_half, double* out_cond, int* out_info) {
  __shared__ double red[NQ_ORB_NW];
  if (!orb_kind_ok(a, false)) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  int o0, m;
  long long base;
  bool failed;
  if (!orb_mol(a, b, o0, m, base, failed)) return;               // uniform: a state overwritten since nq_orb_init
  // at most two levels per thread (m <= 1024 = 2 x 512)
  const int k0 = tid, k1 = tid + NQ_ORB_NT;
  const bool h0 = k0 < m, h1 = k1 < m;
  const double s0 = h0 ? a.eps[o0 + k0] : 1.0, s1 = h1 ? a.eps[o0 + k1] : 1.0;
  const double nan = nq_nan_f64();
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double bad = (lw_bad_level(s0) || lw_bad_level(s1)) ? 1.0 : 0.0;
  bad = orb_block_sum(bad, red);                                 // a count: exact, the same bits in every thread
  if (failed || bad != 0.0) {
    if (h0) out_half[o0 + k0] = nan, out_inv_half[o0 + k0] = nan;
    if (h1) out_half[o0 + k1] = nan, out_inv_half[o0 + k1] = nan;
    if (tid == 0) out_cond[b] = nan, out_info[b] = 1;
    return;
  }
  const double smax = orb_block_max(fmax(h0 ? s0 : -inf, h1 ? s1 : -inf), red);
  const double smin = -orb_block_max(fmax(h0 ? -s0 : -inf, h1 ? -s1 : -inf), red);
  if (h0) {
    const double r = sqrt(s0);
    out_half[o0 + k0] = r;
    out_inv_half[o0 + k0] = 1.0 / r;
  }
  if (h1) {
    const double r = sqrt(s1);
    out_half[o0 + k1] = r;
    out_inv_half[o0 + k1] = 1.0 / r;
  }
  if (tid == 0) out_cond[b] = smax / smin, out_info[b] = 0;
}

// ---- Y = M X ----------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_low_product(OrbArgs a, int tr, const void* Ms, int m_f64, const double* Xs, double* out) {
  __shared__ double lds[2 * NQ_RS_TILE];
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, tr * tr, q)) return;
  const int m = q.m, ti = q.t / tr, tj = q.t - ti * tr;
  const int i0 = ti * NQ_ORB_TILE, j0 = tj * NQ_ORB_TILE;
  if (i0 >= m || j0 >= m) return;                              // uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const double nan = nq_nan_f64();
  double* Y = out + q.base;
  const BdOperand oM = {m_f64 ? (const void*)((const double*)Ms + q.base) : (const void*)((const float*)Ms + q.base), m_f64, 1, 0};
  const BdOperand oX = {Xs + q.base, 1, 1, 0};
  orb_f64x4 acc[4];
  rs_zero(acc);
  if (!q.failed) bd_gemm<false>(oM, oX, oM, oX, m, i0, j0, 4, lds, acc);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + lk + 4 * r;
      if (i < m && j < m) Y[(long long)i * m + j] = q.failed ? nan : acc[s][r];
    }
  }
}

// ---- alpha sym(X E) and alpha sym(E X) ----------------------------------------------------------------------------------------------------------------------------
// two workgroups per SIMD, the bound of k_orb_bond_backward, whose product loop this is
__global__ __launch_bounds__(NQ_RS_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_orb_low_symprod(OrbArgs a, int nt, const double* E, const double* Xs, int side, double alpha,
                                                                                                       double* out) {
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
  const bool left = side == 0;                                 // sym(X E), else sym(E X)
  double* Z = out + q.base;
  const double nan = nq_nan_f64();
  orb_f64x4 acc[4];
  rs_zero(acc);
  // sym(X E): X[i][k] E[k][j] + E[k][i] X[k][j];  sym(E X): E[i][k] X[k][j] + X[i][k] E[j][k].  One call, so that the product loop exists once in the kernel.
  const BdOperand oE = {E + q.base, 1, 0, left ? 0 : 1};
  const BdOperand oX = {Xs + q.base, 1, 1, 0};
  if (!q.failed) bd_gemm<true>(left ? oX : oE, left ? oE : oX, left ? oE : oX, left ? oX : oE, m, i0, j0, nsub, lds, acc);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= nsub) continue;
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + lk + 4 * r;
      if (i < m && j <= i) {
        const double v = q.failed ? nan : alpha * (0.5 * acc[s][r]);
        Z[(long long)i * m + j] = v;
        if (j != i) Z[(long long)j * m + i] = v;
      }
    }
  }
}

// ---- out = (G + G^T) / 2 ------------------------------------------------------------------------------------------------------------------------------------------------
// one workgroup per (molecule, lower-triangle 64 x 64 tile): the transposed tile comes through LDS, so that both global reads and both stores run along rows
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_low_symmetrize(OrbArgs a, int nt, const double* G, double* out) { orb_symmetrize_kernel<false, false>(a, nt, G, out); }

// ---- A_out = K o (U^T T) ------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_low_mo(OrbArgs a, int tr, int kind, const double* T, double* A_out) {
  __shared__ double lds[3 * NQ_RS_TILE];
  __shared__ int flagged;
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_SOLVE>(a, tr, q)) return;
  const int b = q.b, o0 = q.o0, m = q.m;
  const long long base = q.base;
  const int i0 = q.t * NQ_ORB_TILE;                              // the workgroup's 64 rows of W; it walks the columns itself
  if (i0 >= m) return;                                         // uniform
  const double* Ct = a.coeff + base;
  const double* eps = a.eps + o0;
  if (threadIdx.x == 0) flagged = 0;
  __syncthreads();
  bool mine = false;
  for (int k = threadIdx.x; k < m; k += NQ_RS_NT) mine = mine || lw_bad_level(eps[k]);
  if (mine) flagged = 1;                                       // every writer stores the same value
  __syncthreads();
  const bool failed = q.failed || flagged != 0;              // what k_orb_low_weights reports as info 1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const double nan = nq_nan_f64();
  double ai[4];                                                // this thread's four rows
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + wave * 16 + lk + 4 * r;
    ai[r] = sqrt(i < m ? eps[i] : 1.0);
  }
  double* X0 = A_out + base;
  for (int j0 = 0; j0 < m; j0 += NQ_ORB_TILE) {                // uniform over the workgroup
    orb_f64x4 acc0[4], acc1[4];
    rs_zero(acc0);
    rs_zero(acc1);
    if (!failed) rs_gemm<true, false, false>(Ct, nullptr, m, T + base, m, 0, m, i0, m, j0, m, lds, acc0, acc1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = j0 + s * 16 + lc;
      if (j >= m) continue;
      const double aj = sqrt(eps[j]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wave * 16 + lk + 4 * r;
        if (i >= m) continue;
        const double sum = ai[r] + aj;
        const double K = kind == 0 ? 1.0 / sum : -1.0 / ((ai[r] * aj) * sum);
        X0[(long long)i * m + j] = failed ? nan : K * acc0[s][r];
      }
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int nq_orb_low_weights(void* state, int32_t B, int32_t M, int64_t P, double* out_half, double* out_inv_half, double* out_cond, int32_t* out_info, void* stream) {
  NQ_TRY(orb_check_launch("nq_orb_low_weights", state, B, M, P, ORB_GRID_MOL));
  if (!out_half || !out_inv_half || !out_cond || !out_info) return nq_fail(NQ_ERR_ARG, "nq_orb_low_weights: null argument");
  if (out_half == out_inv_half) return nq_fail(NQ_ERR_ARG, "nq_orb_low_weights: the outputs must be arrays of their own");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_low_weights");
  hipLaunchKernelGGL(k_orb_low_weights, dim3(B), dim3(NQ_ORB_NT), 0, st, orb_args(state, B, M, P), out_half, out_inv_half, out_cond, (int*)out_info);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_low_product(void* state, int32_t B, int32_t M, int64_t P, const void* Msym, int32_t m_f64, const double* X, double* out_Y, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_low_product", state, B, M, P, ORB_GRID_SQUARE, &tr));
  if (!Msym || !X || !out_Y) return nq_fail(NQ_ERR_ARG, "nq_orb_low_product: null argument");
  if ((const void*)out_Y == Msym || out_Y == X) return nq_fail(NQ_ERR_ARG, "nq_orb_low_product: the output must not be an operand");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_low_product");
  hipLaunchKernelGGL(k_orb_low_product, dim3(B * tr * tr), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), tr, Msym, m_f64, X, out_Y);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_low_symprod(void* state, int32_t B, int32_t M, int64_t P, const double* E, const double* X, int32_t side, double alpha, double* out, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_low_symprod", state, B, M, P, ORB_GRID_LOWER, &tr));
  if (!E || !X || !out) return nq_fail(NQ_ERR_ARG, "nq_orb_low_symprod: null argument");
  if (side != 0 && side != 1) return nq_fail(NQ_ERR_ARG, "nq_orb_low_symprod: side=%d is neither 0 (sym(X E)) nor 1 (sym(E X))", side);
  if (out == E || out == X) return nq_fail(NQ_ERR_ARG, "nq_orb_low_symprod: the output must not be an operand");
  const int nt = tr * (tr + 1) / 2;
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, side == 0 ? "orb_low_symprod_left" : "orb_low_symprod_right");
  hipLaunchKernelGGL(k_orb_low_symprod, dim3(B * nt), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), nt, E, X, side, alpha, out);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_low_symmetrize(void* state, int32_t B, int32_t M, int64_t P, const double* G, double* out, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_low_symmetrize", state, B, M, P, ORB_GRID_LOWER, &tr));
  if (!G || !out) return nq_fail(NQ_ERR_ARG, "nq_orb_low_symmetrize: null argument");
  if (out == G) return nq_fail(NQ_ERR_ARG, "nq_orb_low_symmetrize: the output must not be the operand");
  const int nt = tr * (tr + 1) / 2;
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_low_symmetrize");
  hipLaunchKernelGGL(k_orb_low_symmetrize, dim3(B * nt), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), nt, G, out);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_low_mo(void* state, int32_t B, int32_t M, int64_t P, int32_t kind, const double* T, double* A_out, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_low_mo", state, B, M, P, ORB_GRID_ROWS, &tr));
  if (!T || !A_out) return nq_fail(NQ_ERR_ARG, "nq_orb_low_mo: null argument");
  if (kind != 0 && kind != 1) return nq_fail(NQ_ERR_ARG, "nq_orb_low_mo: kind=%d is neither 0 (S^(1/2)) nor 1 (S^(-1/2))", kind);
  if (A_out == T) return nq_fail(NQ_ERR_ARG, "nq_orb_low_mo: the output must not be the operand");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, kind == 0 ? "orb_low_mo_half" : "orb_low_mo_inv_half");
  hipLaunchKernelGGL(k_orb_low_mo, dim3(B * tr), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), tr, kind, T, A_out);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
