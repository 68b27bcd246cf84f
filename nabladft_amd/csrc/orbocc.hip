// ALL occupied orbital energies and coefficients WITHOUT a full solve: a pivoted Cholesky factor of the projector a purification (orbpurify.hip) leaves on the
// device, Rayleigh-Ritz on the n_occ x n_occ matrix it reduces the Hamiltonian to, and the back-transform.  Serves the same empty slots of the reference as the
// solver (phisnet/nn/neural_network.py:969-993), for the occupied levels only.
//
// Per molecule: Ht (symmetric, the orthogonalised Hamiltonian, state part `work` of the purification), X (the projector on the n_occ lowest levels of Ht, state
// part `coeff`).  An exact orthogonal projector of rank r has the pivoted Cholesky factor X = Q^T Q with Q r x m stored by rows; X^2 = X forces Q Q^T = I, every
// Schur complement is again a projector, so every pivot is >= (remaining rank) / m >= 1 / m and the rows need no re-orthonormalisation (DESIGN_details.md).
//
// k_occ_factor    one 512-thread workgroup per molecule, the largest molecules first: a left-looking pivoted Cholesky of X for exactly n_occ steps.  Step j:
//                 p = the largest remaining diagonal entry (the first on ties; the diagonal lives in LDS), q_j = (X[p][:] - sum_{k<j} q_k[p] q_k) / sqrt(pivot) with
//                 the entries of earlier pivots exactly 0, diag -= q_j^2.  The row of X and the earlier rows of Q are streamed with coalesced reads (lanes along
//                 the row, eight rows in flight), the sum over k runs in the order of k with fma().  Outputs: Q rows 0 .. n_occ - 1 of the molecule's packed block
//                 (the other rows untouched), pivots int32 [M] (-1 in the slots k >= n_occ), the smallest pivot (+inf for n_occ = 0) and the largest |left-over
//                 diagonal| per molecule, a status word per molecule: the state's own when that is not 0 (1, 4), 5 for a pivot < 1 / (2 m) or not finite, or a
//                 left-over diagonal entry >= 1 / (2 m) in magnitude (a step more would find a pivot): X is not a projector of rank n_occ; else 0.  status != 0: NaN in the molecule's rows of Q, its smallest pivot and its defect, -1 in its pivots.
// k_occ_reduce    Hs = Q T with T = Ht Q^T (occupied-packed [m][n_occ]: nq_orb_resp_project on the state that holds Q in its `coeff` forms it), n_occ x n_occ into a
//                 reduced packed layout whose blocks have max(n_occ, 1) rows (n_occ = 0: the 1 x 1 block [0]).  One 256-thread workgroup per lower-triangle 64 x 64
//                 tile, mirrored: exactly symmetric.  status != 0: a zero block (the NaN of that molecule's results comes from k_occ_finish).
// k_occ_back<1>   U = V Q         occupied-packed [n_occ][m]: V = the vectors of the reduced solve, row k = level k (the `coeff` of the reduced state)
// k_occ_back<2>   C = U W         into rows k < n_occ of the state's `coeff` (W general, [mu][nu]: the lower-triangular Z of nq_orb_pur_orthogonalizer or a symmetric
//                 S^(-1/2) alike; without W the step is skipped).  One 256-thread workgroup per (molecule, 64 orbitals along the m side) for both, like k_orb_resp<3>.
// k_occ_finish    one 512-thread workgroup per molecule, a row per wavefront: the solver's sign rule (the largest-magnitude component positive, the first on ties),
//                 eps[k] = the reduced levels for k < n_occ, NaN in every other eps slot and coefficient row; the status word of the factor, else that of the
//                 reduced solve, into the state and the caller's array; status != 0: NaN in all the molecule's eps slots and rows.
//
// The three products go through rs_gemm of orbresp_tiles.h (padded LDS tiles, v_mfma_f64_16x16x4_f64, one K tile in LDS and one in flight).  No atomics; every sum
// has an order that depends on the molecule alone: bitwise reproducible, independent of the rest of the batch.  Other dimensions than nq_orb_init: header status
// -2; nq_orb_occ_factor on a state that holds no purification, the others on one that does: header status -3; nothing else is touched.  Compiled with
// -ffp-contract=off like its siblings: fma() where one is wanted.
//
// Resources (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage):
//   k_occ_factor    78 VGPRs, 0 AGPRs, 65 SGPRs, no scratch, 20640 B of LDS (diagonal, multipliers, pivot flags)
//   k_occ_reduce    220 VGPRs, 8 AGPRs, 53 SGPRs, no scratch, 30720 B of LDS (three operand tiles), 2 waves per SIMD
//   k_occ_back<1>   124 VGPRs, 8 AGPRs, 64 SGPRs, no scratch, 30720 B of LDS;  k_occ_back<2>: 126 VGPRs, 66 SGPRs, the same LDS; 3 waves per SIMD
//   k_occ_finish    27 VGPRs, 46 SGPRs, no scratch, no LDS
#include "orbresp_tiles.h"

#define NQ_OCC_STATUS 5       // the per-molecule status of a projector that is not one

// x - sum_{k < n} h[k] Qb[k][i], subtracted in the order of k; eight loads in flight
__device__ __forceinline__ double occ_strip(const double* __restrict__ Qb, int n, int m, int i, const double* h, double x) {
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    double l[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) l[u] = Qb[(long long)(k + u) * m + i];
#pragma unroll
    for (int u = 0; u < 8; ++u) x = fma(-h[k + u], l[u], x);
  }
  for (; k < n; ++k) x = fma(-h[k], Qb[(long long)k * m + i], x);
  return x;
}

__global__ __launch_bounds__(NQ_ORB_NT) void k_occ_factor(OrbArgs a, const int* n_occ, double* Qall, int* pivots, double* min_pivot, double* defect, int* status) {
  __shared__ double d[NQ_ORB_MAX_M];
  __shared__ double h[NQ_ORB_MAX_M];
  __shared__ int done[NQ_ORB_MAX_M];
  __shared__ double red[NQ_ORB_NW];
  __shared__ double redv[NQ_ORB_NW];
  __shared__ int redi[NQ_ORB_NW];
  if (!orb_kind_ok(a, true)) return;
  if ((int)blockIdx.x >= a.B) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = a.order[blockIdx.x];
  if (b < 0 || b >= a.B) return;
  int o0, m;
  long long base;
  bool failed;
  if (!orb_mol(a, b, o0, m, base, failed)) return;                   // uniform: a state overwritten since nq_orb_init
  const double nan = nq_nan_f64();
  int no = n_occ[b];
  no = no < 0 ? 0 : (no > m ? m : no);
  const double* X = a.coeff + base;
  double* Qb = Qall + base;
  int* piv_out = pivots + o0;
  int stat = failed ? a.status[b] : 0;
  double pmin = INFINITY;
  for (int i = tid; i < m; i += NQ_ORB_NT) {
    d[i] = X[(long long)i * m + i];
    done[i] = 0;
    piv_out[i] = -1;
  }
  __syncthreads();
  const double floor_piv = 0.5 / (double)m;
  for (int j = 0; j < no && stat == 0; ++j) {                        // stat is uniform
    double best = -INFINITY;
    int at = m;
    for (int i = tid; i < m; i += NQ_ORB_NT) {
      const double v = d[i];
      if (!done[i] && v > best) { best = v; at = i; }                // i ascends: the first on ties; a NaN never wins
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const double ob = __shfl_xor(best, s, 64);
      const int oa = __shfl_xor(at, s, 64);
      if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if (lane == 0) { redv[wave] = best; redi[wave] = at; }
    __syncthreads();
    best = redv[0];
    at = redi[0];
#pragma unroll
    for (int w = 1; w < NQ_ORB_NW; ++w)
      if (redv[w] > best || (redv[w] == best && redi[w] < at)) { best = redv[w]; at = redi[w]; }
    const int p = at;
    const double piv = best;
    if (p >= m || !(piv >= floor_piv) || !(piv < INFINITY)) {          // uniform: every thread read the same words
      stat = NQ_OCC_STATUS;
      break;
    }
    for (int k = tid; k < j; k += NQ_ORB_NT) h[k] = Qb[(long long)k * m + p];
    __syncthreads();
    const double r = sqrt(piv);
    for (int i = tid; i < m; i += NQ_ORB_NT) {
      double x = 0.0;
      if (!done[i]) {
        x = occ_strip(Qb, j, m, i, h, X[(long long)p * m + i]) / r;
        d[i] = d[i] - x * x;
        if (i == p) done[i] = 1;
      }
      Qb[(long long)j * m + i] = x;
    }
    if (tid == 0) piv_out[j] = p;
    pmin = fmin(pmin, piv);
    __threadfence_block();                                           // the row is read again, by other threads, in the steps that follow
    __syncthreads();
  }
  double left = 0.0;
  for (int i = tid; i < m; i += NQ_ORB_NT) left = fmax(left, fabs(d[i]));
  left = orb_block_max(left, red);
  if (stat == 0 && !(left < floor_piv)) stat = NQ_OCC_STATUS;        // a step more would find a pivot: the rank exceeds n_occ (or the diagonal is not finite)
  if (stat != 0) {
    for (long long e = tid; e < (long long)no * m; e += NQ_ORB_NT) Qb[e] = nan;
    for (int i = tid; i < m; i += NQ_ORB_NT) piv_out[i] = -1;
  }
  if (tid == 0) {
    min_pivot[b] = stat != 0 ? nan : pmin;
    defect[b] = stat != 0 ? nan : left;
    status[b] = stat;
  }
}

// ---- Hs = Q T on the lower-triangle tiles of the n_occ x n_occ block, mirrored ----------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_occ_reduce(OrbArgs a, int nt, const int* n_occ, const long long* occ_ptr, long long O, const double* T,
                                                         const int* status, const long long* red_ptr, long long R, double* Hs) {
  __shared__ double lds[3 * NQ_RS_TILE];
  RsMol q;
  if (!rs_mol(a, nt, n_occ, occ_ptr, O, q)) return;
  const int m = q.m, no = q.no, rows = no > 0 ? no : 1;
  const long long rbase = red_ptr[q.b];
  if (rbase < 0 || rbase + (long long)rows * rows > R) return;       // uniform
  if (no == 0) {
    if (q.t == 0 && threadIdx.x == 0) Hs[rbase] = 0.0;
    return;
  }
  if (q.t >= orb_tile_count(no)) return;                             // uniform: the barriers are reached by the whole workgroup or not at all
  int ti, tj;
  orb_tile_decode(q.t, &ti, &tj);
  const int i0 = ti * NQ_ORB_TILE, j0 = tj * NQ_ORB_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const bool bad = q.failed || status[q.b] != 0;
  orb_f64x4 acc0[4], acc1[4];
  rs_zero(acc0);
  rs_zero(acc1);
  if (!bad) rs_gemm<true, false, false>(a.coeff + q.base, nullptr, m, T + q.obase, no, 0, m, i0, no, j0, no, lds, acc0, acc1);
  double* out = Hs + rbase;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + lk + 4 * r;
      if (i < no && j <= i) {
        const double v = bad ? 0.0 : acc0[s][r];
        out[(long long)i * no + j] = v;
        if (j != i) out[(long long)j * no + i] = v;
      }
    }
  }
}

// the reduced state's block of molecule b: max(n_occ, 1) orbitals; false: not the state the reduced layout was built for (uniform)
__device__ __forceinline__ bool occ_red_mol(const OrbArgs& r, int b, int no, int& ro0, long long& rbase) {
  const int rows = no > 0 ? no : 1;
  ro0 = r.orb_ptr[b];
  rbase = r.pack_ptr[b];
  return r.orb_ptr[b + 1] - ro0 == rows && ro0 >= 0 && ro0 + rows <= r.M && rbase >= 0 && rbase + (long long)rows * rows <= r.P;
}

// ---- STEP 1: U = V Q; STEP 2: C = U W into the state's coeff ---------------------------------------------------------------------------------------------------------
template <int STEP>
__global__ __launch_bounds__(NQ_RS_NT) void k_occ_back(OrbArgs a, OrbArgs r, int tr, const int* n_occ, const long long* occ_ptr, long long O, const double* W,
                                                       const int* status, double* U) {
  __shared__ double lds[3 * NQ_RS_TILE];
  RsMol q;
  if (!rs_mol(a, tr, n_occ, occ_ptr, O, q)) return;
  if (!orb_dims_ok(r) || r.B != a.B) return;
  const int m = q.m, no = q.no;
  int ro0;
  long long rbase;
  if (!occ_red_mol(r, q.b, no, ro0, rbase)) return;
  const int m0 = q.t * NQ_ORB_TILE;
  if (m0 >= m || status[q.b] != 0 || q.failed) return;               // uniform; a failed molecule's rows are k_occ_finish's
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  double* out = STEP == 1 ? U + q.obase : a.coeff + q.base;
  for (int n0 = 0; n0 < no; n0 += NQ_ORB_TILE) {                     // uniform over the workgroup
    orb_f64x4 acc0[4], acc1[4];
    rs_zero(acc0);
    rs_zero(acc1);
    if (STEP == 1) rs_gemm<true, false, false>(r.coeff + rbase, nullptr, no, a.coeff + q.base, m, 0, no, n0, no, m0, m, lds, acc0, acc1);
    else rs_gemm<true, false, false>(U + q.obase, nullptr, m, W + q.base, m, 0, m, n0, no, m0, m, lds, acc0, acc1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = m0 + s * 16 + lc;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int i = n0 + wave * 16 + lk + 4 * rr;
        if (i < no && j < m) out[(long long)i * m + j] = acc0[s][rr];
      }
    }
  }
}

// ---- the sign rule, the levels, NaN in what is not an occupied level ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_ORB_NT) void k_occ_finish(OrbArgs a, OrbArgs r, const int* n_occ, const long long* occ_ptr, long long O, const double* U,
                                                          int from_u, int* status) {
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_SOLVE>(a, 1, q)) return;
  if (!orb_dims_ok(r) || r.B != a.B) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = q.m, b = q.b;
  int no = n_occ[b];
  no = no < 0 ? 0 : (no > m ? m : no);
  const long long obase = occ_ptr[b];
  int ro0;
  long long rbase;
  if (!occ_red_mol(r, b, no, ro0, rbase) || obase < 0 || obase + (long long)no * m > O) return;
  const int stat = q.failed ? a.status[b] : (status[b] != 0 ? status[b] : r.status[b]);
  __syncthreads();                                                   // every thread has read the words thread 0 writes below
  const double nan = nq_nan_f64();
  double* C = a.coeff + q.base;
  const double* src = from_u ? U + obase : C;
  for (int k = wave; k < m; k += NQ_ORB_NW) {
    double* row = C + (long long)k * m;
    if (k >= no || stat != 0) {
      for (int i = lane; i < m; i += 64) row[i] = nan;
      continue;
    }
    const double* s = src + (long long)k * m;
    double best = -1.0, val = 0.0;
    int at = m;
    for (int i = lane; i < m; i += 64) {
      const double x = s[i];
      if (fabs(x) > best) { best = fabs(x); val = x; at = i; }
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
      const double ob = __shfl_xor(best, sh, 64), ov = __shfl_xor(val, sh, 64);
      const int oa = __shfl_xor(at, sh, 64);
      if (ob > best || (ob == best && oa < at)) { best = ob; val = ov; at = oa; }
    }
    const double sg = val < 0.0 ? -1.0 : 1.0;
    for (int i = lane; i < m; i += 64) row[i] = sg * s[i];
  }
  for (int k = tid; k < m; k += NQ_ORB_NT) a.eps[q.o0 + k] = (k < no && stat == 0) ? r.eps[ro0 + k] : nan;
  if (tid == 0) {
    a.status[b] = stat;
    status[b] = stat;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int nq_orb_occ_factor(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, double* Q, int32_t* pivots, double* min_pivot, double* defect,
                      int32_t* status, void* stream) {
  NQ_TRY(orb_check_launch("nq_orb_occ_factor", state, B, M, P, ORB_GRID_MOL));
  if (!n_occ) return nq_fail(NQ_ERR_ARG, "nq_orb_occ_factor: n_occ is missing");
  if (!Q || !pivots || !min_pivot || !defect || !status) return nq_fail(NQ_ERR_ARG, "nq_orb_occ_factor: null argument");
  if (min_pivot == defect || Q == min_pivot || Q == defect || (const void*)pivots == (const void*)status || (const void*)pivots == (const void*)n_occ ||
      (const void*)status == (const void*)n_occ)
    return nq_fail(NQ_ERR_ARG, "nq_orb_occ_factor: the outputs must be different arrays from each other and from the inputs");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_occ_factor");
  hipLaunchKernelGGL(k_occ_factor, dim3(B), dim3(NQ_ORB_NT), 0, st, orb_args(state, B, M, P), (const int*)n_occ, Q, (int*)pivots, min_pivot, defect, (int*)status);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_occ_reduce(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, const double* T, const int32_t* status,
                      const int64_t* red_ptr, int64_t R, double* Hs, void* stream) {
  int tr = 0;
  NQ_TRY(rs_check("nq_orb_occ_reduce", state, B, M, P, n_occ, occ_ptr, O, &tr));
  if (!T || !status || !red_ptr || !Hs) return nq_fail(NQ_ERR_ARG, "nq_orb_occ_reduce: null argument");
  if (R < B || R > P + B) return nq_fail(NQ_ERR_ARG, "nq_orb_occ_reduce: R=%lld reduced entries do not fit B=%d molecules of P=%lld", (long long)R, B, (long long)P);
  if (Hs == T) return nq_fail(NQ_ERR_ARG, "nq_orb_occ_reduce: Hs must not be T");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_occ_reduce");
  const int nt = tr * (tr + 1) / 2;
  hipLaunchKernelGGL(k_occ_reduce, dim3(B * nt), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), nt, (const int*)n_occ, (const long long*)occ_ptr, (long long)O, T,
                     (const int*)status, (const long long*)red_ptr, (long long)R, Hs);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_occ_back(void* state, void* reduced_state, int32_t B, int32_t M, int64_t P, int32_t Mr, int64_t Pr, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O,
                    const double* W_or_null, int32_t* status, double* U, void* stream) {
  int tr = 0;
  NQ_TRY(rs_check("nq_orb_occ_back", state, B, M, P, n_occ, occ_ptr, O, &tr));
  if (!reduced_state) return nq_fail(NQ_ERR_ARG, "nq_orb_occ_back: null argument (reduced_state)");
  if (reduced_state == state) return nq_fail(NQ_ERR_ARG, "nq_orb_occ_back: the reduced state must not be the state");
  if (orb_check_dims(B, Mr, Pr) != NQ_OK || Mr > M + B || Pr > P + B)
    return nq_fail(NQ_ERR_ARG, "nq_orb_occ_back: the reduced dimensions Mr=%d, Pr=%lld do not fit B=%d, M=%d, P=%lld", Mr, (long long)Pr, B, M, (long long)P);
  if (!status || !U) return nq_fail(NQ_ERR_ARG, "nq_orb_occ_back: null argument");
  if (W_or_null && W_or_null == U) return nq_fail(NQ_ERR_ARG, "nq_orb_occ_back: U must not be W");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, W_or_null ? "orb_occ_back_w" : "orb_occ_back");
  const OrbArgs a = orb_args(state, B, M, P), r = orb_args(reduced_state, B, Mr, Pr);
  hipLaunchKernelGGL(k_occ_back<1>, dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, r, tr, (const int*)n_occ, (const long long*)occ_ptr, (long long)O, (const double*)nullptr,
                     (const int*)status, U);
  NQ_LAUNCH_CHECK();
  if (W_or_null) {
    hipLaunchKernelGGL(k_occ_back<2>, dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, r, tr, (const int*)n_occ, (const long long*)occ_ptr, (long long)O, W_or_null,
                       (const int*)status, U);
    NQ_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_occ_finish, dim3(B), dim3(NQ_ORB_NT), 0, st, a, r, (const int*)n_occ, (const long long*)occ_ptr, (long long)O, (const double*)U,
                     W_or_null ? 0 : 1, (int*)status);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
