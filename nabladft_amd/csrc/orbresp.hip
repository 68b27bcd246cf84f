// The response of the closed-shell density matrix D = 2 C_o C_o^T to H and S, and the reverse of the population kernel: what a loss on densities, populations
// or Tr(D H) needs after a batched solve of H C = S C diag(eps) (orbitals.hip).  Serves the same empty slots of the reference as the solver
// (phisnet/nn/neural_network.py:969-993).
//
// With Gs = (G + G^T) / 2 for an upstream G = dL/dD, o = the first n_occ orbitals, v = the rest (the state stores C^T: row k of a block = orbital k):
//
//   k_orb_resp_sym      Gs                                            packed [m][m], lower-triangle 64 x 64 tiles through LDS, mirrored (orbresp_tiles.h)
//   k_orb_resp<1>       T[mu][i]  = sum_nu Gs[nu][mu] Ct[i][nu]       occupied-packed [m][n_o]  (= Gs C_o; nq_orb_resp_project launches both)
//   k_orb_resp<2>       W[k][i]   = sum_mu Ct[k][mu] T[mu][i]         and its epilogue: k >= n_o: A_H = 4 W / (eps_i - eps_k), A_S = -eps_i A_H;
//                                                                     k < n_o: A_H = 0, A_S = -2 W          occupied-packed [m][n_o]  (nq_orb_resp_mo)
//   k_orb_resp<3>       Rt_X[i][mu] = sum_k A_X[k][i] Ct[k][mu]       occupied-packed [n_o][m]; X = H alone, or H and S from the same loads of Ct (nq_orb_resp_back)
//   k_orb_syr2k         X[mu][nu] = 1/2 sum_{i < n_o} (Rt[i][mu] Ct[i][nu] + Ct[i][mu] Rt[i][nu])   packed [m][m], for one or two Rt from the same loads of Ct
//
// The only division is the epilogue's, by occupied-virtual differences: equal levels inside o or inside v never meet.  n_o = m: A_H = 0, so dL/dH = 0.
//
// Orientation.  T and A are stored [m][n_o], Rt [n_o][m]: the contraction index is then the slow one of every operand except Ct in the first two products
// (there is no stored C).  All five products stage their operands through LDS: a K-slow operand as [16][64 + 16] (the four k rows of one matrix instruction
// fall on disjoint halves of the 64 banks), a K-fast operand (Ct) as [64][16 + 2] read along a 128-byte line per row, so global reads are contiguous in both
// cases and the ds_read_b64 of the 32 lanes of a half-wave hit 32 distinct bank pairs.  Each thread fetches the next K tile into registers before the matrix
// instructions of the current one: one tile in LDS, one in flight, so a K tile costs one global-load round trip (README: where these kernels lose).
//
// One 256-thread workgroup per (molecule, 64 orbitals along the m side) for the three rectangular products: it walks the 64 x 64 output tiles along the n_o
// side itself (one workgroup per tile was 2.9 and 4.0 times slower for the first two products at 512 molecules, 10 % faster for the third); one workgroup
// per (molecule, 64 x 64 lower-triangle tile) for the last, where walking a tile row was 2.6 times slower.  The grid holds the tiles of the largest molecule
// the dimensions allow for every molecule, a surplus workgroup exits.
// Each wavefront owns a 16-row strip: four 16 x 16 accumulators per output, v_mfma_f64_16x16x4_f64 (lane l feeds A[i0 + (l & 15)]
// and B[j0 + (l & 15)] at k = k0 + (l >> 4); result register r of lane l is row (l >> 4) + 4 r, column l & 15).  Operands beyond m, n_o or the K range are zero,
// stores are masked.  No atomics; k runs in steps of 4 from a multiple of 4 with the instruction's fixed order inside a step: bitwise reproducible, independent
// of the rest of the batch.  status != 0: NaN in the molecule's own block of every output.  n_o is clamped to 0..m; an occupied-packed block that does not
// lie inside [0, O) is not touched.
//
// k_orb_population_backward  one 512-thread workgroup per molecule, elementwise: from g_pop [N], g_nelec [B], g_eband [B] (each may be NULL: zero) the
//                 gradients of nq_orb_population with respect to symmetric D, S and H (the convention of nq_orb_wgram), lower triangles of S and H only:
//                   dD_ij = (g_ij + g_ne) S_ij + g_eb H_ij,  g_ij = (g_A(i) + g_A(j)) / 2      (S = NULL: the identity)
//                   dS_ij = ((g_A(i) + g_ne) D_ij + (g_A(j) + g_ne) D_ji) / 2                  dH_ij = g_eb (D_ij + D_ji) / 2
//
// Compiled with -ffp-contract=off like orbitals.hip and orbdens.hip.
#include "orbresp_tiles.h"

// ---- Gs = (G + G^T) / 2 ---------------------------------------------------------------------------------------------------------------------------------------------
// The tile routine of orbresp_tiles.h.  A failed molecule's Gs stays the finite average: the NaN of its outputs comes from the products that follow.  The range
// test of the molecule's first orbital that the shared lookup adds to this kernel cannot fail on a state that passed orb_dims_ok (nq_orb_init wrote orb_ptr
// and pack_ptr together).
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_resp_sym(OrbArgs a, int nt, const double* G, double* Gs) { orb_symmetrize_kernel<false, true>(a, nt, G, Gs); }

// ---- steps 1 to 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
// STEP 1: T = Gs C_o; STEP 2: A_H (out0), A_S (out1, TWO) from W = Ct T; STEP 3: Rt_H (out0), Rt_S (out1, TWO) from A_H (in0), A_S (in1)
template <int STEP, bool TWO>
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_resp(OrbArgs a, int tr, const int* n_occ, const long long* occ_ptr, long long O, const double* in0,
                                                       const double* in1, double* out0, double* out1) {
  __shared__ double lds[3 * NQ_RS_TILE];
  RsMol q;
  if (!rs_mol(a, tr, n_occ, occ_ptr, O, q)) return;
  const int m = q.m, no = q.no;
  const int R = STEP == 3 ? no : m, Cn = STEP == 3 ? m : no;   // the output is R x Cn, row-major
  const int m0 = q.t * NQ_ORB_TILE;                            // the workgroup's 64 orbitals along the m side; it walks the n_o side itself
  if (m0 >= m) return;
  const double* Ct = a.coeff + q.base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const double nan = nq_nan_f64();
  const double* eps = a.eps + q.o0;
  double* X0 = out0 + q.obase;
  double* X1 = TWO ? out1 + q.obase : nullptr;
  for (int n0 = 0; n0 < no; n0 += NQ_ORB_TILE) {               // uniform over the workgroup
    const int i0 = STEP == 3 ? n0 : m0, j0 = STEP == 3 ? m0 : n0;
    orb_f64x4 acc0[4], acc1[4];
    rs_zero(acc0);
    rs_zero(acc1);
    if (!q.failed) {
      if (STEP == 1) rs_gemm<false, true, false>(in0 + q.base, nullptr, m, Ct, m, 0, m, i0, R, j0, Cn, lds, acc0, acc1);
      if (STEP == 2) rs_gemm<true, false, false>(Ct, nullptr, m, in0 + q.obase, no, 0, m, i0, R, j0, Cn, lds, acc0, acc1);
      // A_H is zero over k < n_o: without A_S the sum starts at the multiple of 4 below n_o, which leaves the steps of the matrix instruction where they are
      if (STEP == 3) rs_gemm<false, false, TWO>(in0 + q.obase, TWO ? in1 + q.obase : nullptr, no, Ct, m, TWO ? 0 : (no & ~3), m, i0, R, j0, Cn, lds, acc0, acc1);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = j0 + s * 16 + lc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wave * 16 + lk + 4 * r;
        if (i >= R || j >= Cn) continue;
        double v0 = acc0[s][r], v1 = acc1[s][r];
        if (STEP == 2) {                                       // row i = orbital k, column j = occupied orbital
          const double w = v0;
          if (i >= no) {
            v0 = 4.0 * w / (eps[j] - eps[i]);
            v1 = -eps[j] * v0;
          } else {
            v0 = 0.0;
            v1 = -2.0 * w;
          }
        }
        X0[(long long)i * Cn + j] = q.failed ? nan : v0;
        if (TWO) X1[(long long)i * Cn + j] = q.failed ? nan : v1;
      }
    }
  }
}

// ---- step 4 ---------------------------------------------------------------------------------------------------------------------------------------------------------
template <bool TWO>
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_syr2k(OrbArgs a, int nt, const int* n_occ, const long long* occ_ptr, long long O, const double* rt0,
                                                        const double* rt1, double* out0, double* out1) {
  __shared__ double lds[6 * NQ_RS_TILE];
  RsMol q;
  if (!rs_mol(a, nt, n_occ, occ_ptr, O, q)) return;
  const int m = q.m, no = q.no;
  if (q.t >= orb_tile_count(m)) return;
  int ti, tj;
  orb_tile_decode(q.t, &ti, &tj);
  const int i0 = ti * NQ_ORB_TILE, j0 = tj * NQ_ORB_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const bool rows = i0 + wave * 16 < m;
  const int nsub = ti == tj ? wave + 1 : 4;                    // a diagonal tile: the sub-tiles on and below the diagonal
  const double* Ct = a.coeff + q.base;
  const double* R0 = rt0 + q.obase;
  const double* R1 = TWO ? rt1 + q.obase : nullptr;
  double* tCi = lds;                                           // rows i0..: Ct, Rt0, Rt1; columns j0..: Ct, Rt0, Rt1
  double* tR0i = lds + NQ_RS_TILE;
  double* tR1i = lds + 2 * NQ_RS_TILE;
  double* tCj = lds + 3 * NQ_RS_TILE;
  double* tR0j = lds + 4 * NQ_RS_TILE;
  double* tR1j = lds + 5 * NQ_RS_TILE;
  const double nan = nq_nan_f64();
  double* X0 = out0 + q.base;
  double* X1 = TWO ? out1 + q.base : nullptr;
  orb_f64x4 acc0[4], acc1[4];
  rs_zero(acc0);
  rs_zero(acc1);
  if (!q.failed && no > 0) {
    double rci[NQ_RS_PER], r0i[NQ_RS_PER], r1i[NQ_RS_PER], rcj[NQ_RS_PER], r0j[NQ_RS_PER], r1j[NQ_RS_PER];
    auto fetch = [&](int k0) {
      rs_fetch<false>(rci, Ct, m, k0, no, i0, m);
      rs_fetch<false>(r0i, R0, m, k0, no, i0, m);
      rs_fetch<false>(rcj, Ct, m, k0, no, j0, m);
      rs_fetch<false>(r0j, R0, m, k0, no, j0, m);
      if (TWO) {
        rs_fetch<false>(r1i, R1, m, k0, no, i0, m);
        rs_fetch<false>(r1j, R1, m, k0, no, j0, m);
      }
    };
    fetch(0);
    for (int k0 = 0; k0 < no; k0 += NQ_RS_KT) {
      __syncthreads();
      rs_stage<false>(tCi, rci);
      rs_stage<false>(tR0i, r0i);
      rs_stage<false>(tCj, rcj);
      rs_stage<false>(tR0j, r0j);
      if (TWO) {
        rs_stage<false>(tR1i, r1i);
        rs_stage<false>(tR1j, r1j);
      }
      __syncthreads();
      if (k0 + NQ_RS_KT < no) fetch(k0 + NQ_RS_KT);
      if (rows) {
#pragma unroll
        for (int kk = 0; kk < NQ_RS_KT; kk += 4) {
          if (k0 + kk >= no) break;
          const int x = wave * 16 + lc;
          const double ac = rs_get<false>(tCi, kk + lk, x), ar0 = rs_get<false>(tR0i, kk + lk, x);
          const double ar1 = TWO ? rs_get<false>(tR1i, kk + lk, x) : 0.0;
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if (s < nsub && j0 + s * 16 < m) {
              const double bc = rs_get<false>(tCj, kk + lk, s * 16 + lc), br0 = rs_get<false>(tR0j, kk + lk, s * 16 + lc);
              acc0[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar0, bc, acc0[s], 0, 0, 0);
              acc0[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac, br0, acc0[s], 0, 0, 0);
              if (TWO) {
                const double br1 = rs_get<false>(tR1j, kk + lk, s * 16 + lc);
                acc1[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar1, bc, acc1[s], 0, 0, 0);
                acc1[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac, br1, acc1[s], 0, 0, 0);
              }
            }
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= nsub) continue;
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + lk + 4 * r;
      if (i < m && j <= i) {
        const double v0 = q.failed ? nan : 0.5 * acc0[s][r];
        X0[(long long)i * m + j] = v0;
        if (j != i) X0[(long long)j * m + i] = v0;
        if (TWO) {
          const double v1 = q.failed ? nan : 0.5 * acc1[s][r];
          X1[(long long)i * m + j] = v1;
          if (j != i) X1[(long long)j * m + i] = v1;
        }
      }
    }
  }
}

// ---- the reverse of k_orb_population ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_ORB_NT) void k_orb_population_backward(OrbArgs a, const double* g_pop, const double* g_nelec, const double* g_eband,
                                                                       const double* D, const void* H, int h_f64, const void* S, int s_f64, int N,
                                                                       const int* mol_ptr, const long long* atom_orb_ptr, double* gD, double* gS, double* gH) {
  __shared__ double gorb[NQ_ORB_MAX_M];
  if (!orb_dims_ok(a)) return;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int o0 = a.orb_ptr[b], m = a.orb_ptr[b + 1] - o0;
  const long long base = a.pack_ptr[b];
  if (m < 1 || m > NQ_ORB_MAX_M || base < 0 || base + (long long)m * m > a.P) return;   // uniform: a state overwritten since nq_orb_init
  const int a0 = mol_ptr[b], a1 = mol_ptr[b + 1];
  const bool atoms_ok = a0 >= 0 && a1 >= a0 && a1 <= N;
  const double nan = nq_nan_f64();
  for (int i = tid; i < m; i += NQ_ORB_NT) gorb[i] = g_pop ? nan : 0.0;                  // an orbital no atom owns: as the forward, NaN
  __syncthreads();
  if (g_pop && atoms_ok)
    for (int at = a0 + tid; at < a1; at += NQ_ORB_NT) {
      const long long r0 = atom_orb_ptr[at] - o0, r1 = atom_orb_ptr[at + 1] - o0;
      if (r0 >= 0 && r1 >= r0 && r1 <= m)
        for (long long k = r0; k < r1; ++k) gorb[k] = g_pop[at];
    }
  __syncthreads();
  const double gne = g_nelec ? g_nelec[b] : 0.0, geb = (g_eband && H) ? g_eband[b] : 0.0;
  for (long long e = tid; e < (long long)m * m; e += NQ_ORB_NT) {
    const int i = (int)(e / m), j = (int)(e - (long long)i * m);
    const long long low = base + (j <= i ? (long long)i * m + j : (long long)j * m + i);   // the lower-triangle copy of element (i, j)
    const double gi = gorb[i] + gne, gj = gorb[j] + gne;
    double d = 0.0;
    if (S) d = (0.5 * (gorb[i] + gorb[j]) + gne) * nq_load_f64(S, low, s_f64);
    else if (i == j) d = gi;
    if (H) d = d + geb * nq_load_f64(H, low, h_f64);
    gD[base + e] = d;
    if (gS || gH) {
      const double dij = D[base + e], dji = D[base + (long long)j * m + i];
      if (gS) gS[base + e] = 0.5 * (gi * dij + gj * dji);
      if (gH) gH[base + e] = geb * (0.5 * (dij + dji));
    }
  }
}

// ---- host (rs_check: orbresp_tiles.h) ---------------------------------------------------------------------------------------------------------------------------

extern "C" {

int nq_orb_resp_project(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, const double* G, double* Gs,
                        double* T, void* stream) {
  int tr = 0;
  NQ_TRY(rs_check("nq_orb_resp_project", state, B, M, P, n_occ, occ_ptr, O, &tr));
  if (!G || !Gs || !T) return nq_fail(NQ_ERR_ARG, "nq_orb_resp_project: null argument");
  if (G == Gs) return nq_fail(NQ_ERR_ARG, "nq_orb_resp_project: Gs must not be G");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_resp_project");
  const OrbArgs a = orb_args(state, B, M, P);
  const int nt = tr * (tr + 1) / 2;
  hipLaunchKernelGGL(k_orb_resp_sym, dim3(B * nt), dim3(NQ_RS_NT), 0, st, a, nt, G, Gs);
  NQ_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_orb_resp<1, false>), dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, tr, (const int*)n_occ, (const long long*)occ_ptr, (long long)O,
                     (const double*)Gs, (const double*)nullptr, T, (double*)nullptr);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_resp_mo(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, const double* T, double* A_H,
                   double* A_S, void* stream) {
  int tr = 0;
  NQ_TRY(rs_check("nq_orb_resp_mo", state, B, M, P, n_occ, occ_ptr, O, &tr));
  if (!T || !A_H) return nq_fail(NQ_ERR_ARG, "nq_orb_resp_mo: null argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, A_S ? "orb_resp_mo_two" : "orb_resp_mo_one");
  const OrbArgs a = orb_args(state, B, M, P);
  if (A_S)
    hipLaunchKernelGGL((k_orb_resp<2, true>), dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, tr, (const int*)n_occ, (const long long*)occ_ptr, (long long)O, T,
                       (const double*)nullptr, A_H, A_S);
  else
    hipLaunchKernelGGL((k_orb_resp<2, false>), dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, tr, (const int*)n_occ, (const long long*)occ_ptr, (long long)O, T,
                       (const double*)nullptr, A_H, (double*)nullptr);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_resp_back(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, const double* A_H, const double* A_S,
                     double* Rt_H, double* Rt_S, void* stream) {
  int tr = 0;
  NQ_TRY(rs_check("nq_orb_resp_back", state, B, M, P, n_occ, occ_ptr, O, &tr));
  if (!A_H || !Rt_H) return nq_fail(NQ_ERR_ARG, "nq_orb_resp_back: null argument");
  if (A_S && !Rt_S) return nq_fail(NQ_ERR_ARG, "nq_orb_resp_back: a second input needs a second output");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, A_S ? "orb_resp_back_two" : "orb_resp_back_one");
  const OrbArgs a = orb_args(state, B, M, P);
  if (A_S)
    hipLaunchKernelGGL((k_orb_resp<3, true>), dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, tr, (const int*)n_occ, (const long long*)occ_ptr, (long long)O, A_H,
                       A_S, Rt_H, Rt_S);
  else
    hipLaunchKernelGGL((k_orb_resp<3, false>), dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, tr, (const int*)n_occ, (const long long*)occ_ptr, (long long)O, A_H,
                       (const double*)nullptr, Rt_H, (double*)nullptr);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_syr2k(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, const double* Rt0, const double* Rt1,
                 double* out0, double* out1, void* stream) {
  int tr = 0;
  NQ_TRY(rs_check("nq_orb_syr2k", state, B, M, P, n_occ, occ_ptr, O, &tr));
  if (!Rt0 || !out0) return nq_fail(NQ_ERR_ARG, "nq_orb_syr2k: null argument");
  if (Rt1 && !out1) return nq_fail(NQ_ERR_ARG, "nq_orb_syr2k: a second input needs a second output");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, Rt1 ? "orb_syr2k_two" : "orb_syr2k_one");
  const OrbArgs a = orb_args(state, B, M, P);
  const int nt = tr * (tr + 1) / 2;
  if (Rt1)
    hipLaunchKernelGGL(k_orb_syr2k<true>, dim3(B * nt), dim3(NQ_RS_NT), 0, st, a, nt, (const int*)n_occ, (const long long*)occ_ptr, (long long)O, Rt0, Rt1, out0,
                       out1);
  else
    hipLaunchKernelGGL(k_orb_syr2k<false>, dim3(B * nt), dim3(NQ_RS_NT), 0, st, a, nt, (const int*)n_occ, (const long long*)occ_ptr, (long long)O, Rt0,
                       (const double*)nullptr, out0, (double*)nullptr);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_population_backward(void* state, int32_t B, int32_t M, int64_t P, const double* g_pop, const double* g_nelec, const double* g_eband, const double* D,
                               const void* H, int32_t h_f64, const void* S, int32_t s_f64, int32_t N, const int32_t* mol_ptr, const int64_t* atom_orb_ptr,
                               double* out_gD, double* out_gS, double* out_gH, void* stream) {
  if (!state || !mol_ptr || !atom_orb_ptr || !out_gD) return nq_fail(NQ_ERR_ARG, "nq_orb_population_backward: null argument");
  if ((out_gS || out_gH) && !D) return nq_fail(NQ_ERR_ARG, "nq_orb_population_backward: the gradients of S and H need D");
  if (out_gS && !S) return nq_fail(NQ_ERR_ARG, "nq_orb_population_backward: a gradient of S needs S");
  if ((out_gH || g_eband) && !H) return nq_fail(NQ_ERR_ARG, "nq_orb_population_backward: the band energy needs H");
  NQ_TRY(orb_check_dims(B, M, P));
  if (N < B) return nq_fail(NQ_ERR_ARG, "nq_orb_population_backward: N=%d atoms for B=%d molecules", N, B);
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_population_backward");
  hipLaunchKernelGGL(k_orb_population_backward, dim3(B), dim3(NQ_ORB_NT), 0, st, orb_args(state, B, M, P), g_pop, g_nelec, g_eband, D, H, h_f64, S, s_f64, N,
                     mol_ptr, (const long long*)atom_orb_ptr, out_gD, out_gS, out_gH);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
