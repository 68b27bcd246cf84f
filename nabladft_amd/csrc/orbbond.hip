// Mayer bond orders and atomic valences of a closed-shell density matrix D under the overlap S, and their reverse: what follows nq_orb_wgram / the purified
// density on the device when the question is which atoms share the electrons.  Serves the same empty slots of the reference as the solver
// (phisnet/nn/neural_network.py:969-993).
//
//   P      = D S                                              (S = NULL: P = D, the Wiberg index of an orthogonal basis)
//   B_AB   = sum_{mu in A, nu in B} P[mu][nu] P[nu][mu]       (symmetric, B_AA included)
//   V_A    = sum_{B != A} B_AB
//   reverse: Gamma_AB = gB_AB + (A != B ? gV_A : 0),  E[mu][nu] = (Gamma_A(mu)A(nu) + Gamma_A(nu)A(mu)) P[nu][mu]  (= dL/dP),
//            dL/dD = sym(E S), dL/dS = sym(D E): gradients with respect to symmetric matrices, spread over both triangles (the convention of nq_orb_wgram).
//
// k_orb_bond_product   P = D S, the general m x m product: one 256-thread workgroup per (molecule, 64 x 64 output tile), every tile of the square.
// k_orb_bond_reduce    one wavefront per atom pair A >= B: the at most 32 x 32 products P[mu][nu] P[nu][mu] with fma() along the lane's own elements, then the
//                      butterfly sum; lane 0 writes (A, B) and (B, A) from the same number.  k_orb_bond_valence: one wavefront per atom adds its row of the
//                      table without the diagonal.
// k_orb_bond_e         E from P, gB, gV through an orbital -> atom table in LDS, elementwise (one workgroup per 64 rows of a molecule).
// k_orb_bond_backward  out = 1/2 (A1 B1 + A2 B2) on lower-triangle 64 x 64 tiles, mirrored: blockIdx.y = 0: sym(E S) = 1/2 (E S + S E^T), 1: sym(D E) =
//                      1/2 (D E + E^T D); both contractions of a K tile go into one accumulator set, term 1 before term 2 in every step of four.
//
// Orientation.  D and S are symmetric and only their lower triangles are read, so element (k, x) of an operand tile is stored at [max][min] and either staging
// orientation of orbresp_tiles.h holds the same numbers.  Both padded layouts stage and read without bank conflicts (orbresp.hip's header: K-slow [16][64 + 16],
// the four k rows of a matrix instruction on disjoint halves of the banks; K-fast [64][16 + 2], 32 distinct bank pairs per half-wave), so what decides is the
// global read: a K tile that lies below the tile's x range (k < x) is contiguous along k in memory and is staged K-fast, a 128-byte line per row; a K tile at
// or beyond it (k >= x) is contiguous along x and is staged K-slow.  The choice is uniform over the workgroup and made per operand and K tile; only the at most
// four K tiles that cross the diagonal of a 64-wide range read part of their elements with a stride.  E is a general matrix: E[x][k] is staged K-fast,
// E[k][x] K-slow, both contiguous.  As in the response kernels one K tile is in LDS and the next in registers (256 threads, K tile 16, strides 80 / 18).
//
// Float64 throughout on v_mfma_f64_16x16x4_f64 (lane l feeds A[i0 + (l & 15)] and B[j0 + (l & 15)] at k = k0 + (l >> 4); result register r of lane l is row
// (l >> 4) + 4 r, column l & 15).  No atomics; k runs in steps of 4 from 0 with the instruction's fixed order inside a step: bitwise reproducible, independent
// of the rest of the batch.  status != 0: NaN in the molecule's own blocks of every output.  An atom whose orbital range leaves its molecule or that has more
// than 32 orbitals gives NaN for its row and column of the table (the population kernel's rule); in the reverse its orbitals carry NaN.  The grids are sized
// from (B, M, P); a surplus workgroup exits.  Other dimensions than nq_orb_init: header status -2, nothing touched.  The state's layout is all these kernels
// read of it, so a solver state and a purification state serve alike.
//
// Compiled with -ffp-contract=off like its neighbours; the kernels call fma() where they want one.
#include "orbbond_tiles.h"

#define NQ_BD_MAX_ATOM_ORB 32
#define NQ_BD_CHUNKS 64                                    // workgroups per molecule in the pair and the valence kernels; each walks its share

// the atoms of molecule b and its block of the bond table: n atoms from a0, n * n entries at bp; false: the tables do not describe such a block
struct BdAtoms {
  int a0, n;
  long long bp;
};

__device__ __forceinline__ bool bd_atoms(int b, int N, long long Q, const int* mol_ptr, const long long* bond_ptr, BdAtoms& t) {
  t.a0 = mol_ptr[b];
  const int a1 = mol_ptr[b + 1];
  t.n = a1 - t.a0;
  t.bp = 0;
  if (t.a0 < 0 || a1 < t.a0 || a1 > N) return false;
  if (!bond_ptr) return true;
  t.bp = bond_ptr[b];
  return t.bp >= 0 && bond_ptr[b + 1] - t.bp == (long long)t.n * t.n && t.bp + (long long)t.n * t.n <= Q;
}

// the orbital range [r0, r1) of atom `at` inside a molecule of m orbitals that starts at orbital o0; false: the NaN rule
__device__ __forceinline__ bool bd_range(const long long* atom_orb_ptr, int at, int o0, int m, int* r0, int* r1) {
  const long long lo = atom_orb_ptr[at] - o0, hi = atom_orb_ptr[at + 1] - o0;
  if (lo < 0 || hi < lo || hi > m || hi - lo > NQ_BD_MAX_ATOM_ORB) return false;
  *r0 = (int)lo;
  *r1 = (int)hi;
  return true;
}

// ---- P = D S -----------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_bond_product(OrbArgs a, int tr, const double* D, const void* S, int s_f64, double* out) {
  __shared__ double lds[2 * NQ_RS_TILE];
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, tr * tr, q)) return;
  const int m = q.m, ti = q.t / tr, tj = q.t - ti * tr;
  const int i0 = ti * NQ_ORB_TILE, j0 = tj * NQ_ORB_TILE;
  if (i0 >= m || j0 >= m) return;                              // uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const double nan = nq_nan_f64();
  double* X = out + q.base;
  if (!S || q.failed) {                                        // D made symmetric from its lower triangle, or NaN
    for (int e = threadIdx.x; e < NQ_ORB_TILE * NQ_ORB_TILE; e += NQ_RS_NT) {
      const int i = i0 + (e >> 6), j = j0 + (e & 63);
      if (i < m && j < m) X[(long long)i * m + j] = q.failed ? nan : D[q.base + (j <= i ? (long long)i * m + j : (long long)j * m + i)];
    }
    return;
  }
  const BdOperand oD = {D + q.base, 1, 1, 0};
  const BdOperand oS = {s_f64 ? (const void*)((const double*)S + q.base) : (const void*)((const float*)S + q.base), s_f64, 1, 0};
  orb_f64x4 acc[4];
  rs_zero(acc);
  bd_gemm<false>(oD, oS, oD, oS, m, i0, j0, 4, lds, acc);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + lk + 4 * r;
      if (i < m && j < m) X[(long long)i * m + j] = acc[s][r];
    }
  }
}

// ---- B_AB ---------------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_bond_reduce(OrbArgs a, const double* Pm, int N, long long Q, const int* mol_ptr, const long long* atom_orb_ptr,
                                                              const long long* bond_ptr, double* bond) {
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, NQ_BD_CHUNKS, q)) return;
  BdAtoms t;
  if (!bd_atoms(q.b, N, Q, mol_ptr, bond_ptr, t)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = q.m;
  const long long pairs = (long long)t.n * (t.n + 1) / 2;
  const double nan = nq_nan_f64();
  const double* X = Pm + q.base;
  for (long long p = (long long)q.t * (NQ_RS_NT / 64) + wave; p < pairs; p += (long long)NQ_BD_CHUNKS * (NQ_RS_NT / 64)) {   // uniform over the wavefront
    long long A = (long long)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (A * (A + 1) / 2 > p) --A;                           // the root may be one off either way
    while ((A + 1) * (A + 2) / 2 <= p) ++A;
    const long long Bn = p - A * (A + 1) / 2;                  // Bn <= A < n
    int ra0 = 0, ra1 = 0, rb0 = 0, rb1 = 0;
    const bool ok = bd_range(atom_orb_ptr, t.a0 + (int)A, q.o0, m, &ra0, &ra1) && bd_range(atom_orb_ptr, t.a0 + (int)Bn, q.o0, m, &rb0, &rb1);
    double v = nan;
    if (ok && !q.failed) {
      const int nb = rb1 - rb0, cnt = (ra1 - ra0) * nb;
      double s = 0.0;
      for (int e = lane; e < cnt; e += 64) {
        const int mu = ra0 + e / nb, nu = rb0 + e % nb;
        s = fma(X[(long long)mu * m + nu], X[(long long)nu * m + mu], s);
      }
      v = nq_wave_sum_f64(s);
    }
    if (lane == 0) {
      bond[t.bp + A * t.n + Bn] = v;
      bond[t.bp + Bn * t.n + A] = v;
    }
  }
}

__global__ __launch_bounds__(NQ_RS_NT) void k_orb_bond_valence(OrbArgs a, int N, long long Q, const int* mol_ptr, const long long* bond_ptr, const double* bond,
                                                               double* valence) {
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, NQ_BD_CHUNKS, q)) return;
  BdAtoms t;
  if (!bd_atoms(q.b, N, Q, mol_ptr, bond_ptr, t)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int A = q.t * (NQ_RS_NT / 64) + wave; A < t.n; A += NQ_BD_CHUNKS * (NQ_RS_NT / 64)) {
    const double* row = bond + t.bp + (long long)A * t.n;
    double s = 0.0;
    for (int Bn = lane; Bn < t.n; Bn += 64)
      if (Bn != A) s += row[Bn];
    s = nq_wave_sum_f64(s);
    if (lane == 0) valence[t.a0 + A] = s;
  }
}

// ---- E = dL/dP ----------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_bond_e(OrbArgs a, int tr, const double* gB, const double* gV, const double* Pm, int N, long long Q,
                                                         const int* mol_ptr, const long long* atom_orb_ptr, const long long* bond_ptr, double* E) {
  __shared__ short atom_of[NQ_ORB_MAX_M];
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, tr, q)) return;
  const int m = q.m, i0 = q.t * NQ_ORB_TILE;
  if (i0 >= m) return;                                         // uniform
  BdAtoms t;
  const bool tables = bd_atoms(q.b, N, Q, mol_ptr, gB ? bond_ptr : nullptr, t);
  for (int i = threadIdx.x; i < m; i += NQ_RS_NT) atom_of[i] = -1;      // an orbital no valid atom owns: NaN, as in the forward
  __syncthreads();
  if (tables)
    for (int at = threadIdx.x; at < t.n && at < 32767; at += NQ_RS_NT) {    // the table holds shorts; atoms beyond own no orbital of a molecule of <= 1024
      int r0 = 0, r1 = 0;
      if (bd_range(atom_orb_ptr, t.a0 + at, q.o0, m, &r0, &r1))
        for (int k = r0; k < r1; ++k) atom_of[k] = (short)at;
    }
  __syncthreads();
  const double nan = nq_nan_f64();
  const double* X = Pm + q.base;
  double* out = E + q.base;
  const int rows = m - i0 < NQ_ORB_TILE ? m - i0 : NQ_ORB_TILE;
  for (int e = threadIdx.x; e < rows * m; e += NQ_RS_NT) {
    const int mu = i0 + e / m, nu = e % m;
    const int A = atom_of[mu], Bn = atom_of[nu];
    double v = nan;
    if (!q.failed && A >= 0 && Bn >= 0) {
      double gab = gB ? gB[t.bp + (long long)A * t.n + Bn] : 0.0, gba = gB ? gB[t.bp + (long long)Bn * t.n + A] : 0.0;
      if (gV && A != Bn) {
        gab = gab + gV[t.a0 + A];
        gba = gba + gV[t.a0 + Bn];
      }
      v = (gab + gba) * X[(long long)nu * m + mu];
    }
    out[(long long)mu * m + nu] = v;
  }
}

// ---- sym(E S) and sym(D E) ---------------------------------------------------------------------------------------------------------------------------------------------
// two workgroups per SIMD: without the bound the compiler keeps the LDS reads of a whole K tile in registers and takes two more than half the file
__global__ __launch_bounds__(NQ_RS_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_orb_bond_backward(OrbArgs a, int nt, const double* E, const double* D, const void* S, int s_f64, double* gD,
                                                                double* gS) {
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
  const bool overlap_half = gD == nullptr || blockIdx.y == 1;  // this workgroup's output: sym(D E), else sym(E S)
  double* X = (overlap_half ? gS : gD) + q.base;
  const double* Eb = E + q.base;
  const double nan = nq_nan_f64();
  orb_f64x4 acc[4];
  rs_zero(acc);
  // sym(D E): D[i][k] E[k][j] + E[k][i] D[k][j];  sym(E S): E[i][k] S[k][j] + S[i][k] E[j][k].  One call, so that the product loop exists once in the kernel.
  const void* Sb = !S ? nullptr : s_f64 ? (const void*)((const double*)S + q.base) : (const void*)((const float*)S + q.base);
  const BdOperand oE = {Eb, 1, 0, overlap_half ? 0 : 1};
  const BdOperand oM = {overlap_half ? (const void*)(D + q.base) : Sb, overlap_half ? 1 : s_f64, 1, 0};
  if (!q.failed && oM.p) bd_gemm<true>(overlap_half ? oM : oE, overlap_half ? oE : oM, overlap_half ? oE : oM, overlap_half ? oM : oE, m, i0, j0, nsub, lds, acc);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= nsub) continue;
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + lk + 4 * r;
      if (i < m && j <= i) {
        double v = 0.5 * acc[s][r];
        if (!overlap_half && !S) v = 0.5 * (Eb[(long long)i * m + j] + Eb[(long long)j * m + i]);      // the identity: sym(E)
        if (q.failed) v = nan;
        X[(long long)i * m + j] = v;
        if (j != i) X[(long long)j * m + i] = v;
      }
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// the atom tables every launch that takes them checks: N atoms in B molecules own between N and (N - B + 1)^2 + B - 1 entries of the bond table
static int bd_check_atoms(const char* who, int32_t B, int32_t N, int64_t Q, bool with_table) {
  if (N < B) return nq_fail(NQ_ERR_ARG, "%s: N=%d atoms for B=%d molecules", who, N, B);
  if (!with_table) return NQ_OK;
  const long long big = (long long)N - B + 1;
  if (Q < N || Q > big * big + (B - 1))
    return nq_fail(NQ_ERR_ARG, "%s: Q=%lld bond entries are inconsistent with a mol_ptr of N=%d atoms in B=%d molecules", who, (long long)Q, N, B);
  return NQ_OK;
}

extern "C" {

int nq_orb_bond_product(void* state, int32_t B, int32_t M, int64_t P, const double* D, const void* S, int32_t s_f64, double* out_P, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_bond_product", state, B, M, P, ORB_GRID_SQUARE, &tr));
  if (!D || !out_P) return nq_fail(NQ_ERR_ARG, "nq_orb_bond_product: null argument");
  if (out_P == D || (const void*)out_P == S) return nq_fail(NQ_ERR_ARG, "nq_orb_bond_product: the output must not be an operand");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, S ? "orb_bond_product" : "orb_bond_product_copy");
  hipLaunchKernelGGL(k_orb_bond_product, dim3(B * tr * tr), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), tr, D, S, s_f64, out_P);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_bond_reduce(void* state, int32_t B, int32_t M, int64_t P, const double* Pm, int32_t N, int64_t Q, const int32_t* mol_ptr, const int64_t* atom_orb_ptr,
                       const int64_t* bond_ptr, double* out_bond, double* out_valence, void* stream) {
  NQ_TRY(orb_check_launch("nq_orb_bond_reduce", state, B, M, P, ORB_GRID_MOL, nullptr, NQ_BD_CHUNKS));
  if (!Pm || !mol_ptr || !atom_orb_ptr || !bond_ptr || !out_bond) return nq_fail(NQ_ERR_ARG, "nq_orb_bond_reduce: null argument");
  NQ_TRY(bd_check_atoms("nq_orb_bond_reduce", B, N, Q, true));
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_bond_reduce");
  const OrbArgs a = orb_args(state, B, M, P);
  hipLaunchKernelGGL(k_orb_bond_reduce, dim3(B * NQ_BD_CHUNKS), dim3(NQ_RS_NT), 0, st, a, Pm, N, (long long)Q, mol_ptr, (const long long*)atom_orb_ptr,
                     (const long long*)bond_ptr, out_bond);
  NQ_LAUNCH_CHECK();
  if (out_valence) {
    hipLaunchKernelGGL(k_orb_bond_valence, dim3(B * NQ_BD_CHUNKS), dim3(NQ_RS_NT), 0, st, a, N, (long long)Q, mol_ptr, (const long long*)bond_ptr,
                       (const double*)out_bond, out_valence);
    NQ_LAUNCH_CHECK();
  }
  return NQ_OK;
}

int nq_orb_bond_backward(void* state, int32_t B, int32_t M, int64_t P, const double* gB, const double* gV, const double* Pm, const double* D, const void* S,
                         int32_t s_f64, int32_t N, int64_t Q, const int32_t* mol_ptr, const int64_t* atom_orb_ptr, const int64_t* bond_ptr, double* E,
                         double* out_gD, double* out_gS, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_bond_backward", state, B, M, P, ORB_GRID_LOWER, &tr));
  if (!Pm || !mol_ptr || !atom_orb_ptr || !E) return nq_fail(NQ_ERR_ARG, "nq_orb_bond_backward: null argument");
  if (gB && !bond_ptr) return nq_fail(NQ_ERR_ARG, "nq_orb_bond_backward: null argument (gB needs bond_ptr)");
  if (!out_gD && !out_gS) return nq_fail(NQ_ERR_ARG, "nq_orb_bond_backward: null argument (no output)");
  if (out_gS && !S) return nq_fail(NQ_ERR_ARG, "nq_orb_bond_backward: a gradient of S needs S");
  if (out_gS && !D) return nq_fail(NQ_ERR_ARG, "nq_orb_bond_backward: a gradient of S needs D");
  if (D && !out_gS) return nq_fail(NQ_ERR_ARG, "nq_orb_bond_backward: D is the second input, of out_gS: a second input needs its output");
  if (E == Pm || E == out_gD || E == out_gS || E == D || (const void*)E == S || (out_gD && out_gD == out_gS))
    return nq_fail(NQ_ERR_ARG, "nq_orb_bond_backward: E and the outputs must be arrays of their own");
  NQ_TRY(bd_check_atoms("nq_orb_bond_backward", B, N, Q, gB != nullptr));
  const int nt = tr * (tr + 1) / 2;
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, out_gS ? (out_gD ? "orb_bond_backward_two" : "orb_bond_backward_s") : "orb_bond_backward_one");
  const OrbArgs a = orb_args(state, B, M, P);
  hipLaunchKernelGGL(k_orb_bond_e, dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, tr, gB, gV, Pm, N, (long long)Q, mol_ptr, (const long long*)atom_orb_ptr,
                     (const long long*)bond_ptr, E);
  NQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_orb_bond_backward, dim3(B * nt, out_gD && out_gS ? 2 : 1), dim3(NQ_RS_NT), 0, st, a, nt, (const double*)E, D, S, s_f64, out_gD, out_gS);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
