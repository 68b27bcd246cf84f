// Weighted Gram products of the orbital coefficients and Mulliken populations: what follows a batched solve of H C = S C diag(eps) (orbitals.hip) on the
// device.  Serves the same empty slots of the reference as the solver (phisnet/nn/neural_network.py:969-993): a loss on `orbital_energies` needs their
// gradient, and whoever has `orbital_coefficients` next wants the density matrix and its populations.
//
// k_orb_wgram     X_b[i][j] = sum_{k = lo_b .. hi_b - 1} w[orb_ptr[b] + k] C_b[k][i] C_b[k][j], C_b[k][:] = orbital k = ROW k of the block at pack_ptr[b] of the
//                 state's `coeff`, for one or two weight vectors from the same operand loads:
//                   w = dL/deps                      -> dL/dH   (d eps_k = c_k^T (dH - eps_k dS) c_k: no 1 / (eps_i - eps_j), degenerate orbitals are harmless)
//                   w = -eps dL/deps                 -> dL/dS
//                   w = 2, w = 2 eps over k < n_occ  -> the density matrix D and the energy-weighted density W
//                 One 256-thread workgroup per (molecule, 64 x 64 output tile), lower-triangle tiles only; the grid holds the tiles of the largest molecule the
//                 dimensions allow for every molecule, a workgroup beyond its molecule's own tiles exits (the state has no tile list).  Each wavefront owns a
//                 16-row strip of the tile: four (on a diagonal tile: its column index + 1) 16 x 16 accumulators per weight vector, v_mfma_f64_16x16x4_f64.
//                 Lane l feeds A = w_k C[k][i0 + (l & 15)] and B = C[k][j0 + (l & 15)] at k = k0 + (l >> 4): both are contiguous reads along a row of C, four
//                 rows per instruction; result register r of lane l is X[i0 + (l >> 4) + 4 r][j0 + (l & 15)] (the f64 map, not the f32 one).
//                 The C slab is NOT staged in LDS: a row segment is reused by the four wavefronts of the workgroup only, which the CU's vector L1 serves, and
//                 the operands of step k + 4 are fetched before the products of step k; the job's time is the solve's (README).
//                 Ragged edges: operands beyond m or beyond hi are zero, stores are masked.  Only j <= i is computed and stored to both (i, j) and (j, i):
//                 fl(w c_i) c_j != fl(w c_j) c_i, the mirror makes the result exactly symmetric.  No atomics; the summation order is k = lo, lo + 4, ... with
//                 the instruction's fixed order inside a step: bitwise reproducible, independent of the rest of the batch.
//                 status != 0: NaN in the molecule's block.  Empty range: zeros.
// k_orb_population  one 512-thread workgroup per molecule: pop_mu = sum_nu D_mu,nu S_mu,nu (one row per wavefront, lower triangles of S and H only, S = NULL:
//                 the identity) into LDS, one thread per atom adds its contiguous orbital range; nelec = sum_mu pop_mu, eband = sum_mu,nu D_mu,nu H_mu,nu.
//
// Compiled with -ffp-contract=off like orbitals.hip; the kernels call fma() where they want one.
#include <limits.h>

#include "orbstate.h"

#define NQ_WG_NT 256
typedef double orb_f64x4 __attribute__((ext_vector_type(4)));

struct WgOperands {
  double a0, a1, b[4];
};

template <bool TWO>
__global__ __launch_bounds__(NQ_WG_NT) void k_orb_wgram(OrbArgs a, int nt, const double* w0, const double* w1, const int* k_lo, const int* k_hi, double* out0,
                                                        double* out1) {
  if (!orb_kind_ok(a, false)) return;
  const int b = blockIdx.x / nt, t = blockIdx.x - b * nt;
  if (b >= a.B) return;
  const int o0 = a.orb_ptr[b], m = a.orb_ptr[b + 1] - o0;
  const long long base = a.pack_ptr[b];
  if (m < 1 || m > NQ_ORB_MAX_M || o0 < 0 || o0 + m > a.M || base < 0 || base + (long long)m * m > a.P) return;   // a state overwritten since nq_orb_init
  if (t >= orb_tile_count(m)) return;                                                                              // (the solver says so: status 3)
  int ti, tj;
  orb_tile_decode(t, &ti, &tj);
  int lo = k_lo ? k_lo[b] : 0, hi = k_hi ? k_hi[b] : m;
  lo = lo < 0 ? 0 : lo;
  hi = hi > m ? m : hi;
  const bool failed = a.status[b] != 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const int i0 = ti * NQ_ORB_TILE + wave * 16, j0 = tj * NQ_ORB_TILE;
  if (i0 >= m) return;                                         // uniform over the wavefront; no barrier follows
  const int nsub = ti == tj ? wave + 1 : 4;                    // a diagonal tile: the sub-tiles on and below the diagonal
  const double* C = a.coeff + base;
  const double* W0 = w0 + o0;
  const double* W1 = TWO ? w1 + o0 : nullptr;
  const int ic = i0 + lc;

  auto fetch = [&](int k0, WgOperands& x) {
    const int k = k0 + lk;
    const bool kin = k < hi;
    const double* row = C + (long long)k * m;
    const bool ain = kin && ic < m;
    const double ca = ain ? row[ic] : 0.0;
    x.a0 = ain ? W0[k] * ca : 0.0;
    x.a1 = TWO && ain ? W1[k] * ca : 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int jc = j0 + s * 16 + lc;
      x.b[s] = (s < nsub && kin && jc < m) ? row[jc] : 0.0;
    }
  };

  orb_f64x4 acc0[4], acc1[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    acc0[s] = orb_f64x4{0.0, 0.0, 0.0, 0.0};
    acc1[s] = orb_f64x4{0.0, 0.0, 0.0, 0.0};
  }
  if (!failed && lo < hi) {
    WgOperands cur;
    fetch(lo, cur);
    for (int k0 = lo; k0 < hi; k0 += 4) {
      WgOperands nxt = cur;
      if (k0 + 4 < hi) fetch(k0 + 4, nxt);
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (s < nsub && j0 + s * 16 < m) {                     // uniform over the wavefront
          acc0[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.a0, cur.b[s], acc0[s], 0, 0, 0);
          if (TWO) acc1[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.a1, cur.b[s], acc1[s], 0, 0, 0);
        }
      cur = nxt;
    }
  }
  const double nan = nq_nan_f64();
  double* X0 = out0 + base;
  double* X1 = TWO ? out1 + base : nullptr;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= nsub) continue;
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + lk + 4 * r;                           // the f64 C/D map: row = (lane >> 4) + 4 r, column = lane & 15
      if (i < m && j <= i) {                                   // j <= i < m
        const double v0 = failed ? nan : acc0[s][r];
        X0[(long long)i * m + j] = v0;
        if (j != i) X0[(long long)j * m + i] = v0;
        if (TWO) {
          const double v1 = failed ? nan : acc1[s][r];
          X1[(long long)i * m + j] = v1;
          if (j != i) X1[(long long)j * m + i] = v1;
        }
      }
    }
  }
}

__global__ __launch_bounds__(NQ_ORB_NT) void k_orb_population(OrbArgs a, const double* D, const void* H, int h_f64, const void* S, int s_f64, int N,
                                                              const int* mol_ptr, const long long* atom_orb_ptr, double* atom_pop, double* nelec,
                                                              double* eband) {
  __shared__ double pop[NQ_ORB_MAX_M];
  __shared__ double erow[NQ_ORB_MAX_M];
  __shared__ double red[NQ_ORB_NW];
  if (!orb_dims_ok(a)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int o0 = a.orb_ptr[b], m = a.orb_ptr[b + 1] - o0;
  const long long base = a.pack_ptr[b];
  const int a0 = mol_ptr[b], a1 = mol_ptr[b + 1];
  const bool atoms_ok = a0 >= 0 && a1 >= a0 && a1 <= N;
  const double nan = nq_nan_f64();
  if (m < 1 || m > NQ_ORB_MAX_M || base < 0 || base + (long long)m * m > a.P) {   // uniform: a state overwritten since nq_orb_init
    if (tid == 0) {
      nelec[b] = nan;
      if (eband) eband[b] = nan;
    }
    if (atoms_ok)
      for (int at = a0 + tid; at < a1; at += NQ_ORB_NT) atom_pop[at] = nan;
    return;
  }
  for (int i = wave; i < m; i += NQ_ORB_NW) {
    double p = 0.0, e = 0.0;
    for (int j = lane; j < m; j += 64) {
      const long long low = base + (j <= i ? (long long)i * m + j : (long long)j * m + i);   // the lower-triangle copy of element (i, j)
      const double d = D[base + (long long)i * m + j];
      if (S) p = fma(d, nq_load_f64(S, low, s_f64), p);
      else if (j == i) p = d;
      if (H) e = fma(d, nq_load_f64(H, low, h_f64), e);
    }
    p = nq_wave_sum_f64(p);
    e = nq_wave_sum_f64(e);
    if (lane == 0) { pop[i] = p; erow[i] = e; }
  }
  __syncthreads();
  double sp = 0.0, se = 0.0;
  for (int i = tid; i < m; i += NQ_ORB_NT) { sp += pop[i]; se += erow[i]; }
  sp = orb_block_sum(sp, red);
  se = orb_block_sum(se, red);
  if (tid == 0) {
    nelec[b] = sp;
    if (eband) eband[b] = se;
  }
  if (atoms_ok)
    for (int at = a0 + tid; at < a1; at += NQ_ORB_NT) {         // one thread per atom: its contiguous orbital range, in order
      const long long r0 = atom_orb_ptr[at] - o0, r1 = atom_orb_ptr[at + 1] - o0;
      double s = nan;
      if (r0 >= 0 && r1 >= r0 && r1 <= m) {
        s = 0.0;
        for (long long k = r0; k < r1; ++k) s += pop[k];
      }
      atom_pop[at] = s;
    }
}

extern "C" {

int nq_orb_wgram(void* state, int32_t B, int32_t M, int64_t P, const double* w0, const double* w1, const int32_t* k_lo, const int32_t* k_hi, double* out0,
                 double* out1, void* stream) {
  if (!state || !w0 || !out0) return nq_fail(NQ_ERR_ARG, "null argument");
  if (w1 && !out1) return nq_fail(NQ_ERR_ARG, "nq_orb_wgram: a second weight vector needs a second output");
  NQ_TRY(orb_check_dims(B, M, P));
  const int nt = orb_tile_count(orb_largest_m_bound(B, M, P));
  if ((long long)B * nt > INT_MAX) return nq_fail(NQ_ERR_ARG, "nq_orb_wgram: B=%d molecules of up to %d tiles exceed the grid", B, nt);
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, w1 ? "orb_wgram_two" : "orb_wgram_one");
  const OrbArgs a = orb_args(state, B, M, P);
  if (w1) hipLaunchKernelGGL(k_orb_wgram<true>, dim3(B * nt), dim3(NQ_WG_NT), 0, st, a, nt, w0, w1, k_lo, k_hi, out0, out1);
  else hipLaunchKernelGGL(k_orb_wgram<false>, dim3(B * nt), dim3(NQ_WG_NT), 0, st, a, nt, w0, (const double*)nullptr, k_lo, k_hi, out0, (double*)nullptr);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_population(void* state, int32_t B, int32_t M, int64_t P, const double* D, const void* H, int32_t h_f64, const void* S, int32_t s_f64, int32_t N,
                      const int32_t* mol_ptr, const int64_t* atom_orb_ptr, double* out_atom_pop, double* out_nelec, double* out_eband, void* stream) {
  if (!state || !D || !mol_ptr || !atom_orb_ptr || !out_atom_pop || !out_nelec) return nq_fail(NQ_ERR_ARG, "null argument");
  if (out_eband && !H) return nq_fail(NQ_ERR_ARG, "nq_orb_population: the band energy needs H");
  NQ_TRY(orb_check_dims(B, M, P));
  if (N < B) return nq_fail(NQ_ERR_ARG, "nq_orb_population: N=%d atoms for B=%d molecules", N, B);
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_population");
  hipLaunchKernelGGL(k_orb_population, dim3(B), dim3(NQ_ORB_NT), 0, st, orb_args(state, B, M, P), D, H, h_f64, S, s_f64, N, mol_ptr,
                     (const long long*)atom_orb_ptr, out_atom_pop, out_nelec, out_eband);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
