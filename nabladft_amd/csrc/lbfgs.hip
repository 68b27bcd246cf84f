// Batched L-BFGS for the geometry-optimisation job (nablaDFT/optimization/optimizers.py:437-605, the branch without line search), whole state on the device.
//
// One launch per optimiser step (k_lbfgs_step).  A molecule is owned by one wavefront (<= NQ_MOL_SMALL atoms, four molecules per 256-thread workgroup) or
// by one workgroup (up to NQ_MOL_MAX atoms); a lane owns whole atoms (3 / 2 per lane), so the per-atom quantities -- force norms, step lengths, the
// fixed-atom mask -- never cross lanes and q / z of the two-loop recursion live in registers.  The only cross-lane traffic is the dot product of each history
// entry: a 64-lane xor butterfly (wavefront path: no LDS, no barrier) plus, for the workgroup path, four partial sums through LDS added in a fixed order.  The
// reduction tree of a molecule depends on its own atom count alone, never on the batch or on the launch geometry, and there is no floating-point atomic:
// results are bitwise reproducible and independent of what else shares the batch.  The next history row is loaded before the current one is reduced, so a
// chain link costs the reduction latency, not an HBM round trip.
//
// State buffer (nq_lbfgs_state_layout): header int32[16] {iteration, unconverged of the last step (-2: a step was called with other dimensions than nq_lbfgs_init), latch = first iteration at which no molecule was
// unconverged (-1: never), normalisations, N, B, memory, n_small, accumulator, ticket}, mol_ptr[B+1], order[B] (small molecules first), converged[B],
// rho[memory][B], r[N][3] (float64 master positions), r0, f0, S[memory][N][3], Y[memory][N][3].
#include <vector>

#include "../../include/nablaq.h"
#include "devstate.h"

#define NQ_LBFGS_MAX_MEMORY 1024
#define NQ_LBFGS_HDR 16

enum { H_ITER = 0, H_UNCONV, H_LATCH, H_NORM, H_N, H_B, H_MEM, H_NSMALL, H_ACC, H_TICKET };

enum { LP_HDR = 0, LP_MOL_PTR, LP_ORDER, LP_CONV, LP_RHO, LP_R, LP_R0, LP_F0, LP_S, LP_Y, LP_PARTS };
typedef NqStateLayout<LP_PARTS> LbfgsLayout;

static LbfgsLayout lbfgs_layout(long N, long B, long memory) {
  const size_t row = (size_t)N * 24, hist = (size_t)memory * N * 24;
  const size_t bytes[LP_PARTS] = {NQ_LBFGS_HDR * 4, (size_t)(B + 1) * 4, (size_t)B * 4, (size_t)B * 4, (size_t)memory * B * 8, row, row, row, hist, hist};
  return nq_state_layout(bytes);
}

struct LbfgsArgs {
  int* hdr; const int* mol_ptr; const int* order; int* conv;
  double* rho; double* r; double* r0; double* f0; double* S; double* Y;
  const void* forces; int forces_f64; const unsigned char* fixed;
  float* pos32;
  double fmax2, maxstep, damping, H0;
  int N, B, memory, n_small, evaluate_only;
};

template <int APL>
__device__ __forceinline__ void load_row(const double* base, const int (&off)[APL], const bool (&act)[APL], double (&v)[APL][3]) {
#pragma unroll
  for (int k = 0; k < APL; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[k][c] = act[k] ? base[off[k] + c] : 0.0;
  }
}

template <int APL>
__device__ __forceinline__ double dot_local(const double (&a)[APL][3], const double (&b)[APL][3]) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < APL; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc += a[k][c] * b[k][c];
  }
  return acc;
}

// One molecule.  T threads (64 or 256) own it, thread t holds atoms t, t + T, ...; `alds` is this wavefront's private copy of the a_i of the first loop (every
// lane writes the same value to the same address and later reads what it wrote itself), `red` the workgroup path's partial sums.
template <int APL, bool BLOCK>
__device__ __forceinline__ void lbfgs_molecule(const LbfgsArgs& A, int b, int t, double* alds, double* red) {
  constexpr int T = BLOCK ? 256 : 64;
  const int start = A.mol_ptr[b], n = A.mol_ptr[b + 1] - start;
  const int it = A.hdr[H_ITER];
  int parity = 0;
  int off[APL];
  bool act[APL];
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    const int a = t + k * T;
    act[k] = a < n;
    off[k] = (start + (act[k] ? a : 0)) * 3;
  }
  // forces (fixed atoms zeroed: calculator.py:85-86) and the convergence flag max_i |f_i|^2 < fmax^2 (optimizers.py:462-468)
  double f[APL][3];
  double fn2 = 0.0;
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    const bool live = act[k] && !(A.fixed && A.fixed[off[k] / 3]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double v = 0.0;
      if (live) v = nq_load_f64(A.forces, off[k] + c, A.forces_f64);
      f[k][c] = v;
    }
    fn2 = fmax(fn2, f[k][0] * f[k][0] + f[k][1] * f[k][1] + f[k][2] * f[k][2]);
  }
  fn2 = nq_mol_reduce<BLOCK, true>(fn2, red, parity);
  const bool conv = fn2 < A.fmax2;
  if (t == 0) {
    A.conv[b] = conv ? 1 : 0;
    if (!conv) atomicAdd(&A.hdr[H_ACC], 1);
  }
  if (A.evaluate_only) return;

  double r[APL][3], s[APL][3] = {}, y[APL][3] = {}, q[APL][3];
  load_row<APL>(A.r, off, act, r);
  const int mem = A.memory;
  const int L = it < mem ? it : mem;
  const size_t row = (size_t)A.N * 3;
  double rho_cur = 1.0, rho_new = 1.0;
  if (it > 0) {   // push s = r - r0, y = f0 - f into ring slot (it - 1) % memory (optimizers.py:584-605)
    double r0[APL][3], f0[APL][3];
    load_row<APL>(A.r0, off, act, r0);
    load_row<APL>(A.f0, off, act, f0);
#pragma unroll
    for (int k = 0; k < APL; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        s[k][c] = r[k][c] - r0[k][c];
        y[k][c] = f0[k][c] - f[k][c];
      }
    }
    const double ys = nq_mol_reduce<BLOCK, false>(dot_local<APL>(y, s), red, parity);
    rho_cur = rho_new = ys > 1e-8 ? 1.0 / ys : 1.0;
    const int slot = (it - 1) % mem;
    double* Sw = A.S + (size_t)slot * row;
    double* Yw = A.Y + (size_t)slot * row;
#pragma unroll
    for (int k = 0; k < APL; ++k) {
      if (act[k]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          Sw[off[k] + c] = s[k][c];
          Yw[off[k] + c] = y[k][c];
        }
      }
    }
    if (t == 0) A.rho[(size_t)slot * A.B + b] = rho_cur;
  }
  if (conv) {   // p = 0 (optimizers.py:520): nothing moves, r and pos32 stay; uniform over the owning wavefront / workgroup, so the chain is skipped whole
#pragma unroll
    for (int k = 0; k < APL; ++k) {
      if (act[k]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          A.r0[off[k] + c] = r[k][c];
          A.f0[off[k] + c] = f[k][c];
          A.pos32[off[k] + c] = (float)r[k][c];
        }
      }
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < APL; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) q[k][c] = -f[k][c];
  }
  // first loop, newest -> oldest: entry j = 0 is the pair just pushed (still in registers); row j + 1 is in flight while row j is reduced
  for (int j = 0; j < L; ++j) {
    double sn[APL][3], yn[APL][3];
    double rho_n = 1.0;
    const bool more = j + 1 < L;
    if (more) {
      const int slot = (it - 2 - j) % mem;
      load_row<APL>(A.S + (size_t)slot * row, off, act, sn);
      load_row<APL>(A.Y + (size_t)slot * row, off, act, yn);
      rho_n = A.rho[(size_t)slot * A.B + b];
    }
    const double a = rho_cur * nq_mol_reduce<BLOCK, false>(dot_local<APL>(s, q), red, parity);
    alds[j] = a;
#pragma unroll
    for (int k = 0; k < APL; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) q[k][c] -= a * y[k][c];
    }
    if (more) {
#pragma unroll
      for (int k = 0; k < APL; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          s[k][c] = sn[k][c];
          y[k][c] = yn[k][c];
        }
      }
      rho_cur = rho_n;
    }
  }
#pragma unroll
  for (int k = 0; k < APL; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) q[k][c] *= A.H0;   // z = H0 q
  }
  // second loop, oldest -> newest: starts on the row the first loop ended with
  for (int j = L - 1; j >= 0; --j) {
    double sn[APL][3], yn[APL][3];
    double rho_n = 1.0;
    const bool more = j > 0;
    if (more) {
      const int slot = (it - j) % mem;    // entry j - 1 is pair it - 1 - (j - 1)
      load_row<APL>(A.S + (size_t)slot * row, off, act, sn);
      load_row<APL>(A.Y + (size_t)slot * row, off, act, yn);
      rho_n = j == 1 ? rho_new : A.rho[(size_t)slot * A.B + b];   // the newest rho was stored by lane 0 of this launch: every lane kept its own copy
    }
    const double a = alds[j];
    const double bb = rho_cur * nq_mol_reduce<BLOCK, false>(dot_local<APL>(y, q), red, parity);
    const double w = a - bb;
#pragma unroll
    for (int k = 0; k < APL; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) q[k][c] += s[k][c] * w;
    }
    if (more) {
#pragma unroll
      for (int k = 0; k < APL; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          s[k][c] = sn[k][c];
          y[k][c] = yn[k][c];
        }
      }
      rho_cur = rho_n;
    }
  }
  // p = -z; determine_step (optimizers.py:556-577), damping, update
  double longest = 0.0;
#pragma unroll
  for (int k = 0; k < APL; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) q[k][c] = -q[k][c];
    longest = fmax(longest, sqrt(q[k][0] * q[k][0] + q[k][1] * q[k][1] + q[k][2] * q[k][2]));
  }
  longest = nq_mol_reduce<BLOCK, true>(longest, red, parity);
  const bool clamp = longest >= A.maxstep;
  const double scale = clamp ? A.maxstep / longest : 1.0;
  if (clamp && t == 0) atomicAdd(&A.hdr[H_NORM], 1);
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    if (act[k]) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double dr = q[k][c];
        if (clamp) dr *= scale;
        dr *= A.damping;
        const double rn = r[k][c] + dr;
        A.r[off[k] + c] = rn;
        A.pos32[off[k] + c] = (float)rn;
        A.r0[off[k] + c] = r[k][c];
        A.f0[off[k] + c] = f[k][c];
      }
    }
  }
}

// grid: ceil(n_small / 4) workgroups of four wavefront-owned molecules, then one workgroup per larger molecule.  The last workgroup to finish (ticket) folds
// the unconverged count into the header, latches the first all-converged iteration and advances the iteration counter.
__global__ __launch_bounds__(256) void k_lbfgs_step(LbfgsArgs A) {
  extern __shared__ double lds[];
  double* red = lds;                                      // [2][4]
  const int wave = threadIdx.x >> 6;
  double* alds = lds + 8 + (size_t)wave * A.memory;       // [4][memory]
  const int small_blocks = nq_small_blocks(A.n_small);
  if (A.hdr[H_N] != A.N || A.hdr[H_B] != A.B || A.hdr[H_MEM] != A.memory || A.hdr[H_NSMALL] != A.n_small) {   // not the state nq_lbfgs_init prepared: touch nothing
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicExch(&A.hdr[H_UNCONV], -2);
    return;
  }
  if ((int)blockIdx.x < small_blocks) {
    const int i = blockIdx.x * 4 + wave;
    if (i < A.n_small) lbfgs_molecule<3, false>(A, A.order[i], threadIdx.x & 63, alds, red);
  } else {
    lbfgs_molecule<2, true>(A, A.order[A.n_small + (blockIdx.x - small_blocks)], threadIdx.x, alds, red);
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const int ticket = atomicAdd(&A.hdr[H_TICKET], 1);
    if (ticket == (int)gridDim.x - 1) {
      __threadfence();
      const int it = A.hdr[H_ITER];
      const int cnt = atomicExch(&A.hdr[H_ACC], 0);
      atomicExch(&A.hdr[H_UNCONV], cnt);
      if (cnt == 0) atomicCAS(&A.hdr[H_LATCH], -1, it);
      if (!A.evaluate_only) atomicExch(&A.hdr[H_ITER], it + 1);
      atomicExch(&A.hdr[H_TICKET], 0);
    }
  }
}

static int lbfgs_check_dims(int32_t N, int32_t B, int32_t memory) {
  if (N < 1 || B < 1) return nq_fail(NQ_ERR_ARG, "nq_lbfgs: empty batch (N=%d, B=%d)", N, B);
  if (memory < 1 || memory > NQ_LBFGS_MAX_MEMORY) return nq_fail(NQ_ERR_ARG, "nq_lbfgs: memory=%d out of range [1,%d]", memory, NQ_LBFGS_MAX_MEMORY);
  return NQ_OK;
}

extern "C" {

size_t nq_lbfgs_state_bytes(int32_t N, int32_t B, int32_t memory) {
  return lbfgs_check_dims(N, B, memory) == NQ_OK ? lbfgs_layout(N, B, memory).total : 0;
}

int nq_lbfgs_state_layout(int32_t N, int32_t B, int32_t memory, size_t* offsets_host) {
  if (!offsets_host) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(lbfgs_check_dims(N, B, memory));
  return nq_state_offsets(lbfgs_layout(N, B, memory), offsets_host);
}

int nq_lbfgs_init(void* state, size_t state_bytes, const int32_t* mol_ptr_host, int32_t N, int32_t B, int32_t memory, const void* pos, int32_t pos_f64,
                  float* pos32, int32_t* n_small_host, void* stream) {
  if (!state || !mol_ptr_host || !pos || !pos32 || !n_small_host) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(lbfgs_check_dims(N, B, memory));
  const LbfgsLayout L = lbfgs_layout(N, B, memory);
  NQ_TRY(nq_state_check("nq_lbfgs_init:", state, state_bytes, L.total));
  if (mol_ptr_host[0] != 0 || mol_ptr_host[B] != N) return nq_fail(NQ_ERR_ARG, "nq_lbfgs_init: mol_ptr must run from 0 to N=%d", N);
  // header + mol_ptr + order are contiguous up to the converged flags: one host image, one copy
  std::vector<int> img(L.part[LP_CONV] / 4, 0);
  NQ_TRY(nq_partition_molecules(mol_ptr_host, B, NQ_MOL_SMALL, NQ_MOL_MAX, "nq_lbfgs_init:", img.data() + L.part[LP_ORDER] / 4, n_small_host));
  int* hdr = img.data() + L.part[LP_HDR] / 4;
  hdr[H_LATCH] = -1; hdr[H_N] = N; hdr[H_B] = B; hdr[H_MEM] = memory; hdr[H_NSMALL] = *n_small_host;
  for (int b = 0; b <= B; ++b) img[L.part[LP_MOL_PTR] / 4 + b] = mol_ptr_host[b];
  hipStream_t st = (hipStream_t)stream;
  NQ_TRY(nq_state_upload(state, img.data(), L.part[LP_CONV], st));
  char* base = (char*)state;
  NQ_HIP(hipMemsetAsync(base + L.part[LP_CONV], 0, (size_t)B * 4, st));
  NQ_PROF(st, "lbfgs_init");
  return nq_init_pos_f64(st, pos, pos_f64, nullptr, (long)N * 3, (double*)(base + L.part[LP_R]), nullptr, pos32);
}

int nq_lbfgs_step(void* state, int32_t N, int32_t B, int32_t memory, int32_t n_small, const void* forces, int32_t forces_f64, const uint8_t* fixed_mask,
                  float* pos32, double fmax, double maxstep, double damping, double alpha, int32_t evaluate_only, void* stream) {
  if (!state || !forces || !pos32) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(lbfgs_check_dims(N, B, memory));
  if (n_small < 0 || n_small > B) return nq_fail(NQ_ERR_ARG, "nq_lbfgs_step: n_small=%d outside [0,%d]", n_small, B);
  if (!(maxstep > 0.0)) return nq_fail(NQ_ERR_ARG, "nq_lbfgs_step: maxstep=%g must be positive", maxstep);
  if (!(alpha > 0.0) || !(fmax >= 0.0)) return nq_fail(NQ_ERR_ARG, "nq_lbfgs_step: alpha=%g must be positive and fmax=%g non-negative", alpha, fmax);
  const LbfgsLayout L = lbfgs_layout(N, B, memory);
  char* base = (char*)state;
  LbfgsArgs A;
  A.hdr = (int*)(base + L.part[LP_HDR]); A.mol_ptr = (const int*)(base + L.part[LP_MOL_PTR]); A.order = (const int*)(base + L.part[LP_ORDER]);
  A.conv = (int*)(base + L.part[LP_CONV]); A.rho = (double*)(base + L.part[LP_RHO]); A.r = (double*)(base + L.part[LP_R]); A.r0 = (double*)(base + L.part[LP_R0]);
  A.f0 = (double*)(base + L.part[LP_F0]); A.S = (double*)(base + L.part[LP_S]); A.Y = (double*)(base + L.part[LP_Y]);
  A.forces = forces; A.forces_f64 = forces_f64; A.fixed = fixed_mask; A.pos32 = pos32;
  A.fmax2 = fmax * fmax; A.maxstep = maxstep; A.damping = damping; A.H0 = 1.0 / alpha;
  A.N = N; A.B = B; A.memory = memory; A.n_small = n_small; A.evaluate_only = evaluate_only;
  const size_t lds = (8 + (size_t)4 * memory) * sizeof(double);
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "lbfgs_step");
  hipLaunchKernelGGL(k_lbfgs_step, dim3(nq_owned_grid(n_small, B)), dim3(256), lds, st, A);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
