// Batched normal modes (the job of ase.vibrations.Vibrations behind nablaDFT/optimization/pyg_ase_interface.py:317-334), whole state on the device.
//
// Finite-difference Hessians: the displacement list of a batch is molecule-major over (molecule, free degree of freedom); displacement j owns two images of
// its molecule, "-" then "+".  k_vib_displace writes the float32 positions of the images of a chunk [c0, c1) into the model's input tensor and records the step
// each pair REALISED, h = (double) x32+ - (double) x32- (the models read float32 positions, so float32(x0 +- delta) is not x0 +- delta); k_vib_accumulate
// turns the model's forces of that chunk into rows (F- - F+)[free] / h of each molecule's packed (3 n_free)^2 matrix G; k_vib_finish writes the symmetrised
// Hessian H = (G + G^T) / 2, the asymmetry max |G - G^T| and, over G, the mass-weighted A = m^-1/2 H m^-1/2.
//
// Eigensolver (k_vib_jacobi): one 256-thread workgroup per molecule runs the parallel cyclic two-sided Jacobi method.  Ordering: a round-robin tournament
// over m padded to even, m/2 disjoint pairs per round; a round is three phases separated by barriers: rotation parameters from (a_pp, a_qq, a_pq), all row
// updates, all column updates together with the eigenvector columns.  A lives in LDS when it fits (m <= 141: leading dimension m | 1, so that a column does
// not sit on one bank), else in place in global memory -- the same code, templated on where A lives; the eigenvectors always live in the output buffer.
// A sweep starts with off(A)^2 = sum_{i != j} a_ij^2 summed directly (never as |A|^2 - sum a_ii^2, which cancels) and stops at off <= m 2^-52 |A|_F; at most 30
// sweeps.  The loop bounds and every barrier are uniform: the exit flag is a sum every thread reads from LDS, so a matrix that does not converge (NaN
// included) ends with status 1 and never hangs.
//
// Every kernel is float64, has no atomic and a fixed summation order that depends on the molecule alone: results are bitwise reproducible and independent of
// what else shares the batch.  Compiled with -ffp-contract=off, so that displace / accumulate round like the restatement (tests/vib_ref.py).
//
// State buffer (nq_vib_state_layout): header int32[16] {N, B, D, P low, P high, status (-2: a call came with other dimensions than nq_vib_init, -3: the image
// tensor of a chunk has another size than the plan), n_lds}, mol_ptr[B+1], dof_ptr[B+1], hess_ptr[B+1], order[B] (LDS molecules first), free_atom[D/3],
// disp_mol[D], disp_off[D+1], im[D], r[N][3], h[D], asymmetry[B], sweeps[B], status[B], omega2[D], work[P], hessian[P], modes[P].
#include <vector>

#include "../../include/nablaq.h"
#include "devstate.h"

#define NQ_VIB_MAX_DOF 576
#define NQ_VIB_LDS_BYTES 163840
#define NQ_VIB_MAX_SWEEPS 30
#define NQ_VIB_HDR 16

enum { VH_N = 0, VH_B, VH_D, VH_PLO, VH_PHI, VH_STATUS, VH_NLDS };

enum { VP_HDR = 0, VP_MOL_PTR, VP_DOF_PTR, VP_HESS_PTR, VP_ORDER, VP_FREE_ATOM, VP_DISP_MOL, VP_DISP_OFF, VP_IM, VP_R, VP_H, VP_ASYM, VP_SWEEPS, VP_STATUS,
       VP_OMEGA2, VP_WORK, VP_HESS, VP_MODES, VP_PARTS };
typedef NqStateLayout<VP_PARTS> VibLayout;

static VibLayout vib_layout(long N, long B, long D, long long P) {
  const size_t bytes[VP_PARTS] = {NQ_VIB_HDR * 4, (size_t)(B + 1) * 4, (size_t)(B + 1) * 4, (size_t)(B + 1) * 8, (size_t)B * 4, (size_t)(D / 3) * 4,
                                  (size_t)D * 4, (size_t)(D + 1) * 8, (size_t)D * 8, (size_t)N * 24, (size_t)D * 8, (size_t)B * 8, (size_t)B * 4,
                                  (size_t)B * 4, (size_t)D * 8, (size_t)P * 8, (size_t)P * 8, (size_t)P * 8};
  return nq_state_layout(bytes);
}

// dynamic LDS of k_vib_jacobi: [A: m x (m | 1)] d[m] cs[2 np] red[8] pq[2 np] perm[m], np = pairs per round
__host__ __device__ static inline size_t vib_param_bytes(int m) {
  const int np = (m + (m & 1)) >> 1;
  return (size_t)m * 8 + (size_t)np * 16 + 64 + (size_t)np * 8 + (size_t)m * 4;
}
__host__ __device__ static inline size_t vib_lds_bytes(int m) { return (size_t)m * (m | 1) * 8 + vib_param_bytes(m); }

struct VibArgs {
  int* hdr; const int* mol_ptr; const int* dof_ptr; const long long* hess_ptr; const int* order; const int* free_atom; const int* disp_mol;
  const long long* disp_off; const double* im; const double* r; double* h; double* asym; int* sweeps; int* status; double* omega2; double* work;
  double* hess; double* modes;
  int N, B, D; long long P;
};

__device__ __forceinline__ bool vib_dims_ok(const VibArgs& a) {
  const bool ok = a.hdr[VH_N] == a.N && a.hdr[VH_B] == a.B && a.hdr[VH_D] == a.D && nq_split64_is(a.hdr + VH_PLO, a.P);
  if (!ok && blockIdx.x == 0 && threadIdx.x == 0) a.hdr[VH_STATUS] = -2;   // not the state nq_vib_init prepared: touch nothing else
  return ok;
}

// one 64-thread workgroup per displacement of the chunk
__global__ __launch_bounds__(64) void k_vib_displace(VibArgs a, int c0, int c1, double delta, float* img, long long img_atoms) {
  if (!vib_dims_ok(a)) return;
  if (a.disp_off[c1] - a.disp_off[c0] != img_atoms) {
    if (blockIdx.x == 0 && threadIdx.x == 0) a.hdr[VH_STATUS] = -3;
    return;
  }
  const int j = c0 + blockIdx.x;
  const int b = a.disp_mol[j];
  const int k = j - a.dof_ptr[b];
  const int start = a.mol_ptr[b], n3 = (a.mol_ptr[b + 1] - start) * 3;
  const int coord = (a.free_atom[a.dof_ptr[b] / 3 + k / 3] - start) * 3 + k % 3;
  float* out = img + (a.disp_off[j] - a.disp_off[c0]) * 3;
  for (int t = threadIdx.x; t < n3; t += 64) {
    const double x = a.r[(long)start * 3 + t];
    float xm = (float)x, xp = xm;
    if (t == coord) {
      xm = (float)(x - delta);
      xp = (float)(x + delta);
      a.h[j] = (double)xp - (double)xm;
    }
    out[t] = xm;
    out[n3 + t] = xp;
  }
}

__global__ __launch_bounds__(64) void k_vib_accumulate(VibArgs a, int c0, int c1, const void* forces, int forces_f64, long long img_atoms) {
  if (!vib_dims_ok(a)) return;
  if (a.disp_off[c1] - a.disp_off[c0] != img_atoms) {
    if (blockIdx.x == 0 && threadIdx.x == 0) a.hdr[VH_STATUS] = -3;
    return;
  }
  const int j = c0 + blockIdx.x;
  const int b = a.disp_mol[j];
  const int d0 = a.dof_ptr[b], m = a.dof_ptr[b + 1] - d0;
  const int start = a.mol_ptr[b], n = a.mol_ptr[b + 1] - start;
  const long long base = a.disp_off[j] - a.disp_off[c0];
  const double h = a.h[j];
  double* row = a.work + a.hess_ptr[b] + (long long)(j - d0) * m;
  for (int c = threadIdx.x; c < m; c += 64) {
    const int la = a.free_atom[d0 / 3 + c / 3] - start;
    const long long im = (base + la) * 3 + c % 3, ip = im + (long long)n * 3;
    const double fm = nq_load_f64(forces, im, forces_f64), fp = nq_load_f64(forces, ip, forces_f64);
    row[c] = (fm - fp) / h;
  }
}

// the four wavefronts' partial results meet in red[4] and are combined 0,1,2,3; every thread returns what it read from LDS (uniform)
template <bool MAX>
__device__ __forceinline__ double vib_block_reduce(double v, double* red) {
  v = MAX ? nq_wave_max_f64(v) : nq_wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = MAX ? fmax(fmax(red[0], red[1]), fmax(red[2], red[3])) : ((red[0] + red[1]) + (red[2] + red[3]));
  __syncthreads();
  return r;
}

// one workgroup per molecule; thread handles the pairs (i <= j) it owns, so G -> A in place is race free
__global__ __launch_bounds__(256) void k_vib_finish(VibArgs a) {
  __shared__ double red[4];
  if (!vib_dims_ok(a)) return;
  const int b = blockIdx.x;
  const int d0 = a.dof_ptr[b], m = a.dof_ptr[b + 1] - d0;
  double* G = a.work + a.hess_ptr[b];
  double* H = a.hess + a.hess_ptr[b];
  double asym = 0.0;
  for (int idx = threadIdx.x; idx < m * m; idx += 256) {
    const int i = idx / m, j = idx - i * m;
    if (i > j) continue;
    const double gij = G[idx], gji = G[(long)j * m + i];
    const double hij = 0.5 * (gij + gji);
    asym = fmax(asym, fabs(gij - gji));
    H[idx] = hij;
    H[(long)j * m + i] = hij;
    const double aij = (a.im[d0 + i] * hij) * a.im[d0 + j];
    G[idx] = aij;
    G[(long)j * m + i] = aij;
  }
  asym = vib_block_reduce<true>(asym, red);
  if (threadIdx.x == 0) a.asym[b] = asym;
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_vib_jacobi(VibArgs a, int first, int scale, unsigned lds_bytes) {
  extern __shared__ double sm[];
  if (!vib_dims_ok(a)) return;
  const int tid = threadIdx.x;
  const int b = a.order[first + blockIdx.x];
  const int d0 = a.dof_ptr[b], m = a.dof_ptr[b + 1] - d0;
  if (m == 0) {   // every atom fixed: uniform over the workgroup
    if (tid == 0) { a.sweeps[b] = 0; a.status[b] = 0; }
    return;
  }
  if ((LDS ? vib_lds_bytes(m) : vib_param_bytes(m)) > lds_bytes) {   // not the launch geometry nq_vib_init planned: touch nothing (uniform)
    if (tid == 0) a.status[b] = 2;
    return;
  }
  const int mp = m + (m & 1), np = mp >> 1;
  const int ld = LDS ? (m | 1) : m;
  double* Ag = a.work + a.hess_ptr[b];
  double* A = LDS ? sm : Ag;
  double* dg = LDS ? sm + (size_t)m * ld : sm;
  double* cs = dg + m;
  double* red = cs + 2 * np;
  int* pq = (int*)(red + 8);
  int* perm = pq + 2 * np;
  double* V = a.modes + a.hess_ptr[b];   // V[k * m + i] = component i of eigenvector k
  const int mm = m * m;
  constexpr int U = LDS ? 4 : 8;      // independent items in flight per thread: LDS latency, global-memory latency

  double fro = 0.0;
  for (int idx = tid; idx < mm; idx += 256) {
    const int i = idx / m, j = idx - i * m;
    const double v = Ag[idx];
    if (LDS) A[i * ld + j] = v;
    V[idx] = i == j ? 1.0 : 0.0;
    fro += v * v;
  }
  fro = vib_block_reduce<false>(fro, red);   // its barriers also publish A and V
  const double eps_m = (double)m * NQ_F64_EPS;
  const double thr2 = (eps_m * eps_m) * fro;   // off^2 <= (m 2^-52)^2 |A|_F^2

  int sweeps = 0, status = 1;
  for (int sweep = 0; sweep <= NQ_VIB_MAX_SWEEPS; ++sweep) {
    double off = 0.0;
    for (int idx = tid; idx < mm; idx += 256) {
      const int i = idx / m, j = idx - i * m;
      const double v = A[i * ld + j];
      if (i != j) off += v * v;
    }
    off = vib_block_reduce<false>(off, red);
    if (off <= thr2) { status = 0; break; }      // uniform: `off` was read from LDS by every thread
    if (sweep == NQ_VIB_MAX_SWEEPS) break;
    for (int r = 0; r < mp - 1; ++r) {
      // phase 1: the round's pairs and their rotations
      for (int t = tid; t < np; t += 256) {      // np > 256 above m = 512
        int p, q;
        if (t == 0) { p = mp - 1; q = r; }
        else { p = (r + t) % (mp - 1); q = (r - t + (mp - 1)) % (mp - 1); }
        if (p > q) { const int sw = p; p = q; q = sw; }
        double c = 1.0, s = 0.0;
        if (q < m) {      // q == m: the padding index of an odd m sits this round out
          const double app = A[p * ld + p], aqq = A[q * ld + q], apq = A[p * ld + q];
          if (apq != 0.0) {
            const double tau = (aqq - app) / (2.0 * apq);
            const double tn = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + tn * tn);
            s = tn * c;
          }
        } else {
          q = p;
        }
        pq[2 * t] = p; pq[2 * t + 1] = q;
        cs[2 * t] = c; cs[2 * t + 1] = s;
      }
      __syncthreads();
      // phase 2: rows p and q of every pair.  U independent items per thread and pass: all their loads are issued before the first store, so a pass costs
      // one memory latency instead of U (the items of a round touch disjoint entries)
      for (int base = tid; base < np * m; base += 256 * U) {
        double x[U], y[U], c[U], s[U];
        int ip[U], iq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int it = base + u * 256;
          const bool live = it < np * m;
          const int k = live ? it / m : 0, j = live ? it - k * m : 0;
          s[u] = live ? cs[2 * k + 1] : 0.0;      // 0: identity, the padding pair, or past the end -- nothing to do
          c[u] = cs[2 * k];
          ip[u] = pq[2 * k] * ld + j;
          iq[u] = pq[2 * k + 1] * ld + j;
          if (s[u] != 0.0) { x[u] = A[ip[u]]; y[u] = A[iq[u]]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (s[u] != 0.0) {
            A[ip[u]] = c[u] * x[u] - s[u] * y[u];
            A[iq[u]] = s[u] * x[u] + c[u] * y[u];
          }
        }
      }
      __syncthreads();
      // phase 3: columns p and q of every pair -- items run pair-fastest: the tournament's pairs of a round have consecutive indices, so neighbouring
      // threads touch neighbouring entries of one row (coalesced in global memory, conflict-free in LDS) ...
      for (int base = tid; base < np * m; base += 256 * U) {
        double x[U], y[U], c[U], s[U];
        int ip[U], iq[U];
        bool zp[U], zq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int it = base + u * 256;
          const bool live = it < np * m;
          const int i = live ? it / np : 0, k = live ? it - i * np : 0;
          s[u] = live ? cs[2 * k + 1] : 0.0;
          c[u] = cs[2 * k];
          const int p = pq[2 * k], q = pq[2 * k + 1];
          ip[u] = i * ld + p; iq[u] = i * ld + q;
          zq[u] = i == p; zp[u] = i == q;            // a_pq and a_qp: annihilated by construction
          if (s[u] != 0.0) { x[u] = A[ip[u]]; y[u] = A[iq[u]]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (s[u] != 0.0) {
            const double xn = c[u] * x[u] - s[u] * y[u], yn = s[u] * x[u] + c[u] * y[u];
            A[ip[u]] = zp[u] ? 0.0 : xn;
            A[iq[u]] = zq[u] ? 0.0 : yn;
          }
        }
      }
      // ... and the same rotation of the eigenvectors, whose rows p and q are contiguous: items run component-fastest
      for (int base = tid; base < np * m; base += 256 * U) {
        double vx[U], vy[U], c[U], s[U];
        int jp[U], jq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int it = base + u * 256;
          const bool live = it < np * m;
          const int k = live ? it / m : 0, i = live ? it - k * m : 0;
          s[u] = live ? cs[2 * k + 1] : 0.0;
          c[u] = cs[2 * k];
          jp[u] = pq[2 * k] * m + i; jq[u] = pq[2 * k + 1] * m + i;      // m <= 576: fits an int
          if (s[u] != 0.0) { vx[u] = V[jp[u]]; vy[u] = V[jq[u]]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (s[u] != 0.0) {
            V[jp[u]] = c[u] * vx[u] - s[u] * vy[u];
            V[jq[u]] = s[u] * vx[u] + c[u] * vy[u];
          }
        }
      }
      __syncthreads();
    }
    ++sweeps;
  }

  // ascending order by rank (ties by index)
  for (int i = tid; i < m; i += 256) { dg[i] = A[i * ld + i]; perm[i] = i; }
  __syncthreads();
  nq_rank_perm<256, 3>(dg, m, perm);      // m <= 576 < 3 * 256
  for (int k = tid; k < m; k += 256) a.omega2[d0 + k] = dg[perm[k]];
  // sorted (and mass-scaled) rows: through the matrix's global storage, which nothing needs any more
  for (int idx = tid; idx < mm; idx += 256) {
    const int k = idx / m, i = idx - k * m;
    const double v = V[(long)perm[k] * m + i];
    Ag[idx] = scale ? v * a.im[d0 + i] : v;
  }
  __syncthreads();
  for (int idx = tid; idx < mm; idx += 256) V[idx] = Ag[idx];
  if (tid == 0) { a.sweeps[b] = sweeps; a.status[b] = status; }
}

static int vib_check_dims(int32_t N, int32_t B, int32_t D, int64_t P) {
  if (N < 1 || B < 1) return nq_fail(NQ_ERR_ARG, "nq_vib: empty batch (N=%d, B=%d)", N, B);
  if (D < 0 || D % 3 != 0 || D > 3 * (long)N) return nq_fail(NQ_ERR_ARG, "nq_vib: D=%d is not three times a number of free atoms of N=%d", D, N);
  if (P < 0 || P > (int64_t)D * NQ_VIB_MAX_DOF) return nq_fail(NQ_ERR_ARG, "nq_vib: P=%lld does not fit D=%d", (long long)P, D);
  return NQ_OK;
}

static VibArgs vib_args(void* state, int32_t N, int32_t B, int32_t D, int64_t P) {
  const VibLayout L = vib_layout(N, B, D, P);
  char* s = (char*)state;
  VibArgs a;
  a.hdr = (int*)(s + L.part[VP_HDR]); a.mol_ptr = (const int*)(s + L.part[VP_MOL_PTR]); a.dof_ptr = (const int*)(s + L.part[VP_DOF_PTR]);
  a.hess_ptr = (const long long*)(s + L.part[VP_HESS_PTR]); a.order = (const int*)(s + L.part[VP_ORDER]); a.free_atom = (const int*)(s + L.part[VP_FREE_ATOM]);
  a.disp_mol = (const int*)(s + L.part[VP_DISP_MOL]); a.disp_off = (const long long*)(s + L.part[VP_DISP_OFF]); a.im = (const double*)(s + L.part[VP_IM]);
  a.r = (const double*)(s + L.part[VP_R]); a.h = (double*)(s + L.part[VP_H]); a.asym = (double*)(s + L.part[VP_ASYM]); a.sweeps = (int*)(s + L.part[VP_SWEEPS]);
  a.status = (int*)(s + L.part[VP_STATUS]); a.omega2 = (double*)(s + L.part[VP_OMEGA2]); a.work = (double*)(s + L.part[VP_WORK]);
  a.hess = (double*)(s + L.part[VP_HESS]); a.modes = (double*)(s + L.part[VP_MODES]);
  a.N = N; a.B = B; a.D = D; a.P = P;
  return a;
}

extern "C" {

size_t nq_vib_state_bytes(int32_t N, int32_t B, int32_t D, int64_t P) {
  return vib_check_dims(N, B, D, P) == NQ_OK ? vib_layout(N, B, D, P).total : 0;
}

int nq_vib_state_layout(int32_t N, int32_t B, int32_t D, int64_t P, size_t* offsets_host) {
  if (!offsets_host) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(vib_check_dims(N, B, D, P));
  return nq_state_offsets(vib_layout(N, B, D, P), offsets_host);
}

int nq_vib_init(void* state, size_t state_bytes, const int32_t* mol_ptr_host, const double* masses_host, const uint8_t* fixed_host, int32_t N, int32_t B,
                int32_t D, int64_t P, const void* pos, int32_t pos_f64, int32_t* plan_host, void* stream) {
  if (!state || !mol_ptr_host || !masses_host || !pos || !plan_host) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(vib_check_dims(N, B, D, P));
  const VibLayout L = vib_layout(N, B, D, P);
  NQ_TRY(nq_state_check("nq_vib_init:", state, state_bytes, L.total));
  if (mol_ptr_host[0] != 0 || mol_ptr_host[B] != N) return nq_fail(NQ_ERR_ARG, "nq_vib_init: mol_ptr must run from 0 to N=%d", N);
  // the host-built parts are contiguous from the header up to im: one host image, one copy
  std::vector<char> img(L.part[VP_R], 0);
  int* hdr = (int*)(img.data() + L.part[VP_HDR]);
  int* mol_ptr = (int*)(img.data() + L.part[VP_MOL_PTR]);
  int* dof_ptr = (int*)(img.data() + L.part[VP_DOF_PTR]);
  long long* hess_ptr = (long long*)(img.data() + L.part[VP_HESS_PTR]);
  int* order = (int*)(img.data() + L.part[VP_ORDER]);
  int* free_atom = (int*)(img.data() + L.part[VP_FREE_ATOM]);
  int* disp_mol = (int*)(img.data() + L.part[VP_DISP_MOL]);
  long long* disp_off = (long long*)(img.data() + L.part[VP_DISP_OFF]);
  double* im = (double*)(img.data() + L.part[VP_IM]);
  std::vector<int> in_lds, in_global;
  long dof = 0;
  long long hp = 0, ioff = 0;
  int max_m = 0, max_m_lds = 0;
  for (int b = 0; b < B; ++b) {
    const int start = mol_ptr_host[b], n = mol_ptr_host[b + 1] - start;
    if (n < 1) return nq_fail(NQ_ERR_ARG, "nq_vib_init: molecule %d has %d atoms", b, n);
    mol_ptr[b] = start;
    dof_ptr[b] = (int)dof;
    hess_ptr[b] = hp;
    int m = 0;
    for (int i = start; i < start + n; ++i) {
      if (fixed_host && fixed_host[i]) continue;
      if (!(masses_host[i] > 0.0)) return nq_fail(NQ_ERR_ARG, "nq_vib_init: atom %d has mass %g", i, masses_host[i]);
      if (dof + m + 3 > D) return nq_fail(NQ_ERR_ARG, "nq_vib_init: more than D=%d free degrees of freedom", D);
      free_atom[(dof + m) / 3] = i;
      for (int d = 0; d < 3; ++d) im[dof + m + d] = 1.0 / sqrt(masses_host[i]);
      m += 3;
    }
    if (m > NQ_VIB_MAX_DOF)
      return nq_fail(NQ_ERR_MOL_TOO_LARGE, "nq_vib_init: molecule %d has %d free degrees of freedom, the limit is %d", b, m, NQ_VIB_MAX_DOF);
    for (int k = 0; k < m; ++k) {
      disp_mol[dof + k] = b;
      disp_off[dof + k] = ioff;
      ioff += 2LL * n;
    }
    dof += m;
    hp += (long long)m * m;
    if (hp > P) return nq_fail(NQ_ERR_ARG, "nq_vib_init: the packed matrices need more than P=%lld entries", (long long)P);
    const bool lds = vib_lds_bytes(m) <= NQ_VIB_LDS_BYTES;
    (lds ? in_lds : in_global).push_back(b);
    if (m > max_m) max_m = m;
    if (lds && m > max_m_lds) max_m_lds = m;
  }
  if (dof != D || hp != P) return nq_fail(NQ_ERR_ARG, "nq_vib_init: the batch has D=%ld, P=%lld, the call said D=%d, P=%lld", dof, hp, D, (long long)P);
  mol_ptr[B] = N; dof_ptr[B] = D; hess_ptr[B] = P; disp_off[D] = ioff;
  for (size_t i = 0; i < in_lds.size(); ++i) order[i] = in_lds[i];
  for (size_t i = 0; i < in_global.size(); ++i) order[in_lds.size() + i] = in_global[i];
  hdr[VH_N] = N; hdr[VH_B] = B; hdr[VH_D] = D; nq_split64(P, hdr + VH_PLO); hdr[VH_NLDS] = (int)in_lds.size();
  plan_host[0] = (int32_t)in_lds.size(); plan_host[1] = max_m_lds; plan_host[2] = max_m;
  hipStream_t st = (hipStream_t)stream;
  NQ_TRY(nq_state_upload(state, img.data(), L.part[VP_R], st));
  char* base = (char*)state;
  NQ_HIP(hipMemsetAsync(base + L.part[VP_H], 0, L.part[VP_WORK] - L.part[VP_H], st));   // h, asymmetry, sweeps, status, omega2
  NQ_PROF(st, "vib_init");
  return nq_init_pos_f64(st, pos, pos_f64, nullptr, (long)N * 3, (double*)(base + L.part[VP_R]), nullptr, nullptr);
}

static int vib_check_chunk(const char* who, int32_t D, int32_t c0, int32_t c1, int64_t img_atoms) {
  if (c0 < 0 || c1 <= c0 || c1 > D) return nq_fail(NQ_ERR_ARG, "%s: chunk [%d, %d) outside the %d displacements", who, c0, c1, D);
  if (img_atoms < 2LL * (c1 - c0)) return nq_fail(NQ_ERR_ARG, "%s: %lld image atoms cannot hold %d image pairs", who, (long long)img_atoms, c1 - c0);
  return NQ_OK;
}

int nq_vib_displace(void* state, int32_t N, int32_t B, int32_t D, int64_t P, int32_t c0, int32_t c1, double delta, float* image_pos, int64_t image_atoms,
                    void* stream) {
  if (!state || !image_pos) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(vib_check_dims(N, B, D, P));
  NQ_TRY(vib_check_chunk("nq_vib_displace", D, c0, c1, image_atoms));
  if (!(delta > 0.0)) return nq_fail(NQ_ERR_ARG, "nq_vib_displace: delta=%g must be positive", delta);
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "vib_displace");
  hipLaunchKernelGGL(k_vib_displace, dim3(c1 - c0), dim3(64), 0, st, vib_args(state, N, B, D, P), c0, c1, delta, image_pos, (long long)image_atoms);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_vib_accumulate(void* state, int32_t N, int32_t B, int32_t D, int64_t P, int32_t c0, int32_t c1, const void* forces, int32_t forces_f64,
                      int64_t image_atoms, void* stream) {
  if (!state || !forces) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(vib_check_dims(N, B, D, P));
  NQ_TRY(vib_check_chunk("nq_vib_accumulate", D, c0, c1, image_atoms));
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "vib_accumulate");
  hipLaunchKernelGGL(k_vib_accumulate, dim3(c1 - c0), dim3(64), 0, st, vib_args(state, N, B, D, P), c0, c1, forces, forces_f64, (long long)image_atoms);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_vib_finish(void* state, int32_t N, int32_t B, int32_t D, int64_t P, void* stream) {
  if (!state) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(vib_check_dims(N, B, D, P));
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "vib_finish");
  hipLaunchKernelGGL(k_vib_finish, dim3(B), dim3(256), 0, st, vib_args(state, N, B, D, P));
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_vib_eigh(void* state, int32_t N, int32_t B, int32_t D, int64_t P, int32_t n_lds, int32_t max_m_lds, int32_t max_m, int32_t scale_modes, void* stream) {
  if (!state) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(vib_check_dims(N, B, D, P));
  if (n_lds < 0 || n_lds > B) return nq_fail(NQ_ERR_ARG, "nq_vib_eigh: n_lds=%d outside [0,%d]", n_lds, B);
  if (max_m < 0 || max_m > NQ_VIB_MAX_DOF || max_m_lds < 0 || max_m_lds > max_m || vib_lds_bytes(max_m_lds) > NQ_VIB_LDS_BYTES)
    return nq_fail(NQ_ERR_ARG, "nq_vib_eigh: max_m_lds=%d / max_m=%d are not what nq_vib_init returned", max_m_lds, max_m);
  hipStream_t st = (hipStream_t)stream;
  const VibArgs a = vib_args(state, N, B, D, P);
  if (n_lds > 0) {
    const size_t lds = vib_lds_bytes(max_m_lds);
    NQ_DYN_LDS(k_vib_jacobi<true>, lds);
    NQ_PROF(st, "vib_jacobi_lds");
    hipLaunchKernelGGL(k_vib_jacobi<true>, dim3(n_lds), dim3(256), lds, st, a, 0, scale_modes, (unsigned)lds);
    NQ_LAUNCH_CHECK();
  }
  if (B - n_lds > 0) {
    NQ_PROF(st, "vib_jacobi_global");
    hipLaunchKernelGGL(k_vib_jacobi<false>, dim3(B - n_lds), dim3(256), vib_param_bytes(max_m), st, a, n_lds, scale_modes, (unsigned)vib_param_bytes(max_m));
    NQ_LAUNCH_CHECK();
  }
  return NQ_OK;
}

}  // extern "C"
