// Batched molecular dynamics (NVE velocity Verlet, Langevin NVT) for the MD job of nablaDFT/optimization/pyg_ase_interface.py:207-294 (init_md / run_md /
// _init_velocities: ase VelocityVerlet, Langevin with fix_com, MaxwellBoltzmannDistribution + Stationary + ZeroRotation, FixAtoms), whole state on the device.
// ase is not part of the reference tree: the equations are restated (nabladft_amd/md.py lists them) and unpinned against ase.
//
// One launch per MD step (k_md_step).  Ownership is that of lbfgs.hip: a molecule belongs to one wavefront (<= NQ_MOL_SMALL atoms, four molecules per 256-thread
// workgroup) or to one workgroup (up to NQ_MOL_MAX atoms); a lane owns whole atoms (3 / 2 per lane), so positions, velocities, masses and the noise of an atom never
// cross lanes.  The per-molecule sums (centre of the noise, momentum, angular momentum, kinetic energy) go through a 64-lane xor butterfly plus, on the workgroup
// path, four partial sums through LDS added in a fixed order: the reduction tree of a molecule depends on its own atom count alone, there is no floating-point
// atomic, and the results are bitwise reproducible and independent of what else shares the batch.
//
// A launch receives the forces of the CURRENT positions and does, in order: (a) the second half-kick of the pending step (Langevin: that step's rnd_vel is
// generated again from its counter, nothing was stored), (b) observables / frame of the now consistent (x, v, F), (c) noise, first half-kick and drift of the
// next step, float32 positions for the model.  So a step costs one launch although velocity Verlet kicks twice around a force evaluation.
//
// Random numbers: Philox4x32-10, key = seed, counter = (mol_key low, mol_key high, step, atom_in_molecule << 8 | group << 2 | component); one call gives the two
// Box-Muller normals (float64) of one component: group 0 -> (xi_c, eta_c) of the Langevin step, group 1 -> (zeta_c, spare) of the velocity initialisation.  The
// counter holds the caller's key of the molecule, not its place in the batch.
//
// State buffer (nq_md_state_layout): header int32[32], mol_ptr[B+1], order[B] (small molecules first), mol_key int64[B], mass f64[N], fixed uint8[N],
// r f64[N][3], v f64[N][3], rv f64[N][3] (rnd_vel of a pending step whose noise was injected), log f64[log_cap][B][8], frames f64[frame_cap][N][3],
// velocity frames f64[frame_cap][N][3].
#include <math.h>

#include <vector>

#include "../../include/nablaq.h"
#include "devstate.h"

#define NQ_MD_HDR 32
#define NQ_MD_LOGCOLS 8
#define NQ_MD_RED 9          // widest per-molecule sum (angular momentum + inertia tensor)
#define NQ_MD_FLAG_LOG 1
#define NQ_MD_FLAG_FRAMES 2
#define NQ_MD_FLAG_VEL 4

// CODATA 2014 (the set ase 3.22.1's default `units` uses).  KAPPA: (Hartree / Angstrom) / amu -> Angstrom / fs^2; KB: Hartree / K.  nabladft_amd/md.py computes the
// same two numbers with the same operation order; tests/test_md_cpu.py compares them through nq_md_constants.
static constexpr double MD_EH = 4.359744650e-18, MD_AMU = 1.660539040e-27, MD_KSI = 1.38064852e-23;
static constexpr double MD_KAPPA = MD_EH * (1e-15 * 1e-15) / (MD_AMU * (1e-10 * 1e-10));
static constexpr double MD_KB = MD_KSI / MD_EH;

enum { M_STEP = 0, M_STATUS, M_PENDING, M_LOGROWS, M_FRAMES, M_OVERFLOW, M_N, M_B, M_NSMALL, M_LOGCAP, M_FRAMECAP, M_FLAGS, M_LASTLOG, M_TICKET };

enum { MP_HDR = 0, MP_MOL_PTR, MP_ORDER, MP_KEY, MP_MASS, MP_FIXED, MP_R, MP_V, MP_RV, MP_LOG, MP_FRAMES, MP_VFRAMES, MP_PARTS };
typedef NqStateLayout<MP_PARTS> MdLayout;

static MdLayout md_layout(long N, long B, long log_cap, long frame_cap, int flags) {
  if (!(flags & NQ_MD_FLAG_LOG)) log_cap = 0;      // a ring whose flag is off takes no room
  if (!(flags & NQ_MD_FLAG_FRAMES)) frame_cap = 0;
  const size_t row = (size_t)N * 24, ring = (size_t)frame_cap * N * 24;
  const size_t bytes[MP_PARTS] = {NQ_MD_HDR * 4, (size_t)(B + 1) * 4, (size_t)B * 4, (size_t)B * 8, (size_t)N * 8, (size_t)N, row, row, row,
                                  (size_t)log_cap * B * NQ_MD_LOGCOLS * 8, ring, (flags & NQ_MD_FLAG_VEL) ? ring : 0};
  return nq_state_layout(bytes);
}

struct MdArgs {
  int* hdr; const int* mol_ptr; const int* order; const long long* key; const double* mass; const unsigned char* fixed;
  double* r; double* v; double* rv; double* log; double* frames; double* vframes;
  const void* forces; int forces_f64; const void* energies; int energies_f64; float* pos32;
  const double* xi; const double* eta;
  double dt, kT, fr;
  unsigned long long seed;
  int N, B, n_small, log_cap, frame_cap, flags, mode, interval, finish_only;
  int remove_translation, remove_rotation;      // nq_md_init_velocities
};

// ---- Philox4x32-10 + Box-Muller ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void md_philox(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
  }
}

// the two normals of (molecule key, step, atom inside the molecule, group, component); uniforms: 52 bits + 1/2, so u is never 0 or 1
__device__ __forceinline__ void md_normal_pair(unsigned long long seed, long long key, int step, int atom, int group, int comp, double& z0, double& z1) {
  uint32_t c[4] = {(uint32_t)(unsigned long long)key, (uint32_t)((unsigned long long)key >> 32), (uint32_t)step,
                   ((uint32_t)atom << 8) | ((uint32_t)group << 2) | (uint32_t)comp};
  md_philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u1 = ((double)(((unsigned long long)c[0] << 20) | (unsigned long long)(c[1] >> 12)) + 0.5) * 0x1p-52;
  const double u2 = ((double)(((unsigned long long)c[2] << 20) | (unsigned long long)(c[3] >> 12)) + 0.5) * 0x1p-52;
  const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
  z0 = rad * cos(ang);
  z1 = rad * sin(ang);
}

// ---- per-molecule sums ------------------------------------------------------------------------------------------------------------------
// every sum of this file shares red[2][NQ_MD_RED][4]
template <bool BLOCK, int K>
__device__ __forceinline__ void md_mol_sum(double (&v)[K], double* red, int& parity) {
  nq_mol_reduce<BLOCK, false, K, NQ_MD_RED>(v, red, parity);
}

// what a lane holds of its molecule
template <int APL>
struct MdAtoms {
  int start, n;
  long long key;
  bool act[APL], fix[APL];
  int idx[APL];          // global atom index (0 where inactive)
  int loc[APL];          // index inside the molecule
  double m[APL];         // 1 where inactive
};

template <int APL, int T>
__device__ __forceinline__ void md_load_atoms(const MdArgs& A, int b, int t, MdAtoms<APL>& M) {
  M.start = A.mol_ptr[b];
  M.n = A.mol_ptr[b + 1] - M.start;
  M.key = A.key[b];
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    const int a = t + k * T;
    M.act[k] = a < M.n;
    M.loc[k] = a;
    M.idx[k] = M.start + (M.act[k] ? a : 0);
    M.m[k] = M.act[k] ? A.mass[M.idx[k]] : 1.0;
    M.fix[k] = M.act[k] && A.fixed[M.idx[k]] != 0;
  }
}

template <int APL>
__device__ __forceinline__ void md_load3(const double* base, const MdAtoms<APL>& M, double (&v)[APL][3]) {
#pragma unroll
  for (int k = 0; k < APL; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[k][c] = M.act[k] ? base[(size_t)M.idx[k] * 3 + c] : 0.0;
  }
}

template <int APL>
__device__ __forceinline__ void md_store3(double* base, const MdAtoms<APL>& M, const double (&v)[APL][3]) {
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    if (M.act[k]) {
#pragma unroll
      for (int c = 0; c < 3; ++c) base[(size_t)M.idx[k] * 3 + c] = v[k][c];
    }
  }
}

// Langevin noise of one step (ase Langevin.step with fix_com): rnd_pos = c5 eta, rnd_vel = c3 xi - c4 eta, then per molecule rnd_pos -= mean(rnd_pos) and
// rnd_vel -= sum(m rnd_vel) / (m n), every atom of the molecule counted.  xi / eta: the injected arrays, or the generator at (key, step).
template <int APL, bool BLOCK>
__device__ __forceinline__ void md_noise(const MdArgs& A, const MdAtoms<APL>& M, int step, bool injected, double (&rp)[APL][3], double (&rv)[APL][3], double* red,
                                         int& parity) {
  const double sdt = sqrt(A.dt), dt15 = A.dt * sdt;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    const double sigma = sqrt(2.0 * MD_KAPPA * A.kT * A.fr / M.m[k]);
    const double c3 = sdt * sigma / 2.0 - dt15 * A.fr * sigma / 8.0;
    const double c5 = dt15 * sigma / (2.0 * sqrt(3.0));
    const double c4 = A.fr / 2.0 * c5;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double xi = 0.0, eta = 0.0;
      if (M.act[k]) {
        if (injected) {
          xi = A.xi[(size_t)M.idx[k] * 3 + c];
          eta = A.eta[(size_t)M.idx[k] * 3 + c];
        } else {
          md_normal_pair(A.seed, M.key, step, M.loc[k], 0, c, xi, eta);
        }
      }
      rp[k][c] = c5 * eta;
      rv[k][c] = c3 * xi - c4 * eta;
      s[c] += rp[k][c];
      s[3 + c] += M.m[k] * rv[k][c];
    }
  }
  md_mol_sum<BLOCK, 6>(s, red, parity);
  const double nn = (double)M.n;
#pragma unroll
  for (int k = 0; k < APL; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      rp[k][c] = M.act[k] ? rp[k][c] - s[c] / nn : 0.0;
      rv[k][c] = M.act[k] ? rv[k][c] - s[3 + c] / (M.m[k] * nn) : 0.0;
    }
  }
}

// One molecule, one MD step.  T threads (64 or 256) own it, thread t holds atoms t, t + T, ...
template <int APL, bool BLOCK>
__device__ __forceinline__ void md_molecule(const MdArgs& A, int b, int t, double* red, int step, int pending, int sample, int log_slot, int frame_slot) {
  constexpr int T = BLOCK ? 256 : 64;
  MdAtoms<APL> M;
  md_load_atoms<APL, T>(A, b, t, M);
  int parity = 0;
  double x[APL][3], v[APL][3], acc[APL][3];
  md_load3<APL>(A.r, M, x);
  md_load3<APL>(A.v, M, v);
#pragma unroll
  for (int k = 0; k < APL; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double f = 0.0;
      // not nq_load_f64: with one index shared by both arms the compiler addresses the forces with two instructions instead of one, and the step kernel
      // measured 1 % slower; written out, its code is instruction for instruction what it was
      if (M.act[k]) f = A.forces_f64 ? ((const double*)A.forces)[(size_t)M.idx[k] * 3 + c] : (double)((const float*)A.forces)[(size_t)M.idx[k] * 3 + c];
      acc[k][c] = MD_KAPPA * f / M.m[k];
    }
  }
  const double hdt = 0.5 * A.dt;
  const double c1 = A.dt / 2.0 - A.dt * A.dt * A.fr / 8.0;
  const double c2 = A.dt * A.fr / 2.0 - A.dt * A.dt * A.fr * A.fr / 8.0;
  // (a) second half-kick of the pending step
  if (pending) {
    if (A.mode == 0) {
#pragma unroll
      for (int k = 0; k < APL; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[k][c] = M.fix[k] ? 0.0 : v[k][c] + hdt * acc[k][c];
      }
    } else {
      double rp[APL][3], rv[APL][3];
      if (pending == 2) md_load3<APL>(A.rv, M, rv);                                  // injected noise: stored by the first half
      else md_noise<APL, BLOCK>(A, M, step - 1, false, rp, rv, red, parity);
#pragma unroll
      for (int k = 0; k < APL; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[k][c] = M.fix[k] ? 0.0 : v[k][c] + ((c1 * acc[k][c] - c2 * v[k][c]) + rv[k][c]);
      }
    }
  }
  // (b) x, v and F belong to one time: observables and frame
  if (sample) {
    if ((A.flags & NQ_MD_FLAG_LOG) && log_slot < A.log_cap) {
      double s1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < APL; ++k) {
        if (M.act[k]) {
          s1[0] += M.m[k];
#pragma unroll
          for (int c = 0; c < 3; ++c) s1[1 + c] += M.m[k] * x[k][c];
          s1[4] += M.fix[k] ? 0.0 : 1.0;
        }
      }
      md_mol_sum<BLOCK, 5>(s1, red, parity);
      const double xc[3] = {s1[1] / s1[0], s1[2] / s1[0], s1[3] / s1[0]};
      double s2[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < APL; ++k) {
        if (M.act[k]) {
          const double d[3] = {x[k][0] - xc[0], x[k][1] - xc[1], x[k][2] - xc[2]};
          const double p[3] = {M.m[k] * v[k][0], M.m[k] * v[k][1], M.m[k] * v[k][2]};
          s2[0] += p[0]; s2[1] += p[1]; s2[2] += p[2];
          s2[3] += M.m[k] * (v[k][0] * v[k][0] + v[k][1] * v[k][1] + v[k][2] * v[k][2]);
          s2[4] += d[1] * p[2] - d[2] * p[1];
          s2[5] += d[2] * p[0] - d[0] * p[2];
          s2[6] += d[0] * p[1] - d[1] * p[0];
        }
      }
      md_mol_sum<BLOCK, 7>(s2, red, parity);
      if (t == 0) {
        const double ekin = 0.5 * s2[3] / MD_KAPPA;
        const double dof = 3.0 * s1[4];
        double epot = 0.0;
        if (A.energies) epot = nq_load_f64(A.energies, b, A.energies_f64);
        double* row = A.log + ((size_t)log_slot * A.B + b) * NQ_MD_LOGCOLS;
        row[0] = (double)step;
        row[1] = epot + ekin;
        row[2] = epot;
        row[3] = ekin;
        row[4] = dof > 0.0 ? 2.0 * ekin / (dof * MD_KB) : 0.0;
        row[5] = sqrt(s2[0] * s2[0] + s2[1] * s2[1] + s2[2] * s2[2]);
        row[6] = sqrt(s2[4] * s2[4] + s2[5] * s2[5] + s2[6] * s2[6]);
        row[7] = 0.0;
      }
    }
    if ((A.flags & NQ_MD_FLAG_FRAMES) && frame_slot < A.frame_cap) {
      md_store3<APL>(A.frames + (size_t)frame_slot * A.N * 3, M, x);
      if (A.flags & NQ_MD_FLAG_VEL) md_store3<APL>(A.vframes + (size_t)frame_slot * A.N * 3, M, v);
    }
  }
  if (A.finish_only) {
    if (pending) md_store3<APL>(A.v, M, v);
    return;
  }
  // (c) first half-kick and drift of the next step
  if (A.mode == 0) {
#pragma unroll
    for (int k = 0; k < APL; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (M.fix[k]) {
          v[k][c] = 0.0;
        } else {
          v[k][c] = v[k][c] + hdt * acc[k][c];
          x[k][c] = x[k][c] + A.dt * v[k][c];
        }
      }
    }
  } else {
    double rp[APL][3], rv[APL][3];
    const bool injected = A.xi != nullptr;
    md_noise<APL, BLOCK>(A, M, step, injected, rp, rv, red, parity);
    if (injected) md_store3<APL>(A.rv, M, rv);
#pragma unroll
    for (int k = 0; k < APL; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (M.fix[k]) {
          v[k][c] = 0.0;
        } else {
          const double vh = v[k][c] + ((c1 * acc[k][c] - c2 * v[k][c]) + rv[k][c]);
          const double xn = (x[k][c] + A.dt * vh) + rp[k][c];
          v[k][c] = ((xn - x[k][c]) - rp[k][c]) / A.dt;
          x[k][c] = xn;
        }
      }
    }
  }
  md_store3<APL>(A.v, M, v);
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    if (M.act[k] && !M.fix[k]) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        A.r[(size_t)M.idx[k] * 3 + c] = x[k][c];
        A.pos32[(size_t)M.idx[k] * 3 + c] = (float)x[k][c];
      }
    }
  }
}

__device__ __forceinline__ bool md_header_matches(const MdArgs& A) {
  return A.hdr[M_N] == A.N && A.hdr[M_B] == A.B && A.hdr[M_NSMALL] == A.n_small && A.hdr[M_LOGCAP] == A.log_cap && A.hdr[M_FRAMECAP] == A.frame_cap &&
         A.hdr[M_FLAGS] == A.flags;
}

// grid: ceil(n_small / 4) workgroups of four wavefront-owned molecules, then one workgroup per larger molecule.  Every workgroup reads the header words first;
// the last one to finish (ticket) advances them.
__global__ __launch_bounds__(256) void k_md_step(MdArgs A) {
  __shared__ double red[2 * NQ_MD_RED * 4];
  const int wave = threadIdx.x >> 6;
  const int small_blocks = nq_small_blocks(A.n_small);
  if (!md_header_matches(A)) {   // not the state nq_md_init prepared: touch nothing
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicExch(&A.hdr[M_STATUS], -2);
    return;
  }
  const int step = A.hdr[M_STEP], pending = A.hdr[M_PENDING], log_slot = A.hdr[M_LOGROWS], frame_slot = A.hdr[M_FRAMES];
  const int sample = (step % A.interval == 0) && A.hdr[M_LASTLOG] != step;
  if ((int)blockIdx.x < small_blocks) {
    const int i = blockIdx.x * 4 + wave;
    if (i < A.n_small) md_molecule<3, false>(A, A.order[i], threadIdx.x & 63, red, step, pending, sample, log_slot, frame_slot);
  } else {
    md_molecule<2, true>(A, A.order[A.n_small + (blockIdx.x - small_blocks)], threadIdx.x, red, step, pending, sample, log_slot, frame_slot);
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const int ticket = atomicAdd(&A.hdr[M_TICKET], 1);
    if (ticket == (int)gridDim.x - 1) {
      __threadfence();
      if (sample) {
        if (A.flags & NQ_MD_FLAG_LOG) {
          if (log_slot < A.log_cap) atomicExch(&A.hdr[M_LOGROWS], log_slot + 1);
          else atomicExch(&A.hdr[M_OVERFLOW], 1);
        }
        if (A.flags & NQ_MD_FLAG_FRAMES) {
          if (frame_slot < A.frame_cap) atomicExch(&A.hdr[M_FRAMES], frame_slot + 1);
          else atomicExch(&A.hdr[M_OVERFLOW], 1);
        }
        atomicExch(&A.hdr[M_LASTLOG], step);
      }
      if (A.finish_only) {
        atomicExch(&A.hdr[M_PENDING], 0);
      } else {
        atomicExch(&A.hdr[M_STEP], step + 1);
        atomicExch(&A.hdr[M_PENDING], (A.mode != 0 && A.xi != nullptr) ? 2 : 1);
      }
      atomicExch(&A.hdr[M_TICKET], 0);
    }
  }
}

// ---- velocity initialisation --------------------------------------------------------------------------------------------------------------
// eigenvalues w and eigenvectors (columns of V) of a symmetric 3x3 matrix: cyclic Jacobi, every lane on the same bits
__device__ __forceinline__ void md_sym3_eig(double (&S)[3][3], double (&V)[3][3], double (&w)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 12; ++sweep) {
    if (fabs(S[0][1]) + fabs(S[0][2]) + fabs(S[1][2]) == 0.0) break;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int p = i == 2 ? 1 : 0, q = i == 0 ? 1 : 2;
      const double g = 100.0 * fabs(S[p][q]);
      if (fabs(S[p][p]) + g == fabs(S[p][p]) && fabs(S[q][q]) + g == fabs(S[q][q])) {
        S[p][q] = S[q][p] = 0.0;
      } else if (S[p][q] != 0.0) {
        const double theta = (S[q][q] - S[p][p]) / (2.0 * S[p][q]);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double a = S[k][p], bq = S[k][q];
          S[k][p] = cs * a - sn * bq;
          S[k][q] = sn * a + cs * bq;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double a = S[p][k], bq = S[q][k];
          S[p][k] = cs * a - sn * bq;
          S[q][k] = sn * a + cs * bq;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double a = V[k][p], bq = V[k][q];
          V[k][p] = cs * a - sn * bq;
          V[k][q] = sn * a + cs * bq;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = S[i][i];
}

// _init_velocities (pyg_ase_interface.py:265-282): MaxwellBoltzmannDistribution, Stationary, ZeroRotation; fixed atoms end with v = 0 after every stage
template <int APL, bool BLOCK>
__device__ __forceinline__ void md_init_vel_molecule(const MdArgs& A, int b, int t, double* red) {
  constexpr int T = BLOCK ? 256 : 64;
  MdAtoms<APL> M;
  md_load_atoms<APL, T>(A, b, t, M);
  int parity = 0;
  double x[APL][3], v[APL][3];
  md_load3<APL>(A.r, M, x);
#pragma unroll
  for (int k = 0; k < APL; ++k) {
    const double sd = sqrt(MD_KAPPA * A.kT / M.m[k]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double z0 = 0.0, z1 = 0.0;
      if (M.act[k] && !M.fix[k]) md_normal_pair(A.seed, M.key, 0, M.loc[k], 1, c, z0, z1);
      v[k][c] = z0 * sd;
    }
  }
  if (A.remove_translation) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < APL; ++k) {
      if (M.act[k]) {
        s[0] += M.m[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[1 + c] += M.m[k] * v[k][c];
      }
    }
    md_mol_sum<BLOCK, 4>(s, red, parity);
#pragma unroll
    for (int k = 0; k < APL; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[k][c] = (M.act[k] && !M.fix[k]) ? v[k][c] - s[1 + c] / s[0] : 0.0;
    }
  }
  if (A.remove_rotation) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < APL; ++k) {
      if (M.act[k]) {
        s[0] += M.m[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[1 + c] += M.m[k] * x[k][c];
      }
    }
    md_mol_sum<BLOCK, 4>(s, red, parity);
    const double xc[3] = {s[1] / s[0], s[2] / s[0], s[3] / s[0]};
    double q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // L (3), Ixx Iyy Izz Ixy Ixz Iyz
    double d[APL][3];
#pragma unroll
    for (int k = 0; k < APL; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) d[k][c] = M.act[k] ? x[k][c] - xc[c] : 0.0;
      if (M.act[k]) {
        const double m = M.m[k];
        q[0] += m * (d[k][1] * v[k][2] - d[k][2] * v[k][1]);
        q[1] += m * (d[k][2] * v[k][0] - d[k][0] * v[k][2]);
        q[2] += m * (d[k][0] * v[k][1] - d[k][1] * v[k][0]);
        q[3] += m * (d[k][1] * d[k][1] + d[k][2] * d[k][2]);
        q[4] += m * (d[k][0] * d[k][0] + d[k][2] * d[k][2]);
        q[5] += m * (d[k][0] * d[k][0] + d[k][1] * d[k][1]);
        q[6] -= m * d[k][0] * d[k][1];
        q[7] -= m * d[k][0] * d[k][2];
        q[8] -= m * d[k][1] * d[k][2];
      }
    }
    md_mol_sum<BLOCK, 9>(q, red, parity);
    double S[3][3] = {{q[3], q[6], q[7]}, {q[6], q[4], q[8]}, {q[7], q[8], q[5]}}, V[3][3], w[3];
    const double floor_ = 1e-10 * (q[3] + q[4] + q[5]);
    md_sym3_eig(S, V, w);
    double om[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      if (w[e] > floor_) {      // atoms, diatomics, linear molecules: no rotation about an axis without inertia
        const double lp = (V[0][e] * q[0] + V[1][e] * q[1] + V[2][e] * q[2]) / w[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) om[c] += lp * V[c][e];
      }
    }
#pragma unroll
    for (int k = 0; k < APL; ++k) {
      if (M.act[k] && !M.fix[k]) {
        v[k][0] -= om[1] * d[k][2] - om[2] * d[k][1];
        v[k][1] -= om[2] * d[k][0] - om[0] * d[k][2];
        v[k][2] -= om[0] * d[k][1] - om[1] * d[k][0];
      }
    }
  }
  md_store3<APL>(A.v, M, v);
}

__global__ __launch_bounds__(256) void k_md_init_vel(MdArgs A) {
  __shared__ double red[2 * NQ_MD_RED * 4];
  const int wave = threadIdx.x >> 6;
  const int small_blocks = nq_small_blocks(A.n_small);
  if (!md_header_matches(A)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicExch(&A.hdr[M_STATUS], -2);
    return;
  }
  if ((int)blockIdx.x < small_blocks) {
    const int i = blockIdx.x * 4 + wave;
    if (i < A.n_small) md_init_vel_molecule<3, false>(A, A.order[i], threadIdx.x & 63, red);
  } else {
    md_init_vel_molecule<2, true>(A, A.order[A.n_small + (blockIdx.x - small_blocks)], threadIdx.x, red);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicExch(&A.hdr[M_PENDING], 0);   // new velocities belong to the current positions: no half-kick is owed
}

// one thread per atom: the molecule is found by bisection of mol_ptr
__global__ void k_md_normals(unsigned long long seed, int step, int draw, const int* mol_ptr, const long long* key, int N, int B, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int lo = 0, hi = B;          // mol_ptr[lo] <= i < mol_ptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (mol_ptr[mid] <= i) lo = mid; else hi = mid;
  }
  const long long k = key ? key[lo] : (long long)lo;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double z0, z1;
    md_normal_pair(seed, k, step, i - mol_ptr[lo], draw >> 1, c, z0, z1);
    out[(size_t)i * 3 + c] = (draw & 1) ? z1 : z0;
  }
}

static int md_check_dims(int32_t N, int32_t B, int32_t log_cap, int32_t frame_cap, int32_t flags) {
  if (N < 1 || B < 1) return nq_fail(NQ_ERR_ARG, "nq_md: empty batch (N=%d, B=%d)", N, B);
  if (flags & ~7) return nq_fail(NQ_ERR_ARG, "nq_md: unknown flags %d", flags);
  if ((flags & NQ_MD_FLAG_LOG) && log_cap < 1) return nq_fail(NQ_ERR_ARG, "nq_md: the log ring is requested with capacity %d", log_cap);
  if ((flags & NQ_MD_FLAG_FRAMES) && frame_cap < 1) return nq_fail(NQ_ERR_ARG, "nq_md: the frame ring is requested with capacity %d", frame_cap);
  if ((flags & NQ_MD_FLAG_VEL) && !(flags & NQ_MD_FLAG_FRAMES)) return nq_fail(NQ_ERR_ARG, "nq_md: velocity frames need the frame ring");
  if (log_cap < 0 || frame_cap < 0) return nq_fail(NQ_ERR_ARG, "nq_md: negative ring capacity");
  return NQ_OK;
}

static MdArgs md_args(void* state, int32_t N, int32_t B, int32_t n_small, int32_t log_cap, int32_t frame_cap, int32_t flags) {
  const MdLayout L = md_layout(N, B, log_cap, frame_cap, flags);
  char* base = (char*)state;
  MdArgs A = {};
  A.hdr = (int*)(base + L.part[MP_HDR]); A.mol_ptr = (const int*)(base + L.part[MP_MOL_PTR]); A.order = (const int*)(base + L.part[MP_ORDER]);
  A.key = (const long long*)(base + L.part[MP_KEY]); A.mass = (const double*)(base + L.part[MP_MASS]); A.fixed = (const unsigned char*)(base + L.part[MP_FIXED]);
  A.r = (double*)(base + L.part[MP_R]); A.v = (double*)(base + L.part[MP_V]); A.rv = (double*)(base + L.part[MP_RV]); A.log = (double*)(base + L.part[MP_LOG]);
  A.frames = (double*)(base + L.part[MP_FRAMES]); A.vframes = (double*)(base + L.part[MP_VFRAMES]);
  A.N = N; A.B = B; A.n_small = n_small; A.flags = flags;
  A.log_cap = (flags & NQ_MD_FLAG_LOG) ? log_cap : 0;
  A.frame_cap = (flags & NQ_MD_FLAG_FRAMES) ? frame_cap : 0;
  A.interval = 1;
  return A;
}

extern "C" {

int nq_md_constants(double* kappa_kb_host) {
  if (!kappa_kb_host) return nq_fail(NQ_ERR_ARG, "null argument");
  kappa_kb_host[0] = MD_KAPPA;
  kappa_kb_host[1] = MD_KB;
  return NQ_OK;
}

size_t nq_md_state_bytes(int32_t N, int32_t B, int32_t log_cap, int32_t frame_cap, int32_t flags) {
  return md_check_dims(N, B, log_cap, frame_cap, flags) == NQ_OK ? md_layout(N, B, log_cap, frame_cap, flags).total : 0;
}

int nq_md_state_layout(int32_t N, int32_t B, int32_t log_cap, int32_t frame_cap, int32_t flags, size_t* offsets_host) {
  if (!offsets_host) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(md_check_dims(N, B, log_cap, frame_cap, flags));
  return nq_state_offsets(md_layout(N, B, log_cap, frame_cap, flags), offsets_host);
}

int nq_md_init(void* state, size_t state_bytes, const int32_t* mol_ptr_host, const int64_t* mol_key_host, const double* masses_host, const uint8_t* fixed_host,
               int32_t N, int32_t B, int32_t log_cap, int32_t frame_cap, int32_t flags, const void* pos, int32_t pos_f64, const double* vel, float* pos32,
               int32_t* n_small_host, void* stream) {
  if (!state || !mol_ptr_host || !masses_host || !pos || !pos32 || !n_small_host) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(md_check_dims(N, B, log_cap, frame_cap, flags));
  const MdLayout L = md_layout(N, B, log_cap, frame_cap, flags);
  NQ_TRY(nq_state_check("nq_md_init:", state, state_bytes, L.total));
  if (mol_ptr_host[0] != 0 || mol_ptr_host[B] != N) return nq_fail(NQ_ERR_ARG, "nq_md_init: mol_ptr must run from 0 to N=%d", N);
  // header .. fixed mask are contiguous: one host image, one copy
  std::vector<char> img(L.part[MP_R], 0);
  int n_small = 0;
  NQ_TRY(nq_partition_molecules(mol_ptr_host, B, NQ_MOL_SMALL, NQ_MOL_MAX, "nq_md_init:", (int*)(img.data() + L.part[MP_ORDER]), &n_small));
  for (int i = 0; i < N; ++i) {
    if (!(masses_host[i] > 0.0) || !std::isfinite(masses_host[i])) return nq_fail(NQ_ERR_ARG, "nq_md_init: atom %d has mass %g, masses must be positive", i, masses_host[i]);
  }
  int* hdr = (int*)(img.data() + L.part[MP_HDR]);
  hdr[M_N] = N; hdr[M_B] = B; hdr[M_NSMALL] = n_small; hdr[M_FLAGS] = flags; hdr[M_LASTLOG] = -1;
  hdr[M_LOGCAP] = (flags & NQ_MD_FLAG_LOG) ? log_cap : 0;
  hdr[M_FRAMECAP] = (flags & NQ_MD_FLAG_FRAMES) ? frame_cap : 0;
  int* mp = (int*)(img.data() + L.part[MP_MOL_PTR]);
  for (int b = 0; b <= B; ++b) mp[b] = mol_ptr_host[b];
  long long* key = (long long*)(img.data() + L.part[MP_KEY]);
  for (int b = 0; b < B; ++b) key[b] = mol_key_host ? (long long)mol_key_host[b] : (long long)b;
  double* mass = (double*)(img.data() + L.part[MP_MASS]);
  unsigned char* fixed = (unsigned char*)(img.data() + L.part[MP_FIXED]);
  for (int i = 0; i < N; ++i) {
    mass[i] = masses_host[i];
    fixed[i] = fixed_host && fixed_host[i] ? 1 : 0;
  }
  *n_small_host = n_small;
  hipStream_t st = (hipStream_t)stream;
  NQ_TRY(nq_state_upload(state, img.data(), L.part[MP_R], st));
  char* base = (char*)state;
  NQ_PROF(st, "md_init");
  return nq_init_pos_f64(st, pos, pos_f64, vel, (long)N * 3, (double*)(base + L.part[MP_R]), (double*)(base + L.part[MP_V]), pos32);
}

int nq_md_init_velocities(void* state, int32_t N, int32_t B, int32_t n_small, int32_t log_cap, int32_t frame_cap, int32_t flags, double T_init, int64_t seed,
                          int32_t remove_translation, int32_t remove_rotation, void* stream) {
  if (!state) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(md_check_dims(N, B, log_cap, frame_cap, flags));
  if (n_small < 0 || n_small > B) return nq_fail(NQ_ERR_ARG, "nq_md_init_velocities: n_small=%d outside [0,%d]", n_small, B);
  if (!(T_init >= 0.0) || !std::isfinite(T_init)) return nq_fail(NQ_ERR_ARG, "nq_md_init_velocities: T_init=%g must be non-negative", T_init);
  MdArgs A = md_args(state, N, B, n_small, log_cap, frame_cap, flags);
  A.kT = MD_KB * T_init; A.seed = (unsigned long long)seed; A.remove_translation = remove_translation; A.remove_rotation = remove_rotation;
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "md_init_velocities");
  hipLaunchKernelGGL(k_md_init_vel, dim3(nq_owned_grid(n_small, B)), dim3(256), 0, st, A);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_md_step(void* state, int32_t N, int32_t B, int32_t n_small, int32_t log_cap, int32_t frame_cap, int32_t flags, const void* forces, int32_t forces_f64,
               const void* energies, int32_t energies_f64, float* pos32, int32_t mode, double dt, double kT, double fr, int32_t interval, int64_t seed,
               const double* xi, const double* eta, int32_t finish_only, void* stream) {
  if (!state || !forces || !pos32) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(md_check_dims(N, B, log_cap, frame_cap, flags));
  if (n_small < 0 || n_small > B) return nq_fail(NQ_ERR_ARG, "nq_md_step: n_small=%d outside [0,%d]", n_small, B);
  if (mode != 0 && mode != 1) return nq_fail(NQ_ERR_ARG, "nq_md_step: mode=%d (0: NVE, 1: Langevin)", mode);
  if (!(dt > 0.0) || !std::isfinite(dt)) return nq_fail(NQ_ERR_ARG, "nq_md_step: dt=%g must be positive", dt);
  if (!(kT >= 0.0) || !(fr >= 0.0) || !std::isfinite(kT) || !std::isfinite(fr)) return nq_fail(NQ_ERR_ARG, "nq_md_step: kT=%g and fr=%g must be non-negative", kT, fr);
  if (interval < 1) return nq_fail(NQ_ERR_ARG, "nq_md_step: interval=%d must be at least 1", interval);
  if ((xi == nullptr) != (eta == nullptr)) return nq_fail(NQ_ERR_ARG, "nq_md_step: xi and eta are given together or not at all");
  MdArgs A = md_args(state, N, B, n_small, log_cap, frame_cap, flags);
  A.forces = forces; A.forces_f64 = forces_f64; A.energies = energies; A.energies_f64 = energies_f64; A.pos32 = pos32;
  A.xi = mode == 1 ? xi : nullptr; A.eta = mode == 1 ? eta : nullptr;
  A.dt = dt; A.kT = kT; A.fr = mode == 1 ? fr : 0.0; A.seed = (unsigned long long)seed;
  A.mode = mode; A.interval = interval; A.finish_only = finish_only;
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "md_step");
  hipLaunchKernelGGL(k_md_step, dim3(nq_owned_grid(n_small, B)), dim3(256), 0, st, A);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_md_normals(int64_t seed, int32_t step, int32_t draw, const int32_t* mol_ptr, const int64_t* mol_key, int32_t N, int32_t B, double* out, void* stream) {
  if (!mol_ptr || !out) return nq_fail(NQ_ERR_ARG, "null argument");
  if (N < 1 || B < 1) return nq_fail(NQ_ERR_ARG, "nq_md_normals: empty batch (N=%d, B=%d)", N, B);
  if (draw < 0 || draw > 3) return nq_fail(NQ_ERR_ARG, "nq_md_normals: draw=%d (0: xi, 1: eta, 2: zeta, 3: spare)", draw);
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "md_normals");
  hipLaunchKernelGGL(k_md_normals, dim3(nq_cdiv(N, 256)), dim3(256), 0, st, (unsigned long long)seed, step, draw, mol_ptr, (const long long*)mol_key, N, B, out);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
