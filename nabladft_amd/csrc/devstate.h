// What the device-resident batched jobs share (lbfgs.hip, md.hip, vib.hip, orbitals.hip): the layout of the caller-owned state buffer, the float64 reductions
// with their fixed summation orders, the float32-or-float64 input read, the rank permutation of the eigensolvers and the ownership of molecules by wavefronts
// and workgroups.  Header-only and __forceinline__: every file keeps its own -ffp-contract setting, so nothing here holds an a * b + c -- only additions,
// fmax, comparisons and shuffles.  A job keeps for itself its header words, its refusal of a call with other dimensions, its ticket epilogue and its kernels.
#pragma once
#include "common.h"

#define NQ_MOL_SMALL 192      // 64 lanes x 3 atoms: owned by one wavefront
#define NQ_MOL_MAX 512        // 256 threads x 2 atoms: owned by one workgroup (the project's molecule limit)
#define NQ_F64_EPS 0x1p-52

// ---- state buffer: consecutive parts, each aligned to 16 bytes; a job names its parts with an enum --------------------------------------------------------
template <int NPARTS>
struct NqStateLayout {
  size_t part[NPARTS], total;
};

template <int NPARTS>
static inline NqStateLayout<NPARTS> nq_state_layout(const size_t (&bytes)[NPARTS]) {
  NqStateLayout<NPARTS> L;
  size_t o = 0;
  for (int i = 0; i < NPARTS; ++i) {
    L.part[i] = o;
    o = (o + bytes[i] + 15) & ~(size_t)15;
  }
  L.total = o;
  return L;
}

template <int NPARTS>
static inline int nq_state_offsets(const NqStateLayout<NPARTS>& L, size_t* offsets_host) {
  for (int i = 0; i < NPARTS; ++i) offsets_host[i] = L.part[i];
  return NQ_OK;
}

// what every nq_*_init asks of the caller's buffer, then the upload of the host-built leading parts: one host image, one copy
static inline int nq_state_check(const char* who, const void* state, size_t state_bytes, size_t total) {
  if ((reinterpret_cast<uintptr_t>(state) & 15) != 0) return nq_fail(NQ_ERR_ARG, "%s state must be 16-byte aligned", who);
  if (state_bytes < total) return nq_fail(NQ_ERR_WORKSPACE, "%s state too small: %zu < %zu bytes", who, state_bytes, total);
  return NQ_OK;
}
static inline int nq_state_upload(void* state, const void* image, size_t bytes, hipStream_t st) {
  NQ_HIP(hipMemcpyAsync(state, image, bytes, hipMemcpyHostToDevice, st));
  NQ_HIP(hipStreamSynchronize(st));   // the image is a host temporary
  return NQ_OK;
}

// a 64-bit dimension in two int32 header words, low word first
__host__ __device__ static inline void nq_split64(long long v, int* lohi) { lohi[0] = (int)(v & 0xffffffffLL); lohi[1] = (int)(v >> 32); }
__device__ __forceinline__ bool nq_split64_is(const int* lohi, long long v) { return lohi[0] == (int)(v & 0xffffffffLL) && lohi[1] == (int)(v >> 32); }

// ---- molecule ownership (lbfgs.hip, md.hip): small molecules first, four of them per 256-thread workgroup, then one workgroup per larger molecule ----------
static inline int nq_partition_molecules(const int32_t* mol_ptr_host, int B, int small_cap, int max_cap, const char* who, int* order_out, int* n_small) {
  int ns = 0;
  for (int b = 0; b < B; ++b) {
    const int n = mol_ptr_host[b + 1] - mol_ptr_host[b];
    if (n < 1) return nq_fail(NQ_ERR_ARG, "%s molecule %d has %d atoms", who, b, n);
    if (n > max_cap) return nq_fail(NQ_ERR_MOL_TOO_LARGE, "%s molecule %d has %d atoms, the limit is %d", who, b, n, max_cap);
    if (n <= small_cap) order_out[ns++] = b;
  }
  *n_small = ns;
  for (int b = 0; b < B; ++b)
    if (mol_ptr_host[b + 1] - mol_ptr_host[b] > small_cap) order_out[ns++] = b;
  return NQ_OK;
}
__host__ __device__ static inline int nq_small_blocks(int n_small) { return (n_small + 3) >> 2; }
__host__ __device__ static inline int nq_owned_grid(int n_small, int B) { return nq_small_blocks(n_small) + (B - n_small); }

// ---- float64 reductions: the summation order is behaviour (results are compared bit for bit) ---------------------------------------------------------------
__device__ __forceinline__ double nq_wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);   // pairwise butterfly: every lane ends with the same bits
  return v;
}
__device__ __forceinline__ double nq_wave_max_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}

// K sums (or maxima) over the owners of a molecule.  BLOCK: four wavefronts own it; their partial results meet in red[2][KMAX][4] (alternating halves: one
// barrier per reduction) and are combined (0 + 1) + (2 + 3).  KMAX: the widest K of the reductions that share `red`.
template <bool BLOCK, bool MAX, int K, int KMAX = K>
__device__ __forceinline__ void nq_mol_reduce(double (&v)[K], double* red, int& parity) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = MAX ? nq_wave_max_f64(v[k]) : nq_wave_sum_f64(v[k]);
  if (BLOCK) {
    double* buf = red + parity * (KMAX * 4);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) buf[k * 4 + (threadIdx.x >> 6)] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double* b = buf + k * 4;
      v[k] = MAX ? fmax(fmax(b[0], b[1]), fmax(b[2], b[3])) : ((b[0] + b[1]) + (b[2] + b[3]));
    }
    parity ^= 1;
  }
}
template <bool BLOCK, bool MAX>
__device__ __forceinline__ double nq_mol_reduce(double v, double* red, int& parity) {
  double a[1] = {v};
  nq_mol_reduce<BLOCK, MAX, 1>(a, red, parity);
  return a[0];
}

// ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double nq_nan_f64() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double nq_load_f64(const void* p, long long i, int is_f64) { return is_f64 ? ((const double*)p)[i] : (double)((const float*)p)[i]; }

// float64 master positions from the caller's float32 / float64 ones; optionally the float32 copy the model reads and the velocities (null vel: zero).
// Templates, so that only the files that launch the kernel hold a copy of it.
template <int THREADS>
__global__ void k_nq_init_pos_f64(const void* pos, int pos_f64, const double* vel, long count, double* r, double* v, float* pos32) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const double x = nq_load_f64(pos, i, pos_f64);
  r[i] = x;
  if (pos32) pos32[i] = (float)x;
  if (v) v[i] = vel ? vel[i] : 0.0;
}
template <int THREADS = 256>
static inline int nq_init_pos_f64(hipStream_t st, const void* pos, int pos_f64, const double* vel, long count, double* r, double* v, float* pos32) {
  hipLaunchKernelGGL(k_nq_init_pos_f64<THREADS>, dim3(nq_cdiv(count, THREADS)), dim3(THREADS), 0, st, pos, pos_f64, vel, count, r, v, pos32);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

// ---- eigenvalue order --------------------------------------------------------------------------------------------------------------------------------------
// perm[k] = index of the k-th smallest of d[0..m) (ties by index), NT threads, m <= NT * PER_THREAD; d and perm in LDS.  The caller fills d and
// sets perm to the identity before its own barrier: NaNs, whose ranks collide, then leave perm in range.
template <int NT, int PER_THREAD>
__device__ __forceinline__ void nq_rank_perm(const double* d, int m, int* perm) {
  const int tid = threadIdx.x;
  int rank[PER_THREAD];
#pragma unroll
  for (int u = 0; u < PER_THREAD; ++u) {
    const int i = tid + u * NT;
    rank[u] = -1;
    if (i < m) {
      const double di = d[i];
      int rk = 0;
      for (int j = 0; j < m; ++j) rk += (d[j] < di || (d[j] == di && j < i)) ? 1 : 0;
      rank[u] = rk;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < PER_THREAD; ++u)
    if (rank[u] >= 0) perm[rank[u]] = tid + u * NT;
  __syncthreads();
}
