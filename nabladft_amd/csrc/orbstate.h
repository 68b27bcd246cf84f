// What the files of the orbital family share (orbitals.hip: the solver and its figures; orbdens.hip: weighted Gram products of the coefficient blocks and
// populations; and, through orbresp_tiles.h, every orb*.hip after them): the parts of the caller-owned state buffer, the kernels' view of it, the refusal of a
// call that comes with other dimensions than nq_orb_init, the workgroup -> (molecule, tile) map with its one bounds test (orb_mol, orb_tile_mol), the workgroup
// sum and maximum, the arithmetic that maps a workgroup to a lower-triangle output tile, and the host-side check every entry point makes first: the state
// pointer, the dimensions and the grid (orb_check_launch).  Header-only, every function static or __forceinline__ (each file keeps its own copy and its own
// flags); no a * b + c in here.
#pragma once
#include <limits.h>
#include <math.h>

#include "../../include/nablaq.h"
#include "devstate.h"

#define NQ_ORB_MAX_M 1024
#define NQ_ORB_NT 512
#define NQ_ORB_NW (NQ_ORB_NT / 64)
#define NQ_ORB_HDR 16
#define NQ_ORB_TILE 64        // edge of a workgroup's output tile in k_orb_wgram: 4 x 4 MFMA tiles of 16 x 16

enum { OH_B = 0, OH_M, OH_PLO, OH_PHI, OH_STATUS, OH_MAXM, OH_KIND };
#define NQ_ORB_KIND_PURIFY 2  // OH_KIND once orbpurify.hip has used the state: coeff / work / chol hold X, Ht, Y, not coefficients, A and L (0: as nq_orb_init left it)
enum { OP_HDR = 0, OP_ORB_PTR, OP_PACK_PTR, OP_ORDER, OP_STATUS, OP_INFO, OP_ITERS, OP_EPS, OP_COEFF, OP_WORK, OP_CHOL, OP_PARTS };
typedef NqStateLayout<OP_PARTS> OrbLayout;

static inline OrbLayout orb_layout(long B, long M, long long P) {
  const size_t bytes[OP_PARTS] = {NQ_ORB_HDR * 4, (size_t)(B + 1) * 4, (size_t)(B + 1) * 8, (size_t)B * 4, (size_t)B * 4, (size_t)B * 4, (size_t)B * 4,
                                  (size_t)M * 8, (size_t)P * 8, (size_t)P * 8, (size_t)P * 8};
  return nq_state_layout(bytes);
}

struct OrbArgs {
  int* hdr; const int* orb_ptr; const long long* pack_ptr; const int* order; int* status; int* info; int* iters; double* eps; double* coeff; double* work;
  double* chol;
  int B, M; long long P;
};

__device__ __forceinline__ bool orb_dims_ok(const OrbArgs& a) {
  const bool ok = a.hdr[OH_B] == a.B && a.hdr[OH_M] == a.M && nq_split64_is(a.hdr + OH_PLO, a.P);
  if (!ok && blockIdx.x == 0 && threadIdx.x == 0) a.hdr[OH_STATUS] = -2;   // not the state nq_orb_init prepared: touch nothing else
  return ok;
}

// The entry points that read orbital coefficients or energies (nq_orb_wgram, the response and the smear families) refuse a state that holds a purification,
// the purification entry points every other state: header status -3, nothing else is touched.
__device__ __forceinline__ bool orb_kind_ok(const OrbArgs& a, bool purify) {
  if (!orb_dims_ok(a)) return false;
  const bool ok = (a.hdr[OH_KIND] == NQ_ORB_KIND_PURIFY) == purify;
  if (!ok && blockIdx.x == 0 && threadIdx.x == 0) a.hdr[OH_STATUS] = -3;
  return ok;
}

// ---- which molecule (and which of its tiles) a workgroup serves; false: exit (uniform over the workgroup) -------------------------------------------------------
// Molecule b's first orbital o0, its orbital count m, the start of its packed m x m block and whether its status word reports a failure.  false: the block
// does not lie inside the state (a state overwritten since nq_orb_init).  A kernel that does not read `failed` does not load the status word.
__device__ __forceinline__ bool orb_mol(const OrbArgs& a, int b, int& o0, int& m, long long& base, bool& failed) {
  o0 = a.orb_ptr[b];
  m = a.orb_ptr[b + 1] - o0;
  base = a.pack_ptr[b];
  if (m < 1 || m > NQ_ORB_MAX_M || o0 < 0 || o0 + m > a.M || base < 0 || base + (long long)m * m > a.P) return false;
  failed = a.status[b] != 0;
  return true;
}

struct OrbTile {
  int b, t, m, o0;
  long long base;
  bool failed;
};

// what a kernel needs of the state's header: its layout alone, the coefficients and energies of a solve, or the iterates of a purification (orb_kind_ok)
enum OrbHeader { ORB_HDR_DIMS = 0, ORB_HDR_SOLVE, ORB_HDR_PURIFY };

// workgroup blockIdx.x is workgroup t of the `per` that serve molecule b
template <OrbHeader HDR>
__device__ __forceinline__ bool orb_tile_mol(const OrbArgs& a, int per, OrbTile& q) {
  if (!(HDR == ORB_HDR_DIMS ? orb_dims_ok(a) : orb_kind_ok(a, HDR == ORB_HDR_PURIFY))) return false;
  q.b = blockIdx.x / per;
  q.t = blockIdx.x - q.b * per;
  if (q.b >= a.B) return false;
  return orb_mol(a, q.b, q.o0, q.m, q.base, q.failed);
}

// the wavefronts' partial sums meet in red[NQ_ORB_NW] and are added in wavefront order; every thread returns what it read from LDS (uniform)
__device__ __forceinline__ double orb_block_sum(double v, double* red) {
  v = nq_wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
#pragma unroll
  for (int w = 0; w < NQ_ORB_NW; ++w) r += red[w];
  __syncthreads();
  return r;
}

// the same for the maximum (fmax: a NaN is dropped)
__device__ __forceinline__ double orb_block_max(double v, double* red) {
  v = nq_wave_max_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int w = 1; w < NQ_ORB_NW; ++w) r = fmax(r, red[w]);
  __syncthreads();
  return r;
}

static inline int orb_check_dims(int32_t B, int32_t M, int64_t P) {
  if (B < 1) return nq_fail(NQ_ERR_ARG, "nq_orb: empty batch (B=%d)", B);
  if (M < B || (int64_t)M > (int64_t)B * NQ_ORB_MAX_M) return nq_fail(NQ_ERR_ARG, "nq_orb: M=%d orbitals do not fit B=%d molecules of 1..%d", M, B, NQ_ORB_MAX_M);
  if (P < M || P > (int64_t)M * NQ_ORB_MAX_M) return nq_fail(NQ_ERR_ARG, "nq_orb: P=%lld does not fit M=%d", (long long)P, M);
  return NQ_OK;
}

static inline OrbArgs orb_args(void* state, int32_t B, int32_t M, int64_t P) {
  const OrbLayout L = orb_layout(B, M, P);
  char* s = (char*)state;
  OrbArgs a;
  a.hdr = (int*)(s + L.part[OP_HDR]); a.orb_ptr = (const int*)(s + L.part[OP_ORB_PTR]); a.pack_ptr = (const long long*)(s + L.part[OP_PACK_PTR]);
  a.order = (const int*)(s + L.part[OP_ORDER]); a.status = (int*)(s + L.part[OP_STATUS]); a.info = (int*)(s + L.part[OP_INFO]);
  a.iters = (int*)(s + L.part[OP_ITERS]); a.eps = (double*)(s + L.part[OP_EPS]); a.coeff = (double*)(s + L.part[OP_COEFF]);
  a.work = (double*)(s + L.part[OP_WORK]); a.chol = (double*)(s + L.part[OP_CHOL]);
  a.B = B; a.M = M; a.P = P;
  return a;
}

// ---- lower-triangle tiles of an m x m output (k_orb_wgram): tile t = ti (ti + 1) / 2 + tj, tj <= ti ------------------------------------------------------------
__host__ __device__ static inline int orb_tile_rows(int m) { return (m + NQ_ORB_TILE - 1) / NQ_ORB_TILE; }
__host__ __device__ static inline int orb_tile_count(int m) { const int r = orb_tile_rows(m); return r * (r + 1) / 2; }
__host__ __device__ static inline void orb_tile_decode(int t, int* ti, int* tj) {
  int r = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while (r * (r + 1) / 2 > t) --r;               // the float root may be one off either way
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  *ti = r; *tj = t - r * (r + 1) / 2;
}
// The largest m a batch of these dimensions can hold: the other B - 1 molecules have at least one orbital each.  The host sizes the grid of k_orb_wgram by
// it (it does not read the state); a workgroup whose tile lies beyond its molecule's own count exits.
static inline int orb_largest_m_bound(int32_t B, int32_t M, int64_t P) {
  long long b = (long long)M - (B - 1);
  const long long p = P - (B - 1);
  if (b > NQ_ORB_MAX_M) b = NQ_ORB_MAX_M;
  while (b > 1 && b * b > p) --b;
  return b < 1 ? 1 : (int)b;
}

// ---- host: what every entry point of the family checks first ------------------------------------------------------------------------------------------------------
// The workgroups a launch gives every molecule: `per_mol` of them (one, unless the kernel splits a molecule's work into a fixed number of shares), one per 64
// orbitals, one per lower-triangle 64 x 64 tile, or one per tile of the square.  tr = the tile rows of the largest molecule the dimensions allow.
enum OrbGrid { ORB_GRID_MOL = 0, ORB_GRID_ROWS, ORB_GRID_LOWER, ORB_GRID_SQUARE };

static int orb_check_launch(const char* who, const void* state, int32_t B, int32_t M, int64_t P, OrbGrid grid, int* tr = nullptr, int per_mol = 1) {
  if (!state) return nq_fail(NQ_ERR_ARG, "%s: null argument (state)", who);
  NQ_TRY(orb_check_dims(B, M, P));
  const long long r = orb_tile_rows(orb_largest_m_bound(B, M, P));
  const long long per = grid == ORB_GRID_MOL ? per_mol : grid == ORB_GRID_ROWS ? r : grid == ORB_GRID_LOWER ? r * (r + 1) / 2 : r * r;
  if ((long long)B * per > INT_MAX) return nq_fail(NQ_ERR_ARG, "%s: B=%d molecules of up to %lld workgroups exceed the grid", who, B, per);
  if (tr) *tr = (int)r;
  return NQ_OK;
}
