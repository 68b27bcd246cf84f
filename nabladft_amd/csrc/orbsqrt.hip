// Eigensolver-free S^(1/2) and S^(-1/2) of every molecule of a batch: the coupled Newton-Schulz iteration (Higham, Functions of Matrices, ch. 6) on the float64
// matrix cores.  With the SP2 purification of orbpurify.hip on the Löwdin Hamiltonian S^(-1/2) H S^(-1/2) a whole SCF target needs no solve.  Serves the same
// empty slots of the reference as the solver (phisnet/nn/neural_network.py:969-993).
//
// Per molecule (S symmetric positive definite m x m):
//
//   k_sq_init     c = the largest absolute row sum of S (Gershgorin: c >= s_max), one row per wavefront in a fixed order, the lower triangle mirrored;
//                 Y_0 = S / c, Z_0 = I into buffer 0; ctl and log cleared.  c not finite or <= 0: status 1.  One 512-thread workgroup per molecule, largest first.
//   k_sq_t        T = (3 I - sym(Z Y)) / 2 on lower-triangle 64 x 64 tiles, mirrored ("sym": the lower triangle of the product); every diagonal tile d leaves
//                 its partial tr(Z Y) in slot d of the molecule
//   k_sq_update   every workgroup of the molecule sums the slots in slot order, delta_k = m - tr(Z Y), and decides alike: stop with (Y, Z) = (Y_k, Z_k) when
//                 delta_k = 0, or when k >= 1 and |delta_k| < 1e-9 m and |delta_k| >= |delta_k-1|; else Y' = Y T and Z' = T Z as FULL general products into the
//                 other buffer pair, from one pass over the contraction index: workgroup (ti, tj) forms Y'(ti, tj) and the transpose of Z'(tj, ti), which both
//                 contract with the same staged tile T[k][j0 ..] (T is exactly symmetric).  The first workgroup logs the entry (1: updated, 3: stopped),
//                 delta_k and iters.
//   k_sq_finish   half = sqrt(c) times the mirrored lower triangle of Y, inv_half = the mirrored lower triangle of Z divided by sqrt(c), from the buffer pair the
//                 molecule's last update wrote (iters & 1).  Status 1, or a last log entry that is an update (not stopped in max_iter iterations: status 4,
//                 info 1): NaN in the molecule's own blocks of both.
//
// Y and Z are NOT symmetrised between iterations: mirroring or averaging Y T and T Z makes the iteration diverge a few steps after it reaches its rounding floor
// (DESIGN_details.md), so the two buffer pairs hold general matrices.  Iteration k of a molecule runs only if the molecule is not failed and (k = 0 or
// log[k - 1] is an update): the workgroups of a finished or failed molecule exit at once, and nq_orb_sqrt_run enqueues max_iter iterations with no host round
// trip.  Iteration k reads buffer pair k & 1 and writes the other: an output never aliases an operand of its launch.
//
// Where things live.  The state of nq_orb_init supplies the layout and the status (0, 1: c unusable, 4: not converged) / info / iters words; none of its
// P-sized parts is read or written, so the state is not marked and a solver state's coefficients survive.  Caller-owned, float64 on the device: Y, Z, T, Y2, Z2
// [P each], ctl double [B][24 + max_iter] = {c, sqrt(c), tr(Z Y) of the last iteration, 0 .., 16 slots of partial traces from word 8, delta_k for every
// iteration from word 24} and log int32 [B][max_iter].
//
// Products: the staging and matrix-instruction pieces of orbresp_tiles.h (K tile 16, one tile in LDS, one in flight), v_mfma_f64_16x16x4_f64, k in steps of 4
// from 0.  No atomics; every sum has an order that depends on the molecule alone: bitwise reproducible, independent of the rest of the batch.
//
// Resources (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage): see DESIGN_details.md.
// Compiled with -ffp-contract=off like its siblings.
#include "orbresp_tiles.h"

#define NQ_SQ_SLOTS (NQ_ORB_MAX_M / NQ_ORB_TILE)
#define NQ_SQ_CTL 24
#define NQ_SQ_MAX_ITER 10000
#define NQ_SQ_TP (NQ_ORB_TILE + 1)                          // row pitch of the transposing tile
#define NQ_SQ_LDS (NQ_ORB_TILE * NQ_SQ_TP > 3 * NQ_RS_TILE ? NQ_ORB_TILE * NQ_SQ_TP : 3 * NQ_RS_TILE)
enum { SC_C = 0, SC_ROOT, SC_TR, SC_SLOT = 8 };

__device__ __forceinline__ bool sq_runs(const OrbArgs& a, const OrbTile& q, const int* log, int k) { return a.status[q.b] == 0 && (k == 0 || log[k - 1] == 1); }

// ---- c, Y_0 = S / c, Z_0 = I -------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_ORB_NT) void k_sq_init(OrbArgs a, const void* S, int s_f64, int max_iter, double* Yall, double* Zall, double* ctl_all, int* log_all) {
  __shared__ double wtop[NQ_ORB_NW];
  if (!orb_dims_ok(a)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = a.order[blockIdx.x];
  if (b < 0 || b >= a.B) return;
  const int o0 = a.orb_ptr[b], m = a.orb_ptr[b + 1] - o0;
  const long long base = a.pack_ptr[b];
  if (m < 1 || m > NQ_ORB_MAX_M || base < 0 || base + (long long)m * m > a.P) return;   // uniform: a state overwritten since nq_orb_init
  double* ctl = ctl_all + (long long)b * (NQ_SQ_CTL + max_iter);
  int* log = log_all + (long long)b * max_iter;
  for (int k = tid; k < max_iter; k += NQ_ORB_NT) log[k] = 0;
  for (int k = tid; k < NQ_SQ_CTL + max_iter; k += NQ_ORB_NT) ctl[k] = 0.0;
  double top = 0.0;                                                 // one row per wavefront, a fixed order inside the row
  bool bad = false;
  for (int i = wave; i < m; i += NQ_ORB_NW) {
    double s = 0.0;
    for (int j = lane; j < m; j += 64) s += fabs(nq_load_f64(S, base + (j <= i ? (long long)i * m + j : (long long)j * m + i), s_f64));
    s = nq_wave_sum_f64(s);
    bad = bad || !(s < INFINITY);
    top = fmax(top, s);
  }
  if (lane == 0) wtop[wave] = bad ? nq_nan_f64() : top;
  __syncthreads();
  double c = wtop[0];
  bad = !(c == c);
  for (int w = 1; w < NQ_ORB_NW; ++w) {
    bad = bad || !(wtop[w] == wtop[w]);
    c = fmax(c, wtop[w]);
  }
  const bool fail = bad || !(c > 0.0);
  if (tid == 0) {
    ctl[SC_C] = fail ? nq_nan_f64() : c;
    ctl[SC_ROOT] = fail ? nq_nan_f64() : sqrt(c);
    a.status[b] = fail ? 1 : 0;
    a.info[b] = 0;
    a.iters[b] = 0;
  }
  if (fail) return;
  double* Y = Yall + base;
  double* Z = Zall + base;
  for (int idx = tid; idx < m * m; idx += NQ_ORB_NT) {
    const int i = idx / m, j = idx - i * m;
    Y[idx] = nq_load_f64(S, base + (j <= i ? (long long)i * m + j : (long long)j * m + i), s_f64) / c;
    Z[idx] = i == j ? 1.0 : 0.0;
  }
}

// ---- T = (3 I - sym(Z Y)) / 2 ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_sq_t(OrbArgs a, int nt, int k, int max_iter, const double* Y0, const double* Z0, const double* Y1, const double* Z1,
                                                   double* Tall, double* ctl_all, const int* log_all) {
  __shared__ double lds[3 * NQ_RS_TILE];
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, nt, q)) return;
  const int m = q.m;
  if (q.t >= orb_tile_count(m) || !sq_runs(a, q, log_all + (long long)q.b * max_iter, k)) return;
  int ti, tj;
  orb_tile_decode(q.t, &ti, &tj);
  const int i0 = ti * NQ_ORB_TILE, j0 = tj * NQ_ORB_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const double* Y = ((k & 1) ? Y1 : Y0) + q.base;
  const double* Z = ((k & 1) ? Z1 : Z0) + q.base;
  double* T = Tall + q.base;
  orb_f64x4 acc[4], none[4];
  rs_zero(acc);
  rs_zero(none);
  rs_gemm<true, false, false>(Z, nullptr, m, Y, m, 0, m, i0, m, j0, m, lds, acc, none);   // sum_k Z[i][k] Y[k][j]
  __syncthreads();                                                   // the last tile has been consumed: lds is free for the diagonal
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + lk + 4 * r;
      if (i >= m || j > i) continue;
      const double zy = acc[s][r];
      const double t = 0.5 * ((j == i ? 3.0 : 0.0) - zy);
      T[(long long)i * m + j] = t;
      if (j != i) T[(long long)j * m + i] = t;
      else lds[i - i0] = zy;
    }
  }
  if (ti == tj) {                                                    // uniform
    __syncthreads();
    if (wave == 0) {
      const int i = i0 + lane;
      const double tr = nq_wave_sum_f64(i < m ? lds[lane] : 0.0);
      if (lane == 0) ctl_all[(long long)q.b * (NQ_SQ_CTL + max_iter) + SC_SLOT + ti] = tr;
    }
  }
}

// ---- accY[s] += Y(i0 + 16 wave .., k) T(k, j0 + 16 s ..) and accZ[s] += Z(k, i0 + 16 wave ..) T(k, j0 + 16 s ..) over all k: the loop of rs_gemm with two A
// operands of different orientation against one staged B tile.  Every thread of the workgroup must call it (barriers inside).  lds: 3 tiles.
__device__ __forceinline__ void sq_gemm2(const double* Y, const double* Z, const double* T, int m, int i0, int j0, double* lds, orb_f64x4 (&accY)[4],
                                         orb_f64x4 (&accZ)[4]) {
  double* tY = lds;
  double* tZ = lds + NQ_RS_TILE;
  double* tT = lds + 2 * NQ_RS_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const bool rows = i0 + wave * 16 < m;                        // uniform over the wavefront
  double ry[NQ_RS_PER], rz[NQ_RS_PER], rt[NQ_RS_PER];
  rs_fetch<true>(ry, Y, m, 0, m, i0, m);
  rs_fetch<false>(rz, Z, m, 0, m, i0, m);
  rs_fetch<false>(rt, T, m, 0, m, j0, m);
  for (int k0 = 0; k0 < m; k0 += NQ_RS_KT) {
    __syncthreads();                                           // the previous tile has been consumed
    rs_stage<true>(tY, ry);
    rs_stage<false>(tZ, rz);
    rs_stage<false>(tT, rt);
    __syncthreads();
    if (k0 + NQ_RS_KT < m) {
      rs_fetch<true>(ry, Y, m, k0 + NQ_RS_KT, m, i0, m);
      rs_fetch<false>(rz, Z, m, k0 + NQ_RS_KT, m, i0, m);
      rs_fetch<false>(rt, T, m, k0 + NQ_RS_KT, m, j0, m);
    }
    if (rows) {
#pragma unroll
      for (int kk = 0; kk < NQ_RS_KT; kk += 4) {
        if (k0 + kk >= m) break;                               // uniform
        const double ay = rs_get<true>(tY, kk + lk, wave * 16 + lc);
        const double az = rs_get<false>(tZ, kk + lk, wave * 16 + lc);
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (j0 + s * 16 < m) {                               // uniform
            const double bv = rs_get<false>(tT, kk + lk, s * 16 + lc);
            accY[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, bv, accY[s], 0, 0, 0);
            accZ[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(az, bv, accZ[s], 0, 0, 0);
          }
      }
    }
  }
}

// ---- the decision, then Y' = Y T and Z' = T Z; one workgroup per 64 x 64 tile ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_sq_update(OrbArgs a, int tr, int k, int max_iter, double* Y0, double* Z0, double* Y1, double* Z1, const double* Tall,
                                                        double* ctl_all, int* log_all) {
  __shared__ double lds[NQ_SQ_LDS];
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, tr * tr, q)) return;
  const int m = q.m, ti = q.t / tr, tj = q.t - ti * tr;
  if (ti * NQ_ORB_TILE >= m || tj * NQ_ORB_TILE >= m) return;
  int* log = log_all + (long long)q.b * max_iter;
  if (!sq_runs(a, q, log, k)) return;
  double* ctl = ctl_all + (long long)q.b * (NQ_SQ_CTL + max_iter);
  double trzy = 0.0;
  const int nd = orb_tile_rows(m);
  for (int d = 0; d < nd; ++d) trzy += ctl[SC_SLOT + d];
  const double delta = (double)m - trzy, prev = k > 0 ? ctl[NQ_SQ_CTL + k - 1] : 0.0;
  const bool stop = delta == 0.0 || (k >= 1 && fabs(delta) < 1e-9 * (double)m && fabs(delta) >= fabs(prev));
  if (q.t == 0 && threadIdx.x == 0) {                                // nobody reads these words in this launch
    log[k] = stop ? 3 : 1;
    ctl[NQ_SQ_CTL + k] = delta;
    ctl[SC_TR] = trzy;
    a.iters[q.b] = stop ? k : k + 1;
  }
  if (stop) return;
  const int i0 = ti * NQ_ORB_TILE, j0 = tj * NQ_ORB_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const double* Y = ((k & 1) ? Y1 : Y0) + q.base;
  const double* Z = ((k & 1) ? Z1 : Z0) + q.base;
  double* Yn = ((k & 1) ? Y0 : Y1) + q.base;
  double* Zn = ((k & 1) ? Z0 : Z1) + q.base;
  orb_f64x4 accY[4], accZ[4];
  rs_zero(accY);
  rs_zero(accZ);
  sq_gemm2(Y, Z, Tall + q.base, m, i0, j0, lds, accY, accZ);
  __syncthreads();                                                   // the last tile has been consumed: lds is free for the transposition
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int cj = s * 16 + lc, j = j0 + cj;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ci = wave * 16 + lk + 4 * r, i = i0 + ci;
      if (i < m && j < m) Yn[(long long)i * m + j] = accY[s][r];
      lds[cj * NQ_SQ_TP + ci] = accZ[s][r];                          // element (j, i) of Z'
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < NQ_ORB_TILE * NQ_ORB_TILE; e += NQ_RS_NT) {
    const int cj = e >> 6, ci = e & 63, j = j0 + cj, i = i0 + ci;
    if (i < m && j < m) Zn[(long long)j * m + i] = lds[cj * NQ_SQ_TP + ci];
  }
}

// ---- half = sqrt(c) Y and inv_half = Z / sqrt(c), lower triangles mirrored; one workgroup per lower-triangle 64 x 64 tile ------------------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_sq_finish(OrbArgs a, int nt, int max_iter, const double* Y0, const double* Z0, const double* Y1, const double* Z1,
                                                        const double* ctl_all, const int* log_all, double* half, double* inv_half) {
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, nt, q)) return;
  const int m = q.m;
  if (q.t >= orb_tile_count(m)) return;
  int ti, tj;
  orb_tile_decode(q.t, &ti, &tj);
  const bool late = log_all[(long long)q.b * max_iter + max_iter - 1] == 1;   // the log is zero unless the molecule iterated
  const bool failed = a.status[q.b] != 0 || late;                            // status goes 0 -> 4 below only where `late` holds: every workgroup decides alike
  if (late && q.t == 0 && threadIdx.x == 0) { a.status[q.b] = 4; a.info[q.b] = 1; }
  const int cur = a.iters[q.b] & 1;
  const double* Y = (cur ? Y1 : Y0) + q.base;
  const double* Z = (cur ? Z1 : Z0) + q.base;
  const double root = ctl_all[(long long)q.b * (NQ_SQ_CTL + max_iter) + SC_ROOT], nan = nq_nan_f64();
  double* A = half + q.base;
  double* Ai = inv_half + q.base;
  for (int e = threadIdx.x; e < NQ_ORB_TILE * NQ_ORB_TILE; e += NQ_RS_NT) {
    const int i = ti * NQ_ORB_TILE + (e >> 6), j = tj * NQ_ORB_TILE + (e & 63);
    if (i >= m || j > i) continue;
    const long long ij = (long long)i * m + j, ji = (long long)j * m + i;
    const double x = failed ? nan : root * Y[ij], xi = failed ? nan : Z[ij] / root;
    A[ij] = x;
    Ai[ij] = xi;
    if (j != i) { A[ji] = x; Ai[ji] = xi; }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------------------------
static int sq_check_iter(const char* who, int32_t k, int32_t max_iter) {
  if (max_iter < 1 || max_iter > NQ_SQ_MAX_ITER) return nq_fail(NQ_ERR_ARG, "%s: max_iter=%d outside 1..%d", who, max_iter, NQ_SQ_MAX_ITER);
  if (k < 0 || k >= max_iter) return nq_fail(NQ_ERR_ARG, "%s: iteration k=%d outside 0..max_iter-1=%d", who, k, max_iter - 1);
  return NQ_OK;
}

// the five iterates and whatever else the call names (NULL entries of `more` are skipped) must be arrays of their own
static int sq_check_arrays(const char* who, const double* Y, const double* Z, const double* T, const double* Y2, const double* Z2, const void* ctl, const void* log,
                           const void* more0, const void* more1) {
  if (!Y || !Z || !T || !Y2 || !Z2 || !ctl || !log) return nq_fail(NQ_ERR_ARG, "%s: null argument", who);
  const void* p[9] = {Y, Z, T, Y2, Z2, ctl, log, more0, more1};
  for (int i = 0; i < 9; ++i)
    for (int j = i + 1; j < 9; ++j)
      if (p[i] && p[i] == p[j]) return nq_fail(NQ_ERR_ARG, "%s: Y, Z, T, Y2, Z2, ctl, log and the other arrays of the call must be different arrays", who);
  return NQ_OK;
}

static int sq_step(const OrbArgs& a, int tr, int32_t k, int32_t max_iter, double* Y, double* Z, double* T, double* Y2, double* Z2, double* ctl, int32_t* log,
                   hipStream_t st) {
  const int nt = tr * (tr + 1) / 2;
  hipLaunchKernelGGL(k_sq_t, dim3(a.B * nt), dim3(NQ_RS_NT), 0, st, a, nt, (int)k, (int)max_iter, (const double*)Y, (const double*)Z, (const double*)Y2,
                     (const double*)Z2, T, ctl, (const int*)log);
  NQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sq_update, dim3(a.B * tr * tr), dim3(NQ_RS_NT), 0, st, a, tr, (int)k, (int)max_iter, Y, Z, Y2, Z2, (const double*)T, ctl, (int*)log);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

extern "C" {

int nq_orb_sqrt_init(void* state, int32_t B, int32_t M, int64_t P, const void* S, int32_t s_f64, int32_t max_iter, double* Y, double* Z, double* ctl, int32_t* log,
                     void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_sqrt_init", state, B, M, P, ORB_GRID_SQUARE, &tr));
  NQ_TRY(sq_check_iter("nq_orb_sqrt_init", 0, max_iter));
  if (!S || !Y || !Z || !ctl || !log) return nq_fail(NQ_ERR_ARG, "nq_orb_sqrt_init: null argument");
  if ((const void*)Y == S || (const void*)Z == S || Y == Z || (void*)ctl == (void*)log || (void*)ctl == (void*)Y || (void*)ctl == (void*)Z ||
      (void*)log == (void*)Y || (void*)log == (void*)Z || (const void*)ctl == S || (const void*)log == S)
    return nq_fail(NQ_ERR_ARG, "nq_orb_sqrt_init: S, Y, Z, ctl and log must be different arrays");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_sqrt_init");
  hipLaunchKernelGGL(k_sq_init, dim3(B), dim3(NQ_ORB_NT), 0, st, orb_args(state, B, M, P), S, (int)s_f64, (int)max_iter, Y, Z, ctl, (int*)log);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_sqrt_step(void* state, int32_t B, int32_t M, int64_t P, int32_t k, int32_t max_iter, double* Y, double* Z, double* T, double* Y2, double* Z2, double* ctl,
                     int32_t* log, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_sqrt_step", state, B, M, P, ORB_GRID_SQUARE, &tr));
  NQ_TRY(sq_check_iter("nq_orb_sqrt_step", k, max_iter));
  NQ_TRY(sq_check_arrays("nq_orb_sqrt_step", Y, Z, T, Y2, Z2, ctl, log, nullptr, nullptr));
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_sqrt_step");
  return sq_step(orb_args(state, B, M, P), tr, k, max_iter, Y, Z, T, Y2, Z2, ctl, log, st);
}

int nq_orb_sqrt_run(void* state, int32_t B, int32_t M, int64_t P, int32_t max_iter, double* Y, double* Z, double* T, double* Y2, double* Z2, double* ctl, int32_t* log,
                    void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_sqrt_run", state, B, M, P, ORB_GRID_SQUARE, &tr));
  NQ_TRY(sq_check_iter("nq_orb_sqrt_run", 0, max_iter));
  NQ_TRY(sq_check_arrays("nq_orb_sqrt_run", Y, Z, T, Y2, Z2, ctl, log, nullptr, nullptr));
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_sqrt_run");
  const OrbArgs a = orb_args(state, B, M, P);
  for (int k = 0; k < max_iter; ++k) NQ_TRY(sq_step(a, tr, k, max_iter, Y, Z, T, Y2, Z2, ctl, log, st));
  return NQ_OK;
}

int nq_orb_sqrt_finish(void* state, int32_t B, int32_t M, int64_t P, int32_t max_iter, const double* Y, const double* Z, const double* Y2, const double* Z2,
                       const double* ctl, const int32_t* log, double* half, double* inv_half, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_sqrt_finish", state, B, M, P, ORB_GRID_SQUARE, &tr));
  NQ_TRY(sq_check_iter("nq_orb_sqrt_finish", 0, max_iter));
  if (!half || !inv_half) return nq_fail(NQ_ERR_ARG, "nq_orb_sqrt_finish: null argument");
  NQ_TRY(sq_check_arrays("nq_orb_sqrt_finish", Y, Z, half, Y2, Z2, ctl, log, inv_half, nullptr));
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_sqrt_finish");
  const int nt = tr * (tr + 1) / 2;
  hipLaunchKernelGGL(k_sq_finish, dim3(B * nt), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), nt, (int)max_iter, Y, Z, Y2, Z2, ctl, (const int*)log, half,
                     inv_half);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
