// Eigensolver-free closed-shell density matrices and their gradients: second-order spectral-projection purification (SP2; Niklasson 2002) and the
// density-matrix-perturbation recursion along it (Niklasson & Challacombe 2004).  Serves the same empty slots of the reference as the solver
// (phisnet/nn/neural_network.py:969-993) for the quantities that need the occupied subspace only: D, populations, Tr(D S), Tr(D H).
//
// Per molecule (H, S symmetric m x m, n_occ doubly occupied orbitals):
//
//   k_pur_orth          S = L L^T with the arithmetic and the pivot rule of k_orb_solve (status 1, info = the 1-based pivot), then Z = L^-1 in place, column by
//                       column from the last, the upper triangle written as zero.  One 512-thread workgroup per molecule, largest first; latency-bound.
//   k_pur_load          out = alpha A from the lower triangle of A (float32 or float64) mirrored, or alpha (A + A^T) / 2: exactly symmetric either way
//   k_pur_prod<0..3>    the two triangular products of a congruence, contraction ranges cut to the non-zero part of Z:
//                         T = A Z^T (0), out = alpha Z T (1): out = alpha sym(Z A Z^T);   T = A Z (2), out = alpha Z^T T (3): out = alpha sym(Z^T A Z)
//                       (1) and (3) compute the lower-triangle 64 x 64 tiles and mirror them ("sym": the lower triangle of the product)
//   k_pur_prod<4>       out = alpha A B + beta C, full m x m (the few general products of the S half of the gradient)
//   k_pur_init          Ht symmetric into the state, Gershgorin bounds e_min <= spec(Ht) <= e_max in a fixed order, X_0 = (e_max I - Ht) / (e_max - e_min);
//                       n_occ <= 0: X = 0, n_occ >= m or e_max = e_min: X = I, neither iterates
//   k_pur_square<false> Y = X X, lower-triangle tiles mirrored; every diagonal tile d leaves its partial tr X and tr Y in slot d of the molecule
//   k_pur_update<false> every workgroup of the molecule sums the slots in slot order, t = tr X, t2 = tr Y, delta_k = t - t2, and decides alike:
//                       stop with X = X_k when delta_k = 0, or when k >= 2 and |delta_k| >= |delta_k-1| and |delta_k-1| < 1e-6 max(1, n_occ); else
//                       X = Y if |t2 - n_occ| <= |2 t - t2 - n_occ| (log 1), else X = 2 X - Y (log 2), elementwise.  The first workgroup logs the entry
//                       (3: stopped), delta_k and, on a stop, iters.
//   k_pur_finish        a molecule whose last log entry is a branch did not stop in max_iter iterations: status 4, X = NaN
//   k_pur_resp_init     X = X_0 again, X1_0 = -Gt / (e_max - e_min) for the symmetric upstream Gt of the orthonormal basis
//   k_pur_square<true>  Y = X X and Q = X1 X + X X1 (= P + P^T for P = X X1) from the same staged tiles of X; Y by the instruction sequence of the forward
//   k_pur_update<true>  by the logged branch: (X, X1) = (Y, Q) or (2 X - Y, 2 X1 - Q).  No traces, no decisions: the X sequence is the forward's bit for bit.
//
// Iteration k of a molecule runs only if the molecule is not failed, not trivial and (k = 0 or log[k - 1] is a branch): the workgroups of a finished or
// failed molecule exit at once, and nq_orb_pur_run / nq_orb_pur_response_run enqueue max_iter iterations with no host round trip.
//
// Where things live.  The state of nq_orb_init: `coeff` holds X, `work` Ht, `chol` Y; status (0, 1: the orthogonaliser failed, 4: not converged), info,
// iters and the header are the solver's.  Caller-owned: Z [P] (one orthogonaliser serves any number of states of the same batch), X1, Q, the scratch of the
// congruence [P each], ctl double [B][40 + max_iter] = {e_min, e_max, kind (0 iterate, 1 X = 0, 2 X = I), n_occ, tr X, tr Y of the last iteration, 0, 0,
// 16 slots of (tr X, tr Y), delta_k for every iteration} and log int32 [B][max_iter].  The first call here sets the header word OH_KIND (orbstate.h).
//
// Products: rs_gemm of orbresp_tiles.h unchanged (K tile 16, one tile in LDS, one in flight: no deeper prefetch), v_mfma_f64_16x16x4_f64, k in steps of 4 from
// a multiple of 4.  No atomics; every sum has an order that depends on the molecule alone: bitwise reproducible, independent of the rest of the batch.
// status != 0: NaN in the molecule's own block of X and X1, which every product hands on.  Compiled with -ffp-contract=off like its siblings.
#include "orbresp_tiles.h"

#define NQ_PUR_SLOTS (NQ_ORB_MAX_M / NQ_ORB_TILE)
#define NQ_PUR_CTL 40
#define NQ_PUR_MAX_ITER 10000
enum { PC_EMIN = 0, PC_EMAX, PC_KIND, PC_NOCC, PC_T, PC_T2, PC_SLOT = 8 };

// KIND kernels read X, Ht or Y from the state (orb_tile_mol<ORB_HDR_PURIFY>); the others use its layout only (ORB_HDR_DIMS)
__device__ __forceinline__ bool pur_branch(int entry) { return entry == 1 || entry == 2; }
__device__ __forceinline__ double pur_x0(double h, bool diag, double e_min, double e_max) { return ((diag ? e_max : 0.0) - h) / (e_max - e_min); }

// ---- the orthogonaliser ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_ORB_NT) void k_pur_orth(OrbArgs a, const void* S, int s_f64, double* Zall) {
  __shared__ double v[NQ_ORB_MAX_M];
  if (!orb_dims_ok(a)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x == 0 && tid == 0) a.hdr[OH_KIND] = NQ_ORB_KIND_PURIFY;
  const int b = a.order[blockIdx.x];
  if (b < 0 || b >= a.B) return;
  const int o0 = a.orb_ptr[b], m = a.orb_ptr[b + 1] - o0;
  const long long base = a.pack_ptr[b];
  if (m < 1 || m > NQ_ORB_MAX_M || base < 0 || base + (long long)m * m > a.P) return;   // uniform: a state overwritten since nq_orb_init
  double* L = Zall + base;
  for (int i = wave; i < m; i += NQ_ORB_NW)
    for (int j = lane; j < m; j += 64) L[i * m + j] = j <= i ? nq_load_f64(S, base + (long long)i * m + j, s_f64) : 0.0;
  __syncthreads();
  int fail = 0;
  for (int j = 0; j < m; ++j) {
    const double piv = L[j * m + j];   // every thread reads the same entry: the branch below is uniform
    if (!(piv > 0.0) || !(piv < INFINITY)) { fail = j + 1; break; }
    const double r = sqrt(piv);
    __syncthreads();                   // everybody has read the pivot
    for (int i = j + 1 + tid; i < m; i += NQ_ORB_NT) {
      const double x = L[i * m + j] / r;
      L[i * m + j] = x;
      v[i] = x;
    }
    if (tid == 0) L[j * m + j] = r;
    __syncthreads();
    for (int i = j + 1 + wave; i < m; i += NQ_ORB_NW) {
      const double ci = v[i];
      for (int k = j + 1 + lane; k <= i; k += 64) L[i * m + k] = fma(-ci, v[k], L[i * m + k]);
    }
    __syncthreads();
  }
  if (fail) {
    const double nan = nq_nan_f64();
    for (int idx = tid; idx < m * m; idx += NQ_ORB_NT) L[idx] = nan;
    if (tid == 0) { a.status[b] = 1; a.info[b] = fail; a.iters[b] = 0; }
    return;
  }
  // Z L = I, column j of Z from the columns after it: Z[i][j] = -(sum_{j < k <= i} Z[i][k] L[k][j]) / L[j][j]; one row per wavefront
  for (int j = m - 1; j >= 0; --j) {
    const double ljj = L[j * m + j];
    for (int i = j + 1 + tid; i < m; i += NQ_ORB_NT) v[i] = L[i * m + j];
    __syncthreads();                   // the column is staged and everybody has read the pivot
    for (int i = j + 1 + wave; i < m; i += NQ_ORB_NW) {
      double s = 0.0;
      for (int k = j + 1 + lane; k <= i; k += 64) s = fma(L[i * m + k], v[k], s);
      s = nq_wave_sum_f64(s);
      if (lane == 0) L[i * m + j] = -s / ljj;
    }
    if (tid == 0) L[j * m + j] = 1.0 / ljj;
    __syncthreads();
  }
  if (tid == 0) { a.status[b] = 0; a.info[b] = 0; a.iters[b] = 0; }
}

// ---- out = alpha A, symmetric: the lower triangle mirrored (sym = 0) or (A + A^T) / 2 (sym = 1); one workgroup per 64 x 64 tile --------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_pur_load(OrbArgs a, int tr, const void* A, int a_f64, int sym, double alpha, double* out) {
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, tr * tr, q)) return;
  const int m = q.m, ti = q.t / tr, tj = q.t - ti * tr;
  if (ti * NQ_ORB_TILE >= m || tj * NQ_ORB_TILE >= m) return;
  for (int e = threadIdx.x; e < NQ_ORB_TILE * NQ_ORB_TILE; e += NQ_RS_NT) {
    const int i = ti * NQ_ORB_TILE + (e >> 6), j = tj * NQ_ORB_TILE + (e & 63);
    if (i >= m || j >= m) continue;
    const long long ij = q.base + (long long)i * m + j, ji = q.base + (long long)j * m + i;
    double x;
    if (sym) x = 0.5 * (nq_load_f64(A, ij, a_f64) + nq_load_f64(A, ji, a_f64));
    else x = nq_load_f64(A, j <= i ? ij : ji, a_f64);
    out[ij] = alpha * x;
  }
}

// ---- the products ---------------------------------------------------------------------------------------------------------------------------------------------------
// MODE 0: out = A Z^T; 1: out = alpha Z T, lower tiles mirrored; 2: out = A Z; 3: out = alpha Z^T T, lower tiles mirrored; 4: out = alpha A B + beta C.
// Z is the operand called Z below: Bm in modes 0 and 2, A in modes 1 and 3.
template <int MODE>
__global__ __launch_bounds__(NQ_RS_NT) void k_pur_prod(OrbArgs a, int nt, int tr, const double* A, const double* Bm, const double* Cin, double alpha, double beta,
                                                       double* out) {
  __shared__ double lds[3 * NQ_RS_TILE];
  constexpr bool LOWER = MODE == 1 || MODE == 3;
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, nt, q)) return;
  const int m = q.m;
  int ti, tj;
  if (LOWER) {
    if (q.t >= orb_tile_count(m)) return;
    orb_tile_decode(q.t, &ti, &tj);
  } else {
    ti = q.t / tr;
    tj = q.t - ti * tr;
    if (ti * NQ_ORB_TILE >= m || tj * NQ_ORB_TILE >= m) return;
  }
  const int i0 = ti * NQ_ORB_TILE, j0 = tj * NQ_ORB_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const double* Ap = A + q.base;
  const double* Bp = Bm + q.base;
  orb_f64x4 acc[4], none[4];
  rs_zero(acc);
  rs_zero(none);
  {
    const int jend = j0 + NQ_ORB_TILE < m ? j0 + NQ_ORB_TILE : m, iend = i0 + NQ_ORB_TILE < m ? i0 + NQ_ORB_TILE : m;
    if (MODE == 0) rs_gemm<true, true, false>(Ap, nullptr, m, Bp, m, 0, jend, i0, m, j0, m, lds, acc, none);    // sum_{k <= j} A[i][k] Z[j][k]
    if (MODE == 1) rs_gemm<true, false, false>(Ap, nullptr, m, Bp, m, 0, iend, i0, m, j0, m, lds, acc, none);   // sum_{k <= i} Z[i][k] T[k][j]
    if (MODE == 2) rs_gemm<true, false, false>(Ap, nullptr, m, Bp, m, j0, m, i0, m, j0, m, lds, acc, none);     // sum_{k >= j} A[i][k] Z[k][j]
    if (MODE == 3) rs_gemm<false, false, false>(Ap, nullptr, m, Bp, m, i0, m, i0, m, j0, m, lds, acc, none);    // sum_{k >= i} Z[k][i] T[k][j]
    if (MODE == 4) rs_gemm<true, false, false>(Ap, nullptr, m, Bp, m, 0, m, i0, m, j0, m, lds, acc, none);
  }
  double* X = out + q.base;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + lk + 4 * r;
      if (i >= m || j >= m || (LOWER && j > i)) continue;
      double x = acc[s][r];
      if (MODE == 1 || MODE == 3) x = alpha * x;
      if (MODE == 4) {
        x = alpha * x;
        if (Cin) x = x + beta * Cin[q.base + (long long)i * m + j];
      }
      X[(long long)i * m + j] = x;
      if (LOWER && j != i) X[(long long)j * m + i] = x;
    }
  }
}

// ---- bounds and X_0 ---------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_ORB_NT) void k_pur_init(OrbArgs a, const void* Hsrc, int h_f64, const double* Z, const int* n_occ, int max_iter, double* ctl_all,
                                                        int* log_all) {
  __shared__ double wlo[NQ_ORB_NW], whi[NQ_ORB_NW];
  if (!orb_dims_ok(a)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x == 0 && tid == 0) a.hdr[OH_KIND] = NQ_ORB_KIND_PURIFY;
  const int b = a.order[blockIdx.x];
  if (b < 0 || b >= a.B) return;
  const int o0 = a.orb_ptr[b], m = a.orb_ptr[b + 1] - o0;
  const long long base = a.pack_ptr[b];
  if (m < 1 || m > NQ_ORB_MAX_M || base < 0 || base + (long long)m * m > a.P) return;   // uniform
  double* ctl = ctl_all + (long long)b * (NQ_PUR_CTL + max_iter);
  int* log = log_all + (long long)b * max_iter;
  double* Ht = a.work + base;
  double* X = a.coeff + base;
  const double nan = nq_nan_f64();
  for (int k = tid; k < max_iter; k += NQ_ORB_NT) log[k] = 0;
  for (int k = tid; k < NQ_PUR_CTL + max_iter; k += NQ_ORB_NT) ctl[k] = 0.0;
  int st = a.status[b];                                             // uniform; written below by thread 0 only, after this read
  __syncthreads();
  if (st == 4) st = 0;                                              // what an earlier purification in this state left
  if (Z && !(Z[base] == Z[base])) st = 1;                           // the orthogonaliser (of this or another state) failed on this molecule
  if (tid == 0) { a.status[b] = st; a.iters[b] = 0; }
  if (st != 0) {
    for (int idx = tid; idx < m * m; idx += NQ_ORB_NT) X[idx] = nan;
    return;
  }
  if (Hsrc != (const void*)a.work) {                                // the symmetric float64 copy of the lower triangle
    for (int idx = tid; idx < m * m; idx += NQ_ORB_NT) {
      const int i = idx / m, j = idx - i * m;
      Ht[idx] = nq_load_f64(Hsrc, base + (j <= i ? (long long)i * m + j : (long long)j * m + i), h_f64);
    }
    __threadfence_block();
    __syncthreads();
  }
  double lo = INFINITY, hi = -INFINITY;                             // Gershgorin: one row per wavefront, a fixed order inside the row
  bool bad = false;
  for (int i = wave; i < m; i += NQ_ORB_NW) {
    double s = 0.0;
    for (int j = lane; j < m; j += 64)
      if (j != i) s += fabs(Ht[i * m + j]);
    s = nq_wave_sum_f64(s);
    const double d = Ht[i * m + i];
    lo = fmin(lo, d - s);
    hi = fmax(hi, d + s);
    bad = bad || !(s < INFINITY) || !(fabs(d) < INFINITY);
  }
  if (lane == 0) { wlo[wave] = bad ? nan : lo; whi[wave] = hi; }
  __syncthreads();
  double e_min = wlo[0], e_max = whi[0];
  bad = !(e_min == e_min);
  for (int w = 1; w < NQ_ORB_NW; ++w) {
    bad = bad || !(wlo[w] == wlo[w]);
    e_min = fmin(e_min, wlo[w]);
    e_max = fmax(e_max, whi[w]);
  }
  if (bad) { e_min = nan; e_max = nan; }                             // a non-finite H: every trace is NaN, no stop, status 4
  const int no = n_occ[b];
  const int kind = no <= 0 ? 1 : ((no >= m || e_max == e_min) ? 2 : 0);
  if (tid == 0) { ctl[PC_EMIN] = e_min; ctl[PC_EMAX] = e_max; ctl[PC_KIND] = (double)kind; ctl[PC_NOCC] = (double)no; }
  for (int idx = tid; idx < m * m; idx += NQ_ORB_NT) {
    const int i = idx / m, j = idx - i * m;
    X[idx] = kind == 0 ? pur_x0(Ht[idx], i == j, e_min, e_max) : ((kind == 2 && i == j) ? 1.0 : 0.0);
  }
}

// ---- Y = X X (and Q = X1 X + X X1) ------------------------------------------------------------------------------------------------------------------------------------
template <bool RESP>
__global__ __launch_bounds__(NQ_RS_NT) void k_pur_square(OrbArgs a, int nt, int k, int max_iter, double* ctl_all, const int* log_all, const double* X1all,
                                                         double* Qall) {
  __shared__ double lds[3 * NQ_RS_TILE];
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_PURIFY>(a, nt, q)) return;
  const int m = q.m;
  if (q.t >= orb_tile_count(m) || a.status[q.b] != 0) return;
  const int* log = log_all + (long long)q.b * max_iter;
  if (RESP) {
    if (!pur_branch(log[k])) return;
  } else {
    const double* ctl = ctl_all + (long long)q.b * (NQ_PUR_CTL + max_iter);
    if (ctl[PC_KIND] != 0.0 || (k > 0 && !pur_branch(log[k - 1]))) return;
  }
  int ti, tj;
  orb_tile_decode(q.t, &ti, &tj);
  const int i0 = ti * NQ_ORB_TILE, j0 = tj * NQ_ORB_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const double* X = a.coeff + q.base;
  double* Y = a.chol + q.base;
  orb_f64x4 accY[4], accL[4], accR[4];
  rs_zero(accY);
  rs_zero(accL);
  rs_zero(accR);
  if (RESP) {
    const double* X1 = X1all + q.base;
    rs_gemm<true, false, true>(X, X1, m, X, m, 0, m, i0, m, j0, m, lds, accY, accL);        // X X and X1 X from the same staged tiles of X
    rs_gemm<true, false, false>(X, nullptr, m, X1, m, 0, m, i0, m, j0, m, lds, accR, accL);   // X X1 (accL is not touched)
  } else {
    rs_gemm<true, false, false>(X, nullptr, m, X, m, 0, m, i0, m, j0, m, lds, accY, accL);
  }
  double* Q = RESP ? Qall + q.base : nullptr;
  __syncthreads();                                                   // the last tile has been consumed: lds is free for the diagonal
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j = j0 + s * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wave * 16 + lk + 4 * r;
      if (i >= m || j > i) continue;
      const double y = accY[s][r];
      Y[(long long)i * m + j] = y;
      if (j != i) Y[(long long)j * m + i] = y;
      if (RESP) {
        const double p = accL[s][r] + accR[s][r];
        Q[(long long)i * m + j] = p;
        if (j != i) Q[(long long)j * m + i] = p;
      } else if (j == i) {
        lds[i - i0] = y;
      }
    }
  }
  if (!RESP && ti == tj) {                                           // uniform
    __syncthreads();
    if (wave == 0) {
      const int i = i0 + lane;
      const double tx = nq_wave_sum_f64(i < m ? X[(long long)i * m + i] : 0.0), ty = nq_wave_sum_f64(i < m ? lds[lane] : 0.0);
      if (lane == 0) {
        double* ctl = ctl_all + (long long)q.b * (NQ_PUR_CTL + max_iter);
        ctl[PC_SLOT + 2 * ti] = tx;
        ctl[PC_SLOT + 2 * ti + 1] = ty;
      }
    }
  }
}

// ---- the decision and the elementwise update; one workgroup per 64 x 64 tile of X --------------------------------------------------------------------------------------
template <bool RESP>
__global__ __launch_bounds__(NQ_RS_NT) void k_pur_update(OrbArgs a, int tr, int k, int max_iter, double* ctl_all, int* log_all, double* X1all, const double* Qall) {
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_PURIFY>(a, tr * tr, q)) return;
  const int m = q.m, ti = q.t / tr, tj = q.t - ti * tr;
  if (ti * NQ_ORB_TILE >= m || tj * NQ_ORB_TILE >= m || a.status[q.b] != 0) return;
  int* log = log_all + (long long)q.b * max_iter;
  int entry;
  if (RESP) {
    entry = log[k];
    if (!pur_branch(entry)) return;
  } else {
    double* ctl = ctl_all + (long long)q.b * (NQ_PUR_CTL + max_iter);
    if (ctl[PC_KIND] != 0.0 || (k > 0 && !pur_branch(log[k - 1]))) return;
    double t = 0.0, t2 = 0.0;
    const int nd = orb_tile_rows(m);
    for (int d = 0; d < nd; ++d) {
      t += ctl[PC_SLOT + 2 * d];
      t2 += ctl[PC_SLOT + 2 * d + 1];
    }
    const double no = ctl[PC_NOCC], delta = t - t2, prev = k > 0 ? ctl[NQ_PUR_CTL + k - 1] : 0.0;
    const bool stop = delta == 0.0 || (k >= 2 && fabs(delta) >= fabs(prev) && fabs(prev) < 1e-6 * fmax(1.0, no));
    entry = stop ? 3 : (fabs(t2 - no) <= fabs(2.0 * t - t2 - no) ? 1 : 2);
    if (q.t == 0 && threadIdx.x == 0) {                              // nobody reads these words in this launch
      log[k] = entry;
      ctl[NQ_PUR_CTL + k] = delta;
      ctl[PC_T] = t;
      ctl[PC_T2] = t2;
      a.iters[q.b] = stop ? k : k + 1;
    }
    if (stop) return;
  }
  double* X = a.coeff + q.base;
  const double* Y = a.chol + q.base;
  for (int e = threadIdx.x; e < NQ_ORB_TILE * NQ_ORB_TILE; e += NQ_RS_NT) {
    const int i = ti * NQ_ORB_TILE + (e >> 6), j = tj * NQ_ORB_TILE + (e & 63);
    if (i >= m || j >= m) continue;
    const long long ij = (long long)i * m + j;
    X[ij] = entry == 1 ? Y[ij] : 2.0 * X[ij] - Y[ij];
    if (RESP) X1all[q.base + ij] = entry == 1 ? Qall[q.base + ij] : 2.0 * X1all[q.base + ij] - Qall[q.base + ij];
  }
}

__global__ __launch_bounds__(NQ_RS_NT) void k_pur_finish(OrbArgs a, int tr, int max_iter, const int* log_all) {
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_PURIFY>(a, tr * tr, q)) return;
  const int m = q.m, ti = q.t / tr, tj = q.t - ti * tr;
  if (ti * NQ_ORB_TILE >= m || tj * NQ_ORB_TILE >= m) return;
  if (!pur_branch(log_all[(long long)q.b * max_iter + max_iter - 1])) return;   // the log is zero unless the molecule iterated
  if (q.t == 0 && threadIdx.x == 0) a.status[q.b] = 4;
  double* X = a.coeff + q.base;
  const double nan = nq_nan_f64();
  for (int e = threadIdx.x; e < NQ_ORB_TILE * NQ_ORB_TILE; e += NQ_RS_NT) {
    const int i = ti * NQ_ORB_TILE + (e >> 6), j = tj * NQ_ORB_TILE + (e & 63);
    if (i < m && j < m) X[(long long)i * m + j] = nan;
  }
}

__global__ __launch_bounds__(NQ_RS_NT) void k_pur_resp_init(OrbArgs a, int tr, int max_iter, const double* ctl_all, const double* Gt, double* X1all) {
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_PURIFY>(a, tr * tr, q)) return;
  const int m = q.m, ti = q.t / tr, tj = q.t - ti * tr;
  if (ti * NQ_ORB_TILE >= m || tj * NQ_ORB_TILE >= m) return;
  const double* ctl = ctl_all + (long long)q.b * (NQ_PUR_CTL + max_iter);
  const bool failed = a.status[q.b] != 0, trivial = ctl[PC_KIND] != 0.0;
  const double e_min = ctl[PC_EMIN], e_max = ctl[PC_EMAX], nan = nq_nan_f64();
  double* X = a.coeff + q.base;
  const double* Ht = a.work + q.base;
  for (int e = threadIdx.x; e < NQ_ORB_TILE * NQ_ORB_TILE; e += NQ_RS_NT) {
    const int i = ti * NQ_ORB_TILE + (e >> 6), j = tj * NQ_ORB_TILE + (e & 63);
    if (i >= m || j >= m) continue;
    const long long ij = (long long)i * m + j;
    if (failed) X1all[q.base + ij] = nan;
    else if (trivial) X1all[q.base + ij] = 0.0;
    else {
      X[ij] = pur_x0(Ht[ij], i == j, e_min, e_max);
      X1all[q.base + ij] = -Gt[q.base + ij] / (e_max - e_min);
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------------------------
static int pur_check_iter(const char* who, int32_t k, int32_t max_iter) {
  if (max_iter < 1 || max_iter > NQ_PUR_MAX_ITER) return nq_fail(NQ_ERR_ARG, "%s: max_iter=%d outside 1..%d", who, max_iter, NQ_PUR_MAX_ITER);
  if (k < 0 || k >= max_iter) return nq_fail(NQ_ERR_ARG, "%s: iteration k=%d outside 0..max_iter-1=%d", who, k, max_iter - 1);
  return NQ_OK;
}

static int pur_step(const OrbArgs& a, int tr, int32_t k, int32_t max_iter, double* ctl, int32_t* log, hipStream_t st) {
  const int nt = tr * (tr + 1) / 2;
  hipLaunchKernelGGL(k_pur_square<false>, dim3(a.B * nt), dim3(NQ_RS_NT), 0, st, a, nt, (int)k, (int)max_iter, ctl, (const int*)log, (const double*)nullptr,
                     (double*)nullptr);
  NQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pur_update<false>, dim3(a.B * tr * tr), dim3(NQ_RS_NT), 0, st, a, tr, (int)k, (int)max_iter, ctl, (int*)log, (double*)nullptr,
                     (const double*)nullptr);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

static int pur_resp_step(const OrbArgs& a, int tr, int32_t k, int32_t max_iter, const int32_t* log, double* Q, double* X1, hipStream_t st) {
  const int nt = tr * (tr + 1) / 2;
  hipLaunchKernelGGL(k_pur_square<true>, dim3(a.B * nt), dim3(NQ_RS_NT), 0, st, a, nt, (int)k, (int)max_iter, (double*)nullptr, (const int*)log,
                     (const double*)X1, Q);
  NQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pur_update<true>, dim3(a.B * tr * tr), dim3(NQ_RS_NT), 0, st, a, tr, (int)k, (int)max_iter, (double*)nullptr, (int*)log, X1,
                     (const double*)Q);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

extern "C" {

int nq_orb_pur_orthogonalizer(void* state, int32_t B, int32_t M, int64_t P, const void* S, int32_t s_f64, double* Z, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_pur_orthogonalizer", state, B, M, P, ORB_GRID_SQUARE, &tr));
  if (!S || !Z) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_orthogonalizer: null argument");
  if ((const void*)Z == S) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_orthogonalizer: Z must not be S");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_pur_orthogonalizer");
  hipLaunchKernelGGL(k_pur_orth, dim3(B), dim3(NQ_ORB_NT), 0, st, orb_args(state, B, M, P), S, (int)s_f64, Z);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_pur_congruence(void* state, int32_t B, int32_t M, int64_t P, const double* Z, int32_t trans, const void* A, int32_t a_f64, int32_t a_sym, double alpha,
                          double* tmp, double* out, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_pur_congruence", state, B, M, P, ORB_GRID_SQUARE, &tr));
  if (!A || !out) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_congruence: null argument");
  if (Z && !tmp) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_congruence: the products need the scratch array tmp");
  if (A == (const void*)out || (Z && (tmp == out || A == (const void*)tmp || Z == out || Z == tmp)))
    return nq_fail(NQ_ERR_ARG, "nq_orb_pur_congruence: A, Z, tmp and out must be different arrays");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, Z ? (trans ? "orb_pur_congruence_t" : "orb_pur_congruence_n") : "orb_pur_congruence_load");
  const OrbArgs a = orb_args(state, B, M, P);
  const int nt = tr * (tr + 1) / 2;
  hipLaunchKernelGGL(k_pur_load, dim3(B * tr * tr), dim3(NQ_RS_NT), 0, st, a, tr, A, (int)a_f64, (int)a_sym, Z ? 1.0 : alpha, out);
  NQ_LAUNCH_CHECK();
  if (!Z) return NQ_OK;
  const double* none = nullptr;
  if (trans) {
    hipLaunchKernelGGL(k_pur_prod<2>, dim3(B * tr * tr), dim3(NQ_RS_NT), 0, st, a, tr * tr, tr, (const double*)out, Z, none, 1.0, 0.0, tmp);
    NQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pur_prod<3>, dim3(B * nt), dim3(NQ_RS_NT), 0, st, a, nt, tr, Z, (const double*)tmp, none, alpha, 0.0, out);
  } else {
    hipLaunchKernelGGL(k_pur_prod<0>, dim3(B * tr * tr), dim3(NQ_RS_NT), 0, st, a, tr * tr, tr, (const double*)out, Z, none, 1.0, 0.0, tmp);
    NQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pur_prod<1>, dim3(B * nt), dim3(NQ_RS_NT), 0, st, a, nt, tr, Z, (const double*)tmp, none, alpha, 0.0, out);
  }
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_pur_gemm(void* state, int32_t B, int32_t M, int64_t P, const double* A, const double* Bm, const double* C, double alpha, double beta, double* out,
                    void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_pur_gemm", state, B, M, P, ORB_GRID_SQUARE, &tr));
  if (!A || !Bm || !out) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_gemm: null argument");
  if (out == A || out == Bm) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_gemm: out must not be an operand of the product");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_pur_gemm");
  hipLaunchKernelGGL(k_pur_prod<4>, dim3(B * tr * tr), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), tr * tr, tr, A, Bm, C, alpha, beta, out);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_pur_init(void* state, int32_t B, int32_t M, int64_t P, const void* Ht, int32_t h_f64, const double* Z, const int32_t* n_occ, int32_t max_iter,
                    double* ctl, int32_t* log, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_pur_init", state, B, M, P, ORB_GRID_SQUARE, &tr));
  NQ_TRY(pur_check_iter("nq_orb_pur_init", 0, max_iter));
  if (!n_occ) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_init: n_occ is missing");
  if (!ctl || !log) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_init: null argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_pur_init");
  const OrbArgs a = orb_args(state, B, M, P);
  hipLaunchKernelGGL(k_pur_init, dim3(B), dim3(NQ_ORB_NT), 0, st, a, Ht ? Ht : (const void*)a.work, Ht ? (int)h_f64 : 1, Z, (const int*)n_occ, (int)max_iter, ctl,
                     (int*)log);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_pur_step(void* state, int32_t B, int32_t M, int64_t P, int32_t k, int32_t max_iter, double* ctl, int32_t* log, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_pur_step", state, B, M, P, ORB_GRID_SQUARE, &tr));
  NQ_TRY(pur_check_iter("nq_orb_pur_step", k, max_iter));
  if (!ctl || !log) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_step: null argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_pur_step");
  return pur_step(orb_args(state, B, M, P), tr, k, max_iter, ctl, log, st);
}

int nq_orb_pur_run(void* state, int32_t B, int32_t M, int64_t P, int32_t max_iter, double* ctl, int32_t* log, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_pur_run", state, B, M, P, ORB_GRID_SQUARE, &tr));
  NQ_TRY(pur_check_iter("nq_orb_pur_run", 0, max_iter));
  if (!ctl || !log) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_run: null argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_pur_run");
  const OrbArgs a = orb_args(state, B, M, P);
  for (int k = 0; k < max_iter; ++k) NQ_TRY(pur_step(a, tr, k, max_iter, ctl, log, st));
  hipLaunchKernelGGL(k_pur_finish, dim3(B * tr * tr), dim3(NQ_RS_NT), 0, st, a, tr, (int)max_iter, (const int*)log);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_pur_response_init(void* state, int32_t B, int32_t M, int64_t P, const double* Gt, int32_t max_iter, const double* ctl, double* X1, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_pur_response_init", state, B, M, P, ORB_GRID_SQUARE, &tr));
  NQ_TRY(pur_check_iter("nq_orb_pur_response_init", 0, max_iter));
  if (!Gt || !ctl || !X1) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_response_init: null argument");
  if (Gt == X1) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_response_init: X1 must not be Gt");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_pur_response_init");
  hipLaunchKernelGGL(k_pur_resp_init, dim3(B * tr * tr), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), tr, (int)max_iter, ctl, Gt, X1);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_pur_response_step(void* state, int32_t B, int32_t M, int64_t P, int32_t k, int32_t max_iter, const int32_t* log, double* Q, double* X1, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_pur_response_step", state, B, M, P, ORB_GRID_SQUARE, &tr));
  NQ_TRY(pur_check_iter("nq_orb_pur_response_step", k, max_iter));
  if (!log || !X1) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_response_step: null argument");
  if (!Q) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_response_step: the second input X1 needs the second output Q");
  if (Q == X1) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_response_step: Q must not be X1");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_pur_response_step");
  return pur_resp_step(orb_args(state, B, M, P), tr, k, max_iter, log, Q, X1, st);
}

int nq_orb_pur_response_run(void* state, int32_t B, int32_t M, int64_t P, int32_t max_iter, const int32_t* log, double* Q, double* X1, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_pur_response_run", state, B, M, P, ORB_GRID_SQUARE, &tr));
  NQ_TRY(pur_check_iter("nq_orb_pur_response_run", 0, max_iter));
  if (!log || !X1) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_response_run: null argument");
  if (!Q) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_response_run: the second input X1 needs the second output Q");
  if (Q == X1) return nq_fail(NQ_ERR_ARG, "nq_orb_pur_response_run: Q must not be X1");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_pur_response_run");
  const OrbArgs a = orb_args(state, B, M, P);
  for (int k = 0; k < max_iter; ++k) NQ_TRY(pur_resp_step(a, tr, k, max_iter, log, Q, X1, st));
  return NQ_OK;
}

}  // extern "C"
