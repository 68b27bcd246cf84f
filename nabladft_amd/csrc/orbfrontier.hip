// HOMO, LUMO and their gradients WITHOUT a solve: a projected Lanczos recurrence on what a purification (orbpurify.hip) leaves on the device.  Serves the same
// empty slots of the reference as the solver (phisnet/nn/neural_network.py:969-993), for the two frontier levels only.
//
// Per molecule: Ht (symmetric, the orthogonalised Hamiltonian), X (the projector on the n_occ lowest levels of Ht), e_min <= spec(Ht) <= e_max.  With P = X on
// the HOMO side (side 0) and P = I - X on the LUMO side (side 1):
//
//   eps_HOMO = e_min + lambda_max(P (Ht - e_min I) P),   eps_LUMO = e_max - lambda_max(P (e_max I - Ht) P):   both operators are positive semidefinite.
//
// k_front_lanczos   one 512-thread workgroup per (molecule, side), the largest molecules first.
//   start    r_i = 0.5 + ((2654435761 i + 12345) mod 2^32) / 2^32 (i: the orbital's index inside the molecule; no zero entry, not the all-ones vector),
//            v_0 = P r / |P r|
//   step j   w = P (A0 (P v_j)), A0 = Ht - e_min I or e_max I - Ht: the projector on BOTH sides of every application (rule 1 below);
//            alpha_j = v_j . w;  w -= alpha_j v_j + beta_{j-1} v_{j-1};  two passes of w -= V^T (V w) over all stored vectors (rule 2);  beta_j = |w|;
//            theta = the largest eigenvalue of the tridiagonal T_j by 513-way multisection of a Gershgorin bracket with Sturm counts (six rounds: the bracket ends
//            narrower than an ulp), taken from ABOVE, so that T_j - theta I has negative pivots only; s = its vector by the twisted factorisation (forward
//            and backward pivots, the twist where |gamma| is smallest);  stop when beta_j |s_last| <= tol (e_max - e_min), or after min(m, k_max) steps
//            (conv = 0).  v_{j+1} = w / beta_j only when the recurrence goes on: nothing is divided by a beta that ends it (m = 1, subspace dimension 1).
//   result   y = P (V^T s) / |..|;  eps = y^T Ht y with the unshifted Ht (not theta);  vec = y;  coef_mu = sum_k W[k][mu] y_k (W general; NULL: coef = y).
//   Rule 1: the Krylov space is larger than the subspace by one or more: a rounding-level leak of v_0 into the other subspace is an eigenvector of the projected
//   operator at 0 and is amplified by prod (lambda_i - 0); projecting the output alone, or stopping at dim steps, leaves residuals of 1e-7 .. 1e-3.
//   Rule 2: full reorthogonalisation, two passes, every step.
//   A level that does not exist (HOMO for n_occ <= 0, LUMO for n_occ >= m): conv = -1.  status != 0, a side that did not stop, a vanishing or non-finite
//   start vector, or a workspace slice that is too small: conv = 0.  Either way NaN in the side's own eps, res, vec and coef, and nothing else is touched.
// k_front_gram      out_gH = sum_side g_side c c^T, out_gS = -sum_side (g_side eps_side) c c^T: d eps / dH = c c^T, d eps / dS = -eps c c^T, the convention of the
//                   solver's orbital_energies.  One workgroup per 64 x 64 tile; c_i c_j is formed first, so the blocks are exactly symmetric.  conv = -1
//                   contributes 0; conv = 0 or status != 0: NaN in the molecule's blocks.
//
// Matrix rows are streamed from global memory (one row per wavefront, four rows in flight, lanes along the row: coalesced), the vectors live in LDS (at most
// 8 KB each), the Lanczos vectors in the caller-owned workspace V (2 sum_b min(m_b, k_max) m_b doubles behind vptr int64 [B+1]; side s of molecule b at
// vptr[b] + s min(m, k_max) m).  Memory-bound: plain float64 fma(), no matrix-core instruction.  No atomics; every sum has an order that depends on the
// molecule alone: bitwise reproducible, independent of the rest of the batch.  Only the layout and the status words of the state are read.  Other dimensions
// than nq_orb_init: header status -2, nothing touched.  Compiled with -ffp-contract=off like its siblings: fma() where one is wanted.
//
// Resources (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage):
//   k_front_lanczos  99 VGPRs, 0 AGPRs, 106 SGPRs, no scratch, 57536 B of LDS (seven vectors of 8 KB), one workgroup of eight wavefronts per 57 KB of LDS
//   k_front_gram     24 VGPRs, 38 SGPRs, no scratch, no LDS, 8 waves per SIMD
#include "orbbond_tiles.h"

#define NQ_FR_MAX_K 1024
#define NQ_FR_ROUNDS 6        // 513^6 > 2^54: the bracket ends narrower than an ulp of its ends
#define NQ_FR_ROWS 4          // rows a wavefront has in flight in a matrix-vector product

struct FrWork {
  double *v, *t, *w, *al, *be, *sv, *hv, *red;
};

__device__ __forceinline__ double fr_start(int i) {
  const unsigned int h = 2654435761u * (unsigned int)i + 12345u;
  return 0.5 + (double)h * (1.0 / 4294967296.0);
}

// out = Mat x for a row-major rows x cols block Mat in global memory (x [cols] and out [rows] in LDS, out != x); then by mode, for the square symmetric
// operators: 0 out = Mat x, 1 out = x - Mat x, 2 out = Mat x - c x, 3 out = c x - Mat x.  One row per wavefront, NQ_FR_ROWS rows in flight, lanes along the row.
__device__ __forceinline__ void fr_matvec(const double* __restrict__ Mat, int rows, int cols, const double* x, double* out, int mode, double c) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i0 = wave * NQ_FR_ROWS; i0 < rows; i0 += NQ_ORB_NW * NQ_FR_ROWS) {
    double s[NQ_FR_ROWS];
    const double* row[NQ_FR_ROWS];
#pragma unroll
    for (int r = 0; r < NQ_FR_ROWS; ++r) {
      s[r] = 0.0;
      row[r] = Mat + (long long)(i0 + r < rows ? i0 + r : i0) * cols;           // a surplus row reads the first one again and is dropped
    }
    int j = lane;
    for (; j + 64 < cols; j += 128) {                                          // two columns per lane and row in flight
      double a0[NQ_FR_ROWS], a1[NQ_FR_ROWS];
#pragma unroll
      for (int r = 0; r < NQ_FR_ROWS; ++r) { a0[r] = row[r][j]; a1[r] = row[r][j + 64]; }
      const double x0 = x[j], x1 = x[j + 64];
#pragma unroll
      for (int r = 0; r < NQ_FR_ROWS; ++r) s[r] = fma(a1[r], x1, fma(a0[r], x0, s[r]));
    }
    if (j < cols) {
      const double x0 = x[j];
#pragma unroll
      for (int r = 0; r < NQ_FR_ROWS; ++r) s[r] = fma(row[r][j], x0, s[r]);
    }
#pragma unroll
    for (int r = 0; r < NQ_FR_ROWS; ++r) {
      const double y = nq_wave_sum_f64(s[r]);
      if (lane == 0 && i0 + r < rows) {
        const double xi = mode == 0 ? 0.0 : x[i0 + r];
        out[i0 + r] = mode == 0 ? y : (mode == 1 ? xi - y : (mode == 2 ? y - c * xi : c * xi - y));
      }
    }
  }
  __syncthreads();
}

// x - sum_{q < n} h[q] V[q][i] (subtract) or x + sum_{q < n} h[q] V[q][i], added in the order of q; eight loads in flight
__device__ __forceinline__ double fr_combine(const double* __restrict__ V, int n, int m, int i, const double* h, double x, bool subtract) {
  int q = 0;
  for (; q + 8 <= n; q += 8) {
    double l[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) l[u] = V[(long long)(q + u) * m + i];
#pragma unroll
    for (int u = 0; u < 8; ++u) x = fma(subtract ? -h[q + u] : h[q + u], l[u], x);
  }
  for (; q < n; ++q) x = fma(subtract ? -h[q] : h[q], V[(long long)q * m + i], x);
  return x;
}

__device__ __forceinline__ double fr_dot(const double* a, const double* b, int m, double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < m; i += NQ_ORB_NT) s = fma(a[i], b[i], s);
  return orb_block_sum(s, red);
}

// the number of negative pivots of T - sigma I and the pivots' rule (a zero pivot counts as -pivmin): what the multisection and the twisted factorisation share
__device__ __forceinline__ double fr_pivot(double d, double pivmin) { return d == 0.0 ? -pivmin : d; }

// the top Ritz pair of T_n (al[0..n), be[0..n-1)); the vector, normalised, is left in f.sv; returns |s_last| (every thread: uniform)
__device__ double fr_ritz(const FrWork& f, int n, double* theta_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* dp = f.w;       // free while the residual vector sits in f.t
  double* dm = f.hv;
  double* z = f.sv;
  if (wave == 0) {
    double lo = INFINITY, hi = -INFINITY, b2 = 0.0;
    for (int i = lane; i < n; i += 64) {
      const double bl = i > 0 ? fabs(f.be[i - 1]) : 0.0, br = i < n - 1 ? fabs(f.be[i]) : 0.0;
      lo = fmin(lo, f.al[i] - bl - br);
      hi = fmax(hi, f.al[i] + bl + br);
      b2 = fmax(b2, br * br);
    }
    lo = -nq_wave_max_f64(-lo);
    hi = nq_wave_max_f64(hi);
    b2 = nq_wave_max_f64(b2);
    const double pm = 1e-300 * fmax(1.0, b2);
    if (lane == 0) { f.red[NQ_ORB_NW] = lo; f.red[NQ_ORB_NW + 1] = hi + (fabs(hi) + fabs(lo)) * 0x1p-50 + pm; f.red[NQ_ORB_NW + 2] = pm; }   // every level lies strictly below hi
  }
  __syncthreads();
  double lo = f.red[NQ_ORB_NW], hi = f.red[NQ_ORB_NW + 1];
  const double pivmin = f.red[NQ_ORB_NW + 2];
  for (int round = 0; round < NQ_FR_ROUNDS; ++round) {                // every thread one point of the bracket; all decide alike
    const double p = lo + (hi - lo) * ((double)(tid + 1) / (double)(NQ_ORB_NT + 1));
    double d = fr_pivot(f.al[0] - p, pivmin);
    int cnt = d < 0.0;
    for (int i = 1; i < n; ++i) {
      const double b = f.be[i - 1];
      d = fr_pivot((f.al[i] - p) - b * b / d, pivmin);
      cnt += d < 0.0;
    }
    const unsigned long long mask = __ballot(cnt == n);
    if (lane == 0) f.red[NQ_ORB_NW + 4 + wave] = mask ? (double)(wave * 64 + __ffsll((long long)mask) - 1) : (double)NQ_ORB_NT;
    __syncthreads();
    int first = NQ_ORB_NT;                                            // the lowest point with every level below it
#pragma unroll
    for (int w = 0; w < NQ_ORB_NW; ++w) first = min(first, (int)f.red[NQ_ORB_NW + 4 + w]);
    const double nhi = first < NQ_ORB_NT ? lo + (hi - lo) * ((double)(first + 1) / (double)(NQ_ORB_NT + 1)) : hi;
    const double nlo = first > 0 ? lo + (hi - lo) * ((double)first / (double)(NQ_ORB_NT + 1)) : lo;
    hi = nhi;
    lo = nlo;
    __syncthreads();
  }
  const double theta = hi;
  if (tid == 0) {                                                     // forward pivots: the arithmetic of the count above
    double d = fr_pivot(f.al[0] - theta, pivmin);
    dp[0] = d;
    for (int i = 1; i < n; ++i) {
      const double b = f.be[i - 1];
      d = fr_pivot((f.al[i] - theta) - b * b / d, pivmin);
      dp[i] = d;
    }
  }
  if (tid == 64) {                                                    // backward pivots
    double d = fr_pivot(f.al[n - 1] - theta, pivmin);
    dm[n - 1] = d;
    for (int i = n - 2; i >= 0; --i) {
      const double b = f.be[i];
      d = fr_pivot((f.al[i] - theta) - b * b / d, pivmin);
      dm[i] = d;
    }
  }
  __syncthreads();
  if (tid == 0) {                                                     // the twist: the smallest |gamma|, the first on ties
    int r = 0;
    double best = INFINITY;
    for (int i = 0; i < n; ++i) {
      const double g = fabs((dp[i] + dm[i]) - (f.al[i] - theta));
      if (g < best) { best = g; r = i; }
    }
    f.red[NQ_ORB_NW + 3] = (double)r;
    z[r] = 1.0;
  }
  __syncthreads();
  const int r = (int)f.red[NQ_ORB_NW + 3];
  if (tid == 0)
    for (int i = r - 1; i >= 0; --i) z[i] = -(f.be[i] * z[i + 1]) / dp[i];
  if (tid == 64)
    for (int i = r + 1; i < n; ++i) z[i] = -(f.be[i - 1] * z[i - 1]) / dm[i];
  __syncthreads();
  const double nrm = sqrt(fr_dot(z, z, n, f.red));
  for (int i = tid; i < n; i += NQ_ORB_NT) z[i] = z[i] / nrm;
  __syncthreads();
  *theta_out = theta;
  return fabs(z[n - 1]);
}

__global__ __launch_bounds__(NQ_ORB_NT) void k_front_lanczos(OrbArgs a, const double* __restrict__ Htall, const double* __restrict__ Xall, const double* shift,
                                                             const int* n_occ, const double* __restrict__ Wall, int k_max, double tol, double* Vall,
                                                             const long long* vptr, double* eps, double* vec, double* coef, int* iters, double* res, int* conv) {
  __shared__ double lds[7 * NQ_ORB_MAX_M + 2 * NQ_ORB_NW + 8];
  if (!orb_dims_ok(a)) return;
  const int tid = threadIdx.x;
  const int slot = blockIdx.x >> 1, side = blockIdx.x & 1;
  if (slot >= a.B) return;
  const int b = a.order[slot];
  if (b < 0 || b >= a.B) return;
  const int o0 = a.orb_ptr[b], m = a.orb_ptr[b + 1] - o0;
  const long long base = a.pack_ptr[b];
  if (m < 1 || m > NQ_ORB_MAX_M || o0 < 0 || o0 + m > a.M || base < 0 || base + (long long)m * m > a.P) return;   // uniform: a state overwritten since nq_orb_init
  FrWork f;
  f.v = lds; f.t = lds + NQ_ORB_MAX_M; f.w = lds + 2 * NQ_ORB_MAX_M; f.al = lds + 3 * NQ_ORB_MAX_M; f.be = lds + 4 * NQ_ORB_MAX_M; f.sv = lds + 5 * NQ_ORB_MAX_M;
  f.hv = lds + 6 * NQ_ORB_MAX_M; f.red = lds + 7 * NQ_ORB_MAX_M;
  const double nan = nq_nan_f64();
  const int no = n_occ[b], kk = m < k_max ? m : k_max;
  const long long v0 = vptr[b], vlen = vptr[b + 1] - v0;
  const bool exists = side == 0 ? no >= 1 : no < m;
  const bool usable = a.status[b] == 0 && v0 >= 0 && vlen >= 2ll * kk * m;
  double* outv = vec + (long long)side * a.M + o0;
  double* outc = coef + (long long)side * a.M + o0;
  const int oi = 2 * b + side;
  if (!exists || !usable) {                                           // uniform
    for (int i = tid; i < m; i += NQ_ORB_NT) { outv[i] = nan; outc[i] = nan; }
    if (tid == 0) { eps[oi] = nan; res[oi] = nan; iters[oi] = 0; conv[oi] = exists ? 0 : -1; }
    return;
  }
  const double* Ht = Htall + base;
  const double* X = Xall + base;
  double* V = Vall + v0 + (long long)side * kk * m;
  const double e_min = shift[2 * b], e_max = shift[2 * b + 1];
  const double thr = tol * (e_max - e_min), csh = side == 0 ? e_min : e_max;
  const int pmode = side == 0 ? 0 : 1, hmode = side == 0 ? 2 : 3;

  for (int i = tid; i < m; i += NQ_ORB_NT) f.t[i] = fr_start(i);
  __syncthreads();
  fr_matvec(X, m, m, f.t, f.w, pmode, 0.0);
  double nrm = sqrt(fr_dot(f.w, f.w, m, f.red));
  int steps = 0, done = 0;
  double resid = nan;
  if (nrm > 0.0 && nrm < INFINITY) {                                  // uniform
    for (int i = tid; i < m; i += NQ_ORB_NT) {
      const double x = f.w[i] / nrm;
      f.v[i] = x;
      V[i] = x;
    }
    __threadfence_block();
    __syncthreads();
    double beta_prev = 0.0;
    for (int j = 0; j < kk; ++j) {
      fr_matvec(X, m, m, f.v, f.t, pmode, 0.0);                          // t = P v
      fr_matvec(Ht, m, m, f.t, f.w, hmode, csh);                         // w = A0 t
      fr_matvec(X, m, m, f.w, f.t, pmode, 0.0);                          // t = P w: the new direction
      const double alpha = fr_dot(f.v, f.t, m, f.red);
      for (int i = tid; i < m; i += NQ_ORB_NT) {
        double x = f.t[i] - alpha * f.v[i];
        if (j > 0) x = x - beta_prev * V[(long long)(j - 1) * m + i];
        f.t[i] = x;
      }
      __syncthreads();
      for (int pass = 0; pass < 2; ++pass) {
        fr_matvec(V, j + 1, m, f.t, f.hv, 0, 0.0);                    // h = V t, one stored vector per wavefront
        for (int i = tid; i < m; i += NQ_ORB_NT) f.t[i] = fr_combine(V, j + 1, m, i, f.hv, f.t[i], true);
        __syncthreads();
      }
      const double beta = sqrt(fr_dot(f.t, f.t, m, f.red));
      if (tid == 0) { f.al[j] = alpha; f.be[j] = beta; }
      __syncthreads();
      double theta;
      const double slast = fr_ritz(f, j + 1, &theta);
      steps = j + 1;
      resid = beta * slast;
      if (resid <= thr) { done = 1; break; }                         // uniform: every thread read the same words
      if (j + 1 == kk) break;
      for (int i = tid; i < m; i += NQ_ORB_NT) {
        const double x = f.t[i] / beta;
        f.v[i] = x;
        V[(long long)(j + 1) * m + i] = x;
      }
      __threadfence_block();
      __syncthreads();
      beta_prev = beta;
    }
  }
  if (!done) {
    for (int i = tid; i < m; i += NQ_ORB_NT) { outv[i] = nan; outc[i] = nan; }
    if (tid == 0) { eps[oi] = nan; res[oi] = nan; iters[oi] = steps; conv[oi] = 0; }
    return;
  }
  // y = P (V^T s), normalised; the level is its Rayleigh quotient with the unshifted Ht
  for (int i = tid; i < m; i += NQ_ORB_NT) {
    f.t[i] = fr_combine(V, steps, m, i, f.sv, 0.0, false);
  }
  __syncthreads();
  fr_matvec(X, m, m, f.t, f.w, pmode, 0.0);
  nrm = sqrt(fr_dot(f.w, f.w, m, f.red));
  for (int i = tid; i < m; i += NQ_ORB_NT) f.v[i] = f.w[i] / nrm;
  __syncthreads();
  fr_matvec(Ht, m, m, f.v, f.t, 0, 0.0);
  const double level = fr_dot(f.v, f.t, m, f.red);
  for (int i = tid; i < m; i += NQ_ORB_NT) {
    outv[i] = f.v[i];
    double c = f.v[i];
    if (Wall) {
      c = fr_combine(Wall + base, m, m, i, f.v, 0.0, false);
    }
    outc[i] = c;
  }
  if (tid == 0) { eps[oi] = level; res[oi] = resid; iters[oi] = steps; conv[oi] = 1; }
}

// ---- out_gH = sum_side g c c^T, out_gS = -sum_side g eps c c^T; one workgroup per 64 x 64 tile --------------------------------------------------------------
__global__ __launch_bounds__(NQ_RS_NT) void k_front_gram(OrbArgs a, int tr, const double* g, const double* eps, const double* coef, const int* conv, double* out_gH,
                                                         double* out_gS) {
  OrbTile q;
  if (!orb_tile_mol<ORB_HDR_DIMS>(a, tr * tr, q)) return;
  const int m = q.m, ti = q.t / tr, tj = q.t - ti * tr;
  if (ti * NQ_ORB_TILE >= m || tj * NQ_ORB_TILE >= m) return;
  const int c0 = conv[2 * q.b], c1 = conv[2 * q.b + 1];
  const bool bad = q.failed || c0 == 0 || c1 == 0;
  const double g0 = g[2 * q.b], g1 = g[2 * q.b + 1], nan = nq_nan_f64();
  const double w0 = out_gS ? g0 * eps[2 * q.b] : 0.0, w1 = out_gS ? g1 * eps[2 * q.b + 1] : 0.0;
  const double* ch = coef + q.o0;
  const double* cl = coef + (long long)a.M + q.o0;
  for (int e = threadIdx.x; e < NQ_ORB_TILE * NQ_ORB_TILE; e += NQ_RS_NT) {
    const int i = ti * NQ_ORB_TILE + (e >> 6), j = tj * NQ_ORB_TILE + (e & 63);
    if (i >= m || j >= m) continue;
    const long long ij = q.base + (long long)i * m + j;
    double h = 0.0, s = 0.0;
    if (c0 > 0) {
      const double p = ch[i] * ch[j];
      h = h + g0 * p;
      s = s + w0 * p;
    }
    if (c1 > 0) {
      const double p = cl[i] * cl[j];
      h = h + g1 * p;
      s = s + w1 * p;
    }
    out_gH[ij] = bad ? nan : h;
    if (out_gS) out_gS[ij] = bad ? nan : 0.0 - s;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int nq_orb_front_lanczos(void* state, int32_t B, int32_t M, int64_t P, const double* Ht, const double* X, const double* shift, const int32_t* n_occ,
                         const double* W_or_null, int32_t k_max, double tol, double* V, const int64_t* vptr, double* eps, double* vec, double* coef, int32_t* iters,
                         double* res, int32_t* conv, void* stream) {
  NQ_TRY(orb_check_launch("nq_orb_front_lanczos", state, B, M, P, ORB_GRID_MOL, nullptr, 2));
  if (!Ht || !X || !shift || !V || !vptr || !eps || !vec || !coef || !iters || !res || !conv) return nq_fail(NQ_ERR_ARG, "nq_orb_front_lanczos: null argument");
  if (!n_occ) return nq_fail(NQ_ERR_ARG, "nq_orb_front_lanczos: n_occ is missing");
  if (k_max < 1 || k_max > NQ_FR_MAX_K) return nq_fail(NQ_ERR_ARG, "nq_orb_front_lanczos: k_max=%d outside 1..%d", k_max, NQ_FR_MAX_K);
  if (!(tol > 0.0) || !(tol < 1.0)) return nq_fail(NQ_ERR_ARG, "nq_orb_front_lanczos: tol=%g outside (0, 1)", tol);
  if (vec == coef || eps == res || (const double*)V == Ht || (const double*)V == X || (W_or_null && (const double*)V == W_or_null) || vec == V || coef == V)
    return nq_fail(NQ_ERR_ARG, "nq_orb_front_lanczos: the outputs and the workspace must be different arrays");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_front_lanczos");
  hipLaunchKernelGGL(k_front_lanczos, dim3(2 * B), dim3(NQ_ORB_NT), 0, st, orb_args(state, B, M, P), Ht, X, shift, (const int*)n_occ, W_or_null, (int)k_max, tol, V,
                     (const long long*)vptr, eps, vec, coef, (int*)iters, res, (int*)conv);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_front_gram(void* state, int32_t B, int32_t M, int64_t P, const double* g, const double* eps_or_null, const double* coef, const int32_t* conv, double* out_gH,
                      double* out_gS_or_null, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_front_gram", state, B, M, P, ORB_GRID_SQUARE, &tr));
  if (!g || !coef || !conv || !out_gH) return nq_fail(NQ_ERR_ARG, "nq_orb_front_gram: null argument");
  if (out_gS_or_null && !eps_or_null) return nq_fail(NQ_ERR_ARG, "nq_orb_front_gram: the second output out_gS needs the levels eps");
  if (out_gH == out_gS_or_null || out_gH == coef || out_gH == g || (out_gS_or_null && (out_gS_or_null == coef || out_gS_or_null == g)))
    return nq_fail(NQ_ERR_ARG, "nq_orb_front_gram: the outputs must be different arrays from each other and from the inputs");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_front_gram");
  hipLaunchKernelGGL(k_front_gram, dim3(B * tr * tr), dim3(NQ_RS_NT), 0, st, orb_args(state, B, M, P), tr, g, eps_or_null, coef, (const int*)conv, out_gH,
                     out_gS_or_null);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
