// Batched orbital energies: the generalized symmetric eigenproblem H C = S C diag(eps) of every molecule of a batch, whole state on the device.  Fills the
// slots the reference leaves empty (phisnet/nn/neural_network.py:969-993 returns orbital_energies / orbital_coefficients as zeros).
//
// One 512-thread workgroup per molecule (largest first, through `order`), one launch, float64 throughout, no atomics, no host round trip.  The m x m matrices
// live in the caller-owned state buffer in global memory (the workgroup's L1 / the XCD's L2 keep them warm; an m = 1024 matrix is 8 MiB and streams from the
// Infinity Cache); LDS holds vectors only: d, e, tau, the Householder vector v, p / w, and the (c, s) sequence of one QL sweep (which aliases v and p).
//
//   0. load     A = H, L = S from the lower triangles (j <= i) of the inputs, A mirrored to full storage.
//   1. Cholesky S = L L^T, right-looking: column j is scaled and staged in LDS, the trailing update runs one row per wavefront.  A pivot <= 0 or not finite:
//               status 1, info = its 1-based index, eps / coeff of this molecule NaN.
//   2. reduce   X = L^-1 A by forward substitution as m rank-1 row updates, A = X L^-T the same way over columns, then A = (A + A^T) / 2 exactly.
//   3. tridiag  Householder, LAPACK dsytd2 form: x = A[k][k+1:], beta = -sign(x_0) |x|, tau = (beta - x_0) / beta, v = (1, x_1: / (x_0 - beta));
//               p = tau A22 v (one row per wavefront, four rows in flight), w = p - (tau / 2)(p^T v) v, A22 -= v w^T + w v^T on both triangles with the two
//               products added in one commutative sum (this file is compiled with -ffp-contract=off), so A22 stays exactly symmetric.  A step whose x_1: is
//               zero is skipped: diagonal, zero and tridiagonal matrices reach QL untouched.  The reflectors stay in the rows they annihilated; Q^T is then
//               formed in `coeff` from the identity, last reflector first, so that step k only touches the trailing block.
//   4. QL       implicit shift (EISPACK tql2 / tqli): deflation at |e_i| <= 2^-52 (|d_i| + |d_i+1|), at most 60 sweeps per eigenvalue (status 2).  Lane 0
//               runs the scalar recurrence on d, e in LDS (operands of the next step are fetched before the current one's chain) and leaves the sweep's
//               (c, s) in LDS; after a barrier every thread carries one component down the sweep in a register: eigenvector k is ROW k of `coeff`, a
//               rotation mixes two contiguous rows, one coalesced load (issued eight rotations ahead) and one store per rotation.
//   5. finish   ascending order by rank (ties by index), C = L^-T Y by back substitution as rank-1 updates over the rows of L, the largest-magnitude
//               component of every orbital (first on ties) made positive; eps, coeff (row k = orbital k, C^T S C = I), iters, status, info.
//
// Fixed summation orders that depend on the molecule alone: results are bitwise reproducible and independent of what else shares the batch.
//
// State buffer (nq_orb_state_layout): header int32[16] {B, M, P low, P high, status (-2: a call came with other dimensions than nq_orb_init), max m},
// orb_ptr int32[B+1], pack_ptr int64[B+1], order int32[B], status int32[B] (0 solved, 1 Cholesky pivot, 2 QL sweep cap, 3 state overwritten), info int32[B], iters int32[B], eps f64[M], coeff f64[P], work f64[P], chol f64[P].
#include <algorithm>
#include <math.h>
#include <vector>

#include "orbstate.h"   // the state's parts, OrbArgs, orb_dims_ok, orb_block_sum, orb_check_dims, orb_args: shared with orbdens.hip

#define NQ_ORB_MAX_ITER 60
// dynamic LDS of k_orb_solve: d e tau v p [1024 each], 16 scalars, 8 control words
#define NQ_ORB_LDS_BYTES ((5 * NQ_ORB_MAX_M + 16) * 8 + 8 * 4)

__global__ __launch_bounds__(NQ_ORB_NT) void k_orb_solve(OrbArgs a, const void* H, int h_f64, const void* S, int s_f64) {
  extern __shared__ double sm[];
  if (!orb_dims_ok(a)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = a.order[blockIdx.x];
  const int o0 = a.orb_ptr[b], m = a.orb_ptr[b + 1] - o0;
  if (m < 1 || m > NQ_ORB_MAX_M) {   // nq_orb_init refuses such a batch: only a state overwritten since (uniform over the workgroup)
    if (tid == 0) a.status[b] = 3;
    return;
  }
  const long long base = a.pack_ptr[b];
  double* A = a.work + base;
  double* L = a.chol + base;
  double* T = a.coeff + base;   // T[k * m + i] = component i of vector k
  double* ev = a.eps + o0;
  double* d = sm;
  double* e = d + NQ_ORB_MAX_M;
  double* tau = e + NQ_ORB_MAX_M;
  double* v = tau + NQ_ORB_MAX_M;
  double* p = v + NQ_ORB_MAX_M;
  double* cs = v;               // (c, s) of one QL sweep: 2 m doubles over v and p, which the tridiagonalisation no longer needs by then
  double* sc = p + NQ_ORB_MAX_M;
  int* ctl = (int*)(sc + 16);
  int* perm = (int*)v;          // after the last sweep
  const double nan = nq_nan_f64();

  // ---- 0. load ------------------------------------------------------------------------------------------------------------------------
  for (int i = wave; i < m; i += NQ_ORB_NW)
    for (int j = lane; j <= i; j += 64) {
      const double h = nq_load_f64(H, base + (long long)i * m + j, h_f64);
      A[i * m + j] = h;
      A[j * m + i] = h;
      if (S) L[i * m + j] = nq_load_f64(S, base + (long long)i * m + j, s_f64);
    }
  __syncthreads();

  if (S) {
    // ---- 1. Cholesky ------------------------------------------------------------------------------------------------------------------
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
      for (int k = tid; k < m; k += NQ_ORB_NT) ev[k] = nan;
      for (int idx = tid; idx < m * m; idx += NQ_ORB_NT) T[idx] = nan;
      if (tid == 0) { a.status[b] = 1; a.info[b] = fail; a.iters[b] = 0; }
      return;
    }
    // ---- 2. A = L^-1 A L^-T -------------------------------------------------------------------------------------------------------------
    for (int k = 0; k < m; ++k) {        // X = L^-1 A: row k is final once divided, then leaves every row below it
      const double lkk = L[k * m + k];
      for (int c = tid; c < m; c += NQ_ORB_NT) {
        const double x = A[k * m + c] / lkk;
        A[k * m + c] = x;
        v[c] = x;
      }
      for (int i = k + 1 + tid; i < m; i += NQ_ORB_NT) p[i] = L[i * m + k];
      __syncthreads();
      for (int i = k + 1 + wave; i < m; i += NQ_ORB_NW) {
        const double li = p[i];
        for (int c = lane; c < m; c += 64) A[i * m + c] = fma(-li, v[c], A[i * m + c]);
      }
      __syncthreads();
    }
    for (int k = 0; k < m; ++k) {        // A = X L^-T: the same over columns
      const double lkk = L[k * m + k];
      for (int r = tid; r < m; r += NQ_ORB_NT) {
        const double x = A[r * m + k] / lkk;
        A[r * m + k] = x;
        v[r] = x;
      }
      for (int c = k + 1 + tid; c < m; c += NQ_ORB_NT) p[c] = L[c * m + k];
      __syncthreads();
      for (int r = wave; r < m; r += NQ_ORB_NW) {
        const double xr = v[r];
        for (int c = k + 1 + lane; c < m; c += 64) A[r * m + c] = fma(-xr, p[c], A[r * m + c]);
      }
      __syncthreads();
    }
    for (int i = wave; i < m; i += NQ_ORB_NW)
      for (int j = lane; j <= i; j += 64) {
        const double s = 0.5 * (A[i * m + j] + A[j * m + i]);
        A[i * m + j] = s;
        A[j * m + i] = s;
      }
    __syncthreads();
  }

  // ---- 3. Householder tridiagonalisation --------------------------------------------------------------------------------------------------
  for (int k = 0; k + 1 < m; ++k) {
    const int n = m - k - 1;
    double* row = A + k * m + k + 1;
    double* sub = A + (k + 1) * m + k + 1;
    for (int j = tid; j < n; j += NQ_ORB_NT) v[j] = row[j];
    __syncthreads();
    if (wave == 0) {
      double mx = 0.0;
      for (int j = 1 + lane; j < n; j += 64) mx = fmax(mx, fabs(v[j]));
      mx = nq_wave_max_f64(mx);
      double tk = 0.0, ek = v[0], scal = 0.0;
      if (mx != 0.0) {
        const double alpha = v[0], amx = fmax(mx, fabs(alpha));
        double ss = 0.0;
        for (int j = lane; j < n; j += 64) {
          const double t = v[j] / amx;
          ss += t * t;
        }
        ss = nq_wave_sum_f64(ss);
        const double nrm = amx * sqrt(ss);
        const double beta = alpha >= 0.0 ? -nrm : nrm;
        tk = (beta - alpha) / beta;
        scal = 1.0 / (alpha - beta);
        ek = beta;
      }
      if (lane == 0) { sc[0] = tk; sc[1] = scal; e[k] = ek; d[k] = A[k * m + k]; tau[k] = tk; }
    }
    __syncthreads();
    const double tk = sc[0];
    if (tk == 0.0) continue;             // x_1: is zero already (uniform: read from LDS); the barrier above separates this read from the next write
    const double scal = sc[1];
    for (int j = tid; j < n; j += NQ_ORB_NT) {
      const double x = j == 0 ? 1.0 : v[j] * scal;
      v[j] = x;
      if (j) row[j] = x;                 // the reflector stays in the row it annihilated
    }
    __syncthreads();
    for (int i0 = wave * 4; i0 < n; i0 += NQ_ORB_NW * 4) {   // p = tau A22 v: four rows in flight per wavefront
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      for (int j = lane; j < n; j += 64) {
        const double vj = v[j];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (i0 + u < n) acc[u] = fma(sub[(i0 + u) * m + j], vj, acc[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = nq_wave_sum_f64(acc[u]);
        if (lane == 0 && i0 + u < n) p[i0 + u] = tk * acc[u];
      }
    }
    __syncthreads();
    if (wave == 0) {
      double s = 0.0;
      for (int i = lane; i < n; i += 64) s = fma(p[i], v[i], s);
      s = nq_wave_sum_f64(s);
      if (lane == 0) sc[2] = -0.5 * tk * s;
    }
    __syncthreads();
    const double al = sc[2];
    for (int i = tid; i < n; i += NQ_ORB_NT) p[i] = fma(al, v[i], p[i]);   // w
    __syncthreads();
    for (int i = wave; i < n; i += NQ_ORB_NW) {
      const double vi = v[i], wi = p[i];
      for (int j = lane; j < n; j += 64) sub[i * m + j] -= vi * p[j] + wi * v[j];   // (i, j) and (j, i) add the same two products
    }
    __syncthreads();
  }
  if (tid == 0) { d[m - 1] = A[(m - 1) * m + m - 1]; e[m - 1] = 0.0; }

  // ---- Q^T in T: the identity times H_{m-3} ... H_0, each on the right (a row operation) ----------------------------------------------------------
  for (int i = wave; i < m; i += NQ_ORB_NW)
    for (int j = lane; j < m; j += 64) T[i * m + j] = i == j ? 1.0 : 0.0;
  __syncthreads();
  for (int k = m - 3; k >= 0; --k) {
    const double tk = tau[k];
    if (tk == 0.0) continue;             // uniform
    const int n = m - k - 1;
    const double* row = A + k * m + k + 1;
    for (int j = tid; j < n; j += NQ_ORB_NT) v[j] = j == 0 ? 1.0 : row[j];
    __syncthreads();
    for (int i0 = wave * 4; i0 < n; i0 += NQ_ORB_NW * 4) {
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      for (int j = lane; j < n; j += 64) {
        const double vj = v[j];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (i0 + u < n) acc[u] = fma(T[(k + 1 + i0 + u) * m + k + 1 + j], vj, acc[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = tk * nq_wave_sum_f64(acc[u]);
      for (int j = lane; j < n; j += 64) {
        const double vj = v[j];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (i0 + u < n) T[(k + 1 + i0 + u) * m + k + 1 + j] = fma(-acc[u], vj, T[(k + 1 + i0 + u) * m + k + 1 + j]);
      }
    }
    __syncthreads();
  }

  // ---- 4. implicit-shift QL ---------------------------------------------------------------------------------------------------------------
  if (tid == 0) { ctl[0] = 0; ctl[1] = 0; }
  __syncthreads();
  int total = 0, qlstat = 0;
  for (;;) {
    if (tid == 0) {
      int l = ctl[0], it = ctl[1], flag = 0, lo = 0, hi = 0;
      for (;;) {
        if (l >= m) { flag = 0; break; }
        int mm = l;
        for (; mm < m - 1; ++mm) {
          const double dd = fabs(d[mm]) + fabs(d[mm + 1]);
          if (fabs(e[mm]) <= NQ_F64_EPS * dd) break;
        }
        if (mm == l) { ++l; it = 0; continue; }
        if (it == NQ_ORB_MAX_ITER) { flag = 2; break; }
        ++it;
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
        double r = hypot(g, 1.0);
        g = d[mm] - d[l] + e[l] / (g + copysign(r, g));
        double s = 1.0, c = 1.0, pp = 0.0;
        double ei = e[mm - 1], di = d[mm - 1], di1 = d[mm];   // e_i, d_i, d_{i+1} of the step at hand
        int i = mm - 1;
        lo = l; hi = mm;
        for (; i >= l; --i) {
          double en = 0.0, dn = 0.0;
          if (i > l) { en = e[i - 1]; dn = d[i - 1]; }       // the next step's operands: nothing below writes them
          const double f = s * ei, bb = c * ei;
          r = hypot(f, g);
          e[i + 1] = r;
          if (r == 0.0) {                                    // recover from underflow: the sweep ends here
            d[i + 1] = di1 - pp;
            e[mm] = 0.0;
            lo = i + 1;
            break;
          }
          s = f / r;
          c = g / r;
          g = di1 - pp;
          r = (di - g) * s + 2.0 * c * bb;
          pp = s * r;
          d[i + 1] = g + pp;
          g = c * r - bb;
          cs[2 * i] = c;
          cs[2 * i + 1] = s;
          di1 = di; di = dn; ei = en;
        }
        if (i < l) { d[l] = di1 - pp; e[l] = g; e[mm] = 0.0; }
        flag = 1;
        break;
      }
      ctl[0] = l; ctl[1] = it; ctl[3] = flag; ctl[4] = lo; ctl[5] = hi;
    }
    __syncthreads();
    const int flag = ctl[3];
    if (flag == 1) {
      const int lo = ctl[4], hi = ctl[5];
      for (int x = tid; x < m; x += NQ_ORB_NT) {
        double g = T[hi * m + x];
        double buf[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) buf[u] = hi - 1 - u >= lo ? T[(hi - 1 - u) * m + x] : 0.0;
        for (int i = hi - 1; i >= lo; i -= 8) {
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int r = i - u;
            if (r >= lo) {
              const double t = buf[u];
              if (r - 8 >= lo) buf[u] = T[(r - 8) * m + x];
              const double c = cs[2 * r], s = cs[2 * r + 1];
              T[(r + 1) * m + x] = s * t + c * g;
              g = c * t - s * g;
            }
          }
        }
        T[lo * m + x] = g;
      }
      ++total;
    }
    __syncthreads();
    if (flag != 1) { qlstat = flag; break; }
  }

  // ---- 5. order, back-transform, sign ------------------------------------------------------------------------------------------------------
  for (int i = tid; i < m; i += NQ_ORB_NT) perm[i] = i;   // the identity first, so that NaNs leave it in range
  __syncthreads();
  nq_rank_perm<NQ_ORB_NT, NQ_ORB_MAX_M / NQ_ORB_NT>(d, m, perm);
  for (int k = tid; k < m; k += NQ_ORB_NT) ev[k] = d[perm[k]];
  for (int k = wave; k < m; k += NQ_ORB_NW) {            // sorted rows into the matrix's storage, which nothing needs any more
    const double* src = T + perm[k] * m;
    for (int i = lane; i < m; i += 64) A[k * m + i] = src[i];
  }
  __syncthreads();
  if (S) {
    for (int i = m - 1; i >= 0; --i) {                   // every row y of A: L^T c = y; component i is final once divided, then leaves the components before it
      const double lii = L[i * m + i];
      for (int k = tid; k < m; k += NQ_ORB_NT) {
        const double x = A[k * m + i] / lii;
        A[k * m + i] = x;
        p[k] = x;
      }
      for (int j = tid; j < i; j += NQ_ORB_NT) tau[j] = L[i * m + j];
      __syncthreads();
      for (int k = wave; k < m; k += NQ_ORB_NW) {
        const double wk = p[k];
        for (int j = lane; j < i; j += 64) A[k * m + j] = fma(-wk, tau[j], A[k * m + j]);
      }
      __syncthreads();
    }
  }
  for (int k = wave; k < m; k += NQ_ORB_NW) {
    double best = -1.0, val = 0.0;
    int at = m;
    for (int i = lane; i < m; i += 64) {
      const double x = A[k * m + i];
      if (fabs(x) > best) { best = fabs(x); val = x; at = i; }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const double ob = __shfl_xor(best, s, 64), ov = __shfl_xor(val, s, 64);
      const int oa = __shfl_xor(at, s, 64);
      if (ob > best || (ob == best && oa < at)) { best = ob; val = ov; at = oa; }
    }
    const double sg = val < 0.0 ? -1.0 : 1.0;
    for (int i = lane; i < m; i += 64) T[k * m + i] = sg * A[k * m + i];
  }
  if (tid == 0) { a.status[b] = qlstat; a.info[b] = 0; a.iters[b] = total; }
}

// one thread per molecule
__global__ void k_orb_frontier(OrbArgs a, const int* n_occ, double* homo, double* lumo, double* gap) {
  if (!orb_dims_ok(a)) return;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const int o0 = a.orb_ptr[b], m = a.orb_ptr[b + 1] - o0, no = n_occ[b];
  const double nan = nq_nan_f64();
  double h = nan, l = nan;
  if (no >= 1 && no <= m) {
    h = a.eps[o0 + no - 1];
    if (no < m) l = a.eps[o0 + no];
  }
  homo[b] = h;
  lumo[b] = l;
  gap[b] = l - h;
}

// one workgroup per molecule: a (predicted) against t (target); the full symmetric S goes through a's work buffer
__global__ __launch_bounds__(NQ_ORB_NT) void k_orb_compare(OrbArgs a, OrbArgs t, const void* S, int s_f64, const int* n_occ, double* out) {
  __shared__ double v[NQ_ORB_MAX_M];
  __shared__ double red[NQ_ORB_NW];
  const bool oka = orb_dims_ok(a), okt = orb_dims_ok(t);
  if (!oka || !okt) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = a.order[blockIdx.x], B = a.B;
  const int o0 = a.orb_ptr[b], m = a.orb_ptr[b + 1] - o0, no = n_occ[b];
  const double nan = nq_nan_f64();
  if (m < 1 || m > NQ_ORB_MAX_M || no < 1 || no > m || t.orb_ptr[b] != o0 || t.orb_ptr[b + 1] != o0 + m) {   // uniform
    if (tid < 7) out[(long)tid * B + b] = nan;
    return;
  }
  const long long base = a.pack_ptr[b];
  const double* ea = a.eps + o0;
  const double* et = t.eps + o0;
  const double* ca = a.coeff + base;
  const double* ct = t.coeff + base;
  double* W = a.work + base;
  double so = 0.0, sa = 0.0;
  for (int k = tid; k < m; k += NQ_ORB_NT) {
    const double df = fabs(ea[k] - et[k]);
    sa += df;
    if (k < no) so += df;
  }
  so = orb_block_sum(so, red);
  sa = orb_block_sum(sa, red);
  if (S) {
    for (int i = wave; i < m; i += NQ_ORB_NW)
      for (int j = lane; j <= i; j += 64) {
        const double s = nq_load_f64(S, base + (long long)i * m + j, s_f64);
        W[i * m + j] = s;
        W[j * m + i] = s;
      }
    __syncthreads();
  }
  double sim = 0.0, simmin = INFINITY;   // thread 0's
  for (int k = 0; k < no; ++k) {
    double acc = 0.0;
    if (S) {
      for (int i = tid; i < m; i += NQ_ORB_NT) v[i] = ct[k * m + i];
      __syncthreads();
      for (int i0 = wave * 4; i0 < m; i0 += NQ_ORB_NW * 4) {
        double dot[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = lane; j < m; j += 64) {
          const double vj = v[j];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (i0 + u < m) dot[u] = fma(W[(i0 + u) * m + j], vj, dot[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          dot[u] = nq_wave_sum_f64(dot[u]);
          if (i0 + u < m) acc = fma(ca[k * m + i0 + u], dot[u], acc);   // the same in every lane
        }
      }
    } else {
      for (int i = tid; i < m; i += NQ_ORB_NT) acc = fma(ca[k * m + i], ct[k * m + i], acc);
      acc = nq_wave_sum_f64(acc);
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) {
      double r = 0.0;
      for (int w = 0; w < NQ_ORB_NW; ++w) r += red[w];
      r = fabs(r);
      sim += r;
      simmin = fmin(simmin, r);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double ha = ea[no - 1], ht = et[no - 1];
    const double la = no < m ? ea[no] : nan, lt = no < m ? et[no] : nan;
    out[0L * B + b] = so / (double)no;
    out[1L * B + b] = sa / (double)m;
    out[2L * B + b] = sim / (double)no;
    out[3L * B + b] = fabs(ha - ht);
    out[4L * B + b] = fabs(la - lt);
    out[5L * B + b] = fabs((la - ha) - (lt - ht));
    out[6L * B + b] = simmin;
  }
}

extern "C" {

size_t nq_orb_state_bytes(int32_t B, int32_t M, int64_t P) {
  return orb_check_dims(B, M, P) == NQ_OK ? orb_layout(B, M, P).total : 0;
}

int nq_orb_state_layout(int32_t B, int32_t M, int64_t P, size_t* offsets_host) {
  if (!offsets_host) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(orb_check_dims(B, M, P));
  return nq_state_offsets(orb_layout(B, M, P), offsets_host);
}

int nq_orb_init(void* state, size_t state_bytes, const int32_t* orb_ptr_host, int32_t B, int32_t M, int64_t P, int32_t* plan_host, void* stream) {
  if (!state || !orb_ptr_host || !plan_host) return nq_fail(NQ_ERR_ARG, "null argument");
  if (B >= 1) {   // the size limit comes before every other complaint about the dimensions
    for (int b = 0; b < B; ++b) {
      const long m = (long)orb_ptr_host[b + 1] - orb_ptr_host[b];
      if (m > NQ_ORB_MAX_M) return nq_fail(NQ_ERR_MOL_TOO_LARGE, "nq_orb_init: molecule %d has %ld orbitals, the limit is %d", b, m, NQ_ORB_MAX_M);
    }
  }
  NQ_TRY(orb_check_dims(B, M, P));
  const OrbLayout L = orb_layout(B, M, P);
  NQ_TRY(nq_state_check("nq_orb_init:", state, state_bytes, L.total));
  if (orb_ptr_host[0] != 0 || orb_ptr_host[B] != M) return nq_fail(NQ_ERR_ARG, "nq_orb_init: orb_ptr must run from 0 to M=%d", M);
  // the host-built parts are contiguous from the header up to order: one host image, one copy
  std::vector<char> img(L.part[OP_STATUS], 0);
  int* hdr = (int*)(img.data() + L.part[OP_HDR]);
  int* orb_ptr = (int*)(img.data() + L.part[OP_ORB_PTR]);
  long long* pack_ptr = (long long*)(img.data() + L.part[OP_PACK_PTR]);
  int* order = (int*)(img.data() + L.part[OP_ORDER]);
  long long pp = 0;
  int max_m = 0;
  for (int b = 0; b < B; ++b) {
    const int m = orb_ptr_host[b + 1] - orb_ptr_host[b];
    if (m < 1) return nq_fail(NQ_ERR_ARG, "nq_orb_init: molecule %d has %d orbitals", b, m);
    orb_ptr[b] = orb_ptr_host[b];
    pack_ptr[b] = pp;
    pp += (long long)m * m;
    if (pp > P) return nq_fail(NQ_ERR_ARG, "nq_orb_init: the packed matrices need more than P=%lld entries", (long long)P);
    order[b] = b;
    if (m > max_m) max_m = m;
  }
  if (pp != P) return nq_fail(NQ_ERR_ARG, "nq_orb_init: orb_ptr packs to P=%lld entries, the call said P=%lld", pp, (long long)P);
  orb_ptr[B] = M; pack_ptr[B] = P;
  std::stable_sort(order, order + B, [&](int x, int y) { return orb_ptr_host[x + 1] - orb_ptr_host[x] > orb_ptr_host[y + 1] - orb_ptr_host[y]; });   // largest first
  hdr[OH_B] = B; hdr[OH_M] = M; nq_split64(P, hdr + OH_PLO); hdr[OH_MAXM] = max_m;
  plan_host[0] = max_m; plan_host[1] = NQ_ORB_LDS_BYTES;
  hipStream_t st = (hipStream_t)stream;
  NQ_TRY(nq_state_upload(state, img.data(), L.part[OP_STATUS], st));
  NQ_HIP(hipMemsetAsync((char*)state + L.part[OP_STATUS], 0, L.part[OP_COEFF] - L.part[OP_STATUS], st));   // status, info, iters, eps
  return NQ_OK;
}

int nq_orb_solve(void* state, int32_t B, int32_t M, int64_t P, const void* H, int32_t h_f64, const void* S, int32_t s_f64, void* stream) {
  if (!state || !H) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(orb_check_dims(B, M, P));
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, S ? "orb_solve_general" : "orb_solve_standard");
  hipLaunchKernelGGL(k_orb_solve, dim3(B), dim3(NQ_ORB_NT), NQ_ORB_LDS_BYTES, st, orb_args(state, B, M, P), H, h_f64, S, s_f64);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_frontier(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, double* out_homo, double* out_lumo, double* out_gap, void* stream) {
  if (!state || !n_occ || !out_homo || !out_lumo || !out_gap) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(orb_check_dims(B, M, P));
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_frontier");
  hipLaunchKernelGGL(k_orb_frontier, dim3(nq_cdiv(B, 256)), dim3(256), 0, st, orb_args(state, B, M, P), n_occ, out_homo, out_lumo, out_gap);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_compare(void* state_pred, void* state_target, int32_t B, int32_t M, int64_t P, const void* S, int32_t s_f64, const int32_t* n_occ, double* out,
                   void* stream) {
  if (!state_pred || !state_target || !n_occ || !out) return nq_fail(NQ_ERR_ARG, "null argument");
  NQ_TRY(orb_check_dims(B, M, P));
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_compare");
  hipLaunchKernelGGL(k_orb_compare, dim3(B), dim3(NQ_ORB_NT), 0, st, orb_args(state_pred, B, M, P), orb_args(state_target, B, M, P), S, s_f64, n_occ, out);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
