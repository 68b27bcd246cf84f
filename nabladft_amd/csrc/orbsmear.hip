// Fermi-Dirac occupations and the response of the smeared density matrix D = sum_k F_k c_k c_k^T to H and S, after a batched solve of H C = S C diag(eps)
// (orbitals.hip).  F_k = 2 f((eps_k - mu) / kT) with the chemical potential mu fixed by sum_k F_k = n_elec: D is a smooth function of H and S also where
// levels coincide or cross, and its response is a matrix of divided differences of F that is evaluated WITHOUT dividing by a difference of orbital energies
// (orbsmear_math.h).  Serves the same empty slots of the reference as the solver (phisnet/nn/neural_network.py:969-993).
//
//   k_orb_fermi        one 512-thread workgroup per molecule: mu by a safeguarded Newton iteration that keeps a bracket, then occ = F, docc = dF/d eps at fixed
//                      mu (<= 0) and the entropy -2 sum (f ln f + (1 - f) ln(1 - f)).  info: 0 ok; 1: n_elec outside (0, 2m), kT not a positive finite number,
//                      non-finite eps or a failed solve -- NaN in the molecule's outputs.
//   (T = Gs C          is nq_orb_resp_project of orbresp.hip with n_occ = m and occ_ptr = pack_ptr)
//   k_orb_smear_mo     W[k][i] = sum_mu Ct[k][mu] T[mu][i] over all orbital pairs and its epilogue: off the diagonal A_H = K o W and (TWO) A_S = KS o W,
//                      K_ki the divided difference of F, KS_ki = -((F_k + F_i) / 2 + (eps_k + eps_i) / 2 K_ki); the diagonal goes to wdiag [M] = W_kk
//   k_orb_smear_diag   one 512-thread workgroup per molecule: gF_k = g_occ_k + g_ent x_k + W_kk, p_k = F'_k / sum F' (evaluated as a softmax of -|x|, so that a
//                      sum of derivatives that underflows inside a wide gap divides nothing), e_k = g_eps_k + F'_k (gF_k - sum_j p_j gF_j) + p_k g_mu;
//                      A_H[k][k] = e_k, A_S[k][k] = -eps_k e_k - F_k W_kk
//   k_orb_smear_back   Rt_X[i][mu] = sum_k A_X[k][i] Ct[k][mu] over all k; X = H alone, or H and S from the same loads of Ct
//   (C A C^T           is nq_orb_syr2k of orbresp.hip on Rt with n_occ = m: exactly symmetric)
//
// The products are those of orbresp.hip (orbresp_tiles.h): one 256-thread workgroup per (molecule, 64 orbitals), which walks the 64 x 64 output tiles of the
// other side itself; v_mfma_f64_16x16x4_f64 on operands staged through padded LDS; operands beyond m are zero, stores are masked.  No atomics, fixed summation
// orders: bitwise reproducible, independent of the rest of the batch.  status != 0: NaN in the molecule's own block of every output.
//
// Compiled with -ffp-contract=off like orbresp.hip.
#include "orbresp_tiles.h"
#include "orbsmear_math.h"

#define NQ_SM_KT_MAX 1e300    // a larger kT (inf and NaN too) is refused with info = 1: kT (log(2m / n_elec) + 2) must stay finite for the bracket of mu
#define NQ_SM_MAX_ITER 4096  // a bisection step at least every third iteration: 3 x (the 1075 halvings from the widest bracket of doubles to one ulp) fits

// ---- the chemical potential and the occupations ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_ORB_NT) void k_orb_fermi(OrbArgs a, const double* n_elec, const double* kT_in, double* out_mu, double* out_occ, double* out_docc,
                                                         double* out_ent, int* out_info) {
  __shared__ double red[NQ_ORB_NW];
  if (!orb_kind_ok(a, false)) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  int o0, m;
  long long base;
  bool failed;
  if (!orb_mol(a, b, o0, m, base, failed)) return;               // uniform: a state overwritten since nq_orb_init
  const double n = n_elec[b], kT = kT_in[b];
  const double nan = nq_nan_f64();
  // at most two levels per thread (m <= 1024 = 2 x 512)
  const int k0 = tid, k1 = tid + NQ_ORB_NT;
  const bool h0 = k0 < m, h1 = k1 < m;
  const double e0 = h0 ? a.eps[o0 + k0] : 0.0, e1 = h1 ? a.eps[o0 + k1] : 0.0;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double bad = ((h0 && !isfinite(e0)) || (h1 && !isfinite(e1))) ? 1.0 : 0.0;
  bad = orb_block_sum(bad, red);
  const bool ok = !failed && bad == 0.0 && kT > 0.0 && kT < NQ_SM_KT_MAX && n > 0.0 && n < 2.0 * (double)m;   // NaN n_elec fails both comparisons
  if (!ok) {
    if (h0) out_occ[o0 + k0] = nan, out_docc[o0 + k0] = nan;
    if (h1) out_occ[o0 + k1] = nan, out_docc[o0 + k1] = nan;
    if (tid == 0) out_mu[b] = nan, out_ent[b] = nan, out_info[b] = 1;
    return;
  }
  const double emax = orb_block_max(fmax(h0 ? e0 : -inf, h1 ? e1 : -inf), red);
  const double emin = -orb_block_max(fmax(h0 ? -e0 : -inf, h1 ? -e1 : -inf), red);
  // the bracket: below lo every F_k <= 2 e^-x sums to less than n_elec / e^2, above hi the holes sum to less than (2m - n_elec) / e^2
  double lo = emin - kT * (log(2.0 * (double)m / n) + 2.0), hi = emax + kT * (log(2.0 * (double)m / (2.0 * (double)m - n)) + 2.0);
  if (!(lo < emin)) lo = nextafter(emin, -inf);                  // kT below the spacing of doubles at eps: x is then clamped to -+1e300 one ulp away
  if (!(hi > emax)) hi = nextafter(emax, inf);
  double rlo = -inf, rhi = inf;                                  // the residuals sum F - n_elec at the ends, as far as known
  double mu = lo + 0.5 * (hi - lo), wprev = inf;
  bool exact = false;
  int slow = 0;
  for (int it = 0; it < NQ_SM_MAX_ITER; ++it) {                  // everything below is uniform over the workgroup: the sums end with the same bits in every thread
    // The residual sum F - n_elec as particles above mu minus holes below mu minus (n_elec - 2 x the levels below mu): the tails are summed among themselves,
    // so inside a gap much wider than kT, where sum F itself rounds to an integer over a whole interval of mu, the residual still tells which way mu lies.
    double sf = 0.0, sd = 0.0, below = 0.0;
    if (h0) {
      const double x = nq_smear_x(e0, mu, kT), e = nq_smear_e(x);
      sf = nq_smear_tail_e(x, e);
      sd = -nq_smear_docc_e(e, kT);
      below = x > 0.0 ? 0.0 : 1.0;
    }
    if (h1) {
      const double x = nq_smear_x(e1, mu, kT), e = nq_smear_e(x);
      sf = sf + nq_smear_tail_e(x, e);
      sd = sd - nq_smear_docc_e(e, kT);
      below = below + (x > 0.0 ? 0.0 : 1.0);
    }
    sf = orb_block_sum(sf, red);
    sd = orb_block_sum(sd, red);                                 // d (sum F) / d mu >= 0
    below = orb_block_sum(below, red);                           // a count: exact
    const double r = sf - (n - 2.0 * below);
    if (r == 0.0) {
      exact = true;
      break;
    }
    if (r < 0.0) lo = mu, rlo = r;
    else hi = mu, rhi = r;
    const double w = hi - lo, mid = lo + 0.5 * w;
    if (!(mid > lo && mid < hi)) break;                          // the bracket is one ulp wide
    slow = w > 0.5 * wprev ? slow + 1 : 0;                       // the bracket did not halve: Newton keeps arriving from the same side
    wprev = w;
    const double step = -r / sd;
    double c = slow == 0 ? mu + step : (slow == 1 ? mu + 2.0 * step : mid);   // Newton; Newton overshot to catch the root from the other side; bisection
    if (slow >= 2) slow = 0;
    if (!(c > lo && c < hi)) c = mid;                            // also NaN and inf (sd underflowed inside a gap)
    mu = c;
  }
  if (!exact) mu = fabs(rlo) <= fabs(rhi) ? lo : hi;             // the end with the smaller residual
  double ent = 0.0;
  if (h0) {
    const double x = nq_smear_x(e0, mu, kT), e = nq_smear_e(x);
    out_occ[o0 + k0] = nq_smear_occ_e(x, e);
    out_docc[o0 + k0] = nq_smear_docc_e(e, kT);
    ent = nq_smear_entropy(x);
  }
  if (h1) {
    const double x = nq_smear_x(e1, mu, kT), e = nq_smear_e(x);
    out_occ[o0 + k1] = nq_smear_occ_e(x, e);
    out_docc[o0 + k1] = nq_smear_docc_e(e, kT);
    ent = ent + nq_smear_entropy(x);
  }
  ent = orb_block_sum(ent, red);
  if (tid == 0) out_mu[b] = mu, out_ent[b] = ent, out_info[b] = 0;
}

// ---- which molecule and 64 orbitals a workgroup of the two products serves; false: exit (uniform over the workgroup) --------------------------------------------
__device__ __forceinline__ bool sm_mol(const OrbArgs& a, int tr, OrbTile& q) {
  if (!orb_tile_mol<ORB_HDR_SOLVE>(a, tr, q)) return false;
  if (q.t * NQ_ORB_TILE >= q.m) return false;                    // two early returns, not one `return a && b`: k_orb_smear_back's register count hangs on it
  return true;                                                   // (profiles/orbital_refactor_resources.txt)
}

// ---- W = C^T T and the divided differences -------------------------------------------------------------------------------------------------------------------------
template <bool TWO>
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_smear_mo(OrbArgs a, int tr, const double* mu_in, const double* kT_in, const double* T, double* A_H, double* A_S,
                                                           double* wdiag) {
  __shared__ double lds[3 * NQ_RS_TILE];
  OrbTile q;
  if (!sm_mol(a, tr, q)) return;
  const int m = q.m, i0 = q.t * NQ_ORB_TILE;                     // the workgroup's 64 rows of W; it walks the columns itself
  const double* Ct = a.coeff + q.base;
  const double* eps = a.eps + q.o0;
  const double mu = mu_in[q.b], kT = kT_in[q.b];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const double nan = nq_nan_f64();
  double xi[4], ei[4], Fi[4], epi[4];                            // this thread's four rows
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + wave * 16 + lk + 4 * r;
    epi[r] = i < m ? eps[i] : 0.0;
    xi[r] = nq_smear_x(epi[r], mu, kT);
    ei[r] = nq_smear_e(xi[r]);
    Fi[r] = nq_smear_occ_e(xi[r], ei[r]);
  }
  double* X0 = A_H + q.base;
  double* X1 = TWO ? A_S + q.base : nullptr;
  for (int j0 = 0; j0 < m; j0 += NQ_ORB_TILE) {                  // uniform over the workgroup
    orb_f64x4 acc0[4], acc1[4];
    rs_zero(acc0);
    rs_zero(acc1);
    if (!q.failed) rs_gemm<true, false, false>(Ct, nullptr, m, T + q.base, m, 0, m, i0, m, j0, m, lds, acc0, acc1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = j0 + s * 16 + lc;
      if (j >= m) continue;
      const double epj = eps[j], xj = nq_smear_x(epj, mu, kT), ej = nq_smear_e(xj), Fj = nq_smear_occ_e(xj, ej);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wave * 16 + lk + 4 * r;
        if (i >= m) continue;
        const double w = acc0[s][r];
        if (i == j) {
          wdiag[q.o0 + i] = q.failed ? nan : w;                  // the diagonal of A is k_orb_smear_diag's
          continue;
        }
        const double K = nq_smear_K_e(xi[r], ei[r], xj, ej, kT);
        X0[(long long)i * m + j] = q.failed ? nan : K * w;
        if (TWO) X1[(long long)i * m + j] = q.failed ? nan : nq_smear_KS_e(xi[r], ei[r], xj, ej, Fi[r], Fj, epi[r], epj, kT) * w;
      }
    }
  }
}

// ---- the diagonals of A_H and A_S -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_ORB_NT) void k_orb_smear_diag(OrbArgs a, const double* mu_in, const double* kT_in, const double* occ, const double* docc,
                                                              const double* wdiag, const double* g_eps, const double* g_occ, const double* g_mu,
                                                              const double* g_ent, double* A_H, double* A_S) {
  __shared__ double red[NQ_ORB_NW];
  if (!orb_kind_ok(a, false)) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  int o0, m;
  long long base;
  bool failed;
  if (!orb_mol(a, b, o0, m, base, failed)) return;
  const double mu = mu_in[b], kT = kT_in[b], gm = g_mu ? g_mu[b] : 0.0, ge = g_ent ? g_ent[b] : 0.0;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double x[2], gF[2], u[2];
  double amin = inf;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int k = tid + s * NQ_ORB_NT;
    x[s] = gF[s] = u[s] = 0.0;
    if (k < m) {
      x[s] = nq_smear_x(a.eps[o0 + k], mu, kT);
      gF[s] = ((g_occ ? g_occ[o0 + k] : 0.0) + ge * x[s]) + wdiag[o0 + k];
      amin = fmin(amin, fabs(x[s]));
    }
  }
  amin = -orb_block_max(-amin, red);
  double su = 0.0, sg = 0.0;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int k = tid + s * NQ_ORB_NT;
    if (k < m) {
      const double q = 1.0 + nq_smear_e(x[s]);
      u[s] = exp(-(fabs(x[s]) - amin)) / (q * q);                // F'_k up to the factor -(2 / kT) e^-amin: the level nearest to mu has u >= 1 / 4
      su = su + u[s];
      sg = sg + u[s] * gF[s];
    }
  }
  su = orb_block_sum(su, red);
  sg = orb_block_sum(sg, red);
  const double gbar = sg / su;
  const double nan = nq_nan_f64();
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int k = tid + s * NQ_ORB_NT;
    if (k < m) {
      const double e = ((g_eps ? g_eps[o0 + k] : 0.0) + docc[o0 + k] * (gF[s] - gbar)) + (u[s] / su) * gm;
      const long long d = base + (long long)k * m + k;
      A_H[d] = failed ? nan : e;
      if (A_S) A_S[d] = failed ? nan : -(a.eps[o0 + k] * e) - occ[o0 + k] * wdiag[o0 + k];
    }
  }
}

// ---- Rt = A^T C^T ----------------------------------------------------------------------------------------------------------------------------------------------------
template <bool TWO>
__global__ __launch_bounds__(NQ_RS_NT) void k_orb_smear_back(OrbArgs a, int tr, const double* A_H, const double* A_S, double* Rt_H, double* Rt_S) {
  __shared__ double lds[3 * NQ_RS_TILE];
  OrbTile q;
  if (!sm_mol(a, tr, q)) return;
  const int m = q.m, j0 = q.t * NQ_ORB_TILE;                     // the workgroup's 64 basis functions mu; it walks the orbitals i itself
  const double* Ct = a.coeff + q.base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const double nan = nq_nan_f64();
  double* X0 = Rt_H + q.base;
  double* X1 = TWO ? Rt_S + q.base : nullptr;
  for (int i0 = 0; i0 < m; i0 += NQ_ORB_TILE) {
    orb_f64x4 acc0[4], acc1[4];
    rs_zero(acc0);
    rs_zero(acc1);
    if (!q.failed) rs_gemm<false, false, TWO>(A_H + q.base, TWO ? A_S + q.base : nullptr, m, Ct, m, 0, m, i0, m, j0, m, lds, acc0, acc1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = j0 + s * 16 + lc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wave * 16 + lk + 4 * r;
        if (i >= m || j >= m) continue;
        X0[(long long)i * m + j] = q.failed ? nan : acc0[s][r];
        if (TWO) X1[(long long)i * m + j] = q.failed ? nan : acc1[s][r];
      }
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int nq_orb_fermi(void* state, int32_t B, int32_t M, int64_t P, const double* n_elec, const double* kT, double* out_mu, double* out_occ, double* out_docc,
                 double* out_entropy, int32_t* out_info, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_fermi", state, B, M, P, ORB_GRID_ROWS, &tr));
  if (!n_elec || !kT || !out_mu || !out_occ || !out_docc || !out_entropy || !out_info) return nq_fail(NQ_ERR_ARG, "nq_orb_fermi: null argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_fermi");
  hipLaunchKernelGGL(k_orb_fermi, dim3(B), dim3(NQ_ORB_NT), 0, st, orb_args(state, B, M, P), n_elec, kT, out_mu, out_occ, out_docc, out_entropy, (int*)out_info);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_smear_mo(void* state, int32_t B, int32_t M, int64_t P, const double* mu, const double* kT, const double* T, double* A_H, double* A_S, double* wdiag,
                    void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_smear_mo", state, B, M, P, ORB_GRID_ROWS, &tr));
  if (!mu || !kT || !T || !A_H || !wdiag) return nq_fail(NQ_ERR_ARG, "nq_orb_smear_mo: null argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, A_S ? "orb_smear_mo_two" : "orb_smear_mo_one");
  const OrbArgs a = orb_args(state, B, M, P);
  if (A_S)
    hipLaunchKernelGGL(k_orb_smear_mo<true>, dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, tr, mu, kT, T, A_H, A_S, wdiag);
  else
    hipLaunchKernelGGL(k_orb_smear_mo<false>, dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, tr, mu, kT, T, A_H, (double*)nullptr, wdiag);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_smear_diag(void* state, int32_t B, int32_t M, int64_t P, const double* mu, const double* kT, const double* occ, const double* docc,
                      const double* wdiag, const double* g_eps, const double* g_occ, const double* g_mu, const double* g_ent, double* A_H, double* A_S,
                      void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_smear_diag", state, B, M, P, ORB_GRID_ROWS, &tr));
  if (!mu || !kT || !occ || !docc || !wdiag || !A_H) return nq_fail(NQ_ERR_ARG, "nq_orb_smear_diag: null argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "orb_smear_diag");
  hipLaunchKernelGGL(k_orb_smear_diag, dim3(B), dim3(NQ_ORB_NT), 0, st, orb_args(state, B, M, P), mu, kT, occ, docc, wdiag, g_eps, g_occ, g_mu, g_ent, A_H, A_S);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_orb_smear_back(void* state, int32_t B, int32_t M, int64_t P, const double* A_H, const double* A_S, double* Rt_H, double* Rt_S, void* stream) {
  int tr = 0;
  NQ_TRY(orb_check_launch("nq_orb_smear_back", state, B, M, P, ORB_GRID_ROWS, &tr));
  if (!A_H || !Rt_H) return nq_fail(NQ_ERR_ARG, "nq_orb_smear_back: null argument");
  if (A_S && !Rt_S) return nq_fail(NQ_ERR_ARG, "nq_orb_smear_back: a second input needs a second output");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, A_S ? "orb_smear_back_two" : "orb_smear_back_one");
  const OrbArgs a = orb_args(state, B, M, P);
  if (A_S)
    hipLaunchKernelGGL(k_orb_smear_back<true>, dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, tr, A_H, A_S, Rt_H, Rt_S);
  else
    hipLaunchKernelGGL(k_orb_smear_back<false>, dim3(B * tr), dim3(NQ_RS_NT), 0, st, a, tr, A_H, (const double*)nullptr, Rt_H, (double*)nullptr);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
