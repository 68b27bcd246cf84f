// The scalar mathematics of Fermi-Dirac smearing (orbsmear.hip), as __host__ __device__ inline functions so that a host program can test them
// (tests/host/orbsmear_host_check.hip).  Everything is written in x = (eps - mu) / kT and e = exp(-|x|) <= 1, so that no exponential overflows and no
// difference of orbital energies is divided by:
//
//   F(x)  = 2 / (1 + e^x)                         = 2 e / (1 + e)  (x > 0),   2 / (1 + e)  (x <= 0)
//   F'(x) = dF / d eps at fixed mu                = -(2 / kT) e / (1 + e)^2            (<= 0, even in x)
//   s(x)  = -2 (f ln f + (1 - f) ln(1 - f))       = 2 (log1p(e) + |x| e / (1 + e))     (f = F / 2; 0 ln 0 = 0 comes out by itself)
//   K(x_i, x_j) = (F_i - F_j) / (eps_i - eps_j)   = -(1 / (2 kT)) sinhc((x_i - x_j) / 2) / (cosh(x_i / 2) cosh(x_j / 2))
//               = -(1 / kT) E r(t) / ((1 + e_i) (1 + e_j)),    t = |x_i - x_j| / 2,   r(t) = (1 - e^{-2t}) / t  (r(0) = 2),
//                 E = exp(t - (|x_i| + |x_j|) / 2) = exp(-min(|x_i|, |x_j|)) where x_i and x_j have the same sign, 1 where they do not
//   KS_ij = -((F_i + F_j) / 2 + (eps_i + eps_j) / 2 K_ij)  = -((F_i + F_j) / 2 - ((eps_i + eps_j) / (2 kT) r) c),   c = E / ((1 + e_i) (1 + e_j))
//
// K is symmetric in its arguments operation by operation, <= 0, finite for every pair of finite x, and equal to F' at x_i == x_j (the same operations).
// Another smearing function replaces F, F', s and K here and nothing else.  No a * b + c in here: the including files are compiled with -ffp-contract=off.
#pragma once
#include <math.h>

#ifndef __host__
#define __host__
#define __device__
#endif

#define NQ_SMEAR_X_MAX 1e300

// x = (eps - mu) / kT, clamped to +-1e300 so that differences and halves of x stay finite
__host__ __device__ static inline double nq_smear_x(double eps, double mu, double kT) {
  const double x = (eps - mu) / kT;
  return x > NQ_SMEAR_X_MAX ? NQ_SMEAR_X_MAX : (x < -NQ_SMEAR_X_MAX ? -NQ_SMEAR_X_MAX : x);
}

// e = exp(-|x|)
__host__ __device__ static inline double nq_smear_e(double x) { return exp(-fabs(x)); }

__host__ __device__ static inline double nq_smear_occ_e(double x, double e) { return x > 0.0 ? 2.0 * e / (1.0 + e) : 2.0 / (1.0 + e); }
__host__ __device__ static inline double nq_smear_occ(double x) { return nq_smear_occ_e(x, nq_smear_e(x)); }

// the tail of a level: its particles F where it lies above mu (x > 0), minus its holes 2 - F where it does not; F = tail + (x > 0 ? 0 : 2)
__host__ __device__ static inline double nq_smear_tail_e(double x, double e) {
  const double t = 2.0 * e / (1.0 + e);
  return x > 0.0 ? t : -t;
}

__host__ __device__ static inline double nq_smear_docc_e(double e, double kT) {
  const double q = 1.0 + e;
  return -(2.0 / kT) * (e / (q * q));
}
__host__ __device__ static inline double nq_smear_docc(double x, double kT) { return nq_smear_docc_e(nq_smear_e(x), kT); }

// the entropy term of one level, in units of k_B
__host__ __device__ static inline double nq_smear_entropy(double x) {
  const double e = nq_smear_e(x);
  const double tail = e == 0.0 ? 0.0 : fabs(x) * (e / (1.0 + e));
  return 2.0 * (log1p(e) + tail);
}

// The divided difference of F is K = -(1 / kT) c r with r = r(t) in (0, 2] and c = E / ((1 + e_i) (1 + e_j)) in (0, 1]; ei = exp(-|xi|), ej = exp(-|xj|).
__host__ __device__ static inline void nq_smear_K_parts(double xi, double ei, double xj, double ej, double* c, double* r) {
  if (xi == xj) {                                                               // the operations of nq_smear_docc_e
    const double q = 1.0 + ei;
    *c = ei / (q * q);
    *r = 2.0;
    return;
  }
  const double t = fabs(0.5 * xi - 0.5 * xj);
  *r = t == 0.0 ? 2.0 : -expm1(-2.0 * t) / t;                                   // t == 0: the halves of two denormals
  const bool same = (xi > 0.0) == (xj > 0.0) && xi != 0.0 && xj != 0.0;
  const double E = same ? (fabs(xi) < fabs(xj) ? ei : ej) : 1.0;                // exp(-min(|xi|, |xj|)): e of the argument nearer to zero
  *c = E / ((1.0 + ei) * (1.0 + ej));
}
__host__ __device__ static inline double nq_smear_K_e(double xi, double ei, double xj, double ej, double kT) {
  double c, r;
  nq_smear_K_parts(xi, ei, xj, ej, &c, &r);
  return xi == xj ? -(2.0 / kT) * c : -(1.0 / kT) * (c * r);
}
__host__ __device__ static inline double nq_smear_K(double xi, double xj, double kT) { return nq_smear_K_e(xi, nq_smear_e(xi), xj, nq_smear_e(xj), kT); }

// KS = -((F_i + F_j) / 2 + (eps_i + eps_j) / 2 K), with (eps_i + eps_j) / (2 kT) multiplied by r first: where c r underflows (levels 1e300 kT apart) the product
// with a huge mean level keeps its digits.  The mean level over kT is clamped like x.
__host__ __device__ static inline double nq_smear_KS_e(double xi, double ei, double xj, double ej, double Fi, double Fj, double eps_i, double eps_j, double kT) {
  double c, r;
  nq_smear_K_parts(xi, ei, xj, ej, &c, &r);
  double a = (0.5 * eps_i + 0.5 * eps_j) / kT;
  a = a > NQ_SMEAR_X_MAX ? NQ_SMEAR_X_MAX : (a < -NQ_SMEAR_X_MAX ? -NQ_SMEAR_X_MAX : a);
  return -(0.5 * (Fi + Fj) - (a * r) * c);
}
__host__ __device__ static inline double nq_smear_KS(double xi, double xj, double eps_i, double eps_j, double kT) {
  const double ei = nq_smear_e(xi), ej = nq_smear_e(xj);
  return nq_smear_KS_e(xi, ei, xj, ej, nq_smear_occ_e(xi, ei), nq_smear_occ_e(xj, ej), eps_i, eps_j, kT);
}
