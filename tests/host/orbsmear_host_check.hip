// Stand-alone host program (its own main, no Python, no device work): the host code that the entry points of csrc/orbsmear.hip add -- argument checks, the grid
// arithmetic -- and the scalar functions of csrc/orbsmear_math.h on a grid of arguments, run under the host sanitizers.  tests/test_orbsmear_host_cpu.py
// builds and runs it and compares the values it prints with an extended-precision evaluation:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/orbsmear_host_check.hip nabladft_amd/csrc/orbsmear.hip -o orbsmear_host_check && ./orbsmear_host_check
//
// Every call below is refused by the argument checks before a stream or a kernel is touched, so the program needs no GPU.  The error and profiler hooks,
// EXPECT / REFUSED and the final report are host_check.h's.
#include "host_check.h"
#include "../../nabladft_amd/csrc/orbsmear_math.h"

int main() {
  // ---- the scalar functions on the grid: every pair of the base values, equal pairs among them, and every value against its neighbours one ulp away ----------
  const double base[] = {0.0, 1e-300, 1e-9, 1e-3, 1.0, 30.0, 700.0, 1e4, 1e300};
  std::vector<double> xs;
  for (double b : base) {
    xs.push_back(b);
    if (b != 0.0) xs.push_back(-b);
  }
  std::vector<std::pair<double, double>> pairs;
  for (double a : xs)
    for (double b : xs) pairs.push_back({a, b});
  for (double a : xs) {
    pairs.push_back({a, nextafter(a, INFINITY)});
    pairs.push_back({nextafter(a, -INFINITY), a});
  }
  const double kTs[] = {0.01, 1.0};
  for (double kT : kTs)
    for (const auto& pr : pairs) {
      const double xi = pr.first, xj = pr.second;
      const double Fi = nq_smear_occ(xi), Fj = nq_smear_occ(xj), dFi = nq_smear_docc(xi, kT), si = nq_smear_entropy(xi);
      const double K = nq_smear_K(xi, xj, kT), Kt = nq_smear_K(xj, xi, kT);
      const double ei = kT * xi, ej = kT * xj;                 // mu = 0
      const double KS = nq_smear_KS(xi, xj, ei, ej, kT);
      EXPECT(isfinite(Fi) && isfinite(dFi) && isfinite(si) && isfinite(K) && isfinite(KS));
      EXPECT(Fi >= 0.0 && Fi <= 2.0 && dFi <= 0.0 && si >= 0.0 && si <= 2.0 * log(2.0) * (1.0 + 1e-15));
      EXPECT(K == Kt && K <= 0.0);
      EXPECT(nq_smear_K(xi, xi, kT) == dFi);
      EXPECT(!isnan(nq_smear_x(ei, 0.0, kT)) && fabs(nq_smear_x(ei, 0.0, kT)) <= NQ_SMEAR_X_MAX);
      printf("V %a %a %a %a %a %a %a %a\n", kT, xi, xj, Fi, dFi, si, K, KS);
    }
  // the clamp keeps x finite where kT is tiny
  EXPECT(nq_smear_x(1.0, 0.0, 1e-320) == NQ_SMEAR_X_MAX && nq_smear_x(-1.0, 0.0, 1e-320) == -NQ_SMEAR_X_MAX && nq_smear_occ(NQ_SMEAR_X_MAX) == 0.0);
  EXPECT(nq_smear_occ(-NQ_SMEAR_X_MAX) == 2.0 && nq_smear_entropy(NQ_SMEAR_X_MAX) == 0.0 && nq_smear_K(NQ_SMEAR_X_MAX, -NQ_SMEAR_X_MAX, 1.0) <= 0.0);

  // ---- refusals: NQ_ERR_ARG before any device work; the stand-in arrays are never read or written -----------------------------------------------------------
  std::vector<double> host(64, 0.0);
  double* p = host.data();
  int32_t* ip = (int32_t*)p;
  const long long dims[][3] = {{0, 0, 0}, {-1, 8, 34}, {2, 1, 1}, {2, 8, 7}, {1, 1025, 1025LL * 1025}, {2, 8, 8 * 1024 + 1}, {2, 2147483647, 34}};
  for (const auto& d : dims) {
    const int32_t B = (int32_t)d[0], M = (int32_t)d[1];
    EXPECT(nq_orb_fermi(p, B, M, d[2], p, p, p, p, p, p, ip, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_smear_mo(p, B, M, d[2], p, p, p, p, p, p, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_smear_diag(p, B, M, d[2], p, p, p, p, p, nullptr, nullptr, nullptr, nullptr, p, p, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_smear_back(p, B, M, d[2], p, p, p, p, nullptr) == NQ_ERR_ARG);
  }
  EXPECT(nq_orb_fermi(nullptr, 2, 8, 34, p, p, p, p, p, p, ip, nullptr) == NQ_ERR_ARG && strstr(nq_err_buf, "null"));
  for (int miss = 0; miss < 7; ++miss) {
    double* a[6] = {p, p, p, p, p, p};
    if (miss < 6) a[miss] = nullptr;
    EXPECT(nq_orb_fermi(p, 2, 8, 34, a[0], a[1], a[2], a[3], a[4], a[5], miss == 6 ? nullptr : ip, nullptr) == NQ_ERR_ARG && strstr(nq_err_buf, "null"));
  }
  EXPECT(nq_orb_smear_mo(nullptr, 2, 8, 34, p, p, p, p, p, p, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_smear_mo(p, 2, 8, 34, nullptr, p, p, p, p, p, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_smear_mo(p, 2, 8, 34, p, nullptr, p, p, p, p, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_smear_mo(p, 2, 8, 34, p, p, nullptr, p, p, p, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_smear_mo(p, 2, 8, 34, p, p, p, nullptr, p, p, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_smear_mo(p, 2, 8, 34, p, p, p, p, nullptr, nullptr, nullptr) == NQ_ERR_ARG && strstr(nq_err_buf, "null"));
  EXPECT(nq_orb_smear_diag(nullptr, 2, 8, 34, p, p, p, p, p, p, p, p, p, p, p, nullptr) == NQ_ERR_ARG);
  for (int miss = 0; miss < 6; ++miss) {
    double* a[6] = {p, p, p, p, p, p};
    a[miss] = nullptr;
    EXPECT(nq_orb_smear_diag(p, 2, 8, 34, a[0], a[1], a[2], a[3], a[4], p, p, p, p, a[5], p, nullptr) == NQ_ERR_ARG && strstr(nq_err_buf, "null"));
  }
  EXPECT(nq_orb_smear_back(nullptr, 2, 8, 34, p, nullptr, p, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_smear_back(p, 2, 8, 34, nullptr, nullptr, p, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_smear_back(p, 2, 8, 34, p, nullptr, nullptr, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_smear_back(p, 2, 8, 34, p, p, p, nullptr, nullptr) == NQ_ERR_ARG && strstr(nq_err_buf, "second output"));
  // the grid of the products: one workgroup per (molecule, 64 orbitals) of the largest molecule the dimensions allow
  EXPECT(orb_tile_rows(orb_largest_m_bound(1, 1024, 1024LL * 1024)) == 16 && orb_tile_rows(orb_largest_m_bound(3, 10, 38)) == 1);
  EXPECT(orb_tile_rows(orb_largest_m_bound(2, 66, 65LL * 65 + 1)) == 2);
  for (double v : host) EXPECT(v == 0.0);
  return host_check_report("orbsmear_host_check");
}
