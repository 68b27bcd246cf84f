// Stand-alone host program (its own main, no Python, no device work): the host code that the entry points of csrc/orbfrontier.hip add -- argument checks, the
// limits of k_max and tol, the refusal of aliased arrays and of a second output without its input, the grid arithmetic -- run under the host sanitizers.
// tests/test_orb_host_cpu.py builds and runs it:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/orbfrontier_host_check.hip nabladft_amd/csrc/orbfrontier.hip -o orbfrontier_host_check && ./orbfrontier_host_check
//
// Every call below is refused by the argument checks before a stream or a kernel is touched, so the program needs no GPU.  The error and profiler hooks,
// EXPECT / REFUSED and the final report are host_check.h's.
#include "host_check.h"

int main() {
  std::vector<double> host(16 * 64, 0.0);
  double* p = host.data();        // distinct stand-in arrays, never read or written
  double *Ht = p + 64, *X = p + 128, *shift = p + 192, *W = p + 256, *V = p + 320, *eps = p + 384, *vec = p + 448, *coef = p + 512, *res = p + 576, *g = p + 640,
         *gH = p + 704, *gS = p + 768;
  int32_t *nocc = (int32_t*)(p + 832), *iters = (int32_t*)(p + 896), *conv = (int32_t*)(p + 960);
  int64_t* vptr = (int64_t*)(p + 1000);
  const double tol = ldexp(1.0, -44);
#define LANCZOS(st, B, M, P, Ht, X, shift, nocc, W, k, tol, V, vptr, eps, vec, coef, iters, res, conv) \
  nq_orb_front_lanczos(st, B, M, P, Ht, X, shift, nocc, W, k, tol, V, vptr, eps, vec, coef, iters, res, conv, nullptr)
  // ---- dimensions no batch can have ------------------------------------------------------------------------------------------------------------------------------
  const long long dims[][3] = {{0, 0, 0}, {-1, 8, 34}, {2, 1, 1}, {2, 8, 7}, {1, 1025, 1025LL * 1025}, {2, 8, 8 * 1024 + 1}, {2, 2147483647, 34}};
  for (const auto& d : dims) {
    const int32_t B = (int32_t)d[0], M = (int32_t)d[1];
    EXPECT(LANCZOS(p, B, M, d[2], Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, vec, coef, iters, res, conv) == NQ_ERR_ARG);
    EXPECT(nq_orb_front_gram(p, B, M, d[2], g, eps, coef, conv, gH, gS, nullptr) == NQ_ERR_ARG);
  }
  REFUSED(nq_orb_front_gram(p, 0, 0, 0, g, eps, coef, conv, gH, gS, nullptr), "empty batch");
  // ---- null arguments ----------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(LANCZOS(nullptr, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, vec, coef, iters, res, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, nullptr, X, shift, nocc, W, 256, tol, V, vptr, eps, vec, coef, iters, res, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, nullptr, shift, nocc, W, 256, tol, V, vptr, eps, vec, coef, iters, res, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, nullptr, nocc, W, 256, tol, V, vptr, eps, vec, coef, iters, res, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nullptr, W, 256, tol, V, vptr, eps, vec, coef, iters, res, conv), "n_occ");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, nullptr, vptr, eps, vec, coef, iters, res, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, nullptr, eps, vec, coef, iters, res, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, vptr, nullptr, vec, coef, iters, res, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, nullptr, coef, iters, res, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, vec, nullptr, iters, res, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, vec, coef, nullptr, res, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, vec, coef, iters, nullptr, conv), "null");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, vec, coef, iters, res, nullptr), "null");
  REFUSED(nq_orb_front_gram(nullptr, 2, 8, 34, g, eps, coef, conv, gH, gS, nullptr), "null");
  REFUSED(nq_orb_front_gram(p, 2, 8, 34, nullptr, eps, coef, conv, gH, gS, nullptr), "null");
  REFUSED(nq_orb_front_gram(p, 2, 8, 34, g, eps, nullptr, conv, gH, gS, nullptr), "null");
  REFUSED(nq_orb_front_gram(p, 2, 8, 34, g, eps, coef, nullptr, gH, gS, nullptr), "null");
  REFUSED(nq_orb_front_gram(p, 2, 8, 34, g, eps, coef, conv, nullptr, gS, nullptr), "null");
  // ---- a second output without its input ---------------------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_front_gram(p, 2, 8, 34, g, nullptr, coef, conv, gH, gS, nullptr), "second output");
  // ---- aliased arrays --------------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, vec, vec, iters, res, conv), "different arrays");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, vec, coef, iters, eps, conv), "different arrays");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, Ht, vptr, eps, vec, coef, iters, res, conv), "different arrays");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, X, vptr, eps, vec, coef, iters, res, conv), "different arrays");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, W, vptr, eps, vec, coef, iters, res, conv), "different arrays");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, V, coef, iters, res, conv), "different arrays");
  REFUSED(nq_orb_front_gram(p, 2, 8, 34, g, eps, coef, conv, gH, gH, nullptr), "different arrays");
  REFUSED(nq_orb_front_gram(p, 2, 8, 34, g, eps, coef, conv, coef, gS, nullptr), "different arrays");
  REFUSED(nq_orb_front_gram(p, 2, 8, 34, g, eps, coef, conv, gH, g, nullptr), "different arrays");
  // ---- k_max and tol -----------------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 0, tol, V, vptr, eps, vec, coef, iters, res, conv), "k_max");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, -5, tol, V, vptr, eps, vec, coef, iters, res, conv), "k_max");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 1025, tol, V, vptr, eps, vec, coef, iters, res, conv), "k_max");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, 0.0, V, vptr, eps, vec, coef, iters, res, conv), "tol");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, -tol, V, vptr, eps, vec, coef, iters, res, conv), "tol");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, 1.0, V, vptr, eps, vec, coef, iters, res, conv), "tol");
  REFUSED(LANCZOS(p, 2, 8, 34, Ht, X, shift, nocc, W, 256, (double)NAN, V, vptr, eps, vec, coef, iters, res, conv), "tol");
  // ---- the grids: two workgroups per molecule, and B molecules of up to 256 tiles, must fit a 31-bit grid ------------------------------------------------------------------------
  const int32_t Bhuge = 1 << 30;
  REFUSED(LANCZOS(p, Bhuge, Bhuge, (int64_t)Bhuge, Ht, X, shift, nocc, W, 256, tol, V, vptr, eps, vec, coef, iters, res, conv), "exceed the grid");
  const int32_t Bbig = 1 << 23, Mbig = Bbig + 1023;
  const int64_t Pbig = (int64_t)(Bbig - 1) + 1024LL * 1024;
  REFUSED(nq_orb_front_gram(p, Bbig, Mbig, Pbig, g, eps, coef, conv, gH, gS, nullptr), "exceed the grid");
  EXPECT(orb_tile_rows(orb_largest_m_bound(Bbig, Mbig, Pbig)) == 16 && (long long)Bbig * 256 > INT_MAX);
  EXPECT(orb_tile_rows(orb_largest_m_bound(3, 10, 38)) == 1 && orb_tile_rows(65) == 2 && orb_tile_rows(64) == 1 && orb_tile_rows(1024) == 16);
  for (double v : host) EXPECT(v == 0.0);
  return host_check_report("orbfrontier_host_check");
}
