// Stand-alone host program (its own main, no Python, no device work): the host code that the entry points of csrc/orbsqrt.hip add -- argument checks, the
// iteration limits, the refusal of aliased arrays, the grid arithmetic -- run under the host sanitizers.  tests/test_orb_host_cpu.py builds and runs it:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/orbsqrt_host_check.hip nabladft_amd/csrc/orbsqrt.hip -o orbsqrt_host_check && ./orbsqrt_host_check
//
// Every call below is refused by the argument checks before a stream or a kernel is touched, so the program needs no GPU.  The error and profiler hooks,
// EXPECT / REFUSED and the final report are host_check.h's.
#include "host_check.h"

int main() {
  std::vector<double> host(11 * 64, 0.0);
  double* p = host.data();        // distinct stand-in arrays, never read or written
  double *S = p + 64, *Y = p + 128, *Z = p + 192, *T = p + 256, *Y2 = p + 320, *Z2 = p + 384, *ctl = p + 448, *half = p + 576, *inv = p + 640;
  int32_t* log = (int32_t*)(p + 512);
  // ---- dimensions no batch can have ------------------------------------------------------------------------------------------------------------------------------
  const long long dims[][3] = {{0, 0, 0}, {-1, 8, 34}, {2, 1, 1}, {2, 8, 7}, {1, 1025, 1025LL * 1025}, {2, 8, 8 * 1024 + 1}, {2, 2147483647, 34}};
  for (const auto& d : dims) {
    const int32_t B = (int32_t)d[0], M = (int32_t)d[1];
    EXPECT(nq_orb_sqrt_init(p, B, M, d[2], S, 1, 100, Y, Z, ctl, log, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_sqrt_step(p, B, M, d[2], 0, 100, Y, Z, T, Y2, Z2, ctl, log, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_sqrt_run(p, B, M, d[2], 100, Y, Z, T, Y2, Z2, ctl, log, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_sqrt_finish(p, B, M, d[2], 100, Y, Z, Y2, Z2, ctl, log, half, inv, nullptr) == NQ_ERR_ARG);
  }
  REFUSED(nq_orb_sqrt_run(p, 0, 0, 0, 100, Y, Z, T, Y2, Z2, ctl, log, nullptr), "empty batch");
  // ---- null arguments ----------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_sqrt_init(nullptr, 2, 8, 34, S, 1, 100, Y, Z, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, nullptr, 1, 100, Y, Z, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 0, 100, nullptr, Z, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 0, 100, Y, nullptr, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 1, 100, Y, Z, nullptr, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 1, 100, Y, Z, ctl, nullptr, nullptr), "null");
  REFUSED(nq_orb_sqrt_step(nullptr, 2, 8, 34, 0, 100, Y, Z, T, Y2, Z2, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_step(p, 2, 8, 34, 0, 100, nullptr, Z, T, Y2, Z2, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_step(p, 2, 8, 34, 0, 100, Y, Z, nullptr, Y2, Z2, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_step(p, 2, 8, 34, 0, 100, Y, Z, T, Y2, nullptr, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_run(nullptr, 2, 8, 34, 100, Y, Z, T, Y2, Z2, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_run(p, 2, 8, 34, 100, Y, nullptr, T, Y2, Z2, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_run(p, 2, 8, 34, 100, Y, Z, T, nullptr, Z2, ctl, log, nullptr), "null");
  REFUSED(nq_orb_sqrt_run(p, 2, 8, 34, 100, Y, Z, T, Y2, Z2, ctl, nullptr, nullptr), "null");
  REFUSED(nq_orb_sqrt_finish(nullptr, 2, 8, 34, 100, Y, Z, Y2, Z2, ctl, log, half, inv, nullptr), "null");
  REFUSED(nq_orb_sqrt_finish(p, 2, 8, 34, 100, Y, Z, Y2, Z2, nullptr, log, half, inv, nullptr), "null");
  REFUSED(nq_orb_sqrt_finish(p, 2, 8, 34, 100, Y, Z, Y2, Z2, ctl, log, nullptr, inv, nullptr), "null");
  REFUSED(nq_orb_sqrt_finish(p, 2, 8, 34, 100, Y, Z, Y2, Z2, ctl, log, half, nullptr, nullptr), "null");
  // ---- aliased arrays --------------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 1, 100, S, Z, ctl, log, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 1, 100, Y, S, ctl, log, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 1, 100, Y, Y, ctl, log, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 1, 100, Y, Z, Y, log, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 1, 100, Y, Z, ctl, (int32_t*)ctl, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_step(p, 2, 8, 34, 0, 100, Y, Z, T, Y, Z2, ctl, log, nullptr), "different arrays");       // a product's output must not be its operand
  REFUSED(nq_orb_sqrt_step(p, 2, 8, 34, 0, 100, Y, Z, T, Y2, Z, ctl, log, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_step(p, 2, 8, 34, 0, 100, Y, Z, Y, Y2, Z2, ctl, log, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_step(p, 2, 8, 34, 0, 100, Y, Z, T, Y2, Y2, ctl, log, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_run(p, 2, 8, 34, 100, Y, Y, T, Y2, Z2, ctl, log, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_run(p, 2, 8, 34, 100, Y, Z, T, Y2, Z2, T, log, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_finish(p, 2, 8, 34, 100, Y, Z, Y2, Z2, ctl, log, half, half, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_finish(p, 2, 8, 34, 100, Y, Z, Y2, Z2, ctl, log, Y, inv, nullptr), "different arrays");
  REFUSED(nq_orb_sqrt_finish(p, 2, 8, 34, 100, Y, Z, Y2, Z2, ctl, log, half, Z2, nullptr), "different arrays");
  // ---- iteration limits -------------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 1, 0, Y, Z, ctl, log, nullptr), "max_iter");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 1, 10001, Y, Z, ctl, log, nullptr), "max_iter");
  REFUSED(nq_orb_sqrt_init(p, 2, 8, 34, S, 1, -3, Y, Z, ctl, log, nullptr), "max_iter");
  REFUSED(nq_orb_sqrt_step(p, 2, 8, 34, 5, 5, Y, Z, T, Y2, Z2, ctl, log, nullptr), "iteration");
  REFUSED(nq_orb_sqrt_step(p, 2, 8, 34, -1, 5, Y, Z, T, Y2, Z2, ctl, log, nullptr), "iteration");
  REFUSED(nq_orb_sqrt_step(p, 2, 8, 34, 0, 0, Y, Z, T, Y2, Z2, ctl, log, nullptr), "max_iter");
  REFUSED(nq_orb_sqrt_run(p, 2, 8, 34, 10001, Y, Z, T, Y2, Z2, ctl, log, nullptr), "max_iter");
  REFUSED(nq_orb_sqrt_finish(p, 2, 8, 34, 0, Y, Z, Y2, Z2, ctl, log, half, inv, nullptr), "max_iter");
  // ---- the grids: B molecules of up to 256 full tiles must fit a 31-bit grid --------------------------------------------------------------------------------------------------
  const int32_t Bbig = 1 << 23, Mbig = Bbig + 1023;
  const int64_t Pbig = (int64_t)(Bbig - 1) + 1024LL * 1024;
  REFUSED(nq_orb_sqrt_step(p, Bbig, Mbig, Pbig, 0, 100, Y, Z, T, Y2, Z2, ctl, log, nullptr), "exceed the grid");
  REFUSED(nq_orb_sqrt_run(p, Bbig, Mbig, Pbig, 100, Y, Z, T, Y2, Z2, ctl, log, nullptr), "exceed the grid");
  REFUSED(nq_orb_sqrt_finish(p, Bbig, Mbig, Pbig, 100, Y, Z, Y2, Z2, ctl, log, half, inv, nullptr), "exceed the grid");
  EXPECT(orb_tile_rows(orb_largest_m_bound(Bbig, Mbig, Pbig)) == 16 && (long long)Bbig * 256 > INT_MAX);
  EXPECT(orb_tile_rows(orb_largest_m_bound(3, 10, 38)) == 1 && orb_tile_count(65) == 3 && orb_tile_count(64) == 1 && orb_tile_count(1024) == 136);
  for (int t = 0; t < 136; ++t) {                                  // every lower-triangle tile of the largest molecule decodes to a pair on or below the diagonal
    int ti, tj;
    orb_tile_decode(t, &ti, &tj);
    EXPECT(tj >= 0 && tj <= ti && ti < 16 && ti * (ti + 1) / 2 + tj == t);
  }
  for (double v : host) EXPECT(v == 0.0);
  return host_check_report("orbsqrt_host_check");
}
