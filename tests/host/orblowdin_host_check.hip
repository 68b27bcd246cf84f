// Stand-alone host program (its own main, no Python, no device work): the host code that the entry points of csrc/orblowdin.hip add -- argument checks, the
// refusal of aliased outputs, the grid arithmetic -- run under the host sanitizers.  tests/test_orb_host_cpu.py builds and runs it:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/orblowdin_host_check.hip nabladft_amd/csrc/orblowdin.hip -o orblowdin_host_check && ./orblowdin_host_check
//
// Every call below is refused by the argument checks before a stream or a kernel is touched, so the program needs no GPU.  The error and profiler hooks,
// EXPECT / REFUSED and the final report are host_check.h's.
#include "host_check.h"

int main() {
  std::vector<double> host(320, 0.0);
  double* p = host.data();        // five distinct stand-in arrays, never read or written
  double* q = p + 64;
  double* r = p + 128;
  double* s = p + 192;
  double* e = p + 256;
  int32_t* ie = (int32_t*)e;
  // ---- dimensions no batch can have ------------------------------------------------------------------------------------------------------------------------------
  const long long dims[][3] = {{0, 0, 0}, {-1, 8, 34}, {2, 1, 1}, {2, 8, 7}, {1, 1025, 1025LL * 1025}, {2, 8, 8 * 1024 + 1}, {2, 2147483647, 34}};
  for (const auto& d : dims) {
    const int32_t B = (int32_t)d[0], M = (int32_t)d[1];
    EXPECT(nq_orb_low_weights(p, B, M, d[2], q, r, s, ie, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_low_product(p, B, M, d[2], q, 1, r, s, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_low_symprod(p, B, M, d[2], q, r, 0, 1.0, s, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_low_mo(p, B, M, d[2], 0, q, r, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_low_symmetrize(p, B, M, d[2], q, r, nullptr) == NQ_ERR_ARG);
  }
  REFUSED(nq_orb_low_mo(p, 0, 0, 0, 1, q, r, nullptr), "empty batch");
  // ---- null arguments ----------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_low_weights(nullptr, 2, 8, 34, q, r, s, ie, nullptr), "null");
  REFUSED(nq_orb_low_weights(p, 2, 8, 34, nullptr, r, s, ie, nullptr), "null");
  REFUSED(nq_orb_low_weights(p, 2, 8, 34, q, nullptr, s, ie, nullptr), "null");
  REFUSED(nq_orb_low_weights(p, 2, 8, 34, q, r, nullptr, ie, nullptr), "null");
  REFUSED(nq_orb_low_weights(p, 2, 8, 34, q, r, s, nullptr, nullptr), "null");
  REFUSED(nq_orb_low_weights(p, 2, 8, 34, q, q, s, ie, nullptr), "of their own");
  REFUSED(nq_orb_low_product(nullptr, 2, 8, 34, q, 1, r, s, nullptr), "null");
  REFUSED(nq_orb_low_product(p, 2, 8, 34, nullptr, 1, r, s, nullptr), "null");
  REFUSED(nq_orb_low_product(p, 2, 8, 34, q, 0, nullptr, s, nullptr), "null");
  REFUSED(nq_orb_low_product(p, 2, 8, 34, q, 1, r, nullptr, nullptr), "null");
  REFUSED(nq_orb_low_product(p, 2, 8, 34, q, 1, r, q, nullptr), "operand");
  REFUSED(nq_orb_low_product(p, 2, 8, 34, q, 0, r, r, nullptr), "operand");
  REFUSED(nq_orb_low_symprod(nullptr, 2, 8, 34, q, r, 0, 1.0, s, nullptr), "null");
  REFUSED(nq_orb_low_symprod(p, 2, 8, 34, nullptr, r, 0, 1.0, s, nullptr), "null");
  REFUSED(nq_orb_low_symprod(p, 2, 8, 34, q, nullptr, 1, 2.0, s, nullptr), "null");
  REFUSED(nq_orb_low_symprod(p, 2, 8, 34, q, r, 1, 2.0, nullptr, nullptr), "null");
  REFUSED(nq_orb_low_symprod(p, 2, 8, 34, q, r, 1, 2.0, q, nullptr), "operand");
  REFUSED(nq_orb_low_symprod(p, 2, 8, 34, q, r, 0, 1.0, r, nullptr), "operand");
  REFUSED(nq_orb_low_symmetrize(nullptr, 2, 8, 34, q, r, nullptr), "null");
  REFUSED(nq_orb_low_symmetrize(p, 2, 8, 34, nullptr, r, nullptr), "null");
  REFUSED(nq_orb_low_symmetrize(p, 2, 8, 34, q, nullptr, nullptr), "null");
  REFUSED(nq_orb_low_symmetrize(p, 2, 8, 34, q, q, nullptr), "operand");
  REFUSED(nq_orb_low_mo(nullptr, 2, 8, 34, 0, q, r, nullptr), "null");
  REFUSED(nq_orb_low_mo(p, 2, 8, 34, 0, nullptr, r, nullptr), "null");
  REFUSED(nq_orb_low_mo(p, 2, 8, 34, 1, q, nullptr, nullptr), "null");
  REFUSED(nq_orb_low_mo(p, 2, 8, 34, 1, q, q, nullptr), "operand");
  // ---- a side or a kind that does not exist -----------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_low_symprod(p, 2, 8, 34, q, r, 2, 1.0, s, nullptr), "neither 0");
  REFUSED(nq_orb_low_symprod(p, 2, 8, 34, q, r, -1, 1.0, s, nullptr), "neither 0");
  REFUSED(nq_orb_low_mo(p, 2, 8, 34, 2, q, r, nullptr), "neither 0");
  REFUSED(nq_orb_low_mo(p, 2, 8, 34, -1, q, r, nullptr), "neither 0");
  // ---- the grids: B molecules of up to 16 x 16 tiles (product), 136 (symprod, symmetrize) or 16 tile rows (mo) must fit a 31-bit grid ---------------------------------------
  const int32_t Bbig = 1 << 23, Mbig = Bbig + 1023;
  const int64_t Pbig = (int64_t)(Bbig - 1) + 1024LL * 1024;
  REFUSED(nq_orb_low_product(p, Bbig, Mbig, Pbig, q, 1, r, s, nullptr), "exceed the grid");
  REFUSED(nq_orb_low_symprod(p, 1 << 24, (1 << 24) + 1023, (int64_t)((1 << 24) - 1) + 1024LL * 1024, q, r, 0, 1.0, s, nullptr), "exceed the grid");
  REFUSED(nq_orb_low_symmetrize(p, 1 << 24, (1 << 24) + 1023, (int64_t)((1 << 24) - 1) + 1024LL * 1024, q, r, nullptr), "exceed the grid");
  REFUSED(nq_orb_low_mo(p, 1 << 27, (1 << 27) + 1023, (int64_t)((1 << 27) - 1) + 1024LL * 1024, 0, q, r, nullptr), "exceed the grid");
  EXPECT(orb_tile_rows(orb_largest_m_bound(Bbig, Mbig, Pbig)) == 16 && orb_tile_count(1024) == 136 && orb_tile_rows(orb_largest_m_bound(3, 10, 38)) == 1);
  for (double v : host) EXPECT(v == 0.0);
  return host_check_report("orblowdin_host_check");
}
