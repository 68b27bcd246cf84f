// Stand-alone host program (its own main, no Python, no device work): the host code that the entry points of csrc/orbcomm.hip add -- argument checks, the
// refusal of aliased outputs, the grid arithmetic -- run under the host sanitizers.  tests/test_orb_host_cpu.py builds and runs it:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/orbcomm_host_check.hip nabladft_amd/csrc/orbcomm.hip -o orbcomm_host_check && ./orbcomm_host_check
//
// Every call below is refused by the argument checks before a stream or a kernel is touched, so the program needs no GPU.  The error and profiler hooks,
// EXPECT / REFUSED and the final report are host_check.h's.
#include "host_check.h"

int main() {
  std::vector<double> host(256, 0.0);
  double* p = host.data();        // four distinct stand-in arrays, never read or written
  double* q = p + 64;
  double* r = p + 128;
  double* s = p + 192;
  // ---- dimensions no batch can have ------------------------------------------------------------------------------------------------------------------------------
  const long long dims[][3] = {{0, 0, 0}, {-1, 8, 34}, {2, 1, 1}, {2, 8, 7}, {1, 1025, 1025LL * 1025}, {2, 8, 8 * 1024 + 1}, {2, 2147483647, 34}};
  for (const auto& d : dims) {
    const int32_t B = (int32_t)d[0], M = (int32_t)d[1];
    EXPECT(nq_orb_comm_product(p, B, M, d[2], q, 0, r, 1.0, s, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_comm_product(p, B, M, d[2], q, 1, r, -1.0, s, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_comm_antisymmetrize(p, B, M, d[2], q, r, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_comm_norms(p, B, M, d[2], q, r, s, nullptr) == NQ_ERR_ARG);
  }
  REFUSED(nq_orb_comm_norms(p, 0, 0, 0, q, r, s, nullptr), "empty batch");
  // ---- null arguments ----------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_comm_product(nullptr, 2, 8, 34, q, 0, r, 1.0, s, nullptr), "null");
  REFUSED(nq_orb_comm_product(p, 2, 8, 34, nullptr, 0, r, 1.0, s, nullptr), "null");
  REFUSED(nq_orb_comm_product(p, 2, 8, 34, q, 1, nullptr, 1.0, s, nullptr), "null");
  REFUSED(nq_orb_comm_product(p, 2, 8, 34, q, 1, r, 2.0, nullptr, nullptr), "null");
  REFUSED(nq_orb_comm_antisymmetrize(nullptr, 2, 8, 34, q, r, nullptr), "null");
  REFUSED(nq_orb_comm_antisymmetrize(p, 2, 8, 34, nullptr, r, nullptr), "null");
  REFUSED(nq_orb_comm_antisymmetrize(p, 2, 8, 34, q, nullptr, nullptr), "null");
  REFUSED(nq_orb_comm_norms(nullptr, 2, 8, 34, q, r, s, nullptr), "null");
  REFUSED(nq_orb_comm_norms(p, 2, 8, 34, nullptr, r, s, nullptr), "null");
  REFUSED(nq_orb_comm_norms(p, 2, 8, 34, q, nullptr, s, nullptr), "null");
  REFUSED(nq_orb_comm_norms(p, 2, 8, 34, q, r, nullptr, nullptr), "null");
  // ---- aliased outputs -----------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_comm_product(p, 2, 8, 34, q, 0, r, 1.0, q, nullptr), "operand");
  REFUSED(nq_orb_comm_product(p, 2, 8, 34, q, 1, r, 1.0, r, nullptr), "operand");
  REFUSED(nq_orb_comm_antisymmetrize(p, 2, 8, 34, q, q, nullptr), "operand");
  REFUSED(nq_orb_comm_norms(p, 2, 8, 34, q, r, r, nullptr), "of their own");
  REFUSED(nq_orb_comm_norms(p, 2, 8, 34, q, q, s, nullptr), "operand");
  REFUSED(nq_orb_comm_norms(p, 2, 8, 34, q, r, q, nullptr), "operand");
  // ---- a symmetry that does not exist ----------------------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_comm_product(p, 2, 8, 34, q, 2, r, 1.0, s, nullptr), "neither 0");
  REFUSED(nq_orb_comm_product(p, 2, 8, 34, q, -1, r, 1.0, s, nullptr), "neither 0");
  // ---- the grids: B molecules of up to 136 lower-triangle tiles must fit a 31-bit grid; the norms launch one workgroup per molecule ------------------------------------
  const int32_t Bbig = 1 << 24, Mbig = Bbig + 1023;
  const int64_t Pbig = (int64_t)(Bbig - 1) + 1024LL * 1024;
  REFUSED(nq_orb_comm_product(p, Bbig, Mbig, Pbig, q, 0, r, 1.0, s, nullptr), "exceed the grid");
  REFUSED(nq_orb_comm_product(p, Bbig, Mbig, Pbig, q, 1, r, 1.0, s, nullptr), "exceed the grid");
  REFUSED(nq_orb_comm_antisymmetrize(p, Bbig, Mbig, Pbig, q, r, nullptr), "exceed the grid");
  EXPECT(orb_tile_rows(orb_largest_m_bound(Bbig, Mbig, Pbig)) == 16 && orb_tile_count(1024) == 136 && (long long)Bbig * 136 > INT_MAX);
  EXPECT(orb_tile_rows(orb_largest_m_bound(3, 10, 38)) == 1 && orb_tile_count(65) == 3 && orb_tile_count(64) == 1 && orb_tile_count(129) == 6);
  for (int t = 0; t < 136; ++t) {                                  // every tile of the largest molecule decodes to a pair on or below the diagonal, in order
    int ti, tj;
    orb_tile_decode(t, &ti, &tj);
    EXPECT(tj >= 0 && tj <= ti && ti < 16 && ti * (ti + 1) / 2 + tj == t);
  }
  for (double v : host) EXPECT(v == 0.0);
  return host_check_report("orbcomm_host_check");
}
