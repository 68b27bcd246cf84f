// Stand-alone host program (its own main, no Python, no device work): the host code that the entry points of csrc/orbpurify.hip add -- argument checks, the
// iteration limits, the grid arithmetic -- run under the host sanitizers.  tests/test_orb_host_cpu.py builds and runs it:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/orbpurify_host_check.hip nabladft_amd/csrc/orbpurify.hip -o orbpurify_host_check && ./orbpurify_host_check
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
  int32_t* ip = (int32_t*)p;
  int32_t* iq = (int32_t*)q;
  // ---- dimensions no batch can have ------------------------------------------------------------------------------------------------------------------------------
  const long long dims[][3] = {{0, 0, 0}, {-1, 8, 34}, {2, 1, 1}, {2, 8, 7}, {1, 1025, 1025LL * 1025}, {2, 8, 8 * 1024 + 1}, {2, 2147483647, 34}};
  for (const auto& d : dims) {
    const int32_t B = (int32_t)d[0], M = (int32_t)d[1];
    EXPECT(nq_orb_pur_orthogonalizer(p, B, M, d[2], q, 1, r, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_pur_congruence(p, B, M, d[2], q, 0, r, 1, 0, 1.0, s, p, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_pur_gemm(p, B, M, d[2], q, r, nullptr, 1.0, 0.0, s, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_pur_init(p, B, M, d[2], q, 1, nullptr, ip, 100, r, iq, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_pur_step(p, B, M, d[2], 0, 100, r, iq, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_pur_run(p, B, M, d[2], 100, r, iq, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_pur_response_init(p, B, M, d[2], q, 100, r, s, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_pur_response_step(p, B, M, d[2], 0, 100, iq, r, s, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_pur_response_run(p, B, M, d[2], 100, iq, r, s, nullptr) == NQ_ERR_ARG);
  }
  // ---- missing and aliased arrays ------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_pur_orthogonalizer(nullptr, 2, 8, 34, q, 1, r, nullptr), "null");
  REFUSED(nq_orb_pur_orthogonalizer(p, 2, 8, 34, nullptr, 1, r, nullptr), "null");
  REFUSED(nq_orb_pur_orthogonalizer(p, 2, 8, 34, q, 1, nullptr, nullptr), "null");
  REFUSED(nq_orb_pur_orthogonalizer(p, 2, 8, 34, q, 1, q, nullptr), "must not be S");
  REFUSED(nq_orb_pur_congruence(nullptr, 2, 8, 34, q, 0, r, 1, 0, 1.0, s, p, nullptr), "null");
  REFUSED(nq_orb_pur_congruence(p, 2, 8, 34, q, 0, nullptr, 1, 0, 1.0, s, p, nullptr), "null");
  REFUSED(nq_orb_pur_congruence(p, 2, 8, 34, q, 0, r, 1, 0, 1.0, s, nullptr, nullptr), "null");
  REFUSED(nq_orb_pur_congruence(p, 2, 8, 34, q, 0, r, 1, 0, 1.0, nullptr, p, nullptr), "tmp");
  REFUSED(nq_orb_pur_congruence(p, 2, 8, 34, q, 1, r, 1, 0, 1.0, s, r, nullptr), "different arrays");      // A is out
  REFUSED(nq_orb_pur_congruence(p, 2, 8, 34, q, 1, r, 1, 0, 1.0, s, s, nullptr), "different arrays");      // tmp is out
  REFUSED(nq_orb_pur_congruence(p, 2, 8, 34, q, 1, r, 1, 0, 1.0, r, s, nullptr), "different arrays");      // A is tmp
  REFUSED(nq_orb_pur_congruence(p, 2, 8, 34, q, 1, r, 1, 0, 1.0, s, q, nullptr), "different arrays");      // Z is out
  REFUSED(nq_orb_pur_congruence(p, 2, 8, 34, q, 1, r, 1, 0, 1.0, q, s, nullptr), "different arrays");      // Z is tmp
  REFUSED(nq_orb_pur_congruence(p, 2, 8, 34, nullptr, 0, r, 1, 1, 2.0, nullptr, r, nullptr), "different arrays");
  REFUSED(nq_orb_pur_gemm(p, 2, 8, 34, nullptr, r, nullptr, 1.0, 0.0, s, nullptr), "null");
  REFUSED(nq_orb_pur_gemm(p, 2, 8, 34, q, nullptr, nullptr, 1.0, 0.0, s, nullptr), "null");
  REFUSED(nq_orb_pur_gemm(p, 2, 8, 34, q, r, nullptr, 1.0, 0.0, nullptr, nullptr), "null");
  REFUSED(nq_orb_pur_gemm(p, 2, 8, 34, q, r, nullptr, 1.0, 0.0, q, nullptr), "operand");
  REFUSED(nq_orb_pur_gemm(p, 2, 8, 34, q, r, nullptr, 1.0, 0.0, r, nullptr), "operand");
  REFUSED(nq_orb_pur_init(nullptr, 2, 8, 34, q, 1, nullptr, ip, 100, r, iq, nullptr), "null");
  REFUSED(nq_orb_pur_init(p, 2, 8, 34, q, 1, nullptr, nullptr, 100, r, iq, nullptr), "n_occ");
  REFUSED(nq_orb_pur_init(p, 2, 8, 34, q, 1, nullptr, ip, 100, nullptr, iq, nullptr), "null");
  REFUSED(nq_orb_pur_init(p, 2, 8, 34, q, 1, nullptr, ip, 100, r, nullptr, nullptr), "null");
  // ---- the iteration limits ------------------------------------------------------------------------------------------------------------------------------------------
  const int bad_iter[] = {0, -1, 10001, 2147483647};
  for (int mi : bad_iter) {
    REFUSED(nq_orb_pur_init(p, 2, 8, 34, q, 1, nullptr, ip, mi, r, iq, nullptr), "max_iter");
    REFUSED(nq_orb_pur_step(p, 2, 8, 34, 0, mi, r, iq, nullptr), "max_iter");
    REFUSED(nq_orb_pur_run(p, 2, 8, 34, mi, r, iq, nullptr), "max_iter");
    REFUSED(nq_orb_pur_response_init(p, 2, 8, 34, q, mi, r, s, nullptr), "max_iter");
    REFUSED(nq_orb_pur_response_step(p, 2, 8, 34, 0, mi, iq, r, s, nullptr), "max_iter");
    REFUSED(nq_orb_pur_response_run(p, 2, 8, 34, mi, iq, r, s, nullptr), "max_iter");
  }
  REFUSED(nq_orb_pur_step(p, 2, 8, 34, 100, 100, r, iq, nullptr), "iteration");
  REFUSED(nq_orb_pur_step(p, 2, 8, 34, -1, 100, r, iq, nullptr), "iteration");
  REFUSED(nq_orb_pur_response_step(p, 2, 8, 34, 100, 100, iq, r, s, nullptr), "iteration");
  REFUSED(nq_orb_pur_step(p, 2, 8, 34, 0, 100, nullptr, iq, nullptr), "null");
  REFUSED(nq_orb_pur_step(p, 2, 8, 34, 0, 100, r, nullptr, nullptr), "null");
  REFUSED(nq_orb_pur_run(p, 2, 8, 34, 100, nullptr, iq, nullptr), "null");
  REFUSED(nq_orb_pur_run(nullptr, 2, 8, 34, 100, r, iq, nullptr), "null");
  // ---- the response: a second input without a second output ----------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_pur_response_init(p, 2, 8, 34, nullptr, 100, r, s, nullptr), "null");
  REFUSED(nq_orb_pur_response_init(p, 2, 8, 34, q, 100, nullptr, s, nullptr), "null");
  REFUSED(nq_orb_pur_response_init(p, 2, 8, 34, q, 100, r, nullptr, nullptr), "null");
  REFUSED(nq_orb_pur_response_init(p, 2, 8, 34, q, 100, r, q, nullptr), "must not be Gt");
  REFUSED(nq_orb_pur_response_step(p, 2, 8, 34, 0, 100, nullptr, r, s, nullptr), "null");
  REFUSED(nq_orb_pur_response_step(p, 2, 8, 34, 0, 100, iq, r, nullptr, nullptr), "null");
  REFUSED(nq_orb_pur_response_step(p, 2, 8, 34, 0, 100, iq, nullptr, s, nullptr), "second output");
  REFUSED(nq_orb_pur_response_step(p, 2, 8, 34, 0, 100, iq, s, s, nullptr), "must not be X1");
  REFUSED(nq_orb_pur_response_run(p, 2, 8, 34, 100, iq, nullptr, s, nullptr), "second output");
  REFUSED(nq_orb_pur_response_run(p, 2, 8, 34, 100, iq, s, s, nullptr), "must not be X1");
  REFUSED(nq_orb_pur_response_run(p, 2, 8, 34, 100, nullptr, r, s, nullptr), "null");
  // the grids: one workgroup per 64 x 64 tile of the largest molecule the dimensions allow
  EXPECT(orb_tile_rows(orb_largest_m_bound(1, 1024, 1024LL * 1024)) == 16 && orb_tile_count(1024) == 136 && orb_tile_rows(orb_largest_m_bound(3, 10, 38)) == 1);
  for (double v : host) EXPECT(v == 0.0);
  return host_check_report("orbpurify_host_check");
}
