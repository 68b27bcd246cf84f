// Stand-alone host program (its own main, no Python, no device work): the host code that the entry points of csrc/orbocc.hip add -- argument checks, the
// refusal of aliased arrays, of reduced dimensions that do not fit the batch and of a reduced state that is the state, the grid arithmetic -- run under the
// host sanitizers.  tests/test_orbocc_host_cpu.py builds and runs it:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/orbocc_host_check.hip nabladft_amd/csrc/orbocc.hip -o orbocc_host_check && ./orbocc_host_check
//
// Every call below is refused by the argument checks before a stream or a kernel is touched, so the program needs no GPU.  The error and profiler hooks,
// EXPECT / REFUSED and the final report are host_check.h's.
#include "host_check.h"

int main() {
  std::vector<double> host(16 * 64, 0.0);
  double* p = host.data();        // distinct stand-in arrays, never read or written
  double *Q = p + 64, *minp = p + 128, *defect = p + 192, *T = p + 256, *Hs = p + 320, *W = p + 384, *U = p + 448, *red = p + 512;
  int32_t *nocc = (int32_t*)(p + 576), *piv = (int32_t*)(p + 640), *status = (int32_t*)(p + 704);
  int64_t *occ_ptr = (int64_t*)(p + 768), *red_ptr = (int64_t*)(p + 832);
  // B = 2, M = 8, P = 34 (m = 3 and 5); n_occ = (1, 2): O = 13, Mr = 3, Pr = R = 5
#define FACTOR(st, B, M, P, nocc, Q, piv, minp, defect, status) nq_orb_occ_factor(st, B, M, P, nocc, Q, piv, minp, defect, status, nullptr)
#define REDUCE(st, B, M, P, nocc, optr, O, T, status, rptr, R, Hs) nq_orb_occ_reduce(st, B, M, P, nocc, optr, O, T, status, rptr, R, Hs, nullptr)
#define BACK(st, rst, B, M, P, Mr, Pr, nocc, optr, O, W, status, U) nq_orb_occ_back(st, rst, B, M, P, Mr, Pr, nocc, optr, O, W, status, U, nullptr)
  // ---- dimensions no batch can have ------------------------------------------------------------------------------------------------------------------------------
  const long long dims[][3] = {{0, 0, 0}, {-1, 8, 34}, {2, 1, 1}, {2, 8, 7}, {1, 1025, 1025LL * 1025}, {2, 8, 8 * 1024 + 1}, {2, 2147483647, 34}};
  for (const auto& d : dims) {
    const int32_t B = (int32_t)d[0], M = (int32_t)d[1];
    EXPECT(FACTOR(p, B, M, d[2], nocc, Q, piv, minp, defect, status) == NQ_ERR_ARG);
    EXPECT(REDUCE(p, B, M, d[2], nocc, occ_ptr, 13, T, status, red_ptr, 5, Hs) == NQ_ERR_ARG);
    EXPECT(BACK(p, red, B, M, d[2], 3, 5, nocc, occ_ptr, 13, W, status, U) == NQ_ERR_ARG);
  }
  REFUSED(FACTOR(p, 0, 0, 0, nocc, Q, piv, minp, defect, status), "empty batch");
  // ---- null arguments ----------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(FACTOR(nullptr, 2, 8, 34, nocc, Q, piv, minp, defect, status), "null");
  REFUSED(FACTOR(p, 2, 8, 34, nullptr, Q, piv, minp, defect, status), "n_occ");
  REFUSED(FACTOR(p, 2, 8, 34, nocc, nullptr, piv, minp, defect, status), "null");
  REFUSED(FACTOR(p, 2, 8, 34, nocc, Q, nullptr, minp, defect, status), "null");
  REFUSED(FACTOR(p, 2, 8, 34, nocc, Q, piv, nullptr, defect, status), "null");
  REFUSED(FACTOR(p, 2, 8, 34, nocc, Q, piv, minp, nullptr, status), "null");
  REFUSED(FACTOR(p, 2, 8, 34, nocc, Q, piv, minp, defect, nullptr), "null");
  REFUSED(REDUCE(nullptr, 2, 8, 34, nocc, occ_ptr, 13, T, status, red_ptr, 5, Hs), "null");
  REFUSED(REDUCE(p, 2, 8, 34, nullptr, occ_ptr, 13, T, status, red_ptr, 5, Hs), "n_occ");
  REFUSED(REDUCE(p, 2, 8, 34, nocc, nullptr, 13, T, status, red_ptr, 5, Hs), "occ_ptr");
  REFUSED(REDUCE(p, 2, 8, 34, nocc, occ_ptr, 13, nullptr, status, red_ptr, 5, Hs), "null");
  REFUSED(REDUCE(p, 2, 8, 34, nocc, occ_ptr, 13, T, nullptr, red_ptr, 5, Hs), "null");
  REFUSED(REDUCE(p, 2, 8, 34, nocc, occ_ptr, 13, T, status, nullptr, 5, Hs), "null");
  REFUSED(REDUCE(p, 2, 8, 34, nocc, occ_ptr, 13, T, status, red_ptr, 5, nullptr), "null");
  REFUSED(BACK(nullptr, red, 2, 8, 34, 3, 5, nocc, occ_ptr, 13, W, status, U), "null");
  REFUSED(BACK(p, nullptr, 2, 8, 34, 3, 5, nocc, occ_ptr, 13, W, status, U), "reduced_state");
  REFUSED(BACK(p, red, 2, 8, 34, 3, 5, nullptr, occ_ptr, 13, W, status, U), "n_occ");
  REFUSED(BACK(p, red, 2, 8, 34, 3, 5, nocc, nullptr, 13, W, status, U), "occ_ptr");
  REFUSED(BACK(p, red, 2, 8, 34, 3, 5, nocc, occ_ptr, 13, W, nullptr, U), "null");
  REFUSED(BACK(p, red, 2, 8, 34, 3, 5, nocc, occ_ptr, 13, W, status, nullptr), "null");
  // ---- the occupied-packed and the reduced layouts ---------------------------------------------------------------------------------------------------------------------------
  REFUSED(REDUCE(p, 2, 8, 34, nocc, occ_ptr, -1, T, status, red_ptr, 5, Hs), "do not fit");
  REFUSED(REDUCE(p, 2, 8, 34, nocc, occ_ptr, 35, T, status, red_ptr, 5, Hs), "do not fit");
  REFUSED(REDUCE(p, 2, 8, 34, nocc, occ_ptr, 13, T, status, red_ptr, 1, Hs), "reduced entries");        // fewer than one entry per molecule
  REFUSED(REDUCE(p, 2, 8, 34, nocc, occ_ptr, 13, T, status, red_ptr, 37, Hs), "reduced entries");       // more than P + B
  REFUSED(BACK(p, red, 2, 8, 34, 1, 5, nocc, occ_ptr, 13, W, status, U), "reduced dimensions");         // Mr < B
  REFUSED(BACK(p, red, 2, 8, 34, 11, 61, nocc, occ_ptr, 13, W, status, U), "reduced dimensions");       // Mr > M + B
  REFUSED(BACK(p, red, 2, 8, 34, 3, 2, nocc, occ_ptr, 13, W, status, U), "reduced dimensions");         // Pr < Mr
  REFUSED(BACK(p, red, 2, 8, 34, 8, 37, nocc, occ_ptr, 13, W, status, U), "reduced dimensions");        // Pr > P + B
  REFUSED(BACK(p, red, 2, 8, 34, 3, 5, nocc, occ_ptr, 35, W, status, U), "do not fit");
  // ---- aliased arrays --------------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(FACTOR(p, 2, 8, 34, nocc, Q, piv, minp, minp, status), "different arrays");
  REFUSED(FACTOR(p, 2, 8, 34, nocc, Q, piv, Q, defect, status), "different arrays");
  REFUSED(FACTOR(p, 2, 8, 34, nocc, Q, piv, minp, Q, status), "different arrays");
  REFUSED(FACTOR(p, 2, 8, 34, nocc, Q, piv, minp, defect, piv), "different arrays");
  REFUSED(FACTOR(p, 2, 8, 34, nocc, Q, nocc, minp, defect, status), "different arrays");
  REFUSED(FACTOR(p, 2, 8, 34, nocc, Q, piv, minp, defect, nocc), "different arrays");
  REFUSED(REDUCE(p, 2, 8, 34, nocc, occ_ptr, 13, T, status, red_ptr, 5, T), "must not be T");
  REFUSED(BACK(p, p, 2, 8, 34, 3, 5, nocc, occ_ptr, 13, W, status, U), "must not be the state");
  REFUSED(BACK(p, red, 2, 8, 34, 3, 5, nocc, occ_ptr, 13, U, status, U), "must not be W");
  // ---- the grids: B molecules of up to 136 lower-triangle tiles must fit a 31-bit grid ------------------------------------------------------------------------------------------
  const int32_t Bbig = 1 << 24, Mbig = Bbig + 1023;
  const int64_t Pbig = (int64_t)(Bbig - 1) + 1024LL * 1024;
  REFUSED(REDUCE(p, Bbig, Mbig, Pbig, nocc, occ_ptr, 13, T, status, red_ptr, Bbig, Hs), "exceed the grid");
  REFUSED(BACK(p, red, Bbig, Mbig, Pbig, Bbig, Bbig, nocc, occ_ptr, 13, W, status, U), "exceed the grid");
  EXPECT(orb_tile_rows(orb_largest_m_bound(Bbig, Mbig, Pbig)) == 16 && (long long)Bbig * 136 > INT_MAX);
  EXPECT(orb_tile_count(83) == 3 && orb_tile_count(64) == 1 && orb_tile_count(1024) == 136);
  for (double v : host) EXPECT(v == 0.0);
  return host_check_report("orbocc_host_check");
}
