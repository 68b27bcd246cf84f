// Stand-alone host program (its own main, no Python, no device work): the host code that nq_orb_wgram / nq_orb_population add -- argument checks, the state
// layout, the tile arithmetic that sizes the grid -- run under the host sanitizers.  tests/test_orb_host_cpu.py builds and runs it:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/orbdens_host_check.hip nabladft_amd/csrc/orbdens.hip -o orbdens_host_check && ./orbdens_host_check
//
// Every call below is refused by the argument checks before a stream or a kernel is touched, so the program needs no GPU.  The error and profiler hooks,
// EXPECT / REFUSED and the final report are host_check.h's.
#include "host_check.h"

int main() {
  // ---- tiles: the decode inverts the enumeration for every tile a molecule of up to 1024 orbitals can have ----------------------------------------------
  EXPECT(orb_tile_rows(1) == 1 && orb_tile_rows(64) == 1 && orb_tile_rows(65) == 2 && orb_tile_rows(1024) == 16);
  EXPECT(orb_tile_count(1) == 1 && orb_tile_count(65) == 3 && orb_tile_count(1024) == 136);
  {
    int t = 0;
    for (int ti = 0; ti < 16; ++ti)
      for (int tj = 0; tj <= ti; ++tj, ++t) {
        int a = -1, b = -1;
        orb_tile_decode(t, &a, &b);
        EXPECT(a == ti && b == tj);
      }
    EXPECT(t == orb_tile_count(NQ_ORB_MAX_M));
  }
  // ---- the grid's bound on the largest molecule: never below the truth, never above the cap ---------------------------------------------------------------
  for (int B = 1; B <= 4; ++B)
    for (int big = 1; big <= NQ_ORB_MAX_M; big += (big < 40 ? 1 : 97))
      for (int rest = 1; rest <= 3; ++rest) {       // B - 1 molecules of `rest` orbitals and one of `big`
        const int M = big + (B - 1) * rest;
        const long long P = (long long)big * big + (long long)(B - 1) * rest * rest;
        const int bound = orb_largest_m_bound(B, M, P);
        EXPECT(bound >= big && (B == 1 || bound >= rest) && bound <= NQ_ORB_MAX_M);
        if (B == 1) EXPECT(bound == big);
      }
  EXPECT(orb_largest_m_bound(512, 512 * 1024, 512LL * 1024 * 1024) == 1024);
  // ---- the layout: eleven parts, ascending, 16-byte aligned, as large as their contents ---------------------------------------------------------------------
  {
    const OrbLayout L = orb_layout(3, 10, 38);
    for (int i = 0; i < OP_PARTS; ++i) EXPECT(L.part[i] % 16 == 0 && (i == 0 || L.part[i] > L.part[i - 1]));
    EXPECT(L.total >= L.part[OP_CHOL] + 38 * 8 && OP_PARTS == 11);
    std::vector<char> image(L.total, 0);
    const OrbArgs a = orb_args(image.data(), 3, 10, 38);
    EXPECT((char*)a.chol + 38 * 8 <= image.data() + L.total && (char*)a.hdr == image.data() && a.B == 3 && a.M == 10 && a.P == 38);
  }
  // ---- refusals: NQ_ERR_ARG before any device work; the stand-in arrays are never read or written -----------------------------------------------------------
  std::vector<double> host(64, 0.0);
  double* p = host.data();
  const int32_t* ip = (const int32_t*)p;
  const int64_t* lp = (const int64_t*)p;
  EXPECT(nq_orb_wgram(nullptr, 2, 8, 34, p, nullptr, nullptr, nullptr, p, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_wgram(p, 2, 8, 34, nullptr, nullptr, nullptr, nullptr, p, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_wgram(p, 2, 8, 34, p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_wgram(p, 2, 8, 34, p, p, nullptr, nullptr, p, nullptr, nullptr) == NQ_ERR_ARG && strstr(nq_err_buf, "second output"));
  const long long dims[][3] = {{0, 0, 0}, {-1, 8, 34}, {2, 1, 1}, {2, 8, 7}, {1, 1025, 1025LL * 1025}, {2, 8, 8 * 1024 + 1}, {2, 2147483647, 34}};
  for (const auto& d : dims) {
    EXPECT(nq_orb_wgram(p, (int32_t)d[0], (int32_t)d[1], d[2], p, nullptr, nullptr, nullptr, p, nullptr, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_population(p, (int32_t)d[0], (int32_t)d[1], d[2], p, nullptr, 0, nullptr, 0, 4, ip, lp, p, p, nullptr, nullptr) == NQ_ERR_ARG);
  }
  EXPECT(nq_orb_population(nullptr, 2, 8, 34, p, nullptr, 0, nullptr, 0, 4, ip, lp, p, p, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_population(p, 2, 8, 34, nullptr, nullptr, 0, nullptr, 0, 4, ip, lp, p, p, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_population(p, 2, 8, 34, p, nullptr, 0, nullptr, 0, 4, nullptr, lp, p, p, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_population(p, 2, 8, 34, p, nullptr, 0, nullptr, 0, 4, ip, nullptr, p, p, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_population(p, 2, 8, 34, p, nullptr, 0, nullptr, 0, 4, ip, lp, nullptr, p, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_population(p, 2, 8, 34, p, nullptr, 0, nullptr, 0, 4, ip, lp, p, nullptr, nullptr, nullptr) == NQ_ERR_ARG);
  EXPECT(nq_orb_population(p, 2, 8, 34, p, nullptr, 0, nullptr, 0, 4, ip, lp, p, p, p, nullptr) == NQ_ERR_ARG && strstr(nq_err_buf, "needs H"));
  EXPECT(nq_orb_population(p, 2, 8, 34, p, nullptr, 0, nullptr, 0, 1, ip, lp, p, p, nullptr, nullptr) == NQ_ERR_ARG && strstr(nq_err_buf, "atoms"));
  for (double v : host) EXPECT(v == 0.0);
  return host_check_report("orbdens_host_check");
}
