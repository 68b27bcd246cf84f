// Stand-alone host program (its own main, no Python, no device work): the host code that the entry points of csrc/orbbond.hip add -- argument checks, the
// consistency of the bond table with the atom counts, the grid arithmetic -- run under the host sanitizers.  tests/test_orb_host_cpu.py builds and runs it:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/orbbond_host_check.hip nabladft_amd/csrc/orbbond.hip -o orbbond_host_check && ./orbbond_host_check
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
  const int32_t* ip = (const int32_t*)p;
  const int64_t* lq = (const int64_t*)q;
  const int64_t* lr = (const int64_t*)r;
  // ---- dimensions no batch can have ------------------------------------------------------------------------------------------------------------------------------
  const long long dims[][3] = {{0, 0, 0}, {-1, 8, 34}, {2, 1, 1}, {2, 8, 7}, {1, 1025, 1025LL * 1025}, {2, 8, 8 * 1024 + 1}, {2, 2147483647, 34}};
  for (const auto& d : dims) {
    const int32_t B = (int32_t)d[0], M = (int32_t)d[1];
    EXPECT(nq_orb_bond_product(p, B, M, d[2], q, r, 1, s, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_bond_reduce(p, B, M, d[2], q, 3, 5, ip, lq, lr, s, e, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_bond_backward(p, B, M, d[2], q, r, s, nullptr, nullptr, 0, 3, 5, ip, lq, lr, e, p, nullptr, nullptr) == NQ_ERR_ARG);
  }
  // ---- null arguments ----------------------------------------------------------------------------------------------------------------------------------------------------
  REFUSED(nq_orb_bond_product(nullptr, 2, 8, 34, q, r, 1, s, nullptr), "null");
  REFUSED(nq_orb_bond_product(p, 2, 8, 34, nullptr, r, 1, s, nullptr), "null");
  REFUSED(nq_orb_bond_product(p, 2, 8, 34, q, r, 1, nullptr, nullptr), "null");
  REFUSED(nq_orb_bond_product(p, 2, 8, 34, q, r, 1, q, nullptr), "operand");
  REFUSED(nq_orb_bond_product(p, 2, 8, 34, q, r, 0, r, nullptr), "operand");
  REFUSED(nq_orb_bond_reduce(nullptr, 2, 8, 34, q, 3, 5, ip, lq, lr, s, e, nullptr), "null");
  REFUSED(nq_orb_bond_reduce(p, 2, 8, 34, nullptr, 3, 5, ip, lq, lr, s, e, nullptr), "null");
  REFUSED(nq_orb_bond_reduce(p, 2, 8, 34, q, 3, 5, nullptr, lq, lr, s, e, nullptr), "null");
  REFUSED(nq_orb_bond_reduce(p, 2, 8, 34, q, 3, 5, ip, nullptr, lr, s, e, nullptr), "null");
  REFUSED(nq_orb_bond_reduce(p, 2, 8, 34, q, 3, 5, ip, lq, nullptr, s, e, nullptr), "null");
  REFUSED(nq_orb_bond_reduce(p, 2, 8, 34, q, 3, 5, ip, lq, lr, nullptr, e, nullptr), "null");
  REFUSED(nq_orb_bond_backward(nullptr, 2, 8, 34, q, r, s, nullptr, nullptr, 0, 3, 5, ip, lq, lr, e, p, nullptr, nullptr), "null");
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, q, r, nullptr, nullptr, nullptr, 0, 3, 5, ip, lq, lr, e, p, nullptr, nullptr), "null");
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, q, r, s, nullptr, nullptr, 0, 3, 5, nullptr, lq, lr, e, p, nullptr, nullptr), "null");
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, q, r, s, nullptr, nullptr, 0, 3, 5, ip, nullptr, lr, e, p, nullptr, nullptr), "null");
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, q, r, s, nullptr, nullptr, 0, 3, 5, ip, lq, nullptr, e, p, nullptr, nullptr), "bond_ptr");
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, q, r, s, nullptr, nullptr, 0, 3, 5, ip, lq, lr, nullptr, p, nullptr, nullptr), "null");
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, q, r, s, nullptr, nullptr, 0, 3, 5, ip, lq, lr, e, nullptr, nullptr, nullptr), "no output");
  // ---- gS without S or D, a second input without its output, aliased scratch -----------------------------------------------------------------------------------
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, nullptr, r, s, q, nullptr, 0, 3, 5, ip, lq, lr, e, nullptr, p, nullptr), "needs S");
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, nullptr, r, s, nullptr, q, 1, 3, 5, ip, lq, lr, e, nullptr, p, nullptr), "needs D");
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, nullptr, r, s, q, q, 1, 3, 5, ip, lq, lr, e, p, nullptr, nullptr), "second input");
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, nullptr, r, s, nullptr, q, 1, 3, 5, ip, lq, lr, s, p, nullptr, nullptr), "of their own");      // E is P
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, nullptr, r, s, nullptr, q, 1, 3, 5, ip, lq, lr, e, e, nullptr, nullptr), "of their own");      // E is out_gD
  REFUSED(nq_orb_bond_backward(p, 2, 8, 34, nullptr, r, s, r, q, 1, 3, 5, ip, lq, lr, e, p, p, nullptr), "of their own");                  // out_gD is out_gS
  // ---- Q against the atom counts: N atoms in B molecules own N .. (N - B + 1)^2 + B - 1 entries ---------------------------------------------------------------
  const long long bad_q[][2] = {{1, 1}, {3, 2}, {3, 6}, {3, -1}, {5, 18}, {2147483647, 1}};
  for (const auto& nq : bad_q) {
    EXPECT(nq_orb_bond_reduce(p, 2, 8, 34, q, (int32_t)nq[0], nq[1], ip, lq, lr, s, e, nullptr) == NQ_ERR_ARG);
    EXPECT(nq_orb_bond_backward(p, 2, 8, 34, q, r, s, nullptr, nullptr, 0, (int32_t)nq[0], nq[1], ip, lq, lr, e, p, nullptr, nullptr) == NQ_ERR_ARG);
  }
  REFUSED(nq_orb_bond_reduce(p, 2, 8, 34, q, 3, 6, ip, lq, lr, s, e, nullptr), "inconsistent");
  REFUSED(nq_orb_bond_reduce(p, 2, 8, 34, q, 1, 1, ip, lq, lr, s, e, nullptr), "atoms for");
  // without gB the reverse does not read the table, and Q is not looked at: the call gets as far as the dimensions
  REFUSED(nq_orb_bond_backward(p, 0, 0, 0, nullptr, r, s, nullptr, nullptr, 0, 3, 99, ip, lq, nullptr, e, p, nullptr, nullptr), "empty batch");
  // ---- the grids: B molecules of up to 16 x 16 tiles (product), 136 (reverse) or 64 chunks (reduce) must fit a 31-bit grid -------------------------------------
  const int32_t Bbig = 1 << 23, Mbig = Bbig + 1023;
  const int64_t Pbig = (int64_t)(Bbig - 1) + 1024LL * 1024;
  REFUSED(nq_orb_bond_product(p, Bbig, Mbig, Pbig, q, r, 1, s, nullptr), "exceed the grid");
  REFUSED(nq_orb_bond_backward(p, 1 << 24, (1 << 24) + 1023, (int64_t)((1 << 24) - 1) + 1024LL * 1024, nullptr, r, s, nullptr, nullptr, 0, 1 << 24, 0, ip, lq, nullptr, e, p,
                               nullptr, nullptr), "exceed the grid");
  REFUSED(nq_orb_bond_reduce(p, 1 << 25, 1 << 25, 1 << 25, q, 1 << 25, 1 << 25, ip, lq, lr, s, e, nullptr), "exceed the grid");
  EXPECT(orb_tile_rows(orb_largest_m_bound(Bbig, Mbig, Pbig)) == 16 && orb_tile_count(1024) == 136 && orb_tile_rows(orb_largest_m_bound(3, 10, 38)) == 1);
  for (double v : host) EXPECT(v == 0.0);
  return host_check_report("orbbond_host_check");
}
