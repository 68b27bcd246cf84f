// Hamiltonian block assembly of QHNet: replaces the Python O(N^2) loop with .item() and
// torch.where per block of QHNet.build_final_matrix (/root/reference/nablaDFT/qhnet/qhnet.py:293-321), the H + H^T of qhnet.py:237,
// and HamiltonianLoss (qhnet/loss.py:9-16) with table-driven gather kernels.  Pure data movement + one add: bit-exact.
//
// Layouts.  Every atom predicts a padded S x S block (S = s_max + 3 p_max + 5 d_max = 32 for def2-SVP up to Br); atom type Z uses the
// slots mask[Z][0..count[Z]) of it (QHNet._get_mask).  The molecule's matrix has M_b = sum of count over its atoms rows; the batch
// result is stored PACKED ([sum_b M_b^2], molecule after molecule, row-major) -- the dense block_diag matrix the reference returns is
// (sum M_b)^2 with zeros everywhere else and is produced on request by k_hb_scatter_dense.
#include "common.h"
#include "../../include/nablaq.h"

static inline dim3 hb_grid(long count, int block) { return dim3((unsigned)((count + block - 1) / block)); }

// one thread per atom: global orbital -> (atom, slot in the padded block)
__global__ void k_hb_orbmap(const int* __restrict__ z, const long long* __restrict__ orb_ptr, int N, const int* __restrict__ mask_table,
                            const int* __restrict__ mask_count, int S, int* __restrict__ ORB_ATOM, int* __restrict__ ORB_SLOT) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int zi = z[i], cnt = mask_count[zi];
  const long long o = orb_ptr[i];
  for (int t = 0; t < cnt; ++t) { ORB_ATOM[o + t] = i; ORB_SLOT[o + t] = mask_table[zi * S + t]; }
}
// one thread per ordered pair e = (row0 = dst, row1 = src): LOOK[molecule pair table][dst_local][src_local] = e
__global__ void k_hb_lookup(const long long* __restrict__ e_dst, const long long* __restrict__ e_src, long long P, const int* __restrict__ atom_mol,
                            const int* __restrict__ mol_ptr, const long long* __restrict__ pair_base, int* __restrict__ LOOK, int* __restrict__ err) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P) return;
  const int d = (int)e_dst[e], s = (int)e_src[e];
  const int b = atom_mol[d];
  if (atom_mol[s] != b || d == s) { atomicOr(err, 1); return; }
  const int a0 = mol_ptr[b], n = mol_ptr[b + 1] - a0;
  LOOK[pair_base[b] + (long long)(d - a0) * n + (s - a0)] = (int)e;
}

__device__ __forceinline__ int hb_find_mol(const long long* __restrict__ pack_ptr, int B, long long q) {
  int lo = 0, hi = B;          // largest b with pack_ptr[b] <= q
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pack_ptr[mid] <= q) lo = mid; else hi = mid; }
  return lo;
}

struct HbArgs {
  const float* diag; const float* nondiag;        // [N][S][S], [P][S][S]
  const int* mol_ptr; const long long* pair_base; const long long* pack_ptr; const long long* mol_orb_ptr;   // [B+1] each (pair_base: [B])
  const int* ORB_ATOM; const int* ORB_SLOT; const int* LOOK;
  int B, S, symmetrize;
};

__device__ __forceinline__ float hb_block_elem(const HbArgs& a, int b, int d, int s, int u, int v, int* err) {
  const int SS = a.S * a.S;
  if (d == s) return a.diag[(long long)d * SS + u * a.S + v];
  const int a0 = a.mol_ptr[b], n = a.mol_ptr[b + 1] - a0;
  const int e = a.LOOK[a.pair_base[b] + (long long)(d - a0) * n + (s - a0)];
  if (e < 0) { atomicOr(err, 2); return 0.f; }   // the pair list is not the full graph of the molecule
  return a.nondiag[(long long)e * SS + u * a.S + v];
}

// one thread per element of the packed result
__global__ void k_hb_assemble(HbArgs a, long long total, float* __restrict__ out, int* __restrict__ err) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  const int b = hb_find_mol(a.pack_ptr, a.B, q);
  const long long o0 = a.mol_orb_ptr[b];
  const int M = (int)(a.mol_orb_ptr[b + 1] - o0);
  const long long loc = q - a.pack_ptr[b];
  const int r = (int)(loc / M), c = (int)(loc % M);
  const int ad = a.ORB_ATOM[o0 + r], as = a.ORB_ATOM[o0 + c], u = a.ORB_SLOT[o0 + r], v = a.ORB_SLOT[o0 + c];
  float val = hb_block_elem(a, b, ad, as, u, v, err);                      // rows: dst atom's orbitals, columns: src atom's (qhnet.py:300-318)
  if (a.symmetrize) val += hb_block_elem(a, b, as, ad, v, u, err);         // + transposed element (qhnet.py:237)
  out[q] = val;
}

// reverse: gradient of the padded blocks from the gradient of the packed result.  One thread per block element.
struct HbRevArgs {
  const float* G;                                   // packed gradient
  const int* z; const int* atom_mol; const long long* orb_ptr; const long long* pack_ptr; const long long* mol_orb_ptr;
  const int* inv_table;                             // [Zt][S] slot -> local orbital or -1
  const long long* e_dst; const long long* e_src;
  int N, S, symmetrize; long long P;
};
__global__ void k_hb_assemble_rev(HbRevArgs a, float* __restrict__ g_diag, float* __restrict__ g_nondiag) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int SS = a.S * a.S;
  const long long nd = (long long)a.N * SS, total = nd + a.P * SS;
  if (idx >= total) return;
  int d, s; float* dstp;
  long long rem;
  if (idx < nd) { d = s = (int)(idx / SS); rem = idx % SS; dstp = g_diag + idx; }
  else { const long long k = idx - nd; const long long e = k / SS; d = (int)a.e_dst[e]; s = (int)a.e_src[e]; rem = k % SS; dstp = g_nondiag + k; }
  const int u = (int)(rem / a.S), v = (int)(rem % a.S);
  const int lu = a.inv_table[a.z[d] * a.S + u], lv = a.inv_table[a.z[s] * a.S + v];
  float g = 0.f;
  if (lu >= 0 && lv >= 0) {
    const int b = a.atom_mol[d];
    const long long o0 = a.mol_orb_ptr[b];
    const int M = (int)(a.mol_orb_ptr[b + 1] - o0);
    const int r = (int)(a.orb_ptr[d] - o0) + lu, c = (int)(a.orb_ptr[s] - o0) + lv;
    g = a.G[a.pack_ptr[b] + (long long)r * M + c];
    if (a.symmetrize) g += a.G[a.pack_ptr[b] + (long long)c * M + r];
  }
  *dstp = g;
}

// packed <-> dense block-diagonal
__global__ void k_hb_scatter_dense(const float* __restrict__ packed, const long long* __restrict__ pack_ptr, const long long* __restrict__ mol_orb_ptr,
                                   int B, long long total, long long Mtot, float* __restrict__ dense, int to_dense) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  const int b = hb_find_mol(pack_ptr, B, q);
  const long long o0 = mol_orb_ptr[b];
  const int M = (int)(mol_orb_ptr[b + 1] - o0);
  const long long loc = q - pack_ptr[b];
  const long long at = (o0 + loc / M) * Mtot + o0 + loc % M;
  if (to_dense) dense[at] = packed[q];
  else const_cast<float*>(packed)[q] = dense[at];
}

// HamiltonianLoss on packed arrays: loss = sqrt(sum d^2 / cnt) + sum |d| / cnt, cnt = number of packed elements (= mask.sum()).
#define HB_RED_BLOCKS 256
__global__ void k_hb_loss_partial(const float* __restrict__ pred, const float* __restrict__ target, long long total, double* __restrict__ part) {
  __shared__ double s2[4], s1[4];
  double a2 = 0.0, a1 = 0.0;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
    const double d = (double)pred[q] - (double)target[q];
    a2 += d * d; a1 += fabs(d);
  }
  for (int off = 32; off > 0; off >>= 1) { a2 += __shfl_down(a2, off); a1 += __shfl_down(a1, off); }
  if ((threadIdx.x & 63) == 0) { s2[threadIdx.x >> 6] = a2; s1[threadIdx.x >> 6] = a1; }
  __syncthreads();
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s2[0] + s2[1] + s2[2] + s2[3]; part[2 * blockIdx.x + 1] = s1[0] + s1[1] + s1[2] + s1[3]; }
}
// out[0] = loss, out[1] = rmse, out[2] = sum |d| (for the masked MAE metric)
__global__ void k_hb_loss_final(const double* __restrict__ part, int nblocks, long long total, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a2 = 0.0, a1 = 0.0;
  for (int i = 0; i < nblocks; ++i) { a2 += part[2 * i]; a1 += part[2 * i + 1]; }
  const double rmse = sqrt(a2 / (double)total);
  out[0] = (float)(rmse + a1 / (double)total); out[1] = (float)rmse; out[2] = (float)a1;
}
__global__ void k_hb_loss_grad(const float* __restrict__ pred, const float* __restrict__ target, long long total, const float* __restrict__ stats,
                               float gscale, float* __restrict__ grad) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  const float d = pred[q] - target[q];
  const float rmse = stats[1];
  const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  grad[q] = gscale * ((rmse > 0.f ? d / (rmse * (float)total) : 0.f) + sg / (float)total);
}

extern "C" {

int nq_hblock_tables(const int32_t* z, const int32_t* atom_mol, const int32_t* mol_ptr, int32_t N, int32_t B, const int64_t* orb_ptr,
                     const int64_t* pair_base, const int64_t* e_dst, const int64_t* e_src, int64_t P, const int32_t* mask_table,
                     const int32_t* mask_count, int32_t S, int32_t* orb_atom, int32_t* orb_slot, int32_t* look, int64_t look_count,
                     int32_t* err_flag, void* stream) {
  if (!z || !atom_mol || !mol_ptr || !orb_ptr || !pair_base || !mask_table || !mask_count || !orb_atom || !orb_slot || !look || !err_flag)
    return nq_fail(NQ_ERR_ARG, "null argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "hblock_tables");
  NQ_HIP(hipMemsetAsync(err_flag, 0, sizeof(int32_t), st));
  NQ_HIP(hipMemsetAsync(look, 0xff, (size_t)look_count * sizeof(int32_t), st));     // -1 = no such pair
  if (N > 0) hipLaunchKernelGGL(k_hb_orbmap, hb_grid(N, 128), dim3(128), 0, st, z, (const long long*)orb_ptr, N, mask_table, mask_count, S, orb_atom, orb_slot);
  NQ_LAUNCH_CHECK();
  if (P > 0) hipLaunchKernelGGL(k_hb_lookup, hb_grid(P, 256), dim3(256), 0, st, (const long long*)e_dst, (const long long*)e_src, (long long)P, atom_mol,
                                mol_ptr, (const long long*)pair_base, look, err_flag);
  NQ_LAUNCH_CHECK();
  (void)B;
  return NQ_OK;
}

int nq_hblock_assemble(const float* diag, const float* nondiag, const int32_t* mol_ptr, const int64_t* pair_base, const int64_t* pack_ptr,
                       const int64_t* mol_orb_ptr, const int32_t* orb_atom, const int32_t* orb_slot, const int32_t* look, int32_t B, int32_t S,
                       int32_t symmetrize, int64_t total, float* out_packed, int32_t* err_flag, void* stream) {
  if (!diag || !mol_ptr || !pair_base || !pack_ptr || !mol_orb_ptr || !orb_atom || !orb_slot || !look || !out_packed || !err_flag)
    return nq_fail(NQ_ERR_ARG, "null argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "hblock_assemble");
  if (total <= 0) return NQ_OK;
  HbArgs a{diag, nondiag, mol_ptr, (const long long*)pair_base, (const long long*)pack_ptr, (const long long*)mol_orb_ptr, orb_atom, orb_slot, look, B, S, symmetrize};
  hipLaunchKernelGGL(k_hb_assemble, hb_grid(total, 256), dim3(256), 0, st, a, (long long)total, out_packed, err_flag);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_hblock_assemble_backward(const float* grad_packed, const int32_t* z, const int32_t* atom_mol, const int64_t* orb_ptr, const int64_t* pack_ptr,
                                const int64_t* mol_orb_ptr, const int32_t* inv_table, const int64_t* e_dst, const int64_t* e_src, int32_t N,
                                int64_t P, int32_t S, int32_t symmetrize, float* grad_diag, float* grad_nondiag, void* stream) {
  if (!grad_packed || !z || !atom_mol || !orb_ptr || !pack_ptr || !mol_orb_ptr || !inv_table || !grad_diag) return nq_fail(NQ_ERR_ARG, "null argument");
  if (N < 0 || P < 0) return nq_fail(NQ_ERR_ARG, "N = %d, P = %lld", N, (long long)P);
  if (P > 0 && (!e_dst || !e_src || !grad_nondiag)) return nq_fail(NQ_ERR_ARG, "P = %lld pairs without a pair list or grad_nondiag", (long long)P);
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "hblock_assemble_rev");
  HbRevArgs a{grad_packed, z, atom_mol, (const long long*)orb_ptr, (const long long*)pack_ptr, (const long long*)mol_orb_ptr, inv_table,
              (const long long*)e_dst, (const long long*)e_src, N, S, symmetrize, (long long)P};
  const long long total = ((long long)N + P) * S * S;
  if (total > 0) hipLaunchKernelGGL(k_hb_assemble_rev, hb_grid(total, 256), dim3(256), 0, st, a, grad_diag, grad_nondiag);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_hblock_packed_dense(float* packed, float* dense, const int64_t* pack_ptr, const int64_t* mol_orb_ptr, int32_t B, int64_t total, int64_t m_total,
                           int32_t to_dense, void* stream) {
  if (!packed || !dense || !pack_ptr || !mol_orb_ptr) return nq_fail(NQ_ERR_ARG, "null argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "hblock_dense");
  if (to_dense) NQ_HIP(hipMemsetAsync(dense, 0, (size_t)m_total * m_total * sizeof(float), st));
  if (total > 0) hipLaunchKernelGGL(k_hb_scatter_dense, hb_grid(total, 256), dim3(256), 0, st, packed, (const long long*)pack_ptr, (const long long*)mol_orb_ptr, B,
                                    (long long)total, (long long)m_total, dense, to_dense);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_hamiltonian_loss(const float* pred_packed, const float* target_packed, int64_t total, float grad_scale, float* stats3, float* grad_packed,
                        double* scratch, void* stream) {
  if (!pred_packed || !target_packed || !stats3 || !scratch || total <= 0) return nq_fail(NQ_ERR_ARG, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "hamiltonian_loss");
  hipLaunchKernelGGL(k_hb_loss_partial, dim3(HB_RED_BLOCKS), dim3(256), 0, st, pred_packed, target_packed, (long long)total, scratch);
  NQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hb_loss_final, dim3(1), dim3(64), 0, st, scratch, HB_RED_BLOCKS, (long long)total, stats3);
  NQ_LAUNCH_CHECK();
  if (grad_packed) {
    hipLaunchKernelGGL(k_hb_loss_grad, hb_grid(total, 256), dim3(256), 0, st, pred_packed, target_packed, (long long)total, stats3, grad_scale, grad_packed);
    NQ_LAUNCH_CHECK();
  }
  return NQ_OK;
}

}  // extern "C"

// =====================================================================================================================================
// PhiSNet: irreducible representations -> matrix blocks (NeuralNetwork.matrix_block / generate_matrix_from_irreps,
// /root/reference/nablaDFT/phisnet/nn/neural_network.py:636-706, and the irreps collection loops of forward, :859-918):
//   block(i, j)[(n_i, m_i), (n_j, m_j)] = sum_L sqrt(2L+1) sum_M CG(l_i m_i, l_j m_j | L M) * f_L[row(i, j)][M][idx(z_i, z_j, n_i, n_j, L)]
// with f = features of the atom (diagonal block) or of the ordered pair (off-diagonal block).  The reference walks atoms x atoms x shells
// x shells x L in Python and stacks per-element-pair tensors; here one thread per packed matrix element evaluates the sum from tables.
// Same packed layout and per-batch tables (orbital -> atom / local orbital, ordered pair -> pair row) as the QHNet assembly above.
// =====================================================================================================================================
#define IR_MAXORB 32      // orbitals per atom (table stride)
#define IR_LMAX 2         // highest shell angular momentum (s, p, d)
#define IR_NL (2 * IR_LMAX + 1)
struct IrTables {
  const int* tz;            // [Zt] element -> type index or -1
  const int* sh_n; const int* sh_l; const int* sh_m;     // [T][IR_MAXORB] local orbital -> shell number, l, m + l
  const int* sh_off;        // [T][IR_MAXORB] shell number -> first local orbital of that shell
  const int* idx_ii;        // [T][S][S][IR_NL] feature index or -1 (S = IR_MAXORB shells max)
  const int* idx_ij;        // [T][T][S][S][IR_NL]
  const float* cgt;         // [3][3][IR_NL][5][5][9] sqrt(2L+1) * CG(l_i, l_j, L)[m_i][m_j][M] (model's sign convention)
  int T, S;
};
struct IrArgs {
  const float* f_ii; const float* f_ij;        // [N][ncomp][Fo], [P][ncomp][Fo]
  const int* z; const int* mol_ptr; const long long* pair_base; const long long* pack_ptr; const long long* mol_orb_ptr; const long long* orb_ptr;
  const int* ORB_ATOM; const int* ORB_SLOT; const int* LOOK;
  int B, ncomp, Fo, symmetrize, unit_diagonal;
};
__device__ __forceinline__ long ir_cg_index(int li, int lj, int L, int mi, int mj, int M) { return ((((long)(li * 3 + lj) * IR_NL + L) * 5 + mi) * 5 + mj) * 9 + M; }

__device__ __forceinline__ float ir_elem(const IrArgs& a, const IrTables& t, int b, int ai, int aj, int ti, int tj, int* err) {
  const int tzi = t.tz[a.z[ai]], tzj = t.tz[a.z[aj]];
  const int ni = t.sh_n[tzi * IR_MAXORB + ti], li = t.sh_l[tzi * IR_MAXORB + ti], mi = t.sh_m[tzi * IR_MAXORB + ti];
  const int nj = t.sh_n[tzj * IR_MAXORB + tj], lj = t.sh_l[tzj * IR_MAXORB + tj], mj = t.sh_m[tzj * IR_MAXORB + tj];
  const float* frow; const int* idx;
  if (ai == aj) {
    frow = a.f_ii + (long)ai * a.ncomp * a.Fo;
    idx = t.idx_ii + (((long)tzi * t.S + ni) * t.S + nj) * IR_NL;
  } else {
    const int a0 = a.mol_ptr[b], n = a.mol_ptr[b + 1] - a0;
    const int e = a.LOOK[a.pair_base[b] + (long)(ai - a0) * n + (aj - a0)];
    if (e < 0) { atomicOr(err, 2); return 0.f; }
    frow = a.f_ij + (long)e * a.ncomp * a.Fo;
    idx = t.idx_ij + ((((long)tzi * t.T + tzj) * t.S + ni) * t.S + nj) * IR_NL;
  }
  float val = 0.f;
  const int Lmin = li > lj ? li - lj : lj - li;
  for (int L = Lmin; L <= li + lj; ++L) {
    const int fi = idx[L];
    if (fi < 0) { atomicOr(err, 4); continue; }      // the model has no irrep for this (element pair, shells, L)
    const float* cg = t.cgt + ir_cg_index(li, lj, L, mi, mj, 0);
    for (int M = 0; M < 2 * L + 1; ++M) val = fmaf(cg[M], frow[(long)(L * L + M) * a.Fo + fi], val);
  }
  return val;
}

__global__ void k_ir_assemble(IrArgs a, IrTables t, long long total, float* __restrict__ out, int* __restrict__ err) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  const int b = hb_find_mol(a.pack_ptr, a.B, q);
  const long long o0 = a.mol_orb_ptr[b];
  const int M = (int)(a.mol_orb_ptr[b + 1] - o0);
  const long long loc = q - a.pack_ptr[b];
  const int r = (int)(loc / M), c = (int)(loc % M);
  if (a.unit_diagonal && r == c) { out[q] = 1.0f; return; }                    // overlap matrix: diagonal = 1 (neural_network.py:964-965)
  const int ai = a.ORB_ATOM[o0 + r], aj = a.ORB_ATOM[o0 + c], ti = a.ORB_SLOT[o0 + r], tj = a.ORB_SLOT[o0 + c];
  float val = ir_elem(a, t, b, ai, aj, ti, tj, err);
  if (a.symmetrize) val += ir_elem(a, t, b, aj, ai, tj, ti, err);              // matrix + matrix^T (neural_network.py:931)
  out[q] = val;
}

// reverse: one thread per feature element (row, component (L, M), feature index).  inv tables: [T][IR_NL][Fo] / [T][T][IR_NL][Fo] -> n_i * S + n_j or -1
struct IrRevArgs {
  const float* G; const int* z; const int* atom_mol; const long long* e_i; const long long* e_j;
  const long long* pack_ptr; const long long* mol_orb_ptr; const long long* orb_ptr;
  const int* inv_ii; const int* inv_ij;
  long long N, P; int ncomp, Fo, symmetrize, unit_diagonal;
};
__global__ void k_ir_assemble_rev(IrRevArgs a, IrTables t, float* __restrict__ g_ii, float* __restrict__ g_ij) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = (long long)a.ncomp * a.Fo, nii = a.N * per, total = nii + a.P * per;
  if (idx >= total) return;
  const bool diag = idx < nii;
  const long long k = diag ? idx : idx - nii;
  const long long row = k / per; const int comp = (int)((k % per) / a.Fo), fo = (int)(k % a.Fo);
  int L = 0;
  while ((L + 1) * (L + 1) <= comp) ++L;
  const int M = comp - L * L;
  float* dst = diag ? g_ii + k : g_ij + k;
  if (L >= IR_NL) { *dst = 0.f; return; }
  const int ai = diag ? (int)row : (int)a.e_i[row], aj = diag ? (int)row : (int)a.e_j[row];
  const int tzi = t.tz[a.z[ai]], tzj = t.tz[a.z[aj]];
  const int code = diag ? a.inv_ii[((long)tzi * IR_NL + L) * a.Fo + fo] : a.inv_ij[(((long)tzi * t.T + tzj) * IR_NL + L) * a.Fo + fo];
  if (code < 0) { *dst = 0.f; return; }
  const int ni = code / t.S, nj = code % t.S;
  const int oi = t.sh_off[tzi * IR_MAXORB + ni], oj = t.sh_off[tzj * IR_MAXORB + nj];
  const int li = t.sh_l[tzi * IR_MAXORB + oi], lj = t.sh_l[tzj * IR_MAXORB + oj];
  const int b = a.atom_mol[ai];
  const long long o0 = a.mol_orb_ptr[b];
  const int Mo = (int)(a.mol_orb_ptr[b + 1] - o0);
  const int r0 = (int)(a.orb_ptr[ai] - o0) + oi, c0 = (int)(a.orb_ptr[aj] - o0) + oj;
  const float* Gm = a.G + a.pack_ptr[b];
  float g = 0.f;
  for (int mi = 0; mi < 2 * li + 1; ++mi)
    for (int mj = 0; mj < 2 * lj + 1; ++mj) {
      const int r = r0 + mi, c = c0 + mj;
      if (a.unit_diagonal && r == c) continue;
      float gg = Gm[(long long)r * Mo + c];
      if (a.symmetrize) gg += Gm[(long long)c * Mo + r];
      g = fmaf(t.cgt[ir_cg_index(li, lj, L, mi, mj, M)], gg, g);
    }
  *dst = g;
}

extern "C" {

int nq_irreps_assemble(const float* f_ii, const float* f_ij, const int32_t* z, const int32_t* mol_ptr, const int64_t* pair_base, const int64_t* pack_ptr,
                       const int64_t* mol_orb_ptr, const int64_t* orb_ptr, const int32_t* orb_atom, const int32_t* orb_local, const int32_t* look,
                       int32_t B, int32_t ncomp, int32_t Fo, const int32_t* tz, const int32_t* sh_n, const int32_t* sh_l, const int32_t* sh_m,
                       const int32_t* sh_off, const int32_t* idx_ii, const int32_t* idx_ij, const float* cg_table, int32_t T, int32_t S,
                       int32_t symmetrize, int32_t unit_diagonal, int64_t total, float* out_packed, int32_t* err_flag, void* stream) {
  if (!f_ii || !z || !mol_ptr || !pair_base || !pack_ptr || !mol_orb_ptr || !orb_ptr || !orb_atom || !orb_local || !look || !tz || !sh_n || !sh_l ||
      !sh_m || !sh_off || !idx_ii || !idx_ij || !cg_table || !out_packed || !err_flag)
    return nq_fail(NQ_ERR_ARG, "null argument");
  if (S > IR_MAXORB) return nq_fail(NQ_ERR_ARG, "more than %d shells per atom", IR_MAXORB);
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "irreps_assemble");
  if (total <= 0) return NQ_OK;
  IrArgs a{f_ii, f_ij, z, mol_ptr, (const long long*)pair_base, (const long long*)pack_ptr, (const long long*)mol_orb_ptr, (const long long*)orb_ptr,
           orb_atom, orb_local, look, B, ncomp, Fo, symmetrize, unit_diagonal};
  IrTables t{tz, sh_n, sh_l, sh_m, sh_off, idx_ii, idx_ij, cg_table, T, S};
  hipLaunchKernelGGL(k_ir_assemble, hb_grid(total, 256), dim3(256), 0, st, a, t, (long long)total, out_packed, err_flag);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_irreps_assemble_backward(const float* grad_packed, const int32_t* z, const int32_t* atom_mol, const int64_t* e_i, const int64_t* e_j,
                                const int64_t* pack_ptr, const int64_t* mol_orb_ptr, const int64_t* orb_ptr, const int32_t* inv_ii, const int32_t* inv_ij,
                                int64_t N, int64_t P, int32_t ncomp, int32_t Fo, const int32_t* tz, const int32_t* sh_n, const int32_t* sh_l,
                                const int32_t* sh_m, const int32_t* sh_off, const float* cg_table, int32_t T, int32_t S, int32_t symmetrize,
                                int32_t unit_diagonal, float* grad_f_ii, float* grad_f_ij, void* stream) {
  if (!grad_packed || !z || !atom_mol || !pack_ptr || !mol_orb_ptr || !orb_ptr || !inv_ii || !inv_ij || !tz || !sh_n || !sh_l || !sh_m || !sh_off ||
      !cg_table || !grad_f_ii)
    return nq_fail(NQ_ERR_ARG, "null argument");
  if (N < 0 || P < 0 || ncomp < 0 || Fo < 0) return nq_fail(NQ_ERR_ARG, "N = %lld, P = %lld, ncomp = %d, Fo = %d", (long long)N, (long long)P, ncomp, Fo);
  if (P > 0 && (!e_i || !e_j || !grad_f_ij)) return nq_fail(NQ_ERR_ARG, "P = %lld pairs without a pair list or grad_f_ij", (long long)P);
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "irreps_assemble_rev");
  IrRevArgs a{grad_packed, z, atom_mol, (const long long*)e_i, (const long long*)e_j, (const long long*)pack_ptr, (const long long*)mol_orb_ptr,
              (const long long*)orb_ptr, inv_ii, inv_ij, (long long)N, (long long)P, ncomp, Fo, symmetrize, unit_diagonal};
  IrTables t{tz, sh_n, sh_l, sh_m, sh_off, nullptr, nullptr, cg_table, T, S};
  const long long total = ((long long)N + P) * ncomp * Fo;
  if (total > 0) hipLaunchKernelGGL(k_ir_assemble_rev, hb_grid(total, 256), dim3(256), 0, st, a, t, grad_f_ii, grad_f_ij);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
