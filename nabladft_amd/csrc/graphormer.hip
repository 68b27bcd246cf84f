// Graphormer3D building blocks (reference nablaDFT/graphormer/graphormer_3d.py):
//   :126-146, :283-293   GaussianLayer on all ordered pairs of a molecule, unit vectors, per-atom sum of the basis      k_g3d_pair_*
//   :300-303             attention bias [pairs][heads] <-> per molecule [heads][n][n]                                  k_g3d_bias_*
//   :40-59               softmax((q scaling) k^T + bias) (dropout keep mask) v, written as [N][E]                      k_g3d_att_*<D, false>
//   :185-224             NodeTaskHead: the same probabilities times the unit vectors, force_proj{1,2,3} folded in      k_g3d_att_*<D, true>
//   :111, :180           exact (erf) GELU;  :311-316 energy_proj.layer2 (E -> 1)                                        k_g3d_gelu_*, k_g3d_rowdot_*
// Ragged layout: atoms [N] behind ptr [B+1]; the n_b^2 ordered pairs (i, j) of molecule b row-major behind pair_ptr [B+1] (int64); no padded rows, no -inf.
// Attention: a lane owns a query row (forward, query adjoint) or a key (key / value / bias adjoints); the other side of the (molecule, head) goes through LDS in
// tiles of 64 rows and is read as broadcasts; exact f32, online softmax over key tiles.  The backward recomputes the probabilities from the saved row
// log-sum-exp.  Every sum has a fixed order, nothing here uses atomics: each element of the accumulated bias adjoint is owned by one thread.
#include "common.h"
#include <math.h>

namespace {

constexpr int G3D_MAX_MOL = 512;      // largest molecule (the bias of one molecule is H n^2 floats)
constexpr int G3D_MAX_K = 256;        // Gaussian kernels: up to 4 per lane
constexpr int G3D_KPL = G3D_MAX_K / 64;
constexpr int G3D_EDGE_TYPES = 64 * 64;
constexpr int G3D_CHUNK = 128;        // rows per partial sum of the column reductions

// ---- column sums in a fixed order: part[chunk][c] = sum of the chunk's rows, then the chunks in order -------------------------------------------------------
__global__ __launch_bounds__(256) void k_g3d_rows_partial(const float* __restrict__ in, long rows, int C, int rows_per_chunk, float* __restrict__ part) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= C) return;
  const long r0 = (long)blockIdx.x * rows_per_chunk, r1 = min(rows, r0 + rows_per_chunk);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  long r = r0;
  for (; r + 3 < r1; r += 4) { a0 += in[r * C + c]; a1 += in[(r + 1) * C + c]; a2 += in[(r + 2) * C + c]; a3 += in[(r + 3) * C + c]; }
  for (; r < r1; ++r) a0 += in[r * C + c];
  part[(long)blockIdx.x * C + c] = (a0 + a1) + (a2 + a3);
}
size_t g3d_colsum_scratch(long rows, int C) { return (size_t)nq_cdiv(rows > 0 ? rows : 1, G3D_CHUNK) * C; }
int g3d_colsum(hipStream_t st, const float* in, long rows, int C, float* out, float* scratch) {
  if (rows <= 0) { NQ_HIP(hipMemsetAsync(out, 0, sizeof(float) * C, st)); return NQ_OK; }
  const int chunks = nq_cdiv(rows, G3D_CHUNK);
  const dim3 g1(chunks, nq_cdiv(C, 256));
  hipLaunchKernelGGL(k_g3d_rows_partial, g1, dim3(256), 0, st, in, rows, C, G3D_CHUNK, chunks == 1 ? out : scratch);
  NQ_LAUNCH_CHECK();
  if (chunks > 1) {
    hipLaunchKernelGGL(k_g3d_rows_partial, dim3(1, nq_cdiv(C, 256)), dim3(256), 0, st, (const float*)scratch, (long)chunks, C, chunks, out);
    NQ_LAUNCH_CHECK();
  }
  return NQ_OK;
}

// ---- pair featuriser: one wavefront per atom row i, lanes stride the Gaussian kernels ---------------------------------------------------------------------------
struct G3dPair {
  const float* pos; const int* z; const int* ptr; const int* atom_mol; const long* pair_ptr;
  const float* mul; const float* bias; const float* means; const float* stds; int N, K;
};
__device__ __forceinline__ float g3d_norm_a() { return (float)__builtin_sqrt(2.0 * 3.14159); }     // the reference's truncated pi (:121-122), folded at compile time

__global__ __launch_bounds__(256) void k_g3d_pair_fwd(G3dPair p, float* __restrict__ gbf, float* __restrict__ unit, float* __restrict__ dist, float* __restrict__ efeat) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= p.N) return;
  const int b = p.atom_mol[i], a0 = p.ptr[b], n = p.ptr[b + 1] - a0;
  const long base = p.pair_ptr[b] + (long)(i - a0) * n;
  const float xi = p.pos[3 * i], yi = p.pos[3 * i + 1], zi = p.pos[3 * i + 2];
  const int ti = p.z[i] * 64;
  float mean[G3D_KPL], sd[G3D_KPL], acc[G3D_KPL];
#pragma unroll
  for (int q = 0; q < G3D_KPL; ++q) {
    const int k = lane + 64 * q;
    mean[q] = k < p.K ? p.means[k] : 0.f; sd[q] = k < p.K ? fabsf(p.stds[k]) + 1e-5f : 1.f; acc[q] = 0.f;
  }
  const float a = g3d_norm_a();
  for (int j = 0; j < n; ++j) {
    const int aj = a0 + j;
    const float dx = p.pos[3 * aj] - xi, dy = p.pos[3 * aj + 1] - yi, dz = p.pos[3 * aj + 2] - zi;
    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
    const int t = ti + p.z[aj];
    const float x = p.mul[t] * d + p.bias[t];
    if (lane == 0) {
      const float den = d + 1e-5f;
      unit[3 * (base + j)] = dx / den; unit[3 * (base + j) + 1] = dy / den; unit[3 * (base + j) + 2] = dz / den;
      dist[base + j] = d;
    }
#pragma unroll
    for (int q = 0; q < G3D_KPL; ++q) {
      const int k = lane + 64 * q;
      if (k < p.K) {
        const float u = (x - mean[q]) / sd[q];
        const float g = expf(-0.5f * (u * u)) / (a * sd[q]);
        gbf[(base + j) * p.K + k] = g;
        acc[q] += g;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < G3D_KPL; ++q) { const int k = lane + 64 * q; if (k < p.K) efeat[(long)i * p.K + k] = acc[q]; }
}

// adjoint of the row: G[(i, j), k] = ggbf[(i, j), k] + gefeat[i, k];  gx[(i, j)] = sum_k G dgbf/dx;  part[i][0][k] = sum_j G dgbf/dmean, part[i][1][k] = ... d/dstds
__global__ __launch_bounds__(256) void k_g3d_pair_bwd(G3dPair p, const float* __restrict__ ggbf, const float* __restrict__ gefeat, const float* __restrict__ dist,
                                                      float* __restrict__ gx, float* __restrict__ part) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= p.N) return;
  const int b = p.atom_mol[i], a0 = p.ptr[b], n = p.ptr[b + 1] - a0;
  const long base = p.pair_ptr[b] + (long)(i - a0) * n;
  const int ti = p.z[i] * 64;
  float mean[G3D_KPL], sd[G3D_KPL], sg[G3D_KPL], ge[G3D_KPL], gm[G3D_KPL], gs[G3D_KPL];
#pragma unroll
  for (int q = 0; q < G3D_KPL; ++q) {
    const int k = lane + 64 * q;
    const float s = k < p.K ? p.stds[k] : 1.f;
    mean[q] = k < p.K ? p.means[k] : 0.f; sd[q] = fabsf(s) + 1e-5f; sg[q] = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
    ge[q] = (k < p.K && gefeat) ? gefeat[(long)i * p.K + k] : 0.f; gm[q] = 0.f; gs[q] = 0.f;
  }
  const float a = g3d_norm_a();
  for (int j = 0; j < n; ++j) {
    const int t = ti + p.z[a0 + j];
    const float x = p.mul[t] * dist[base + j] + p.bias[t];
    float gxa = 0.f;
#pragma unroll
    for (int q = 0; q < G3D_KPL; ++q) {
      const int k = lane + 64 * q;
      if (k < p.K) {
        const float u = (x - mean[q]) / sd[q];
        const float g = expf(-0.5f * (u * u)) / (a * sd[q]);
        const float G = (ggbf ? ggbf[(base + j) * p.K + k] : 0.f) + ge[q];
        const float w = G * g / sd[q];
        gxa -= w * u; gm[q] += w * u; gs[q] += w * (u * u - 1.0f);
      }
    }
    gxa = nq_wave_sum(gxa);
    if (lane == 0) gx[base + j] = gxa;
  }
#pragma unroll
  for (int q = 0; q < G3D_KPL; ++q) {
    const int k = lane + 64 * q;
    if (k < p.K) { part[(long)i * 2 * p.K + k] = gm[q]; part[(long)i * 2 * p.K + p.K + k] = gs[q] * sg[q]; }
  }
}
// gmul[t] = sum gx d, gbias[t] = sum gx over the pairs of edge type t (order: pairs sorted by type, type_ptr [4097]); one workgroup per type, fixed order
__global__ __launch_bounds__(256) void k_g3d_type_grad(const float* __restrict__ gx, const float* __restrict__ dist, const long* __restrict__ order,
                                                       const long* __restrict__ type_ptr, float* __restrict__ gmul, float* __restrict__ gbias) {
  __shared__ float red[2][4];
  const int t = blockIdx.x;
  const long q0 = type_ptr[t], q1 = type_ptr[t + 1];
  if (q0 == q1) { if (threadIdx.x == 0) { gmul[t] = 0.f; gbias[t] = 0.f; } return; }
  float sm = 0.f, sb = 0.f;
  for (long q = q0 + threadIdx.x; q < q1; q += 256) { const long pr = order[q]; const float g = gx[pr]; sm += g * dist[pr]; sb += g; }
  sm = nq_wave_sum(sm); sb = nq_wave_sum(sb);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sm; red[1][threadIdx.x >> 6] = sb; }
  __syncthreads();
  if (threadIdx.x == 0) { gmul[t] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]); gbias[t] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]); }
}

// ---- bias layout: pair-major [P][H] <-> per molecule [H][n][n]; one workgroup per atom row -----------------------------------------------------------------------
template <bool TO_HEADS>
__global__ __launch_bounds__(256) void k_g3d_bias_layout(const float* __restrict__ in, const int* __restrict__ ptr, const int* __restrict__ atom_mol,
                                                         const long* __restrict__ pair_ptr, int H, float* __restrict__ out) {
  const int i = blockIdx.x;
  const int b = atom_mol[i], a0 = ptr[b], n = ptr[b + 1] - a0, li = i - a0;
  const long pb = pair_ptr[b];
  const long pm = (pb + (long)li * n) * H;                 // pair-major start of the row
  const long hm = pb * H + (long)li * n;                   // head-major: + h n^2 + j
  const long nn = (long)n * n;
  for (int idx = threadIdx.x; idx < n * H; idx += 256) {
    const int j = idx / H, h = idx - j * H;
    if (TO_HEADS) out[hm + h * nn + j] = in[pm + idx];
    else out[pm + idx] = in[hm + h * nn + j];
  }
}

// ---- attention ------------------------------------------------------------------------------------------------------------------------------------------------------
struct G3dAtt {
  const float* qkv;            // [N][3E]: q | k | v, head h in columns h D .. (h+1) D of each chunk
  const float* bias;           // head-major ragged
  const unsigned char* mask;   // keep mask in the bias layout, or null
  const float* unit;           // force head: [P][3]
  const float* W3;             // force head: [3][E]
  const int* ptr; const long* pair_ptr;
  int H, E; float scaling, mscale;
};

// stage rows [row0, row0 + 64) of one chunk (column offset col) of molecule rows a0 .. a0 + n into LDS [64][D], clamped to the last row
template <int D>
__device__ __forceinline__ void g3d_stage(const float* __restrict__ src, long ld, int a0, int n, int row0, int col, float scale, float (*dst)[D]) {
  constexpr int V = D / 4;
#pragma unroll
  for (int m = 0; m < V; ++m) {
    const int f = threadIdx.x + 64 * m, r = f / V, c4 = f - r * V;
    const int row = min(row0 + r, n - 1);
    float4 v = *reinterpret_cast<const float4*>(src + (long)(a0 + row) * ld + col + 4 * c4);
    v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
    *reinterpret_cast<float4*>(&dst[r][4 * c4]) = v;
  }
}
// force head: t[c] = v_row . W3[c][h D ..]
template <int D>
__device__ __forceinline__ float4 g3d_vdotw(const float* __restrict__ vrow, const float* __restrict__ W3, int E, int col) {
  float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) { const float v = vrow[c]; t0 += v * W3[col + c]; t1 += v * W3[E + col + c]; t2 += v * W3[2 * E + col + c]; }
  return make_float4(t0, t1, t2, 0.f);
}

// forward: lane = query row.  FORCE: out = fh [N][H][3] (unnormalised by the projections' bias), else out [N][E].
template <int D, bool FORCE>
__global__ __launch_bounds__(64) void k_g3d_att_fwd(G3dAtt p, float* __restrict__ out, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) float Ks[64][D];
  __shared__ __attribute__((aligned(16))) float Vs[FORCE ? 1 : 64][D];
  __shared__ float4 Ts[FORCE ? 64 : 1];
  const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
  const int a0 = p.ptr[b], n = p.ptr[b + 1] - a0;
  const int row0 = blockIdx.y * 64;
  if (row0 >= n) return;
  const int lane = threadIdx.x;
  const bool valid = row0 + lane < n;
  const int r = min(row0 + lane, n - 1);
  const long ld = 3L * p.E;
  const long brow = p.pair_ptr[b] * p.H + (long)h * n * n + (long)r * n;
  const long urow = (p.pair_ptr[b] + (long)r * n) * 3;
  float q[D], o[FORCE ? 3 : D];
  {
    const float* qr = p.qkv + (long)(a0 + r) * ld + h * D;
#pragma unroll
    for (int c = 0; c < D; ++c) q[c] = qr[c] * p.scaling;
  }
#pragma unroll
  for (int c = 0; c < (FORCE ? 3 : D); ++c) o[c] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < n; k0 += 64) {
    __syncthreads();
    g3d_stage<D>(p.qkv, ld, a0, n, k0, p.E + h * D, 1.0f, Ks);
    if (FORCE) Ts[lane] = g3d_vdotw<D>(p.qkv + (long)(a0 + min(k0 + lane, n - 1)) * ld + 2 * p.E + h * D, p.W3, p.E, h * D);
    else g3d_stage<D>(p.qkv, ld, a0, n, k0, 2 * p.E + h * D, 1.0f, Vs);
    __syncthreads();
    const int jn = min(64, n - k0);
    for (int jj = 0; jj < jn; ++jj) {
      float s = p.bias[brow + k0 + jj];
#pragma unroll
      for (int c = 0; c < D; ++c) s += q[c] * Ks[jj][c];
      const float mn = fmaxf(m, s), corr = expf(m - mn), e = expf(s - mn);
      l = l * corr + e; m = mn;
      const float w = p.mask ? (p.mask[brow + k0 + jj] ? e * p.mscale : 0.f) : e;
      if (FORCE) {
        const float4 t = Ts[jj];
        const float* u = p.unit + urow + 3 * (k0 + jj);
        o[0] = o[0] * corr + w * u[0] * t.x; o[1] = o[1] * corr + w * u[1] * t.y; o[2] = o[2] * corr + w * u[2] * t.z;
      } else {
#pragma unroll
        for (int c = 0; c < D; ++c) o[c] = o[c] * corr + w * Vs[jj][c];
      }
    }
  }
  if (!valid) return;
  const float inv = 1.0f / l;
  if (FORCE) {
    float* dst = out + ((long)(a0 + r) * p.H + h) * 3;
    dst[0] = o[0] * inv; dst[1] = o[1] * inv; dst[2] = o[2] * inv;
  } else {
    float* dst = out + (long)(a0 + r) * p.E + h * D;
#pragma unroll
    for (int c = 0; c < D; ++c) dst[c] = o[c] * inv;
  }
  lse[(long)(a0 + r) * p.H + h] = m + logf(l);
}

struct G3dAttBwd {
  const float* out;     // attention: forward output [N][E]; force head: fh [N][H][3]
  const float* gout;    // attention: [N][E]; force head: gf [N][3]
  const float* lse;     // [N][H]
  float* delta;         // [N][H] (written by the query kernel, read by the key kernel)
  float* gqkv;          // [N][3E]
  float* gbias;         // accumulated in place (head-major)
  float* gt;            // force head: [N][H][3] adjoint of v . W3
};

// backward, query side: delta_i = sum_j P_ij gP_ij, gq_i = scaling sum_j gS_ij k_j  (lane = query row)
template <int D, bool FORCE>
__global__ __launch_bounds__(64) void k_g3d_att_bwd_q(G3dAtt p, G3dAttBwd w) {
  __shared__ __attribute__((aligned(16))) float Ks[64][D];
  __shared__ __attribute__((aligned(16))) float Vs[FORCE ? 1 : 64][D];
  __shared__ float4 Ts[FORCE ? 64 : 1];
  const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
  const int a0 = p.ptr[b], n = p.ptr[b + 1] - a0;
  const int row0 = blockIdx.y * 64;
  if (row0 >= n) return;
  const int lane = threadIdx.x;
  const bool valid = row0 + lane < n;
  const int r = min(row0 + lane, n - 1);
  const long ld = 3L * p.E;
  const long brow = p.pair_ptr[b] * p.H + (long)h * n * n + (long)r * n;
  const long urow = (p.pair_ptr[b] + (long)r * n) * 3;
  float q[D], go[FORCE ? 3 : D], gq[D];
  float delta = 0.f;
  {
    const float* qr = p.qkv + (long)(a0 + r) * ld + h * D;
#pragma unroll
    for (int c = 0; c < D; ++c) { q[c] = qr[c] * p.scaling; gq[c] = 0.f; }
    if (FORCE) {
      const float* g = w.gout + (long)(a0 + r) * 3; const float* f = w.out + ((long)(a0 + r) * p.H + h) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) { go[c] = g[c]; delta += g[c] * f[c]; }
    } else {
      const float* g = w.gout + (long)(a0 + r) * p.E + h * D; const float* f = w.out + (long)(a0 + r) * p.E + h * D;
#pragma unroll
      for (int c = 0; c < D; ++c) { go[c] = g[c]; delta += g[c] * f[c]; }
    }
  }
  const float ls = w.lse[(long)(a0 + r) * p.H + h];
  for (int k0 = 0; k0 < n; k0 += 64) {
    __syncthreads();
    g3d_stage<D>(p.qkv, ld, a0, n, k0, p.E + h * D, 1.0f, Ks);
    if (FORCE) Ts[lane] = g3d_vdotw<D>(p.qkv + (long)(a0 + min(k0 + lane, n - 1)) * ld + 2 * p.E + h * D, p.W3, p.E, h * D);
    else g3d_stage<D>(p.qkv, ld, a0, n, k0, 2 * p.E + h * D, 1.0f, Vs);
    __syncthreads();
    const int jn = min(64, n - k0);
    for (int jj = 0; jj < jn; ++jj) {
      float s = p.bias[brow + k0 + jj];
#pragma unroll
      for (int c = 0; c < D; ++c) s += q[c] * Ks[jj][c];
      const float P = expf(s - ls);
      float gP = 0.f;
      if (FORCE) {
        const float4 t = Ts[jj];
        const float* u = p.unit + urow + 3 * (k0 + jj);
        gP = go[0] * u[0] * t.x + go[1] * u[1] * t.y + go[2] * u[2] * t.z;
      } else {
#pragma unroll
        for (int c = 0; c < D; ++c) gP += go[c] * Vs[jj][c];
      }
      if (p.mask) gP = p.mask[brow + k0 + jj] ? gP * p.mscale : 0.f;
      const float gS = P * (gP - delta);
#pragma unroll
      for (int c = 0; c < D; ++c) gq[c] += gS * Ks[jj][c];
    }
  }
  if (!valid) return;
  w.delta[(long)(a0 + r) * p.H + h] = delta;
  float* dst = w.gqkv + (long)(a0 + r) * ld + h * D;
#pragma unroll
  for (int c = 0; c < D; ++c) dst[c] = gq[c] * p.scaling;
}

// backward, key side: lane = key j; gk_j = sum_i gS_ij q_i scaling, gv_j = sum_i P_ij keep_ij go_i, gbias[i][j] += gS_ij
template <int D, bool FORCE>
__global__ __launch_bounds__(64) void k_g3d_att_bwd_kv(G3dAtt p, G3dAttBwd w) {
  __shared__ __attribute__((aligned(16))) float Qs[64][D];
  __shared__ __attribute__((aligned(16))) float Gs[FORCE ? 1 : 64][D];
  __shared__ float4 Gf[FORCE ? 64 : 1];
  __shared__ float2 St[64];                                 // (lse, delta) of the query rows
  const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
  const int a0 = p.ptr[b], n = p.ptr[b + 1] - a0;
  const int key0 = blockIdx.y * 64;
  if (key0 >= n) return;
  const int lane = threadIdx.x;
  const bool valid = key0 + lane < n;
  const int j = min(key0 + lane, n - 1);
  const long ld = 3L * p.E;
  const long bhead = p.pair_ptr[b] * p.H + (long)h * n * n;
  const long ubase = p.pair_ptr[b] * 3;
  float k[D], v[FORCE ? 3 : D], gk[D], gv[FORCE ? 3 : D];
  {
    const float* kr = p.qkv + (long)(a0 + j) * ld + p.E + h * D;
#pragma unroll
    for (int c = 0; c < D; ++c) { k[c] = kr[c]; gk[c] = 0.f; }
    const float* vr = p.qkv + (long)(a0 + j) * ld + 2 * p.E + h * D;
    if (FORCE) { const float4 t = g3d_vdotw<D>(vr, p.W3, p.E, h * D); v[0] = t.x; v[1] = t.y; v[2] = t.z; }
    else {
#pragma unroll
      for (int c = 0; c < D; ++c) v[c] = vr[c];
    }
#pragma unroll
    for (int c = 0; c < (FORCE ? 3 : D); ++c) gv[c] = 0.f;
  }
  for (int i0 = 0; i0 < n; i0 += 64) {
    __syncthreads();
    g3d_stage<D>(p.qkv, ld, a0, n, i0, h * D, p.scaling, Qs);
    const int ri = a0 + min(i0 + lane, n - 1);
    if (FORCE) { const float* g = w.gout + (long)ri * 3; Gf[lane] = make_float4(g[0], g[1], g[2], 0.f); }
    else g3d_stage<D>(w.gout, (long)p.E, a0, n, i0, h * D, 1.0f, Gs);
    St[lane] = make_float2(w.lse[(long)ri * p.H + h], w.delta[(long)ri * p.H + h]);
    __syncthreads();
    const int in_ = min(64, n - i0);
    for (int ii = 0; ii < in_; ++ii) {
      const long bij = bhead + (long)(i0 + ii) * n + j;
      float s = p.bias[bij];
#pragma unroll
      for (int c = 0; c < D; ++c) s += Qs[ii][c] * k[c];
      const float2 st = St[ii];
      const float P = expf(s - st.x);
      const float keep = p.mask ? (p.mask[bij] ? p.mscale : 0.f) : 1.0f;
      float gP = 0.f;
      if (FORCE) {
        const float4 g = Gf[ii];
        const float* u = p.unit + ubase + ((long)(i0 + ii) * n + j) * 3;
        const float c0 = g.x * u[0], c1 = g.y * u[1], c2 = g.z * u[2];
        gP = c0 * v[0] + c1 * v[1] + c2 * v[2];
        const float pk = P * keep;
        gv[0] += pk * c0; gv[1] += pk * c1; gv[2] += pk * c2;
      } else {
        const float pk = P * keep;
#pragma unroll
        for (int c = 0; c < D; ++c) { gP += Gs[ii][c] * v[c]; gv[c] += pk * Gs[ii][c]; }
      }
      const float gS = P * (gP * keep - st.y);
      if (valid) w.gbias[bij] += gS;
#pragma unroll
      for (int c = 0; c < D; ++c) gk[c] += gS * Qs[ii][c];
    }
  }
  if (!valid) return;
  float* dk = w.gqkv + (long)(a0 + j) * ld + p.E + h * D;
  float* dv = w.gqkv + (long)(a0 + j) * ld + 2 * p.E + h * D;
#pragma unroll
  for (int c = 0; c < D; ++c) dk[c] = gk[c];
  if (FORCE) {
    float* gt = w.gt + ((long)(a0 + j) * p.H + h) * 3;
    gt[0] = gv[0]; gt[1] = gv[1]; gt[2] = gv[2];
#pragma unroll
    for (int c = 0; c < D; ++c) dv[c] = gv[0] * p.W3[h * D + c] + gv[1] * p.W3[p.E + h * D + c] + gv[2] * p.W3[2 * p.E + h * D + c];
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) dv[c] = gv[c];
  }
}

// force head: f[i][c] = sum_h fh[i][h][c] + b3[c]
__global__ void k_g3d_force_heads(const float* __restrict__ fh, const float* __restrict__ b3, long N, int H, float* __restrict__ f) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * 3) return;
  const long i = t / 3; const int c = (int)(t - i * 3);
  float s = 0.f;
  for (int h = 0; h < H; ++h) s += fh[(i * H + h) * 3 + c];
  f[t] = s + b3[c];
}
// part[chunk][c][e] = sum over the chunk's atoms of gt[j][h(e)][c] v[j][e]
__global__ __launch_bounds__(256) void k_g3d_force_wgrad(const float* __restrict__ gt, const float* __restrict__ qkv, long N, int H, int E, int D,
                                                         float* __restrict__ part) {
  const int t = blockIdx.y * 256 + threadIdx.x;
  if (t >= 3 * E) return;
  const int c = t / E, e = t - c * E, h = e / D;
  const long j0 = (long)blockIdx.x * G3D_CHUNK, j1 = min(N, j0 + G3D_CHUNK);
  float s = 0.f;
  for (long j = j0; j < j1; ++j) s += gt[(j * H + h) * 3 + c] * qkv[j * 3 * E + 2 * E + e];
  part[(long)blockIdx.x * 3 * E + t] = s;
}

// ---- exact GELU (+ bias over the last axis) ----------------------------------------------------------------------------------------------------------------------
__global__ void k_g3d_gelu(const float* __restrict__ x, const float* __restrict__ bias, const float* __restrict__ g, long count, int C, float* __restrict__ out) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const float v = x[t] + (bias ? bias[t % C] : 0.f);
  const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752f));
  if (g) out[t] = g[t] * (cdf + v * 0.39894228040143268f * expf(-0.5f * v * v));
  else out[t] = v * cdf;
}

// ---- row dot (Linear E -> 1): one wavefront per row ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_g3d_rowdot_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, long rows, int C,
                                                        float* __restrict__ y) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += x[r * C + c] * w[c];
  s = nq_wave_sum(s);
  if (lane == 0) y[r] = s + (b ? b[0] : 0.f);
}
// gx[r][c] = g[r] w[c]; part[chunk][c] = sum_r g[r] x[r][c] (c < C), part[chunk][C] = sum_r g[r]
__global__ __launch_bounds__(256) void k_g3d_rowdot_bwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ g, long rows, int C,
                                                        float* __restrict__ gx, float* __restrict__ part) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c > C) return;
  const long r0 = (long)blockIdx.x * G3D_CHUNK, r1 = min(rows, r0 + G3D_CHUNK);
  float s = 0.f;
  if (c == C) { for (long r = r0; r < r1; ++r) s += g[r]; }
  else {
    const float wc = w[c];
    for (long r = r0; r < r1; ++r) { const float gr = g[r]; s += gr * x[r * C + c]; gx[r * C + c] = gr * wc; }
  }
  part[(long)blockIdx.x * (C + 1) + c] = s;
}

int g3d_check_att(const char* what, const void* qkv, const void* bias, const void* ptr, const void* pair_ptr, int B, long N, int H, int D, int max_mol_atoms) {
  if (!qkv || !bias || !ptr || !pair_ptr || B < 1 || N < 1 || H < 1) return nq_fail(NQ_ERR_ARG, "%s: bad argument", what);
  if (D != 16 && D != 32) return nq_fail(NQ_ERR_ARG, "%s: head dimension %d is not built (16, 32)", what, D);
  if (max_mol_atoms < 1) return nq_fail(NQ_ERR_ARG, "%s: max_mol_atoms < 1", what);
  if (max_mol_atoms > G3D_MAX_MOL) return nq_fail(NQ_ERR_MOL_TOO_LARGE, "%s: a molecule of %d atoms exceeds the limit of %d", what, max_mol_atoms, G3D_MAX_MOL);
  return NQ_OK;
}

template <bool FORCE>
int g3d_att_fwd(hipStream_t st, const G3dAtt& p, int B, int D, int max_mol_atoms, float* out, float* lse) {
  const dim3 grid((unsigned)B * p.H, nq_cdiv(max_mol_atoms, 64));
  if (D == 16) hipLaunchKernelGGL((k_g3d_att_fwd<16, FORCE>), grid, dim3(64), 0, st, p, out, lse);
  else hipLaunchKernelGGL((k_g3d_att_fwd<32, FORCE>), grid, dim3(64), 0, st, p, out, lse);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
template <bool FORCE>
int g3d_att_bwd(hipStream_t st, const G3dAtt& p, const G3dAttBwd& w, int B, int D, int max_mol_atoms) {
  const dim3 grid((unsigned)B * p.H, nq_cdiv(max_mol_atoms, 64));
  if (D == 16) {
    hipLaunchKernelGGL((k_g3d_att_bwd_q<16, FORCE>), grid, dim3(64), 0, st, p, w);
    hipLaunchKernelGGL((k_g3d_att_bwd_kv<16, FORCE>), grid, dim3(64), 0, st, p, w);
  } else {
    hipLaunchKernelGGL((k_g3d_att_bwd_q<32, FORCE>), grid, dim3(64), 0, st, p, w);
    hipLaunchKernelGGL((k_g3d_att_bwd_kv<32, FORCE>), grid, dim3(64), 0, st, p, w);
  }
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // namespace

extern "C" {

int32_t nq_g3d_max_mol_atoms(void) { return G3D_MAX_MOL; }

int nq_g3d_pair_forward(const float* pos, const int32_t* z, const int32_t* ptr, const int32_t* atom_mol, const int64_t* pair_ptr, const float* mul, const float* bias,
                        const float* means, const float* stds, int32_t N, int32_t K, int32_t max_mol_atoms, float* gbf, float* unit, float* dist, float* efeat,
                        void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_pair_fwd");
  if (N <= 0) return NQ_OK;
  if (!pos || !z || !ptr || !atom_mol || !pair_ptr || !mul || !bias || !means || !stds || !gbf || !unit || !dist || !efeat || K < 1 || K > G3D_MAX_K)
    return nq_fail(NQ_ERR_ARG, "g3d_pair_forward: bad argument (1 <= num_kernel <= %d)", G3D_MAX_K);
  if (max_mol_atoms > G3D_MAX_MOL) return nq_fail(NQ_ERR_MOL_TOO_LARGE, "g3d_pair_forward: a molecule of %d atoms exceeds the limit of %d", max_mol_atoms, G3D_MAX_MOL);
  const G3dPair p{pos, z, ptr, atom_mol, (const long*)pair_ptr, mul, bias, means, stds, N, K};
  hipLaunchKernelGGL(k_g3d_pair_fwd, dim3(nq_cdiv(N, 4)), dim3(256), 0, st, p, gbf, unit, dist, efeat);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

size_t nq_g3d_pair_scratch_floats(int32_t N, int64_t P, int32_t K) {
  return (size_t)(P > 0 ? P : 0) + (size_t)(N > 0 ? N : 0) * 2 * K + g3d_colsum_scratch(N, 2 * K) + 2 * (size_t)K + 64;
}
int nq_g3d_pair_backward(const float* pos, const int32_t* z, const int32_t* ptr, const int32_t* atom_mol, const int64_t* pair_ptr, const float* mul, const float* bias,
                         const float* means, const float* stds, const float* dist, const int64_t* order, const int64_t* type_ptr, int32_t N, int64_t P, int32_t K,
                         const float* grad_gbf, const float* grad_efeat, float* grad_means, float* grad_stds, float* grad_mul, float* grad_bias, float* scratch,
                         void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_pair_bwd");
  if (!grad_means || !grad_stds || !grad_mul || !grad_bias || K < 1 || K > G3D_MAX_K) return nq_fail(NQ_ERR_ARG, "g3d_pair_backward: bad argument");
  if (N <= 0) {
    NQ_HIP(hipMemsetAsync(grad_means, 0, sizeof(float) * K, st)); NQ_HIP(hipMemsetAsync(grad_stds, 0, sizeof(float) * K, st));
    NQ_HIP(hipMemsetAsync(grad_mul, 0, sizeof(float) * G3D_EDGE_TYPES, st)); NQ_HIP(hipMemsetAsync(grad_bias, 0, sizeof(float) * G3D_EDGE_TYPES, st));
    return NQ_OK;
  }
  if (!pos || !z || !ptr || !atom_mol || !pair_ptr || !mul || !bias || !means || !stds || !dist || !order || !type_ptr || !scratch || (!grad_gbf && !grad_efeat))
    return nq_fail(NQ_ERR_ARG, "g3d_pair_backward: null argument");
  const G3dPair p{pos, z, ptr, atom_mol, (const long*)pair_ptr, mul, bias, means, stds, N, K};
  float* gx = scratch;
  float* part = gx + P;
  float* red = part + (size_t)N * 2 * K;
  hipLaunchKernelGGL(k_g3d_pair_bwd, dim3(nq_cdiv(N, 4)), dim3(256), 0, st, p, grad_gbf, grad_efeat, dist, gx, part);
  NQ_LAUNCH_CHECK();
  // part rows are [means | stds]: one column sum over the atoms, split afterwards
  float* both = red + g3d_colsum_scratch(N, 2 * K);
  NQ_TRY(g3d_colsum(st, part, N, 2 * K, both, red));
  NQ_HIP(hipMemcpyAsync(grad_means, both, sizeof(float) * K, hipMemcpyDeviceToDevice, st));
  NQ_HIP(hipMemcpyAsync(grad_stds, both + K, sizeof(float) * K, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_g3d_type_grad, dim3(G3D_EDGE_TYPES), dim3(256), 0, st, (const float*)gx, dist, (const long*)order, (const long*)type_ptr, grad_mul, grad_bias);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_g3d_bias_to_heads(const float* pair_major, const int32_t* ptr, const int32_t* atom_mol, const int64_t* pair_ptr, int32_t N, int32_t H, float* head_major,
                         void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_bias_to_heads");
  if (N <= 0) return NQ_OK;
  if (!pair_major || !ptr || !atom_mol || !pair_ptr || !head_major || H < 1) return nq_fail(NQ_ERR_ARG, "g3d_bias_to_heads: bad argument");
  hipLaunchKernelGGL(k_g3d_bias_layout<true>, dim3(N), dim3(256), 0, st, pair_major, ptr, atom_mol, (const long*)pair_ptr, H, head_major);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_g3d_bias_from_heads(const float* head_major, const int32_t* ptr, const int32_t* atom_mol, const int64_t* pair_ptr, int32_t N, int32_t H, float* pair_major,
                           void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_bias_from_heads");
  if (N <= 0) return NQ_OK;
  if (!pair_major || !ptr || !atom_mol || !pair_ptr || !head_major || H < 1) return nq_fail(NQ_ERR_ARG, "g3d_bias_from_heads: bad argument");
  hipLaunchKernelGGL(k_g3d_bias_layout<false>, dim3(N), dim3(256), 0, st, head_major, ptr, atom_mol, (const long*)pair_ptr, H, pair_major);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_g3d_attention_forward(const float* qkv, const float* bias_heads, const uint8_t* keep_mask, float mask_scale, const int32_t* ptr, const int64_t* pair_ptr,
                             int32_t B, int32_t N, int32_t H, int32_t D, int32_t max_mol_atoms, float scaling, float* out, float* lse, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_att_fwd");
  NQ_TRY(g3d_check_att("g3d_attention_forward", qkv, bias_heads, ptr, pair_ptr, B, N, H, D, max_mol_atoms));
  if (!out || !lse) return nq_fail(NQ_ERR_ARG, "g3d_attention_forward: null output");
  const G3dAtt p{qkv, bias_heads, keep_mask, nullptr, nullptr, ptr, (const long*)pair_ptr, H, H * D, scaling, mask_scale};
  return g3d_att_fwd<false>(st, p, B, D, max_mol_atoms, out, lse);
}
int nq_g3d_attention_backward(const float* qkv, const float* bias_heads, const uint8_t* keep_mask, float mask_scale, const int32_t* ptr, const int64_t* pair_ptr,
                              int32_t B, int32_t N, int32_t H, int32_t D, int32_t max_mol_atoms, float scaling, const float* out, const float* lse,
                              const float* grad_out, float* grad_qkv, float* grad_bias_heads, float* scratch, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_att_bwd");
  NQ_TRY(g3d_check_att("g3d_attention_backward", qkv, bias_heads, ptr, pair_ptr, B, N, H, D, max_mol_atoms));
  if (!out || !lse || !grad_out || !grad_qkv || !grad_bias_heads || !scratch) return nq_fail(NQ_ERR_ARG, "g3d_attention_backward: null argument");
  const G3dAtt p{qkv, bias_heads, keep_mask, nullptr, nullptr, ptr, (const long*)pair_ptr, H, H * D, scaling, mask_scale};
  const G3dAttBwd w{out, grad_out, lse, scratch, grad_qkv, grad_bias_heads, nullptr};
  return g3d_att_bwd<false>(st, p, w, B, D, max_mol_atoms);
}

int nq_g3d_force_forward(const float* qkv, const float* bias_heads, const uint8_t* keep_mask, float mask_scale, const float* unit, const float* W3, const float* b3,
                         const int32_t* ptr, const int64_t* pair_ptr, int32_t B, int32_t N, int32_t H, int32_t D, int32_t max_mol_atoms, float scaling,
                         float* head_forces, float* lse, float* forces, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_force_fwd");
  NQ_TRY(g3d_check_att("g3d_force_forward", qkv, bias_heads, ptr, pair_ptr, B, N, H, D, max_mol_atoms));
  if (!unit || !W3 || !b3 || !head_forces || !lse || !forces) return nq_fail(NQ_ERR_ARG, "g3d_force_forward: null argument");
  const G3dAtt p{qkv, bias_heads, keep_mask, unit, W3, ptr, (const long*)pair_ptr, H, H * D, scaling, mask_scale};
  NQ_TRY(g3d_att_fwd<true>(st, p, B, D, max_mol_atoms, head_forces, lse));
  hipLaunchKernelGGL(k_g3d_force_heads, dim3(nq_cdiv((long)N * 3, 256)), dim3(256), 0, st, (const float*)head_forces, b3, (long)N, H, forces);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
size_t nq_g3d_force_scratch_floats(int32_t N, int32_t H, int32_t D) {
  const size_t n = N > 0 ? N : 0;
  return n * H + n * H * 3 + (size_t)nq_cdiv(n ? n : 1, G3D_CHUNK) * 3 * H * D + g3d_colsum_scratch(nq_cdiv(n ? n : 1, G3D_CHUNK), 3 * H * D) + g3d_colsum_scratch(n, 3) + 64;
}
int nq_g3d_force_backward(const float* qkv, const float* bias_heads, const uint8_t* keep_mask, float mask_scale, const float* unit, const float* W3,
                          const int32_t* ptr, const int64_t* pair_ptr, int32_t B, int32_t N, int32_t H, int32_t D, int32_t max_mol_atoms, float scaling,
                          const float* head_forces, const float* lse, const float* grad_forces, float* grad_qkv, float* grad_bias_heads, float* grad_W3,
                          float* grad_b3, float* scratch, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_force_bwd");
  NQ_TRY(g3d_check_att("g3d_force_backward", qkv, bias_heads, ptr, pair_ptr, B, N, H, D, max_mol_atoms));
  if (!unit || !W3 || !head_forces || !lse || !grad_forces || !grad_qkv || !grad_bias_heads || !grad_W3 || !grad_b3 || !scratch)
    return nq_fail(NQ_ERR_ARG, "g3d_force_backward: null argument");
  const int E = H * D;
  const int chunks = nq_cdiv(N, G3D_CHUNK);
  float* delta = scratch;
  float* gt = delta + (size_t)N * H;
  float* part = gt + (size_t)N * H * 3;
  float* red = part + (size_t)chunks * 3 * E;
  float* red3 = red + g3d_colsum_scratch(chunks, 3 * E);
  const G3dAtt p{qkv, bias_heads, keep_mask, unit, W3, ptr, (const long*)pair_ptr, H, E, scaling, mask_scale};
  const G3dAttBwd w{head_forces, grad_forces, lse, delta, grad_qkv, grad_bias_heads, gt};
  NQ_TRY(g3d_att_bwd<true>(st, p, w, B, D, max_mol_atoms));
  hipLaunchKernelGGL(k_g3d_force_wgrad, dim3(chunks, nq_cdiv(3 * E, 256)), dim3(256), 0, st, (const float*)gt, qkv, (long)N, H, E, D, part);
  NQ_LAUNCH_CHECK();
  NQ_TRY(g3d_colsum(st, part, chunks, 3 * E, grad_W3, red));
  NQ_TRY(g3d_colsum(st, grad_forces, N, 3, grad_b3, red3));
  return NQ_OK;
}

int nq_g3d_gelu_forward(const float* x, const float* bias, int64_t rows, int32_t C, float* y, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_gelu_fwd");
  if (rows <= 0) return NQ_OK;
  if (!x || !y || C < 1) return nq_fail(NQ_ERR_ARG, "g3d_gelu_forward: bad argument");
  hipLaunchKernelGGL(k_g3d_gelu, dim3(nq_cdiv(rows * C, 256)), dim3(256), 0, st, x, bias, (const float*)nullptr, (long)rows * C, C, y);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_g3d_gelu_backward(const float* x, const float* bias, const float* grad_y, int64_t rows, int32_t C, float* grad_x, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_gelu_bwd");
  if (rows <= 0) return NQ_OK;
  if (!x || !grad_y || !grad_x || C < 1) return nq_fail(NQ_ERR_ARG, "g3d_gelu_backward: bad argument");
  hipLaunchKernelGGL(k_g3d_gelu, dim3(nq_cdiv(rows * C, 256)), dim3(256), 0, st, x, bias, grad_y, (long)rows * C, C, grad_x);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_g3d_rowdot_forward(const float* x, const float* w, const float* b, int64_t rows, int32_t C, float* y, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_rowdot_fwd");
  if (rows <= 0) return NQ_OK;
  if (!x || !w || !y || C < 1) return nq_fail(NQ_ERR_ARG, "g3d_rowdot_forward: bad argument");
  hipLaunchKernelGGL(k_g3d_rowdot_fwd, dim3(nq_cdiv(rows, 4)), dim3(256), 0, st, x, w, b, (long)rows, C, y);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
size_t nq_g3d_rowdot_scratch_floats(int64_t rows, int32_t C) {
  const long chunks = nq_cdiv(rows > 0 ? rows : 1, G3D_CHUNK);
  return (size_t)chunks * (C + 1) + g3d_colsum_scratch(chunks, C + 1) + (C + 1) + 64;
}
int nq_g3d_rowdot_backward(const float* x, const float* w, const float* grad_y, int64_t rows, int32_t C, float* grad_x, float* grad_w, float* grad_b, float* scratch,
                           void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "g3d_rowdot_bwd");
  if (!grad_w || !grad_b || C < 1) return nq_fail(NQ_ERR_ARG, "g3d_rowdot_backward: bad argument");
  if (rows <= 0) { NQ_HIP(hipMemsetAsync(grad_w, 0, sizeof(float) * C, st)); NQ_HIP(hipMemsetAsync(grad_b, 0, sizeof(float), st)); return NQ_OK; }
  if (!x || !w || !grad_y || !grad_x || !scratch) return nq_fail(NQ_ERR_ARG, "g3d_rowdot_backward: null argument");
  const int chunks = nq_cdiv(rows, G3D_CHUNK);
  float* part = scratch;
  float* red = part + (size_t)chunks * (C + 1);
  float* both = red + g3d_colsum_scratch(chunks, C + 1);
  hipLaunchKernelGGL(k_g3d_rowdot_bwd, dim3(chunks, nq_cdiv(C + 1, 256)), dim3(256), 0, st, x, w, grad_y, (long)rows, C, grad_x, part);
  NQ_LAUNCH_CHECK();
  NQ_TRY(g3d_colsum(st, part, chunks, C + 1, both, red));
  NQ_HIP(hipMemcpyAsync(grad_w, both, sizeof(float) * C, hipMemcpyDeviceToDevice, st));
  NQ_HIP(hipMemcpyAsync(grad_b, both + C, sizeof(float), hipMemcpyDeviceToDevice, st));
  return NQ_OK;
}

}  // extern "C"
