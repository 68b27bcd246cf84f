// DimeNet++ building blocks (the core restated in DESIGN_details.md; wrapper: reference nablaDFT/dimenetplusplus/dimenetplusplus.py):
//   edge geometry d, u = (pos_i - pos_j) / d and its adjoint back to the positions                                   k_dn_geom_*
//   radial basis rbf [E][R] and the radial table Rad [E][S][R] of the spherical basis, evaluated in float64          k_dn_basis_*
//   triplet product m[(j->i)] = sum_{(k->j), k != i} x_kj[(k->j)] * (W_sbf2 (sum_l Y_l(cos theta) Q[(k->j)][l]))      k_dn_trip_*
//   edge helpers: x * gate, the gated sum over an atom's in-edges, the embedding block's gather + SiLU                k_dn_gate*, k_dn_embed_*
// Graph: CSR by target atom (row_ptr [N+1], src [E], dst [E], sources ascending inside a row: nq_es_graph_*); the transposed walks read the edges sorted by
// source (src_order [E], src_ptr [N+1]).  A triplet is never stored: the triplets of edge (j->i) ARE the in-row of j without k = i, and the edges that use
// (k->j) ARE the out-list of j without i = k.  One wavefront per edge, one lane per channel (I = 64 q channels: q registers per lane), the triplet loop is
// wave-uniform.  Every sum has a fixed order; nothing here uses atomics.
#include "common.h"
#include <math.h>

namespace {

constexpr int DN_MAXS = 8;        // spherical degrees l < S <= 8
constexpr int DN_MAXB = 8;        // basis_emb_size <= 8: s_b lives in lanes 0..7 and is broadcast by v_readlane
constexpr int DN_MAXR = 16;
constexpr int DN_CHUNK = 16;      // edges per wavefront of the transposed walk = rows per partial sum of the W_sbf2 gradient

#define DN_GRID(total) dim3((unsigned)(((total) + 255) / 256)), dim3(256), 0, st

// ---- float64 basis ------------------------------------------------------------------------------------------------------------------------------------------
// j_l(x): power series below x = l (the closed forms cancel like 1 / x^(l+1) there), upward recurrence from sin / cos above (stable for x >= l)
__device__ double dn_jl(int l, double x) {
  if (x < (double)l) {
    double pre = 1.0;
    for (int k = 1; k <= l; ++k) pre *= x / (double)(2 * k + 1);
    const double h = -0.5 * x * x;
    double a = 1.0, s = 1.0;
    for (int k = 1; k < 40; ++k) {
      a *= h / ((double)k * (double)(2 * l + 2 * k + 1));
      s += a;
      if (fabs(a) < 1e-18 * fabs(s)) break;
    }
    return pre * s;
  }
  const double sn = sin(x), cs = cos(x);
  double jm = sn / x;
  if (l == 0) return jm;
  double j = (sn / x - cs) / x;
  for (int n = 1; n < l; ++n) { const double jn = (double)(2 * n + 1) / x * j - jm; jm = j; j = jn; }
  return j;
}
__device__ double dn_djl(int l, double x, double jl) { return l == 0 ? -dn_jl(1, x) : dn_jl(l - 1, x) - (double)(l + 1) / x * jl; }
__device__ void dn_env(double x, int p, double& e, double& de) {
  const double a = -0.5 * (p + 1) * (p + 2), b = (double)p * (p + 2), c = -0.5 * p * (p + 1);
  const double xp2 = pow(x, (double)(p - 2));   // p >= 2
  const double xp1 = xp2 * x, xp = xp1 * x;
  e = 1.0 / x + a * xp1 + b * xp + c * xp * x;
  de = -1.0 / (x * x) + a * (p - 1) * xp2 + b * p * xp1 + c * (p + 1) * xp;
}

// thread (e, l): l < S one row of Rad, l == S the rbf row
__global__ __launch_bounds__(256) void k_dn_basis_fwd(const float* __restrict__ d, const float* __restrict__ freq, const double* __restrict__ roots,
                                                      const double* __restrict__ norms, long E, int S, int R, double inv_cutoff, int p, float* __restrict__ rbf,
                                                      float* __restrict__ rad) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= E * (S + 1)) return;
  const long e = t / (S + 1);
  const int l = (int)(t - e * (S + 1));
  const double x = (double)d[e] * inv_cutoff;
  double env, denv;
  dn_env(x, p, env, denv);
  if (l == S) {
    for (int n = 0; n < R; ++n) rbf[e * R + n] = (float)(env * sin((double)freq[n] * x));
  } else {
    for (int n = 0; n < R; ++n) rad[(e * S + l) * R + n] = (float)(env * norms[l * R + n] * dn_jl(l, roots[l * R + n] * x));
  }
}
// thread e: gd[e] = sum g_rbf drbf/dd + sum g_rad dRad/dd; gfreq_rows[e][n] = g_rbf[e][n] drbf/dfreq_n
__global__ __launch_bounds__(256) void k_dn_basis_bwd(const float* __restrict__ d, const float* __restrict__ freq, const double* __restrict__ roots,
                                                      const double* __restrict__ norms, long E, int S, int R, double inv_cutoff, int p,
                                                      const float* __restrict__ g_rbf, const float* __restrict__ g_rad, float* __restrict__ gd,
                                                      float* __restrict__ gfreq_rows) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const double x = (double)d[e] * inv_cutoff;
  double env, denv, acc = 0.0;
  dn_env(x, p, env, denv);
  for (int n = 0; n < R; ++n) {
    const double f = (double)freq[n], g = g_rbf ? (double)g_rbf[e * R + n] : 0.0;
    const double sn = sin(f * x), cs = cos(f * x);
    acc += g * (denv * sn + env * f * cs);
    gfreq_rows[e * R + n] = (float)(g * env * x * cs);
  }
  if (g_rad) {
    for (int l = 0; l < S; ++l)
      for (int n = 0; n < R; ++n) {
        const double z = roots[l * R + n], j = dn_jl(l, z * x);
        acc += (double)g_rad[(e * S + l) * R + n] * norms[l * R + n] * (denv * j + env * z * dn_djl(l, z * x, j));
      }
  }
  gd[e] = (float)(acc * inv_cutoff);
}

// ---- geometry -----------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dn_geom_fwd(const float4* __restrict__ geom, long E, float* __restrict__ d, float* __restrict__ u) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const float4 g = geom[e];              // pos[src] - pos[dst], |.|
  d[e] = g.w;
  u[3 * e] = -g.x / g.w; u[3 * e + 1] = -g.y / g.w; u[3 * e + 2] = -g.z / g.w;
}
// gvec[e] = gd u + (gu - (gu . u) u) / d: the adjoint of pos[dst] - pos[src]
__global__ __launch_bounds__(256) void k_dn_geom_gvec(const float* __restrict__ d, const float* __restrict__ u, const float* __restrict__ gd,
                                                      const float* __restrict__ gu, long E, float* __restrict__ gvec) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const float ux = u[3 * e], uy = u[3 * e + 1], uz = u[3 * e + 2], g = gd ? gd[e] : 0.f;
  float vx = g * ux, vy = g * uy, vz = g * uz;
  if (gu) {
    const float ax = gu[3 * e], ay = gu[3 * e + 1], az = gu[3 * e + 2], dot = ax * ux + ay * uy + az * uz, inv = 1.0f / d[e];
    vx += (ax - dot * ux) * inv; vy += (ay - dot * uy) * inv; vz += (az - dot * uz) * inv;
  }
  gvec[3 * e] = vx; gvec[3 * e + 1] = vy; gvec[3 * e + 2] = vz;
}
// thread (atom, component): + the in-row (this atom is the target), - the out-list (this atom is the source)
__global__ __launch_bounds__(256) void k_dn_geom_gpos(const float* __restrict__ gvec, const int* __restrict__ row_ptr, const int* __restrict__ src_order,
                                                      const int* __restrict__ src_ptr, int N, float* __restrict__ gpos) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 3 * N) return;
  const int i = t / 3, c = t - 3 * i;
  float a = 0.f, b = 0.f;
  for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) a += gvec[3 * (long)e + c];
  for (int q = src_ptr[i]; q < src_ptr[i + 1]; ++q) b += gvec[3 * (long)src_order[q] + c];
  gpos[t] = a - b;
}

// ---- triplet product ----------------------------------------------------------------------------------------------------------------------------------------
struct DnTrip {
  const float* x; const float* Q; const float* u; const float* W2;
  const int* row_ptr; const int* src; const int* dst; const int* src_order; const int* src_ptr;
  int E, S, Bs;
};
// Y_l(c) = sqrt((2l + 1) / 4 pi) P_l(c) and dY_l / dc by the Legendre recurrences (regular at c = +-1)
__device__ __forceinline__ void dn_legendre(float c, int S, float* Y, float* dY) {
  float p0 = 1.f, p1 = c, q0 = 0.f, q1 = 1.f;
#pragma unroll
  for (int l = 0; l < DN_MAXS; ++l) {
    const float nrm = sqrtf((float)(2 * l + 1) * 0.07957747154594767f);
    const float pl = l == 0 ? 1.f : p1, ql = l == 0 ? 0.f : q1;
    Y[l] = l < S ? nrm * pl : 0.f;
    if (dY) dY[l] = l < S ? nrm * ql : 0.f;
    if (l >= 1) {
      const float pn = ((float)(2 * l + 1) * c * p1 - (float)l * p0) / (float)(l + 1);
      const float qn = ((float)(2 * l + 1) * (p1 + c * q1) - (float)l * q0) / (float)(l + 1);
      p0 = p1; p1 = pn; q0 = q1; q1 = qn;
    }
  }
}
__device__ __forceinline__ float dn_lane_bcast(float v, int b) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), b)); }
__device__ __forceinline__ float dn_pick(const float* a, int idx) {       // a[idx] of a register array without dynamic indexing
  float r = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) r = idx == k ? a[k] : r;
  return r;
}

template <int NQ>
__global__ __launch_bounds__(256) void k_dn_trip_fwd(DnTrip p, float* __restrict__ m) {
  constexpr int I = 64 * NQ;
  const int lane = threadIdx.x & 63;
  const int e = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (e >= p.E) return;
  const int j = p.src[e], i = p.dst[e];
  const float ux = p.u[3 * (long)e], uy = p.u[3 * (long)e + 1], uz = p.u[3 * (long)e + 2];
  float w[NQ][DN_MAXB], acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    acc[q] = 0.f;
#pragma unroll
    for (int b = 0; b < DN_MAXB; ++b) w[q][b] = b < p.Bs ? p.W2[(long)(lane + 64 * q) * p.Bs + b] : 0.f;
  }
  const int r0 = p.row_ptr[j], r1 = p.row_ptr[j + 1];
  for (int e2 = r0; e2 < r1; ++e2) {
    if (p.src[e2] == i) continue;
    const float c = ux * p.u[3 * (long)e2] + uy * p.u[3 * (long)e2 + 1] + uz * p.u[3 * (long)e2 + 2];
    float Y[DN_MAXS];
    dn_legendre(c, p.S, Y, nullptr);
    float s = 0.f;
    if (lane < p.Bs) {
      const float* __restrict__ Qe = p.Q + (long)e2 * p.S * p.Bs + lane;
#pragma unroll
      for (int l = 0; l < DN_MAXS; ++l) if (l < p.S) s = fmaf(Y[l], Qe[l * p.Bs], s);
    }
    float t[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) t[q] = 0.f;
#pragma unroll
    for (int b = 0; b < DN_MAXB; ++b) {
      const float sb = dn_lane_bcast(s, b);
#pragma unroll
      for (int q = 0; q < NQ; ++q) t[q] = fmaf(sb, w[q][b], t[q]);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = fmaf(p.x[(long)e2 * I + lane + 64 * q], t[q], acc[q]);
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) m[(long)e * I + lane + 64 * q] = acc[q];
}

// g_s[b] = sum_c gm[e][c] x[e2][c] W2[c][b] (wave sums), then g_c = sum_{l, b} dY_l(c) Q[e2][l][b] g_s[b] with lane = l Bs + b
template <int NQ>
__device__ __forceinline__ void dn_gs(const float (&gt)[NQ], const float (&w)[NQ][DN_MAXB], float* gs) {
#pragma unroll
  for (int b = 0; b < DN_MAXB; ++b) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) v = fmaf(gt[q], w[q][b], v);
    gs[b] = nq_wave_sum(v);
  }
}

// owner e = (j->i): gu[e] = sum over its triplets of g_c u[e2]
template <int NQ>
__global__ __launch_bounds__(256) void k_dn_trip_bwd_out(DnTrip p, const float* __restrict__ gm, float* __restrict__ gu) {
  constexpr int I = 64 * NQ;
  const int lane = threadIdx.x & 63;
  const int e = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (e >= p.E) return;
  const int j = p.src[e], i = p.dst[e];
  const float ux = p.u[3 * (long)e], uy = p.u[3 * (long)e + 1], uz = p.u[3 * (long)e + 2];
  float w[NQ][DN_MAXB], g[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    g[q] = gm[(long)e * I + lane + 64 * q];
#pragma unroll
    for (int b = 0; b < DN_MAXB; ++b) w[q][b] = b < p.Bs ? p.W2[(long)(lane + 64 * q) * p.Bs + b] : 0.f;
  }
  const int SB = p.S * p.Bs, myl = lane / p.Bs, myb = lane - myl * p.Bs;
  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int e2 = p.row_ptr[j]; e2 < p.row_ptr[j + 1]; ++e2) {
    if (p.src[e2] == i) continue;
    const float vx = p.u[3 * (long)e2], vy = p.u[3 * (long)e2 + 1], vz = p.u[3 * (long)e2 + 2];
    const float c = ux * vx + uy * vy + uz * vz;
    float Y[DN_MAXS], dY[DN_MAXS], gt[NQ], gs[DN_MAXB];
    dn_legendre(c, p.S, Y, dY);
#pragma unroll
    for (int q = 0; q < NQ; ++q) gt[q] = g[q] * p.x[(long)e2 * I + lane + 64 * q];
    dn_gs<NQ>(gt, w, gs);
    const float v = lane < SB ? p.Q[(long)e2 * SB + lane] * dn_pick(gs, myb) * dn_pick(dY, myl) : 0.f;
    const float gc = nq_wave_sum(v);
    ax = fmaf(gc, vx, ax); ay = fmaf(gc, vy, ay); az = fmaf(gc, vz, az);
  }
  if (lane == 0) { gu[3 * (long)e] = ax; gu[3 * (long)e + 1] = ay; gu[3 * (long)e + 2] = az; }
}

// owner e2 = (k->j), a chunk of DN_CHUNK of them per wavefront: gx[e2], gQ[e2], gu[e2] += ..., and the chunk's partial of gW2 [I][Bs]
template <int NQ>
__global__ __launch_bounds__(256) void k_dn_trip_bwd_in(DnTrip p, const float* __restrict__ gm, float* __restrict__ gx, float* __restrict__ gQ,
                                                        float* __restrict__ gu, float* __restrict__ gW2_part) {
  constexpr int I = 64 * NQ;
  const int lane = threadIdx.x & 63;
  const int chunk = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int e_lo = chunk * DN_CHUNK;
  if (e_lo >= p.E) return;
  const int e_hi = min(p.E, e_lo + DN_CHUNK);
  const int SB = p.S * p.Bs, myl = lane / p.Bs, myb = lane - myl * p.Bs;
  float w[NQ][DN_MAXB], gw[NQ][DN_MAXB];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int b = 0; b < DN_MAXB; ++b) { w[q][b] = b < p.Bs ? p.W2[(long)(lane + 64 * q) * p.Bs + b] : 0.f; gw[q][b] = 0.f; }
  for (int e2 = e_lo; e2 < e_hi; ++e2) {
    const int k = p.src[e2], j = p.dst[e2];
    const float vx = p.u[3 * (long)e2], vy = p.u[3 * (long)e2 + 1], vz = p.u[3 * (long)e2 + 2];
    float xq[NQ], acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { xq[q] = p.x[(long)e2 * I + lane + 64 * q]; acc[q] = 0.f; }
    float Qcol[DN_MAXS];                                   // lane b < Bs: Q[e2][l][b]
#pragma unroll
    for (int l = 0; l < DN_MAXS; ++l) Qcol[l] = (lane < p.Bs && l < p.S) ? p.Q[(long)e2 * SB + l * p.Bs + lane] : 0.f;
    const float Qmine = lane < SB ? p.Q[(long)e2 * SB + lane] : 0.f;
    float gq = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
    for (int s_ = p.src_ptr[j]; s_ < p.src_ptr[j + 1]; ++s_) {
      const int e = p.src_order[s_];
      if (p.dst[e] == k) continue;
      const float ux = p.u[3 * (long)e], uy = p.u[3 * (long)e + 1], uz = p.u[3 * (long)e + 2];
      const float c = ux * vx + uy * vy + uz * vz;
      float Y[DN_MAXS], dY[DN_MAXS], gt[NQ], gs[DN_MAXB], g[NQ], t[NQ];
      dn_legendre(c, p.S, Y, dY);
      float s = 0.f;
#pragma unroll
      for (int l = 0; l < DN_MAXS; ++l) s = fmaf(Y[l], Qcol[l], s);
#pragma unroll
      for (int q = 0; q < NQ; ++q) { g[q] = gm[(long)e * I + lane + 64 * q]; gt[q] = g[q] * xq[q]; t[q] = 0.f; }
#pragma unroll
      for (int b = 0; b < DN_MAXB; ++b) {
        const float sb = dn_lane_bcast(s, b);
#pragma unroll
        for (int q = 0; q < NQ; ++q) { t[q] = fmaf(sb, w[q][b], t[q]); gw[q][b] = fmaf(gt[q], sb, gw[q][b]); }
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = fmaf(g[q], t[q], acc[q]);
      dn_gs<NQ>(gt, w, gs);
      const float gsb = dn_pick(gs, myb);
      gq = fmaf(dn_pick(Y, myl), gsb, gq);
      const float gc = nq_wave_sum(Qmine * gsb * dn_pick(dY, myl));
      ax = fmaf(gc, ux, ax); ay = fmaf(gc, uy, ay); az = fmaf(gc, uz, az);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) gx[(long)e2 * I + lane + 64 * q] = acc[q];
    if (lane < SB) gQ[(long)e2 * SB + lane] = gq;
    if (lane == 0) { gu[3 * (long)e2] += ax; gu[3 * (long)e2 + 1] += ay; gu[3 * (long)e2 + 2] += az; }
  }
  if (gW2_part) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int b = 0; b < DN_MAXB; ++b)
        if (b < p.Bs) gW2_part[((long)chunk * I + lane + 64 * q) * p.Bs + b] = gw[q][b];
  }
}

// ---- edge helpers -------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dn_gate_fwd(const float* __restrict__ x, const float* __restrict__ g, long count, float* __restrict__ y) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < count) y[t] = x[t] * g[t];
}
__global__ __launch_bounds__(256) void k_dn_gate_bwd(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ gy, long count,
                                                     float* __restrict__ gx, float* __restrict__ gg) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < count) { const float v = gy[t]; gx[t] = v * g[t]; gg[t] = v * x[t]; }
}
__global__ __launch_bounds__(256) void k_dn_gatesum_fwd(const float* __restrict__ x, const float* __restrict__ g, const int* __restrict__ row_ptr, int N, int H,
                                                        float* __restrict__ out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)N * H) return;
  const int i = (int)(t / H), c = (int)(t - (long)i * H);
  float a = 0.f;
  for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) a = fmaf(x[(long)e * H + c], g[(long)e * H + c], a);
  out[t] = a;
}
__global__ __launch_bounds__(256) void k_dn_gatesum_bwd(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ gout,
                                                        const int* __restrict__ dst, long E, int H, float* __restrict__ gx, float* __restrict__ gg) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= E * H) return;
  const long e = t / H;
  const int c = (int)(t - e * H);
  const float v = gout[(long)dst[e] * H + c];
  gx[t] = v * g[t]; gg[t] = v * x[t];
}
// pre[e] = AB[dst[e]][:H] + AB[src[e]][H:] + Cr[e] + bias, y = silu(pre)
__global__ __launch_bounds__(256) void k_dn_embed_fwd(const float* __restrict__ AB, const float* __restrict__ Cr, const float* __restrict__ bias,
                                                      const int* __restrict__ src, const int* __restrict__ dst, long E, int H, float* __restrict__ pre,
                                                      float* __restrict__ y) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= E * H) return;
  const long e = t / H;
  const int c = (int)(t - e * H);
  const float v = AB[(long)dst[e] * 2 * H + c] + AB[(long)src[e] * 2 * H + H + c] + Cr[t] + bias[c];
  pre[t] = v; y[t] = nq_silu(v);
}
__global__ __launch_bounds__(256) void k_dn_embed_gpre(const float* __restrict__ pre, const float* __restrict__ gy, long count, float* __restrict__ gpre) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < count) gpre[t] = gy[t] * nq_dsilu(pre[t]);
}
__global__ __launch_bounds__(256) void k_dn_embed_gab(const float* __restrict__ gpre, const int* __restrict__ row_ptr, const int* __restrict__ src_order,
                                                      const int* __restrict__ src_ptr, int N, int H, float* __restrict__ gAB) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)N * 2 * H) return;
  const int i = (int)(t / (2 * H)), c2 = (int)(t - (long)i * 2 * H);
  float a = 0.f;
  if (c2 < H) {
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) a += gpre[(long)e * H + c2];
  } else {
    for (int q = src_ptr[i]; q < src_ptr[i + 1]; ++q) a += gpre[(long)src_order[q] * H + c2 - H];
  }
  gAB[t] = a;
}

// ---- second sweep (a loss on the forces): tangents along a position displacement and their reverses ------------------------------------------------------------
// The adjoint that reaches the first-backward node of a kernel is the kernel's tangent (JVP) along the displacement v = dL/dF; what flows on to the parameters is the
// reverse of that tangent with respect to the parameter-dependent inputs.  d, u, rbf and Rad depend on the positions only: no adjoint of u or d is formed here.
struct DnTan { const float* tx; const float* tQ; const float* tu; };       // each nullable = a zero tangent (the arithmetic is the same, so the bits are too)

// w = tpos[dst] - tpos[src]: td = w . u, tu = (w - (w . u) u) / d
__global__ __launch_bounds__(256) void k_dn_geom_tan(const float* __restrict__ d, const float* __restrict__ u, const float* __restrict__ tpos,
                                                     const int* __restrict__ src, const int* __restrict__ dst, long E, float* __restrict__ td,
                                                     float* __restrict__ tu) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const long a = 3L * dst[e], b = 3L * src[e];
  const float wx = tpos[a] - tpos[b], wy = tpos[a + 1] - tpos[b + 1], wz = tpos[a + 2] - tpos[b + 2];
  const float ux = u[3 * e], uy = u[3 * e + 1], uz = u[3 * e + 2], dot = wx * ux + wy * uy + wz * uz, inv = 1.0f / d[e];
  td[e] = dot;
  tu[3 * e] = (wx - dot * ux) * inv; tu[3 * e + 1] = (wy - dot * uy) * inv; tu[3 * e + 2] = (wz - dot * uz) * inv;
}

// thread (e, l): l < S the row t[e] dRad[e][l][:]/dd, l == S the rows t[e] drbf[e][:]/dd and t[e] g_rbf[e][n] d2rbf/(dd dfreq_n)
__global__ __launch_bounds__(256) void k_dn_basis_tan(const float* __restrict__ d, const float* __restrict__ freq, const double* __restrict__ roots,
                                                      const double* __restrict__ norms, long E, int S, int R, double inv_cutoff, int p,
                                                      const float* __restrict__ t, const float* __restrict__ g_rbf, float* __restrict__ rbf_t,
                                                      float* __restrict__ rad_t, float* __restrict__ freq_rows) {
  const long th = (long)blockIdx.x * 256 + threadIdx.x;
  if (th >= E * (S + 1)) return;
  const long e = th / (S + 1);
  const int l = (int)(th - e * (S + 1));
  const double x = (double)d[e] * inv_cutoff, te = (double)t[e] * inv_cutoff;
  double env, denv;
  dn_env(x, p, env, denv);
  if (l == S) {
    for (int n = 0; n < R; ++n) {
      const double f = (double)freq[n], sn = sin(f * x), cs = cos(f * x), g = g_rbf ? (double)g_rbf[e * R + n] : 0.0;
      rbf_t[e * R + n] = (float)(te * (denv * sn + env * f * cs));
      freq_rows[e * R + n] = (float)(te * g * (denv * x * cs + env * cs - env * f * x * sn));
    }
  } else {
    for (int n = 0; n < R; ++n) {
      const double z = roots[l * R + n], j = dn_jl(l, z * x);
      rad_t[(e * S + l) * R + n] = (float)(te * norms[l * R + n] * (denv * j + env * z * dn_djl(l, z * x, j)));
    }
  }
}

// the walk of k_dn_trip_fwd: mt[e][c] = sum_{e2} sum_b W2[c][b] (tx[e2][c] s_b + x[e2][c] st_b), st_b = sum_l (Y_l tQ[e2][l][b] + Y_l' cdot Q[e2][l][b])
template <int NQ>
__global__ __launch_bounds__(256) void k_dn_trip_tan_fwd(DnTrip p, DnTan t, float* __restrict__ mt) {
  constexpr int I = 64 * NQ;
  const int lane = threadIdx.x & 63;
  const int e = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (e >= p.E) return;
  const int j = p.src[e], i = p.dst[e];
  const float ux = p.u[3 * (long)e], uy = p.u[3 * (long)e + 1], uz = p.u[3 * (long)e + 2];
  const float tux = t.tu ? t.tu[3 * (long)e] : 0.f, tuy = t.tu ? t.tu[3 * (long)e + 1] : 0.f, tuz = t.tu ? t.tu[3 * (long)e + 2] : 0.f;
  float w[NQ][DN_MAXB], acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    acc[q] = 0.f;
#pragma unroll
    for (int b = 0; b < DN_MAXB; ++b) w[q][b] = b < p.Bs ? p.W2[(long)(lane + 64 * q) * p.Bs + b] : 0.f;
  }
  const int r0 = p.row_ptr[j], r1 = p.row_ptr[j + 1];
  for (int e2 = r0; e2 < r1; ++e2) {
    if (p.src[e2] == i) continue;
    const float vx = p.u[3 * (long)e2], vy = p.u[3 * (long)e2 + 1], vz = p.u[3 * (long)e2 + 2];
    const float tvx = t.tu ? t.tu[3 * (long)e2] : 0.f, tvy = t.tu ? t.tu[3 * (long)e2 + 1] : 0.f, tvz = t.tu ? t.tu[3 * (long)e2 + 2] : 0.f;
    const float c = ux * vx + uy * vy + uz * vz;
    const float cd = (tux * vx + tuy * vy + tuz * vz) + (ux * tvx + uy * tvy + uz * tvz);
    float Y[DN_MAXS], dY[DN_MAXS];
    dn_legendre(c, p.S, Y, dY);
    float s = 0.f, sd = 0.f;
    if (lane < p.Bs) {
      const long off = (long)e2 * p.S * p.Bs + lane;
#pragma unroll
      for (int l = 0; l < DN_MAXS; ++l)
        if (l < p.S) {
          const float q = p.Q[off + l * p.Bs], tq = t.tQ ? t.tQ[off + l * p.Bs] : 0.f;
          s = fmaf(Y[l], q, s);
          sd = fmaf(Y[l], tq, fmaf(dY[l] * cd, q, sd));
        }
    }
    float ts[NQ], tt[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) ts[q] = tt[q] = 0.f;
#pragma unroll
    for (int b = 0; b < DN_MAXB; ++b) {
      const float sb = dn_lane_bcast(s, b), sdb = dn_lane_bcast(sd, b);
#pragma unroll
      for (int q = 0; q < NQ; ++q) { ts[q] = fmaf(sb, w[q][b], ts[q]); tt[q] = fmaf(sdb, w[q][b], tt[q]); }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const long at = (long)e2 * I + lane + 64 * q;
      acc[q] = fmaf(p.x[at], tt[q], fmaf(t.tx ? t.tx[at] : 0.f, ts[q], acc[q]));
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) mt[(long)e * I + lane + 64 * q] = acc[q];
}

// the transposed walk of k_dn_trip_bwd_in, owner e2 = (k->j): the adjoints of <g, mt> with respect to x, Q and (as partial sums per chunk) W2.  Nothing is
// written for u or the tangents, so there is no owner-side pass.  lane = l Bs + b holds a_Q[e2][l][b].
template <int NQ>
__global__ __launch_bounds__(256) void k_dn_trip_tan_bwd(DnTrip p, DnTan t, const float* __restrict__ gm, float* __restrict__ ax, float* __restrict__ aQ,
                                                         float* __restrict__ aW2_part) {
  constexpr int I = 64 * NQ;
  const int lane = threadIdx.x & 63;
  const int chunk = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int e_lo = chunk * DN_CHUNK;
  if (e_lo >= p.E) return;
  const int e_hi = min(p.E, e_lo + DN_CHUNK);
  const int SB = p.S * p.Bs, myl = lane / p.Bs, myb = lane - myl * p.Bs;
  float w[NQ][DN_MAXB], gw[NQ][DN_MAXB];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int b = 0; b < DN_MAXB; ++b) { w[q][b] = b < p.Bs ? p.W2[(long)(lane + 64 * q) * p.Bs + b] : 0.f; gw[q][b] = 0.f; }
  for (int e2 = e_lo; e2 < e_hi; ++e2) {
    const int k = p.src[e2], j = p.dst[e2];
    const float vx = p.u[3 * (long)e2], vy = p.u[3 * (long)e2 + 1], vz = p.u[3 * (long)e2 + 2];
    const float tvx = t.tu ? t.tu[3 * (long)e2] : 0.f, tvy = t.tu ? t.tu[3 * (long)e2 + 1] : 0.f, tvz = t.tu ? t.tu[3 * (long)e2 + 2] : 0.f;
    float xq[NQ], txq[NQ], acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const long at = (long)e2 * I + lane + 64 * q;
      xq[q] = p.x[at]; txq[q] = t.tx ? t.tx[at] : 0.f; acc[q] = 0.f;
    }
    float Qcol[DN_MAXS], tQcol[DN_MAXS];                   // lane b < Bs: Q[e2][l][b], tQ[e2][l][b]
#pragma unroll
    for (int l = 0; l < DN_MAXS; ++l) {
      const bool on = lane < p.Bs && l < p.S;
      Qcol[l] = on ? p.Q[(long)e2 * SB + l * p.Bs + lane] : 0.f;
      tQcol[l] = (on && t.tQ) ? t.tQ[(long)e2 * SB + l * p.Bs + lane] : 0.f;
    }
    float gq = 0.f;
    for (int s_ = p.src_ptr[j]; s_ < p.src_ptr[j + 1]; ++s_) {
      const int e = p.src_order[s_];
      if (p.dst[e] == k) continue;
      const float ux = p.u[3 * (long)e], uy = p.u[3 * (long)e + 1], uz = p.u[3 * (long)e + 2];
      const float tux = t.tu ? t.tu[3 * (long)e] : 0.f, tuy = t.tu ? t.tu[3 * (long)e + 1] : 0.f, tuz = t.tu ? t.tu[3 * (long)e + 2] : 0.f;
      const float c = ux * vx + uy * vy + uz * vz;
      const float cd = (tux * vx + tuy * vy + tuz * vz) + (ux * tvx + uy * tvy + uz * tvz);
      float Y[DN_MAXS], dY[DN_MAXS], g1[NQ], g2[NQ], G1[DN_MAXB], G2[DN_MAXB], g[NQ], tt[NQ];
      dn_legendre(c, p.S, Y, dY);
      float s = 0.f, sd = 0.f;
#pragma unroll
      for (int l = 0; l < DN_MAXS; ++l) { s = fmaf(Y[l], Qcol[l], s); sd = fmaf(Y[l], tQcol[l], fmaf(dY[l] * cd, Qcol[l], sd)); }
#pragma unroll
      for (int q = 0; q < NQ; ++q) { g[q] = gm[(long)e * I + lane + 64 * q]; g1[q] = g[q] * txq[q]; g2[q] = g[q] * xq[q]; tt[q] = 0.f; }
#pragma unroll
      for (int b = 0; b < DN_MAXB; ++b) {
        const float sb = dn_lane_bcast(s, b), sdb = dn_lane_bcast(sd, b);
#pragma unroll
        for (int q = 0; q < NQ; ++q) { tt[q] = fmaf(sdb, w[q][b], tt[q]); gw[q][b] = fmaf(g2[q], sdb, fmaf(g1[q], sb, gw[q][b])); }
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = fmaf(g[q], tt[q], acc[q]);
      dn_gs<NQ>(g1, w, G1);
      dn_gs<NQ>(g2, w, G2);
      gq = fmaf(dn_pick(dY, myl) * cd, dn_pick(G2, myb), fmaf(dn_pick(Y, myl), dn_pick(G1, myb), gq));
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) ax[(long)e2 * I + lane + 64 * q] = acc[q];
    if (lane < SB) aQ[(long)e2 * SB + lane] = gq;
  }
  if (aW2_part) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int b = 0; b < DN_MAXB; ++b)
        if (b < p.Bs) aW2_part[((long)chunk * I + lane + 64 * q) * p.Bs + b] = gw[q][b];
  }
}

// a = the adjoint of gp = g silu'(pre): a_g = a silu'(pre), a_pre = a g silu''(pre)
__global__ __launch_bounds__(256) void k_dn_silu_rev2(const float* __restrict__ pre, const float* __restrict__ g, const float* __restrict__ a, long count,
                                                      float* __restrict__ a_g, float* __restrict__ a_pre) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= count) return;
  const float z = pre[t], v = a[t];
  a_g[t] = v * nq_dsilu(z);
  a_pre[t] = v * g[t] * nq_d2silu(z);
}
// gx = g gate, gg = g x with the adjoints a_gx, a_gg (either nullable = zero): a_g = a_gx gate + a_gg x, a_x = a_gg g, a_gate = a_gx g
__global__ __launch_bounds__(256) void k_dn_gate_rev2(const float* __restrict__ x, const float* __restrict__ gate, const float* __restrict__ g,
                                                      const float* __restrict__ a_gx, const float* __restrict__ a_gg, long count, float* __restrict__ a_g,
                                                      float* __restrict__ a_x, float* __restrict__ a_gate) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= count) return;
  const float p = a_gx ? a_gx[t] : 0.f, q = a_gg ? a_gg[t] : 0.f, v = g[t];
  a_g[t] = fmaf(p, gate[t], q * x[t]);
  a_x[t] = q * v; a_gate[t] = p * v;
}

int dn_trip_check(const DnTrip& p, int I) {
  if (!p.x || !p.Q || !p.u || !p.W2 || !p.row_ptr || !p.src || !p.dst) return nq_fail(NQ_ERR_ARG, "dimenet triplet: null argument");
  if (I < 64 || I > 256 || I % 64 != 0) return nq_fail(NQ_ERR_ARG, "dimenet triplet: int_emb_size %d must be 64, 128, 192 or 256", I);
  if (p.S < 1 || p.S > DN_MAXS || p.Bs < 1 || p.Bs > DN_MAXB) return nq_fail(NQ_ERR_ARG, "dimenet triplet: num_spherical 1..8 and basis_emb_size 1..8 are built");
  return NQ_OK;
}
int dn_basis_check(const void* d, const void* freq, const void* roots, const void* norms, long E, int S, int R, double cutoff, int p) {
  if (!d || !freq || !roots || !norms || E < 0 || E > 200000000L) return nq_fail(NQ_ERR_ARG, "dimenet basis: bad argument");
  if (S < 1 || S > DN_MAXS || R < 1 || R > DN_MAXR || !(cutoff > 0.0) || p < 2 || p > 16) return nq_fail(NQ_ERR_ARG, "dimenet basis: sizes outside S 1..8, R 1..16, p 2..16");
  return NQ_OK;
}

}  // namespace

#define DN_DISPATCH(I, KERNEL, GRID, ...)                                                                  \
  switch ((I) / 64) {                                                                                      \
    case 1: hipLaunchKernelGGL(KERNEL<1>, dim3(GRID), dim3(256), 0, st, __VA_ARGS__); break;               \
    case 2: hipLaunchKernelGGL(KERNEL<2>, dim3(GRID), dim3(256), 0, st, __VA_ARGS__); break;               \
    case 3: hipLaunchKernelGGL(KERNEL<3>, dim3(GRID), dim3(256), 0, st, __VA_ARGS__); break;               \
    default: hipLaunchKernelGGL(KERNEL<4>, dim3(GRID), dim3(256), 0, st, __VA_ARGS__); break;              \
  }

extern "C" {

int nq_dn_geom_forward(const float* geom, int64_t E, float* d, float* u, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_geom_fwd");
  if (E == 0) return NQ_OK;
  if (!geom || !d || !u || E < 0) return nq_fail(NQ_ERR_ARG, "dimenet geometry: bad argument");
  if (E > 0) hipLaunchKernelGGL(k_dn_geom_fwd, DN_GRID(E), (const float4*)geom, (long)E, d, u);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dn_geom_backward(const float* d, const float* u, const float* grad_d, const float* grad_u, const int32_t* row_ptr, const int32_t* src_order,
                        const int32_t* src_ptr, int32_t N, int64_t E, float* grad_vec, float* grad_pos, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_geom_bwd");
  if (!row_ptr || !src_ptr || !grad_pos || N < 1 || E < 0 || (E > 0 && (!d || !u || !src_order || !grad_vec))) return nq_fail(NQ_ERR_ARG, "dimenet geometry: bad argument");
  if (E > 0) hipLaunchKernelGGL(k_dn_geom_gvec, DN_GRID(E), d, u, grad_d, grad_u, (long)E, grad_vec);
  NQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_dn_geom_gpos, DN_GRID(3L * N), (const float*)grad_vec, row_ptr, src_order, src_ptr, N, grad_pos);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_dn_basis_forward(const float* d, const float* freq, const double* roots, const double* norms, int64_t E, int32_t S, int32_t R, double cutoff,
                        int32_t envelope_p, float* rbf, float* rad, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_basis_fwd");
  if (E == 0) return NQ_OK;
  NQ_TRY(dn_basis_check(d, freq, roots, norms, E, S, R, cutoff, envelope_p));
  if (!rbf || !rad) return nq_fail(NQ_ERR_ARG, "dimenet basis: null output");
  if (E > 0) hipLaunchKernelGGL(k_dn_basis_fwd, DN_GRID((long)E * (S + 1)), d, freq, roots, norms, (long)E, S, R, 1.0 / cutoff, envelope_p, rbf, rad);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dn_basis_backward(const float* d, const float* freq, const double* roots, const double* norms, int64_t E, int32_t S, int32_t R, double cutoff,
                         int32_t envelope_p, const float* grad_rbf, const float* grad_rad, float* grad_d, float* grad_freq_rows, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_basis_bwd");
  if (E == 0) return NQ_OK;
  NQ_TRY(dn_basis_check(d, freq, roots, norms, E, S, R, cutoff, envelope_p));
  if (!grad_d || !grad_freq_rows) return nq_fail(NQ_ERR_ARG, "dimenet basis: null output");
  if (E > 0) hipLaunchKernelGGL(k_dn_basis_bwd, DN_GRID(E), d, freq, roots, norms, (long)E, S, R, 1.0 / cutoff, envelope_p, grad_rbf, grad_rad, grad_d,
                                grad_freq_rows);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

int nq_dn_triplet_forward(const float* x_kj, const float* Q, const float* u, const float* W_sbf2, const int32_t* row_ptr, const int32_t* src, const int32_t* dst,
                          int32_t E, int32_t I, int32_t S, int32_t Bs, float* m, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_triplet_fwd");
  if (E == 0) return NQ_OK;
  DnTrip p{x_kj, Q, u, W_sbf2, row_ptr, src, dst, nullptr, nullptr, E, S, Bs};
  NQ_TRY(dn_trip_check(p, I));
  if (!m || E < 0) return nq_fail(NQ_ERR_ARG, "dimenet triplet: bad argument");
  DN_DISPATCH(I, k_dn_trip_fwd, nq_cdiv(E, 4), p, m);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
size_t nq_dn_triplet_scratch_floats(int32_t E, int32_t I, int32_t Bs) {
  const long chunks = nq_cdiv(E > 0 ? E : 1, DN_CHUNK);
  return (size_t)chunks * I * Bs + nq_colsum_scratch_floats(chunks, I * Bs);
}
/* grad_W_sbf2 nullable (then no partial sums are written) */
int nq_dn_triplet_backward(const float* x_kj, const float* Q, const float* u, const float* W_sbf2, const int32_t* row_ptr, const int32_t* src, const int32_t* dst,
                           const int32_t* src_order, const int32_t* src_ptr, int32_t E, int32_t I, int32_t S, int32_t Bs, const float* grad_m, float* grad_x,
                           float* grad_Q, float* grad_u, float* grad_W_sbf2, float* scratch, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_triplet_bwd");
  if (E == 0) {
    if (grad_W_sbf2 && I > 0 && Bs > 0) NQ_HIP(hipMemsetAsync(grad_W_sbf2, 0, sizeof(float) * I * Bs, st));
    return NQ_OK;
  }
  DnTrip p{x_kj, Q, u, W_sbf2, row_ptr, src, dst, src_order, src_ptr, E, S, Bs};
  NQ_TRY(dn_trip_check(p, I));
  if (!src_order || !src_ptr || !grad_m || !grad_x || !grad_Q || !grad_u || E < 0 || (grad_W_sbf2 && !scratch))
    return nq_fail(NQ_ERR_ARG, "dimenet triplet: bad argument");
  const int chunks = nq_cdiv(E, DN_CHUNK);
  float* part = grad_W_sbf2 ? scratch : nullptr;
  DN_DISPATCH(I, k_dn_trip_bwd_out, nq_cdiv(E, 4), p, grad_m, grad_u);
  NQ_LAUNCH_CHECK();
  DN_DISPATCH(I, k_dn_trip_bwd_in, nq_cdiv(chunks, 4), p, grad_m, grad_x, grad_Q, grad_u, part);
  NQ_LAUNCH_CHECK();
  if (grad_W_sbf2) NQ_TRY(nq_colsum(st, part, (long)chunks, I * Bs, I * Bs, grad_W_sbf2, scratch + (size_t)chunks * I * Bs));
  return NQ_OK;
}

int nq_dn_gate_forward(const float* x, const float* gate, int64_t count, float* y, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_gate_fwd");
  if (count == 0) return NQ_OK;
  if (!x || !gate || !y || count < 0) return nq_fail(NQ_ERR_ARG, "dimenet gate: bad argument");
  if (count > 0) hipLaunchKernelGGL(k_dn_gate_fwd, DN_GRID(count), x, gate, (long)count, y);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dn_gate_backward(const float* x, const float* gate, const float* grad_y, int64_t count, float* grad_x, float* grad_gate, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_gate_bwd");
  if (count == 0) return NQ_OK;
  if (!x || !gate || !grad_y || !grad_x || !grad_gate || count < 0) return nq_fail(NQ_ERR_ARG, "dimenet gate: bad argument");
  if (count > 0) hipLaunchKernelGGL(k_dn_gate_bwd, DN_GRID(count), x, gate, grad_y, (long)count, grad_x, grad_gate);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dn_gatesum_forward(const float* x, const float* gate, const int32_t* row_ptr, int32_t N, int32_t H, float* out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_gatesum_fwd");
  if (!row_ptr || !out || N < 1 || H < 1) return nq_fail(NQ_ERR_ARG, "dimenet gated sum: bad argument");   // x / gate may be NULL when there is no edge
  hipLaunchKernelGGL(k_dn_gatesum_fwd, DN_GRID((long)N * H), x, gate, row_ptr, N, H, out);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dn_gatesum_backward(const float* x, const float* gate, const float* grad_out, const int32_t* dst, int64_t E, int32_t H, float* grad_x, float* grad_gate,
                           void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_gatesum_bwd");
  if (E == 0) return NQ_OK;
  if (!x || !gate || !grad_out || !dst || !grad_x || !grad_gate || E < 0 || H < 1) return nq_fail(NQ_ERR_ARG, "dimenet gated sum: bad argument");
  if (E > 0) hipLaunchKernelGGL(k_dn_gatesum_bwd, DN_GRID((long)E * H), x, gate, grad_out, dst, (long)E, H, grad_x, grad_gate);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dn_embed_forward(const float* AB, const float* Cr, const float* bias, const int32_t* src, const int32_t* dst, int64_t E, int32_t H, float* pre, float* y,
                        void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_embed_fwd");
  if (E == 0) return NQ_OK;
  if (!AB || !Cr || !bias || !src || !dst || !pre || !y || E < 0 || H < 1) return nq_fail(NQ_ERR_ARG, "dimenet embedding: bad argument");
  if (E > 0) hipLaunchKernelGGL(k_dn_embed_fwd, DN_GRID((long)E * H), AB, Cr, bias, src, dst, (long)E, H, pre, y);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dn_embed_backward(const float* pre, const float* grad_y, const int32_t* row_ptr, const int32_t* src_order, const int32_t* src_ptr, int32_t N, int64_t E,
                         int32_t H, float* grad_pre, float* grad_AB, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_embed_bwd");
  if (!row_ptr || !src_ptr || !grad_AB || N < 1 || E < 0 || H < 1 || (E > 0 && (!pre || !grad_y || !src_order || !grad_pre)))
    return nq_fail(NQ_ERR_ARG, "dimenet embedding: bad argument");
  if (E > 0) hipLaunchKernelGGL(k_dn_embed_gpre, DN_GRID((long)E * H), pre, grad_y, (long)E * H, grad_pre);
  NQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_dn_embed_gab, DN_GRID((long)N * 2 * H), (const float*)grad_pre, row_ptr, src_order, src_ptr, N, H, grad_AB);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

/* ---- second sweep ---- */
int nq_dnt_geom(const float* d, const float* u, const float* tpos, const int32_t* src, const int32_t* dst, int64_t E, float* td, float* tu, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_geom_tan");
  if (E == 0) return NQ_OK;
  if (!d || !u || !tpos || !src || !dst || !td || !tu || E < 0) return nq_fail(NQ_ERR_ARG, "dimenet geometry tangent: bad argument");
  hipLaunchKernelGGL(k_dn_geom_tan, DN_GRID(E), d, u, tpos, src, dst, (long)E, td, tu);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dnt_basis(const float* d, const float* freq, const double* roots, const double* norms, int64_t E, int32_t S, int32_t R, double cutoff, int32_t envelope_p,
                 const float* t, const float* grad_rbf, float* rbf_t, float* rad_t, float* freq_rows, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_basis_tan");
  if (E == 0) return NQ_OK;
  NQ_TRY(dn_basis_check(d, freq, roots, norms, E, S, R, cutoff, envelope_p));
  if (!t || !rbf_t || !rad_t || !freq_rows) return nq_fail(NQ_ERR_ARG, "dimenet basis tangent: null argument");
  hipLaunchKernelGGL(k_dn_basis_tan, DN_GRID((long)E * (S + 1)), d, freq, roots, norms, (long)E, S, R, 1.0 / cutoff, envelope_p, t, grad_rbf, rbf_t, rad_t,
                     freq_rows);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dnt_triplet_forward(const float* x_kj, const float* Q, const float* u, const float* W_sbf2, const float* tx, const float* tQ, const float* tu,
                           const int32_t* row_ptr, const int32_t* src, const int32_t* dst, int32_t E, int32_t I, int32_t S, int32_t Bs, float* mt, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_triplet_tan_fwd");
  if (E == 0) return NQ_OK;
  DnTrip p{x_kj, Q, u, W_sbf2, row_ptr, src, dst, nullptr, nullptr, E, S, Bs};
  NQ_TRY(dn_trip_check(p, I));
  if (!mt || E < 0) return nq_fail(NQ_ERR_ARG, "dimenet triplet tangent: bad argument");
  DnTan t{tx, tQ, tu};
  DN_DISPATCH(I, k_dn_trip_tan_fwd, nq_cdiv(E, 4), p, t, mt);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dnt_triplet_backward(const float* x_kj, const float* Q, const float* u, const float* W_sbf2, const float* tx, const float* tQ, const float* tu,
                            const int32_t* row_ptr, const int32_t* src, const int32_t* dst, const int32_t* src_order, const int32_t* src_ptr, int32_t E, int32_t I,
                            int32_t S, int32_t Bs, const float* g, float* a_x, float* a_Q, float* a_W_sbf2, float* scratch, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_triplet_tan_bwd");
  if (E == 0) {
    if (a_W_sbf2 && I > 0 && Bs > 0) NQ_HIP(hipMemsetAsync(a_W_sbf2, 0, sizeof(float) * I * Bs, st));
    return NQ_OK;
  }
  DnTrip p{x_kj, Q, u, W_sbf2, row_ptr, src, dst, src_order, src_ptr, E, S, Bs};
  NQ_TRY(dn_trip_check(p, I));
  if (!src_order || !src_ptr || !g || !a_x || !a_Q || E < 0 || (a_W_sbf2 && !scratch)) return nq_fail(NQ_ERR_ARG, "dimenet triplet tangent: bad argument");
  const int chunks = nq_cdiv(E, DN_CHUNK);
  float* part = a_W_sbf2 ? scratch : nullptr;
  DnTan t{tx, tQ, tu};
  DN_DISPATCH(I, k_dn_trip_tan_bwd, nq_cdiv(chunks, 4), p, t, g, a_x, a_Q, part);
  NQ_LAUNCH_CHECK();
  if (a_W_sbf2) NQ_TRY(nq_colsum(st, part, (long)chunks, I * Bs, I * Bs, a_W_sbf2, scratch + (size_t)chunks * I * Bs));
  return NQ_OK;
}
int nq_dnt_silu(const float* pre, const float* g, const float* a, int64_t count, float* a_g, float* a_pre, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_silu_rev2");
  if (count == 0) return NQ_OK;
  if (!pre || !g || !a || !a_g || !a_pre || count < 0) return nq_fail(NQ_ERR_ARG, "dimenet SiLU second order: bad argument");
  hipLaunchKernelGGL(k_dn_silu_rev2, DN_GRID(count), pre, g, a, (long)count, a_g, a_pre);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dnt_gate(const float* x, const float* gate, const float* g, const float* a_gx, const float* a_gg, int64_t count, float* a_g, float* a_x, float* a_gate,
                void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_gate_rev2");
  if (count == 0) return NQ_OK;
  if (!x || !gate || !g || !a_g || !a_x || !a_gate || count < 0) return nq_fail(NQ_ERR_ARG, "dimenet gate second order: bad argument");
  hipLaunchKernelGGL(k_dn_gate_rev2, DN_GRID(count), x, gate, g, a_gx, a_gg, (long)count, a_g, a_x, a_gate);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}
int nq_dnt_embed_scatter(const float* rows, const int32_t* row_ptr, const int32_t* src_order, const int32_t* src_ptr, int32_t N, int64_t E, int32_t H, float* out,
                         void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NQ_PROF(st, "dn_embed_scatter");
  if (!row_ptr || !src_ptr || !out || N < 1 || E < 0 || H < 1 || (E > 0 && (!rows || !src_order))) return nq_fail(NQ_ERR_ARG, "dimenet embedding scatter: bad argument");
  hipLaunchKernelGGL(k_dn_embed_gab, DN_GRID((long)N * 2 * H), rows, row_ptr, src_order, src_ptr, N, H, out);
  NQ_LAUNCH_CHECK();
  return NQ_OK;
}

}  // extern "C"
