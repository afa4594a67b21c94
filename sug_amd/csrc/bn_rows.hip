// Train-mode BatchNorm (+ LeakyReLU / ReLU) over the rows of a channel-last [rows, C] tensor, forward and exact
// backward: everything sug_bn_act_rows_fwd / sug_bn_act_rows_bwd (layers.cpp) launch, for one domain group or for all
// groups of a layer per launch (internal.h).  The EdgeConv, PointMLP, SA and pooling layers use the same pieces:
//   col_reduce*       per-workgroup partial rows  sum | sum of squares  about a pivot row (common.h), or the backward
//                     sums dbeta | dgamma; reads y (and z) once
//   reduce_partials*  ordered fp64 fold of the partial rows
//   *_finalize*       partial rows (or fp64 sums) -> coef [5][C] = scale | shift | mean | rstd | unbiased variance, and the
//                     running statistics; bn_replay* repeats that update from stored coefficients
//   affine_act*       out = act(scale * z + shift): reads z (4 B/elem), writes out (4 B/elem)
//   bn_bwd_apply*     dy = a - (scale/M) (dbeta + xhat dgamma): reads a, y (8 B/elem), writes dy (4 B/elem)
#include "common.h"
#include "internal.h"
#include "device_helpers.h"

namespace {

// out[i] = sum over workgroup rows of ws[row][i], in fp64, in a fixed order: 16 strided
// partial sums per column (rows p, p+16, ...) combined in ascending p.  grid = ceil(W/16).
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ ws, int nblk,
                                                              int W, double* __restrict__ out) {
  __shared__ double s_p[16][17];
  ws += (size_t)blockIdx.y * nblk * W;           // blockIdx.y = domain group: its nblk partial rows -> out row g
  out += (size_t)blockIdx.y * W;
  const int cl = threadIdx.x & 15, p = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  double acc = 0.0;
  if (c < W) {
#pragma unroll 8
    for (int b = p; b < nblk; b += 16) acc += (double)ws[(size_t)b * W + c];
  }
  s_p[p][cl] = acc;
  __syncthreads();
  if (p == 0 && c < W) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += s_p[i][cl];
    out[c] = t;
  }
}

// reduce_partials_kernel for every domain group of a layer in one workgroup per 16 columns, plus the group-folded fp32
// copy the parameter gradients want (sug_fold_groups' arithmetic: the groups' fp64 sums added in group order, then
// rounded) -- the separate fold launch of every BatchNorm backward is gone.
__global__ __launch_bounds__(256) void reduce_partials_fold_kernel(const float* __restrict__ ws, int nblk, int W, int groups,
                                                                   double* __restrict__ out, float* __restrict__ folded) {
  __shared__ double s_p[16][17];
  const int cl = threadIdx.x & 15, p = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  double tot = 0.0;
  for (int g = 0; g < groups; ++g) {
    const float* wg = ws + (size_t)g * nblk * W;
    double acc = 0.0;
    if (c < W) {
#pragma unroll 8
      for (int b = p; b < nblk; b += 16) acc += (double)wg[(size_t)b * W + c];
    }
    __syncthreads();
    s_p[p][cl] = acc;
    __syncthreads();
    if (p == 0 && c < W) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) t += s_p[i][cl];
      out[(size_t)g * W + c] = t;
      tot += t;
    }
  }
  if (p == 0 && c < W) folded[c] = (float)tot;
}

// The coefficient rows of channel c from its batch mean and biased variance (fp64) over `count` samples:
// coef[5][C] = scale | shift | mean | rstd | unbiased variance.  Returns what the running buffers take.
struct BnMoments {
  float mean, unbiased;
};
__device__ __forceinline__ BnMoments bn_coef_rows(double mean, double var, double count, float eps,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  float* __restrict__ coef, int C, int c) {
  if (var < 0) var = 0;
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const float scale = gamma[c] * rstd;
  coef[c] = scale;
  coef[C + c] = beta[c] - (float)mean * scale;
  coef[2 * C + c] = (float)mean;
  coef[3 * C + c] = rstd;
  const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
  coef[4 * C + c] = (float)unb;
  return {(float)mean, (float)unb};
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const double* __restrict__ stats,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int C,
                                                          double count, float eps, float momentum,
                                                          float* __restrict__ rmean,
                                                          float* __restrict__ rvar,
                                                          float* __restrict__ coef) {
  for (int c = blockIdx.x * 256 + threadIdx.x; c < C; c += gridDim.x * 256) {
    const double mean = stats[c] / count;
    const double var = stats[C + c] / count - mean * mean;
    const BnMoments m = bn_coef_rows(mean, var, count, eps, gamma, beta, coef, C, c);
    if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * m.mean;
    if (rvar) rvar[c] = (1.f - momentum) * rvar[c] + momentum * m.unbiased;
  }
}

// reduce_partials + bn_finalize in one launch: a workgroup folds the partial rows of 8 channels
// (their sum and sum-of-squares columns c and C+c, same 16-way strided fixed order as
// reduce_partials_kernel) and writes the BN coefficients / running statistics of those channels.
__global__ __launch_bounds__(256) void stats_finalize_kernel(const float* __restrict__ ws, int nblk, int C,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, double count,
                                                             float eps, float momentum, float* __restrict__ rmean,
                                                             float* __restrict__ rvar, float* __restrict__ coef,
                                                             const float* __restrict__ pivot) {
  __shared__ double s_p[16][17];
  __shared__ double s_tot[16];
  const int cl = threadIdx.x & 15, p = threadIdx.x >> 4;
  const int ch = blockIdx.x * 8 + (cl & 7);                 // cl < 8: sum column, cl >= 8: sum of squares
  const int col = (cl < 8) ? ch : C + ch;
  const int W = 2 * C;
  double acc = 0.0;
  if (ch < C) {
#pragma unroll 8
    for (int b = p; b < nblk; b += 16) acc += (double)ws[(size_t)b * W + col];
  }
  s_p[p][cl] = acc;
  __syncthreads();
  if (p == 0) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += s_p[i][cl];
    s_tot[cl] = t;
  }
  __syncthreads();
  if (threadIdx.x < 8 && ch < C) {
    const int c = ch;
    const double m1 = s_tot[threadIdx.x] / count;           // mean of (x - pivot)
    const double var = s_tot[8 + threadIdx.x] / count - m1 * m1;
    const double mean = (pivot ? (double)pivot[c] : 0.0) + m1;
    const BnMoments m = bn_coef_rows(mean, var, count, eps, gamma, beta, coef, C, c);
    if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * m.mean;
    if (rvar) rvar[c] = (1.f - momentum) * rvar[c] + momentum * m.unbiased;
  }
}

// stats_finalize_kernel for `groups` consecutive blocks of nblk partial rows (one BatchNorm call per domain group,
// in group order: the running statistics see the groups' updates one after the other, as separate calls would).
__global__ __launch_bounds__(1024) void stats_finalize_groups_kernel(const float* __restrict__ ws, int nblk, int C, int groups,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, double count,
                                                                    float eps, float momentum, float* __restrict__ rmean,
                                                                    float* __restrict__ rvar, float* __restrict__ coef,
                                                                    const float* __restrict__ pivot) {
  constexpr int GMAX = 4;                        // groups folded in one pass over the partial rows (loads of all
  constexpr int RL = 64;                         // groups in flight together); more groups: further passes.  64 row
  __shared__ double s_p[GMAX][RL][17];           // lanes (1024 threads): hundreds of partial rows, walked serially by
  __shared__ double s_tot[GMAX][16];             // 16 row lanes, made this launch 22 us
  const int cl = threadIdx.x & 15, p = threadIdx.x >> 4;
  const int ch = blockIdx.x * 8 + (cl & 7);                 // cl < 8: sum column, cl >= 8: sum of squares
  const int col = (cl < 8) ? ch : C + ch;
  const int W = 2 * C;
  const bool fin = threadIdx.x < 8 && ch < C;
  float rm = (fin && rmean) ? rmean[ch] : 0.f, rv = (fin && rvar) ? rvar[ch] : 0.f;
  for (int g0 = 0; g0 < groups; g0 += GMAX) {
    const int ng = groups - g0 < GMAX ? groups - g0 : GMAX;
    double acc[GMAX] = {0.0, 0.0, 0.0, 0.0};
    if (ch < C) {
#pragma unroll 4
      for (int b = p; b < nblk; b += RL) {
#pragma unroll
        for (int g = 0; g < GMAX; ++g)
          if (g < ng) acc[g] += (double)ws[((size_t)(g0 + g) * nblk + b) * W + col];
      }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < GMAX; ++g) s_p[g][p][cl] = acc[g];
    __syncthreads();
    if (p < ng) {                                 // row-lane p folds group p
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < RL; ++i) t += s_p[p][i][cl];
      s_tot[p][cl] = t;
    }
    __syncthreads();
    if (fin) {
      const int c = ch;
      for (int g = 0; g < ng; ++g) {               // in group order: the running buffers see one update after the other
        float* cg = coef + (size_t)(g0 + g) * 5 * C;
        const double m1 = s_tot[g][threadIdx.x] / count;      // mean of (x - pivot)
        const double var = s_tot[g][8 + threadIdx.x] / count - m1 * m1;
        const double mean = (pivot ? (double)pivot[(size_t)(g0 + g) * C + c] : 0.0) + m1;
        const BnMoments m = bn_coef_rows(mean, var, count, eps, gamma, beta, cg, C, c);
        rm = (1.f - momentum) * rm + momentum * m.mean;
        rv = (1.f - momentum) * rv + momentum * m.unbiased;
      }
    }
  }
  if (fin) {
    if (rmean) rmean[ch] = rm;
    if (rvar) rvar[ch] = rv;
  }
}

// stats_finalize_kernel for `groups` domain groups that each own a SUG_STATS_BLOCKS * 2C workspace block (nblk partial
// rows + the pivot row at SUG_PIVOT_OFFSET): every group's rows are folded in stats_finalize_kernel's own association
// (16 strided row lanes, then the 16 lane sums in ascending order), so coef and the running buffers carry the bits of
// `groups` stats_finalize_kernel launches; the running statistics take the groups' updates in group order from the one
// thread that owns the channel.  blockDim = 256 * GT: the GT = min(groups, SUG_FIN_GT) groups of a pass over the rows
// are folded side by side, by 256 threads each.
#define SUG_FIN_GT 4
__global__ __launch_bounds__(256 * SUG_FIN_GT) void stats_finalize_own_ws_kernel(const float* __restrict__ ws, int nblk, int C,
                                                                                 int groups, const float* __restrict__ gamma,
                                                                                 const float* __restrict__ beta, double count,
                                                                                 float eps, float momentum,
                                                                                 float* __restrict__ rmean, float* __restrict__ rvar,
                                                                                 float* __restrict__ coef) {
  constexpr int UN = 32;
  __shared__ double s_p[SUG_FIN_GT][16][17];
  __shared__ double s_tot[SUG_FIN_GT][16];
  const int GT = blockDim.x >> 8, gl = threadIdx.x >> 8, t = threadIdx.x & 255;
  const int cl = t & 15, p = t >> 4;
  const int ch = blockIdx.x * 8 + (cl & 7);                 // cl < 8: sum column, cl >= 8: sum of squares
  const int col = (cl < 8) ? ch : C + ch;
  const int W = 2 * C;
  const size_t gstride = (size_t)SUG_STATS_BLOCKS * W;
  const bool fin = threadIdx.x < 8 && ch < C;
  float rm = (fin && rmean) ? rmean[ch] : 0.f, rv = (fin && rvar) ? rvar[ch] : 0.f;
  for (int g0 = 0; g0 < groups; g0 += GT) {
    const int ng = groups - g0 < GT ? groups - g0 : GT;
    double acc = 0.0;
    if (ch < C && gl < ng) {
      // UN rows loaded before the first add (row index clamped, so that no load hangs on a branch: one dependent load
      // per row made this launch 44 us); the adds keep their order, b ascending
      const float* wg = ws + (size_t)(g0 + gl) * gstride + col;
      for (int b = p; b < nblk; b += 16 * UN) {
        float v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) v[u] = wg[(size_t)(b + 16 * u < nblk ? b + 16 * u : b) * W];
#pragma unroll
        for (int u = 0; u < UN; ++u)
          if (b + 16 * u < nblk) acc += (double)v[u];
      }
    }
    __syncthreads();                               // the previous pass has read s_tot
    s_p[gl][p][cl] = acc;
    __syncthreads();
    if (p == 0 && gl < ng) {
      double tt = 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) tt += s_p[gl][i][cl];
      s_tot[gl][cl] = tt;
    }
    __syncthreads();
    if (fin) {
      const int c = ch;
      for (int g = 0; g < ng; ++g) {
        float* cg = coef + (size_t)(g0 + g) * 5 * C;
        const float* pivot = ws + (size_t)(g0 + g) * gstride + SUG_PIVOT_OFFSET(C);
        const double m1 = s_tot[g][threadIdx.x] / count;      // mean of (x - pivot)
        const double var = s_tot[g][8 + threadIdx.x] / count - m1 * m1;
        const BnMoments m = bn_coef_rows((double)pivot[c] + m1, var, count, eps, gamma, beta, cg, C, c);
        rm = (1.f - momentum) * rm + momentum * m.mean;
        rv = (1.f - momentum) * rv + momentum * m.unbiased;
      }
    }
  }
  if (fin) {
    if (rmean) rmean[ch] = rm;
    if (rvar) rvar[ch] = rv;
  }
}

// The running-statistics update of G more train-mode forwards on batches whose statistics are
// already known (coef rows 2 and 4), applied in group order with bn_finalize's arithmetic.
__global__ __launch_bounds__(256) void bn_replay_kernel(const float* __restrict__ coef, int G, int C,
                                                        float momentum, float* __restrict__ rmean,
                                                        float* __restrict__ rvar) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float m = rmean[c], v = rvar[c];
  for (int g = 0; g < G; ++g) {
    const float* cg = coef + (size_t)g * 5 * C;
    m = (1.f - momentum) * m + momentum * cg[2 * C + c];
    v = (1.f - momentum) * v + momentum * cg[4 * C + c];
  }
  rmean[c] = m;
  rvar[c] = v;
}

// bn_replay_kernel for up to SUG_REPLAY_MULTI layers in one launch (the BatchNorm layers of a shared encoder prefix:
// replay_bn_stats): blockIdx.y = layer.
#define SUG_REPLAY_MULTI 16
struct ReplayMulti {
  const float* coef[SUG_REPLAY_MULTI];
  float* rmean[SUG_REPLAY_MULTI];
  float* rvar[SUG_REPLAY_MULTI];
  int G[SUG_REPLAY_MULTI], C[SUG_REPLAY_MULTI];
  float momentum[SUG_REPLAY_MULTI];
};
__global__ __launch_bounds__(256) void bn_replay_multi_kernel(ReplayMulti a) {
  const int l = blockIdx.y, C = a.C[l], G = a.G[l];
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float momentum = a.momentum[l];
  const float* coef = a.coef[l];
  float m = a.rmean[l][c], v = a.rvar[l][c];
  for (int g = 0; g < G; ++g) {
    const float* cg = coef + (size_t)g * 5 * C;
    m = (1.f - momentum) * m + momentum * cg[2 * C + c];
    v = (1.f - momentum) * v + momentum * cg[4 * C + c];
  }
  a.rmean[l][c] = m;
  a.rvar[l][c] = v;
}

__global__ __launch_bounds__(256) void affine_act_kernel(const float* __restrict__ z, int64_t ldz,
                                                         const float* __restrict__ coef, int64_t rows,
                                                         int C, float slope, float* __restrict__ out,
                                                         int64_t ldo) {
  const int64_t total = rows * C;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    const int64_t r = e / C;
    const float u = fmaf(coef[c], z[r * ldz + c], coef[C + c]);
    out[r * ldo + c] = u > 0.f ? u : u * slope;
  }
}

__global__ __launch_bounds__(256) void affine_act_vec4_kernel(const float* __restrict__ z, int64_t ldz,
                                                              const float* __restrict__ coef,
                                                              int64_t rows, int C, float slope,
                                                              float* __restrict__ out, int64_t ldo) {
  const int C4 = C >> 2;
  const int64_t total = rows * C4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e % C4) * 4;
    const int64_t r = e / C4;
    const float4 zv = ld4(z + r * ldz + c), sc = ld4(coef + c), sh = ld4(coef + C + c);
    float4 u;
    u.x = fmaf(sc.x, zv.x, sh.x); u.y = fmaf(sc.y, zv.y, sh.y);
    u.z = fmaf(sc.z, zv.z, sh.z); u.w = fmaf(sc.w, zv.w, sh.w);
    u.x = u.x > 0.f ? u.x : u.x * slope; u.y = u.y > 0.f ? u.y : u.y * slope;
    u.z = u.z > 0.f ? u.z : u.z * slope; u.w = u.w > 0.f ? u.w : u.w * slope;
    st4(out + r * ldo + c, u);
  }
}

// affine_act_vec4_kernel with one coefficient set per block of rows_g rows (domain groups)
__global__ __launch_bounds__(256) void affine_act_vec4_groups_kernel(const float* __restrict__ z, int64_t ldz,
                                                                     const float* __restrict__ coef, int64_t rows,
                                                                     int64_t rows_g, int C, float slope,
                                                                     float* __restrict__ out, int64_t ldo) {
  const int C4 = C >> 2;
  const int64_t total = rows * C4;
  const int64_t stride = (int64_t)gridDim.x * 256;
  constexpr int U = 4;                            // independent 16-byte loads in flight per thread
  for (int64_t e0 = (int64_t)blockIdx.x * 256 + threadIdx.x; e0 < total; e0 += U * stride) {
    float4 zv[U];
    int c[U];
    int64_t r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e = e0 + u * stride;
      const int64_t ee = e < total ? e : e0;
      c[u] = (int)(ee % C4) * 4;
      r[u] = ee / C4;
      zv[u] = ld4(z + r[u] * ldz + c[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e0 + u * stride >= total) continue;
      const float* cg = coef + (r[u] / rows_g) * 5 * C;
      const float4 sc = ld4(cg + c[u]), sh = ld4(cg + C + c[u]);
      float4 v;
      v.x = fmaf(sc.x, zv[u].x, sh.x); v.y = fmaf(sc.y, zv[u].y, sh.y);
      v.z = fmaf(sc.z, zv[u].z, sh.z); v.w = fmaf(sc.w, zv[u].w, sh.w);
      v.x = v.x > 0.f ? v.x : v.x * slope; v.y = v.y > 0.f ? v.y : v.y * slope;
      v.z = v.z > 0.f ? v.z : v.z * slope; v.w = v.w > 0.f ? v.w : v.w * slope;
      st4(out + r[u] * ldo + c[u], v);
    }
  }
}

// Column sums (+ squares) of a [rows, C] channel-last tensor.  MODE 0: plain BN stats.
// MODE 1: EdgeConv backward reduce (also writes a = scale*G).
template <int MODE>
__global__ __launch_bounds__(256) void col_reduce_kernel(const float* __restrict__ y, int64_t ldy,
                                                         const float* __restrict__ z,
                                                         const float* __restrict__ coef, int64_t rows,
                                                         int C, float slope, float* __restrict__ a,
                                                         float* __restrict__ ws, int CW,
                                                         int rows_per_block, int pivoted) {
  extern __shared__ float s_red[];  // [256/CW][2*C]
  const int RY = 256 / CW;
  const int cx = threadIdx.x % CW, ry = threadIdx.x / CW;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  for (int c = cx; c < C; c += CW) {
    float s = 0.f, q = 0.f;
    float scale = 0.f, shift = 0.f, mean = 0.f, rstd = 0.f;
    // MODE 0: sums about the pivot = first row of the data (common.h); workgroup 0 publishes it for the finalize
    const float pv = (MODE == 0 && pivoted) ? y[c] : 0.f;
    if (MODE == 0 && pivoted && blockIdx.x == 0 && ry == 0) ws[SUG_PIVOT_OFFSET(C) + c] = pv;
    if (MODE == 1) {
      scale = coef[c]; shift = coef[C + c]; mean = coef[2 * C + c]; rstd = coef[3 * C + c];
    }
    for (int64_t r = r0 + ry; r < r1; r += RY) {
      if (MODE == 0) {
        const float v = y[r * ldy + c] - pv;
        s += v;
        q = fmaf(v, v, q);
      } else {
        const float zv = z[r * C + c];
        const float u = fmaf(scale, zv, shift);
        const float g = y[r * ldy + c] * (u > 0.f ? 1.f : slope);
        a[r * C + c] = scale * g;
        s += g;
        q = fmaf(g, (zv - mean) * rstd, q);
      }
    }
    s_red[(size_t)ry * 2 * C + c] = s;
    s_red[(size_t)ry * 2 * C + C + c] = q;
  }
  __syncthreads();
  // the row-lanes' partials are folded in fp64, in lane order: with few channels there are up to 256 of them, and a serial
  // fp32 fold of that length cost a sum whose terms cancel 12 ulp (C = 1, 300 rows: dgamma off by 7e-7 of itself)
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    double acc = 0.0;
    for (int r = 0; r < RY; ++r) acc += (double)s_red[(size_t)r * 2 * C + i];
    ws[(size_t)blockIdx.x * 2 * C + i] = (float)acc;
  }
}

// float4 variant (C % 4 == 0, 16-B aligned rows): LX lanes along channels (float4 each), LY
// row-lanes, a workgroup covers `rows_per_block` rows; >= 1024 workgroups at the C2 sizes so
// that enough loads are in flight to approach the HBM rate (the scalar kernel above ran at
// ~0.9 TB/s with 128 workgroups).
template <int MODE>
__global__ __launch_bounds__(256) void col_reduce_vec4_kernel(const float* __restrict__ y, int64_t ldy,
                                                              const float* __restrict__ z,
                                                              const float* __restrict__ coef,
                                                              int64_t rows, int C, float slope,
                                                              float* __restrict__ a,
                                                              float* __restrict__ ws, int LX,
                                                              int rows_per_block, int pivoted, int own_ws) {
  extern __shared__ __attribute__((aligned(16))) float s_red[];  // [LY][2*C]
  // own_ws: every group has a whole SUG_STATS_BLOCKS * 2C workspace block (partial rows from its start, its pivot row
  // at SUG_PIVOT_OFFSET inside it), so that a group may use as many partial rows as a single-group call
  if (own_ws) ws += (size_t)blockIdx.y * SUG_STATS_BLOCKS * 2 * C;
  float* const ws_pivot = ws + SUG_PIVOT_OFFSET(C) + (own_ws ? (size_t)0 : (size_t)blockIdx.y * C);      // pivot row of this group
  // blockIdx.y = domain group: `rows` rows each, consecutive in y / z / a; coefficient set g; partial rows
  // [g * gridDim.x + blockIdx.x]
  const int64_t g0 = (int64_t)blockIdx.y * rows;
  y += g0 * ldy;
  if (MODE >= 1) {
    z += g0 * C;
    if (MODE == 1) a += g0 * C;
    coef += (int64_t)blockIdx.y * 5 * C;
  }
  if (!own_ws) ws += (size_t)blockIdx.y * gridDim.x * 2 * C;
  const int LY = 256 / LX;
  const int lx = threadIdx.x % LX, ly = threadIdx.x / LX;
  const int C4 = C >> 2;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  for (int c4 = lx; c4 < C4; c4 += LX) {
    const int c = c4 * 4;
    float4 s = make_float4(0, 0, 0, 0), q = make_float4(0, 0, 0, 0);
    float4 sc = s, sh = s, mean = s, rstd = s;
    // MODE 0: sums about the pivot = first row of the group's data (common.h); workgroup 0 publishes it
    float4 pv = s;
    if (MODE == 0 && pivoted) {
      pv = *reinterpret_cast<const float4*>(y + c);
      if (blockIdx.x == 0 && ly == 0) *reinterpret_cast<float4*>(ws_pivot + c) = pv;
    }
    if (MODE >= 1) {
      sc = *reinterpret_cast<const float4*>(coef + c);
      sh = *reinterpret_cast<const float4*>(coef + C + c);
      mean = *reinterpret_cast<const float4*>(coef + 2 * C + c);
      rstd = *reinterpret_cast<const float4*>(coef + 3 * C + c);
    }
#pragma unroll 4
    for (int64_t r = r0 + ly; r < r1; r += LY) {
      float4 v = *reinterpret_cast<const float4*>(y + r * ldy + c);
      if (MODE == 0) {
        v.x -= pv.x; v.y -= pv.y; v.z -= pv.z; v.w -= pv.w;
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        q.x = fmaf(v.x, v.x, q.x); q.y = fmaf(v.y, v.y, q.y); q.z = fmaf(v.z, v.z, q.z); q.w = fmaf(v.w, v.w, q.w);
      } else {
        const float4 zv = *reinterpret_cast<const float4*>(z + r * C + c);
        float4 g;
        g.x = v.x * (fmaf(sc.x, zv.x, sh.x) > 0.f ? 1.f : slope);
        g.y = v.y * (fmaf(sc.y, zv.y, sh.y) > 0.f ? 1.f : slope);
        g.z = v.z * (fmaf(sc.z, zv.z, sh.z) > 0.f ? 1.f : slope);
        g.w = v.w * (fmaf(sc.w, zv.w, sh.w) > 0.f ? 1.f : slope);
        if (MODE == 1)      // MODE 2: sums only (the apply kernel recomputes a = scale*G from gout and z)
          *reinterpret_cast<float4*>(a + r * C + c) = make_float4(sc.x * g.x, sc.y * g.y, sc.z * g.z, sc.w * g.w);
        s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
        q.x = fmaf(g.x, (zv.x - mean.x) * rstd.x, q.x); q.y = fmaf(g.y, (zv.y - mean.y) * rstd.y, q.y);
        q.z = fmaf(g.z, (zv.z - mean.z) * rstd.z, q.z); q.w = fmaf(g.w, (zv.w - mean.w) * rstd.w, q.w);
      }
    }
    *reinterpret_cast<float4*>(s_red + (size_t)ly * 2 * C + c) = s;
    *reinterpret_cast<float4*>(s_red + (size_t)ly * 2 * C + C + c) = q;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    float acc = 0.f;
    for (int r = 0; r < LY; ++r) acc += s_red[(size_t)r * 2 * C + i];
    ws[(size_t)blockIdx.x * 2 * C + i] = acc;
  }
}

// float4 variant of bn_bwd_apply_kernel (C % 4 == 0, aligned rows)
__global__ __launch_bounds__(256) void bn_bwd_apply_vec4_kernel(const float* __restrict__ a,
                                                                const float* __restrict__ y, int64_t ldy,
                                                                const float* __restrict__ coef,
                                                                const double* __restrict__ red,
                                                                int64_t rows, int C, float invM,
                                                                float* __restrict__ dy, int64_t lddy) {
  const int C4 = C >> 2;
  const int64_t total = rows * C4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e % C4) * 4;
    const int64_t r = e / C4;
    const float4 av = *reinterpret_cast<const float4*>(a + r * C + c);
    const float4 yv = *reinterpret_cast<const float4*>(y + r * ldy + c);
    const float4 sc = *reinterpret_cast<const float4*>(coef + c);
    const float4 mean = *reinterpret_cast<const float4*>(coef + 2 * C + c);
    const float4 rstd = *reinterpret_cast<const float4*>(coef + 3 * C + c);
    float4 o;
    o.x = av.x - sc.x * invM * ((float)red[c + 0] + (yv.x - mean.x) * rstd.x * (float)red[C + c + 0]);
    o.y = av.y - sc.y * invM * ((float)red[c + 1] + (yv.y - mean.y) * rstd.y * (float)red[C + c + 1]);
    o.z = av.z - sc.z * invM * ((float)red[c + 2] + (yv.z - mean.z) * rstd.z * (float)red[C + c + 2]);
    o.w = av.w - sc.w * invM * ((float)red[c + 3] + (yv.w - mean.w) * rstd.w * (float)red[C + c + 3]);
    *reinterpret_cast<float4*>(dy + r * lddy + c) = o;
  }
}

// bn_bwd_apply_vec4_kernel over `rows` rows in domain groups of rows_g: coefficient set and sums of each row's group.
// FROM_G: `a` is the upstream gradient (row stride lda) and a = scale * g * act'(scale*y + shift) is formed here
// (the reduce kernel then writes no [rows, C] tensor: 5 passes over the layer instead of 6).
template <bool FROM_G>
__global__ __launch_bounds__(256) void bn_bwd_apply_vec4_groups_kernel(const float* __restrict__ a, int64_t lda,
                                                                       const float* __restrict__ y, int64_t ldy,
                                                                       const float* __restrict__ coef,
                                                                       const double* __restrict__ red, int64_t rows,
                                                                       int64_t rows_g, int C, float invM, float slope,
                                                                       float* __restrict__ dy, int64_t lddy) {
  const int C4 = C >> 2;
  const int64_t total = rows * C4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e % C4) * 4;
    const int64_t r = e / C4;
    const int64_t g = r / rows_g;
    const float* cg = coef + g * 5 * C;
    const double* rg = red + g * 2 * C;
    float4 av = *reinterpret_cast<const float4*>(a + r * lda + c);
    const float4 yv = *reinterpret_cast<const float4*>(y + r * ldy + c);
    const float4 sc = *reinterpret_cast<const float4*>(cg + c);
    const float4 mean = *reinterpret_cast<const float4*>(cg + 2 * C + c);
    const float4 rstd = *reinterpret_cast<const float4*>(cg + 3 * C + c);
    if (FROM_G) {
      const float4 sh = *reinterpret_cast<const float4*>(cg + C + c);
      av.x = sc.x * (av.x * (fmaf(sc.x, yv.x, sh.x) > 0.f ? 1.f : slope));
      av.y = sc.y * (av.y * (fmaf(sc.y, yv.y, sh.y) > 0.f ? 1.f : slope));
      av.z = sc.z * (av.z * (fmaf(sc.z, yv.z, sh.z) > 0.f ? 1.f : slope));
      av.w = sc.w * (av.w * (fmaf(sc.w, yv.w, sh.w) > 0.f ? 1.f : slope));
    }
    float4 o;
    o.x = av.x - sc.x * invM * ((float)rg[c + 0] + (yv.x - mean.x) * rstd.x * (float)rg[C + c + 0]);
    o.y = av.y - sc.y * invM * ((float)rg[c + 1] + (yv.y - mean.y) * rstd.y * (float)rg[C + c + 1]);
    o.z = av.z - sc.z * invM * ((float)rg[c + 2] + (yv.z - mean.z) * rstd.z * (float)rg[C + c + 2]);
    o.w = av.w - sc.w * invM * ((float)rg[c + 3] + (yv.w - mean.w) * rstd.w * (float)rg[C + c + 3]);
    *reinterpret_cast<float4*>(dy + r * lddy + c) = o;
  }
}

// dy = a - (scale/M) * (dbeta + xhat * dgamma),  a = scale * G  (exact BN gradient)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ a,
                                                           const float* __restrict__ y, int64_t ldy,
                                                           const float* __restrict__ coef,
                                                           const double* __restrict__ red, int64_t rows,
                                                           int C, float invM, float* __restrict__ dy,
                                                           int64_t lddy) {
  const int64_t total = rows * C;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    const int64_t r = e / C;
    const float f = coef[c] * invM;
    const float xhat = (y[r * ldy + c] - coef[2 * C + c]) * coef[3 * C + c];
    dy[r * lddy + c] = a[r * C + c] - f * ((float)red[c] + xhat * (float)red[C + c]);
  }
}

inline int col_width(int C) {
  int cw = 1;
  while (cw < C && cw < 256) cw <<= 1;
  return cw;
}

}  // namespace

int sug_reduce_partials(const float* ws, int nblk, int W, double* out, hipStream_t st) {
  SUG_REQUIRE(ws && out && nblk > 0 && W > 0, "sug_reduce_partials: bad argument");
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(sug_divup(W, 16)), dim3(256), 0, st, ws, nblk, W, out);
  SUG_LAUNCH_CHECK("sug_reduce_partials");
  return SUG_OK;
}

int sug_stats_finalize(const float* ws, int nblk, int C, const float* gamma, const float* beta, double count, float eps,
                       float momentum, float* running_mean, float* running_var, float* coef, hipStream_t st,
                       const float* pivot) {
  SUG_REQUIRE(ws && gamma && beta && coef && nblk > 0 && C > 0 && count > 0, "sug_stats_finalize: bad argument");
  hipLaunchKernelGGL(stats_finalize_kernel, dim3(sug_divup(C, 8)), dim3(256), 0, st, ws, nblk, C, gamma, beta, count, eps,
                     momentum, running_mean, running_var, coef, pivot);
  SUG_LAUNCH_CHECK("sug_stats_finalize");
  return SUG_OK;
}

extern "C" int sug_bn_finalize(const double* stats, const float* gamma, const float* beta, int C,
                               double count, float eps, float momentum, float* running_mean,
                               float* running_var, float* coef, void* stream) {
  SUG_REQUIRE(stats && gamma && beta && coef, "sug_bn_finalize: null pointer");
  SUG_REQUIRE(C > 0 && count > 0, "sug_bn_finalize: bad shape");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(sug_divup(C, 256)), dim3(256), 0, (hipStream_t)stream,
                     stats, gamma, beta, C, count, eps, momentum, running_mean, running_var, coef);
  SUG_LAUNCH_CHECK("sug_bn_finalize");
  return SUG_OK;
}

extern "C" int sug_bn_replay(const float* coef, int G, int C, float momentum, float* running_mean,
                             float* running_var, void* stream) {
  SUG_REQUIRE(coef && running_mean && running_var, "sug_bn_replay: null pointer");
  SUG_REQUIRE(G > 0 && C > 0, "sug_bn_replay: bad shape");
  hipLaunchKernelGGL(bn_replay_kernel, dim3(sug_divup(C, 256)), dim3(256), 0, (hipStream_t)stream, coef, G, C,
                     momentum, running_mean, running_var);
  SUG_LAUNCH_CHECK("sug_bn_replay");
  return SUG_OK;
}

extern "C" int sug_affine_act(const float* z, int64_t ldz, const float* coef, int64_t rows, int C,
                              float slope, float* out, int64_t ldo, void* stream) {
  SUG_REQUIRE(z && coef && out, "sug_affine_act: null pointer");
  SUG_REQUIRE(rows > 0 && C > 0 && ldz >= C && ldo >= C, "sug_affine_act: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C % 4 == 0) && (ldz % 4 == 0) && (ldo % 4 == 0) && ((uintptr_t)z % 16 == 0) &&
                   ((uintptr_t)out % 16 == 0) && ((uintptr_t)coef % 16 == 0);
  const int64_t total = vec ? rows * (C / 4) : rows * C;
  int64_t g = (total + 255) / 256;
  if (g > 4096) g = 4096;
  if (vec)
    hipLaunchKernelGGL(affine_act_vec4_kernel, dim3((int)g), dim3(256), 0, st, z, ldz, coef, rows, C, slope, out, ldo);
  else
    hipLaunchKernelGGL(affine_act_kernel, dim3((int)g), dim3(256), 0, st, z, ldz, coef, rows, C, slope, out, ldo);
  SUG_LAUNCH_CHECK("sug_affine_act");
  return SUG_OK;
}

extern "C" int sug_bn_replay_multi(int n, const void* const* coef, const int32_t* G, const int32_t* C, const float* momentum,
                                   void* const* running_mean, void* const* running_var, void* stream) {
  SUG_REQUIRE(coef && G && C && momentum && running_mean && running_var, "sug_bn_replay_multi: null pointer");
  SUG_REQUIRE(n >= 1 && n <= SUG_REPLAY_MULTI, "sug_bn_replay_multi: %d layers (1..%d)", n, SUG_REPLAY_MULTI);
  ReplayMulti a;
  int cmax = 0;
  for (int i = 0; i < SUG_REPLAY_MULTI; ++i) {
    const int k = i < n ? i : 0;
    SUG_REQUIRE(coef[k] && running_mean[k] && running_var[k] && G[k] >= 1 && C[k] >= 1, "sug_bn_replay_multi: bad layer %d", k);
    a.coef[i] = (const float*)coef[k];
    a.rmean[i] = (float*)running_mean[k];
    a.rvar[i] = (float*)running_var[k];
    a.G[i] = G[k];
    a.C[i] = C[k];
    a.momentum[i] = momentum[k];
    if (i < n && C[k] > cmax) cmax = C[k];
  }
  hipLaunchKernelGGL(bn_replay_multi_kernel, dim3(sug_divup(cmax, 256), n), dim3(256), 0, (hipStream_t)stream, a);
  SUG_LAUNCH_CHECK("sug_bn_replay_multi");
  return SUG_OK;
}

// rows per block such that the grid stays within SUG_STATS_BLOCKS
static int col_rows_per_block(int64_t rows, int cw) {
  int64_t rpb = 64 * (256 / cw) > 256 ? 64 * (256 / cw) : 256;
  while ((rows + rpb - 1) / rpb > SUG_STATS_ROWS) rpb *= 2;
  return (int)rpb;
}

// Launch the column reduction (vectorised when layout allows); returns the number of partial rows.
// rows = rows per group; groups > 1 (vectorised layout only, else -1): one launch over all groups, partial rows
// [group][block]; returns the number of partial rows PER GROUP.  own_ws: ws holds one SUG_STATS_BLOCKS * 2C block per
// group (partial rows + that group's pivot row) and every group is cut into workgroups exactly as a single-group call
// over its rows would cut it: the partial sums, and with them the statistics, equal those of `groups` separate calls
//
// col_reduce_plan is the whole decision, from numbers alone: launch_col_reduce launches what it says and
// sug_bn_rows_plan hands the same answer to a caller (tests assert the path a shape takes from it).  `aligned`: every
// pointer the mode reads or writes sixteen bytes at a time (y; from MODE 1 on z and coef; in MODE 1 also a) is 16-byte
// aligned.  lanes = LX of the float4 kernel resp. CW of the scalar one; grid = -1: refused, nothing is launched.
struct ColReducePlan {
  int vec, lanes, rpb, grid;
};
static ColReducePlan col_reduce_plan(int64_t rows, int C, int64_t ldy, int groups, int own_ws, int mode, bool aligned) {
  ColReducePlan p;
  p.vec = (C % 4 == 0) && (ldy % 4 == 0) && aligned;
  if (p.vec) {
    int lx = 1;
    while (lx < (C >> 2) && lx < 256) lx <<= 1;
    const int ly = 256 / lx;
    int64_t rpb = (rows * (own_ws ? 1 : groups) + SUG_STATS_ROWS - 1) / SUG_STATS_ROWS;
    if (rpb < 4 * ly) rpb = 4 * ly;
    rpb = (rpb + ly - 1) / ly * ly;
    const int grid = sug_divup(rows, rpb);
    p.lanes = lx;
    p.rpb = (int)rpb;
    p.grid = ((int64_t)grid * (own_ws ? 1 : groups) > SUG_STATS_ROWS || groups > 16) ? -1 : grid;
    return p;
  }
  p.lanes = col_width(C);
  p.rpb = col_rows_per_block(rows, p.lanes);
  p.grid = (groups > 1 || mode == 2) ? -1 : sug_divup(rows, p.rpb);
  return p;
}

template <int MODE>
static int launch_col_reduce(const float* y, int64_t ldy, const float* z, const float* coef, int64_t rows,
                             int C, float slope, float* a, float* ws, hipStream_t st, int groups = 1, int pivoted = 0,
                             int own_ws = 0) {
  const bool aligned = ((uintptr_t)y % 16 == 0) &&
                       (MODE == 0 || (((uintptr_t)z % 16 == 0) && (MODE == 2 || (uintptr_t)a % 16 == 0) && ((uintptr_t)coef % 16 == 0)));
  const ColReducePlan p = col_reduce_plan(rows, C, ldy, groups, own_ws, MODE, aligned);
  if (p.grid < 0) return -1;
  if (p.vec)
    hipLaunchKernelGGL((col_reduce_vec4_kernel<MODE>), dim3(p.grid, groups), dim3(256),
                       (size_t)(256 / p.lanes) * 2 * C * sizeof(float), st, y, ldy, z, coef, rows, C, slope, a, ws, p.lanes,
                       p.rpb, pivoted, own_ws);
  else
    hipLaunchKernelGGL((col_reduce_kernel<MODE>), dim3(p.grid), dim3(256), (size_t)(256 / p.lanes) * 2 * C * sizeof(float),
                       st, y, ldy, z, coef, rows, C, slope, a, ws, p.lanes, p.rpb, pivoted);
  return p.grid;
}

extern "C" int sug_bn_rows_plan(int64_t rows, int C, int64_t ld, int groups, int own_ws, int mode, int aligned,
                                int32_t* plan) {
  SUG_REQUIRE(plan, "sug_bn_rows_plan: null pointer");
  SUG_REQUIRE(rows > 0 && C > 0 && C <= 4096 && ld >= C && groups >= 1 && mode >= 0 && mode <= 2,
              "sug_bn_rows_plan: bad shape");
  const ColReducePlan p = col_reduce_plan(rows, C, ld, groups, own_ws, mode, aligned != 0);
  plan[0] = p.vec;
  plan[1] = p.lanes;
  plan[2] = p.rpb;
  plan[3] = p.grid;
  return SUG_OK;
}

extern "C" int sug_col_stats(const float* y, int64_t ldy, int64_t rows, int C, double* stats,
                             float* ws, void* stream) {
  SUG_REQUIRE(y && stats && ws, "sug_col_stats: null pointer");
  SUG_REQUIRE(rows > 0 && C > 0 && C <= 4096 && ldy >= C, "sug_col_stats: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const int grid = launch_col_reduce<0>(y, ldy, nullptr, nullptr, rows, C, 0.f, nullptr, ws, st);
  SUG_LAUNCH_CHECK("sug_col_stats");
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(sug_divup(2 * C, 16)), dim3(256), 0, st, ws, grid, 2 * C, stats);
  SUG_LAUNCH_CHECK("sug_col_stats(reduce)");
  return SUG_OK;
}

// Column statistics of y [rows,C] + BatchNorm coefficients in two launches (sug_col_stats + sug_bn_finalize fused)
extern "C" int sug_col_stats_bn(const float* y, int64_t ldy, int64_t rows, int C, const float* gamma,
                                const float* beta, float eps, float momentum, float* running_mean,
                                float* running_var, float* coef, float* ws, void* stream) {
  SUG_REQUIRE(y && gamma && beta && coef && ws, "sug_col_stats_bn: null pointer");
  SUG_REQUIRE(rows > 0 && C > 0 && C <= 4096 && ldy >= C, "sug_col_stats_bn: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const int grid = launch_col_reduce<0>(y, ldy, nullptr, nullptr, rows, C, 0.f, nullptr, ws, st, 1, 1);
  SUG_LAUNCH_CHECK("sug_col_stats_bn");
  hipLaunchKernelGGL(stats_finalize_kernel, dim3(sug_divup(C, 8)), dim3(256), 0, st, ws, grid, C, gamma, beta,
                     (double)rows, eps, momentum, running_mean, running_var, coef, ws + SUG_PIVOT_OFFSET(C));
  SUG_LAUNCH_CHECK("sug_col_stats_bn(finalize)");
  return SUG_OK;
}

// ---- the grouped forms (internal.h: what each computes, and the 0 / 1 / negative protocol)
int sug_col_stats_bn_groups(const float* y, int64_t ldy, int64_t rows, int C, int groups, const float* gamma,
                            const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                            float* coef, float* ws, hipStream_t st) {
  const int grid = launch_col_reduce<0>(y, ldy, nullptr, nullptr, rows, C, 0.f, nullptr, ws, st, groups, 1);
  if (grid < 0) return 1;
  SUG_LAUNCH_CHECK("sug_bn_act_rows_fwd(stats)");
  hipLaunchKernelGGL(stats_finalize_groups_kernel, dim3(sug_divup(C, 8)), dim3(1024), 0, st, ws, grid, C, groups, gamma, beta,
                     (double)rows, eps, momentum, running_mean, running_var, coef, ws + SUG_PIVOT_OFFSET(C));
  SUG_LAUNCH_CHECK("sug_bn_act_rows_fwd(finalize)");
  return SUG_OK;
}
int sug_col_stats_bn_own_ws(const float* y, int64_t ldy, int64_t rows, int C, int groups, const float* gamma,
                            const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                            float* coef, float* ws, hipStream_t st) {
  if (groups < 2) return 1;
  const int grid = launch_col_reduce<0>(y, ldy, nullptr, nullptr, rows, C, 0.f, nullptr, ws, st, groups, 1, 1);
  if (grid < 0) return 1;
  SUG_LAUNCH_CHECK("sug_col_stats_bn_groups_exact(stats)");
  hipLaunchKernelGGL(stats_finalize_own_ws_kernel, dim3(sug_divup(C, 8)), dim3(256 * (groups < SUG_FIN_GT ? groups : SUG_FIN_GT)), 0,
                     st, ws, grid, C, groups, gamma, beta,
                     (double)rows, eps, momentum, running_mean, running_var, coef);
  SUG_LAUNCH_CHECK("sug_col_stats_bn_groups_exact(finalize)");
  return SUG_OK;
}
int sug_affine_act_groups(const float* z, int64_t ldz, const float* coef, int64_t rows, int groups, int C, float slope,
                          float* out, int64_t ldo, hipStream_t st) {
  const bool vec = (C % 4 == 0) && (ldz % 4 == 0) && (ldo % 4 == 0) && ((uintptr_t)z % 16 == 0) &&
                   ((uintptr_t)out % 16 == 0) && ((uintptr_t)coef % 16 == 0);
  if (!vec) return 1;
  const int64_t total = rows * groups * (C / 4);
  int64_t g = (total + 1023) / 1024;             // 4 float4 per thread and iteration
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(affine_act_vec4_groups_kernel, dim3((int)g), dim3(256), 0, st, z, ldz, coef, rows * groups, rows, C,
                     slope, out, ldo);
  SUG_LAUNCH_CHECK("sug_bn_act_rows_fwd(act)");
  return SUG_OK;
}
int sug_bwd_reduce_groups(const float* gout, int64_t ldg, const float* z, const float* coef, int64_t rows, int Co,
                          int groups, float slope, float* a, double* red, float* ws, hipStream_t st, float* dgb) {
  const int grid = a ? launch_col_reduce<1>(gout, ldg, z, coef, rows, Co, slope, a, ws, st, groups)
                     : launch_col_reduce<2>(gout, ldg, z, coef, rows, Co, slope, nullptr, ws, st, groups);
  if (grid < 0) return 1;
  SUG_LAUNCH_CHECK("sug_edgeconv_bwd_reduce");
  if (dgb)
    hipLaunchKernelGGL(reduce_partials_fold_kernel, dim3(sug_divup(2 * Co, 16)), dim3(256), 0, st, ws, grid, 2 * Co, groups, red, dgb);
  else
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(sug_divup(2 * Co, 16), groups), dim3(256), 0, st, ws, grid, 2 * Co, red);
  SUG_LAUNCH_CHECK("sug_edgeconv_bwd_reduce(reduce)");
  return SUG_OK;
}

extern "C" int sug_edgeconv_bwd_reduce(const float* gout, int64_t ldg, const float* z, const float* coef,
                                       int64_t rows, int Co, float slope, float* a, double* red,
                                       float* ws, void* stream) {
  SUG_REQUIRE(gout && z && coef && a && red && ws, "sug_edgeconv_bwd_reduce: null pointer");
  SUG_REQUIRE(rows > 0 && Co > 0 && Co <= 4096 && ldg >= Co, "sug_edgeconv_bwd_reduce: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const int grid = launch_col_reduce<1>(gout, ldg, z, coef, rows, Co, slope, a, ws, st);
  SUG_LAUNCH_CHECK("sug_edgeconv_bwd_reduce");
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(sug_divup(2 * Co, 16)), dim3(256), 0, st, ws, grid, 2 * Co, red);
  SUG_LAUNCH_CHECK("sug_edgeconv_bwd_reduce(reduce)");
  return SUG_OK;
}

extern "C" int sug_bn_bwd_apply(const float* a, const float* y, int64_t ldy, const float* coef,
                                const double* red, int64_t rows, int C, float* dy, int64_t lddy,
                                void* stream) {
  SUG_REQUIRE(a && y && coef && red && dy, "sug_bn_bwd_apply: null pointer");
  SUG_REQUIRE(rows > 0 && C > 0 && ldy >= C && lddy >= C, "sug_bn_bwd_apply: bad shape");
  const bool vec = (C % 4 == 0) && (ldy % 4 == 0) && (lddy % 4 == 0) && ((uintptr_t)a % 16 == 0) &&
                   ((uintptr_t)y % 16 == 0) && ((uintptr_t)dy % 16 == 0) && ((uintptr_t)coef % 16 == 0);
  if (vec)
    hipLaunchKernelGGL(bn_bwd_apply_vec4_kernel, dim3(sug_ew_grid(rows * C / 4)), dim3(256), 0, (hipStream_t)stream, a,
                       y, ldy, coef, red, rows, C, (float)(1.0 / (double)rows), dy, lddy);
  else
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(sug_ew_grid(rows * C)), dim3(256), 0, (hipStream_t)stream, a, y,
                       ldy, coef, red, rows, C, (float)(1.0 / (double)rows), dy, lddy);
  SUG_LAUNCH_CHECK("sug_bn_bwd_apply");
  return SUG_OK;
}

int sug_bn_bwd_apply_groups(const float* a, int64_t lda, int from_g, float slope, const float* y, int64_t ldy,
                            const float* coef, const double* red, int64_t rows_g, int groups, int C, float* dy,
                            int64_t lddy, hipStream_t st) {
  const bool vec = (C % 4 == 0) && (ldy % 4 == 0) && (lddy % 4 == 0) && (lda % 4 == 0) && ((uintptr_t)a % 16 == 0) &&
                   ((uintptr_t)y % 16 == 0) && ((uintptr_t)dy % 16 == 0) && ((uintptr_t)coef % 16 == 0);
  if (!vec) return 1;
  const int64_t rows = rows_g * groups;
  const float invM = (float)(1.0 / (double)rows_g);
  if (from_g)
    hipLaunchKernelGGL((bn_bwd_apply_vec4_groups_kernel<true>), dim3(sug_ew_grid(rows * C / 4)), dim3(256), 0, st, a, lda, y, ldy,
                       coef, red, rows, rows_g, C, invM, slope, dy, lddy);
  else
    hipLaunchKernelGGL((bn_bwd_apply_vec4_groups_kernel<false>), dim3(sug_ew_grid(rows * C / 4)), dim3(256), 0, st, a, lda, y, ldy,
                       coef, red, rows, rows_g, C, invM, slope, dy, lddy);
  SUG_LAUNCH_CHECK("sug_bn_bwd_apply");
  return SUG_OK;
}
