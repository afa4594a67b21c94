// The MMD^2 / variance / ratio estimator of the Gaussian multi-kernel matrix (the t-statistic objective) and the
// linear-time estimators over adjacent rows.
// Reference: mix_rbf_mmd2_and_ratio + _mmd2_and_ratio / _mmd2_and_variance, model/mmd.py:263-266, :315-373;
// linear_mmd2 / poly_mmd2, :211-236.
//
// Ratio estimator, four launches forward (stream order is the only hand-off between them):
//   A  pairs   K_ij = sum_s exp(ng_s e_ij), G_ij = sum_s ng_s exp(ng_s e_ij) as [2m, 2m] fp32 -- the arithmetic of
//              mmd.hip's pair_epilogue on the fma chains of mmd_rbf_body / mmd_rbf_small_body (restated here, not shared,
//              so that the existing kernels' code objects do not change), the same choice between the two tilings
//   B1 rows    one wave per row of K: the row sums a = Kt_XX e, b = Kt_YY e, r = K_XY e, c = K_XY^T e, the squared
//              sums of the three blocks and the diagonal, fp64, fixed lane tree
//   B2 scalars one workgroup: the 14 sums over the rows in fp64 (thread-strided, lane tree, wave order), then mmd2,
//              var_est, loss
//   C  coefs   wt_m = d mmd2 / dK . G and wt_v = d var_est / dK . G, symmetrised, zero diagonal, formed in fp64
// Backward, one launch: dZ_i = 2 sum_j (f_m wt_m[i,j] + f_v wt_v[i,j]) (z_i - z_j) with the two sums kept apart and the
// factors (from the three upstream gradients and the forward's own outputs, on the device) applied last.
// No atomics, no memset, no host read: capturable, and bit-reproducible run to run.
#include "common.h"

namespace {

constexpr int TI = 16;
constexpr int DK = 64;

struct RatioCoef {                     // model/mmd.py:360-372, m = rows per domain
  double c1, c2, c3, c4, c5, c6;       // 2/(m^2(m-1)^2), (4m-6)/(m^3(m-1)^3), 4(m-2)/(m^3(m-1)^2), 4(m-3)/(m^3(m-1)^2),
  double cxx, cxy, inv_m;              // (8m-12)/(m^5(m-1)), 8/(m^3(m-1)); mmd2: weight of an XX / YY entry, of an XY entry
};

// rows [9][m] fp64, stats [16] fp64
enum { R_A = 0, R_B, R_R, R_C, R_FXX, R_FYY, R_FXY, R_DX, R_DY };
enum { S_A = 0, S_B, S_C, S_MMD2, S_VAR, S_LOSS };
static_assert(R_DY + 1 == SUG_MMD_RATIO_ROW_FIELDS && S_LOSS < SUG_MMD_RATIO_STATS, "scratch sizes of include/sug_amd.h");

// exponent = Z_norm_sqr - 2*ZZT + Z_norm_sqr.t() (model/mmd.py:247), K and its derivative sum: pair_epilogue's lines
__device__ __forceinline__ void kg_store(int i, int j, int M2, float g, float ni, float nj,
                                         const float* __restrict__ neg_gamma, int ns, float* __restrict__ Km,
                                         float* __restrict__ Gm) {
  const float e = __fadd_rn(__fsub_rn(ni, __fmul_rn(2.0f, g)), nj);
  float K = 0.f, Kp = 0.f;
  for (int s = 0; s < ns; ++s) {
    const float ng = neg_gamma[s];
    const float t = expf(__fmul_rn(ng, e));
    K += t;
    Kp = fmaf(ng, t, Kp);
  }
  Km[(int64_t)i * M2 + j] = K;
  Gm[(int64_t)i * M2 + j] = Kp;
}

// 16 x 16 pair tiles, the two 16-row panels of Z through LDS in chunks of DK features (mmd_rbf_body's loop)
__global__ __launch_bounds__(256) void ratio_pairs_kernel(const float* __restrict__ z, int64_t ldz, int m, int D,
                                                          const float* __restrict__ neg_gamma, int ns,
                                                          float* __restrict__ Km, float* __restrict__ Gm) {
  __shared__ float s_a[TI][DK + 1];
  __shared__ float s_b[TI][DK + 1];
  const int M2 = 2 * m;
  const int ti = threadIdx.x / TI, tj = threadIdx.x % TI;
  const int i0 = blockIdx.y * TI, j0 = blockIdx.x * TI;
  const int i = i0 + ti, j = j0 + tj;
  float g = 0.f, ni = 0.f, nj = 0.f;
  for (int d0 = 0; d0 < D; d0 += DK) {
    __syncthreads();
    for (int e = threadIdx.x; e < TI * DK; e += 256) {
      const int r = e / DK, c = e % DK;
      const int d = d0 + c;
      const int ra = i0 + r, rb = j0 + r;
      s_a[r][c] = (ra < M2 && d < D) ? z[(int64_t)ra * ldz + d] : 0.f;
      s_b[r][c] = (rb < M2 && d < D) ? z[(int64_t)rb * ldz + d] : 0.f;
    }
    __syncthreads();
    const int dm = (D - d0) < DK ? (D - d0) : DK;
    for (int c = 0; c < dm; ++c) {
      const float a = s_a[ti][c], b = s_b[tj][c];
      g = fmaf(a, b, g);
      ni = fmaf(a, a, ni);
      nj = fmaf(b, b, nj);
    }
  }
  if (i < M2 && j < M2) kg_store(i, j, M2, g, ni, nj, neg_gamma, ns, Km, Gm);
}

// 2m <= 128, long rows: 4 x 4 pair tiles, the 16 lanes of a pair split D (mmd_rbf_small_body's loop and xor tree)
__global__ __launch_bounds__(256) void ratio_pairs_small_kernel(const float* __restrict__ z, int64_t ldz, int m, int D,
                                                                const float* __restrict__ neg_gamma, int ns,
                                                                float* __restrict__ Km, float* __restrict__ Gm) {
  const int M2 = 2 * m;
  const int l16 = threadIdx.x & 15, pr = threadIdx.x >> 4;
  const int i = blockIdx.y * 4 + (pr >> 2), j = blockIdx.x * 4 + (pr & 3);
  float g = 0.f, ni = 0.f, nj = 0.f;
  if (i < M2 && j < M2) {
    const float* zi = z + (int64_t)i * ldz;
    const float* zj = z + (int64_t)j * ldz;
    int d = l16;
    for (; d + 15 * 16 < D; d += 16 * 16) {
      float av[16], bv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) { av[u] = zi[d + 16 * u]; bv[u] = zj[d + 16 * u]; }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        g = fmaf(av[u], bv[u], g);
        ni = fmaf(av[u], av[u], ni);
        nj = fmaf(bv[u], bv[u], nj);
      }
    }
    for (; d < D; d += 16) {
      const float a = zi[d], b = zj[d];
      g = fmaf(a, b, g);
      ni = fmaf(a, a, ni);
      nj = fmaf(b, b, nj);
    }
  }
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) {
    g += __shfl_xor(g, o);
    ni += __shfl_xor(ni, o);
    nj += __shfl_xor(nj, o);
  }
  if (l16 == 0 && i < M2 && j < M2) kg_store(i, j, M2, g, ni, nj, neg_gamma, ns, Km, Gm);
}

// one wave per row of K [2m, 2m].  An X row i: a_i, r_i, its parts of |Kt_XX|_F^2 and |K_XY|_F^2, K_ii.  A Y row m + j:
// b_j, its part of |Kt_YY|_F^2, K_jj, and c_j = sum_i K[i, m + j] -- the COLUMN of the upper right block (the reference
// reads K_XY = K[:m, m:] only; K is symmetric to rounding, not bit for bit)
__global__ __launch_bounds__(256) void ratio_rows_kernel(const float* __restrict__ Km, int m, double* __restrict__ rows) {
  const int M2 = 2 * m;
  const int lane = threadIdx.x & (WAVE - 1), row = blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE;
  if (row >= M2) return;
  const float* kr = Km + (int64_t)row * M2;
  const bool isx = row < m;
  const int same0 = isx ? 0 : m;
  double ss = 0.0, qs = 0.0, sx = 0.0, qx = 0.0;
  for (int j = same0 + lane; j < same0 + m; j += WAVE) {
    const double k = (j == row) ? 0.0 : (double)kr[j];
    ss += k;
    qs += k * k;
  }
  if (isx) {
    for (int j = m + lane; j < M2; j += WAVE) {
      const double k = (double)kr[j];
      sx += k;
      qx += k * k;
    }
  } else {
    for (int i = lane; i < m; i += WAVE) sx += (double)Km[(int64_t)i * M2 + row];
  }
  ss = wave_sum_d(ss);
  qs = wave_sum_d(qs);
  sx = wave_sum_d(sx);
  qx = wave_sum_d(qx);
  if (lane != 0) return;
  const double dg = (double)kr[row];
  if (isx) {
    rows[R_A * m + row] = ss;
    rows[R_R * m + row] = sx;
    rows[R_FXX * m + row] = qs;
    rows[R_FXY * m + row] = qx;
    rows[R_DX * m + row] = dg;
  } else {
    const int j = row - m;
    rows[R_B * m + j] = ss;
    rows[R_C * m + j] = sx;
    rows[R_FYY * m + j] = qs;
    rows[R_DY * m + j] = dg;
  }
}

// the sums over the rows, then the three results (one workgroup)
constexpr int NSUM = 14;
__global__ __launch_bounds__(256) void ratio_scalars_kernel(const double* __restrict__ rows, int m, int biased, RatioCoef k,
                                                            double* __restrict__ stats, float* __restrict__ out3) {
  __shared__ double s_red[256 / WAVE][NSUM];
  double v[NSUM];
#pragma unroll
  for (int q = 0; q < NSUM; ++q) v[q] = 0.0;
  for (int i = threadIdx.x; i < m; i += 256) {
    const double a = rows[R_A * m + i], b = rows[R_B * m + i], r = rows[R_R * m + i], c = rows[R_C * m + i];
    v[0] += a;
    v[1] += b;
    v[2] += c;                              // K_XY_sum = K_XY_sums_0.sum()
    v[3] += a * a;
    v[4] += b * b;
    v[5] += r * r;
    v[6] += c * c;
    v[7] += a * r;
    v[8] += b * c;
    v[9] += rows[R_FXX * m + i];
    v[10] += rows[R_FYY * m + i];
    v[11] += rows[R_FXY * m + i];
    v[12] += rows[R_DX * m + i];
    v[13] += rows[R_DY * m + i];
  }
#pragma unroll
  for (int q = 0; q < NSUM; ++q) v[q] = wave_sum_d(v[q]);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
    for (int q = 0; q < NSUM; ++q) s_red[threadIdx.x / WAVE][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[NSUM];
  for (int q = 0; q < NSUM; ++q) t[q] = ((s_red[0][q] + s_red[1][q]) + s_red[2][q]) + s_red[3][q];
  const double A = t[0], B = t[1], C = t[2];
  const double mm = (double)m * (double)m, mm1 = (double)m * (double)(m - 1);
  const double mmd2 = biased ? (A + t[12]) / mm + (B + t[13]) / mm - 2.0 * C / mm : A / mm1 + B / mm1 - 2.0 * C / mm;
  const double var = k.c1 * (2.0 * t[3] - t[9] + 2.0 * t[4] - t[10]) - k.c2 * (A * A + B * B) + k.c3 * (t[5] + t[6]) -
                     k.c4 * t[11] - k.c5 * (C * C) + k.c6 * (k.inv_m * (A + B) * C - t[7] - t[8]);
  const double loss = mmd2 / sqrt(var > 1e-8 ? var : 1e-8);            // torch.clamp(var_est, min=1e-8); NaN stays NaN
  stats[S_A] = A;
  stats[S_B] = B;
  stats[S_C] = C;
  stats[S_MMD2] = mmd2;
  stats[S_VAR] = var;
  stats[S_LOSS] = (var != var) ? var : loss;
  out3[0] = (float)stats[S_LOSS];
  out3[1] = (float)mmd2;
  out3[2] = (float)var;
}

// wt_m / wt_v [2m, 2m]: entry (i, j) = coef_ij G_ij + coef_ji G_ji with coef = d mmd2 / dK resp. d var_est / dK of the
// entries the reference reads (both triangles of K_XX and K_YY without their diagonals, the upper right block K_XY):
// symmetric bit for bit, zero diagonal, so dZ_i = 2 sum_j W_ij (z_i - z_j).
__global__ __launch_bounds__(256) void ratio_coef_kernel(const float* __restrict__ Km, const float* __restrict__ Gm,
                                                         const double* __restrict__ rows, const double* __restrict__ stats,
                                                         int m, RatioCoef k, float* __restrict__ wt_m,
                                                         float* __restrict__ wt_v) {
  const int M2 = 2 * m;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)M2 * M2) return;
  const int i = (int)(e / M2), j = (int)(e - (int64_t)i * M2);
  if (i == j) {
    wt_m[e] = 0.f;
    wt_v[e] = 0.f;
    return;
  }
  const double A = stats[S_A], B = stats[S_B], C = stats[S_C];
  double wm, wv;
  if ((i < m) == (j < m)) {
    const bool isx = i < m;
    const int p = isx ? i : i - m, q = isx ? j : j - m;
    const double* sa = rows + (isx ? R_A : R_B) * m;            // the block's own row sums
    const double* sx = rows + (isx ? R_R : R_C) * m;            // and its rows' sums in K_XY
    const double T = isx ? A : B;
    const int64_t et = (int64_t)j * M2 + i;
    const double kij = (double)Km[e], kji = (double)Km[et], gij = (double)Gm[e], gji = (double)Gm[et];
    const double base = -2.0 * k.c2 * T + k.c6 * k.inv_m * C;
    const double cij = k.c1 * (4.0 * sa[p] - 2.0 * kij) + base - k.c6 * sx[p];
    const double cji = k.c1 * (4.0 * sa[q] - 2.0 * kji) + base - k.c6 * sx[q];
    wm = k.cxx * (gij + gji);
    wv = cij * gij + cji * gji;
  } else {
    const int x = i < m ? i : j, y = (i < m ? j : i) - m;
    const int64_t eu = (int64_t)x * M2 + m + y;                 // the entry of the upper right block
    const double kxy = (double)Km[eu], gxy = (double)Gm[eu];
    const double cv = k.c3 * (2.0 * rows[R_R * m + x] + 2.0 * rows[R_C * m + y]) - 2.0 * k.c4 * kxy - 2.0 * k.c5 * C +
                      k.c6 * (k.inv_m * (A + B) - rows[R_A * m + x] - rows[R_B * m + y]);
    wm = k.cxy * gxy;
    wv = cv * gxy;
  }
  wt_m[e] = (float)wm;
  wt_v[e] = (float)wv;
}

// dZ[i, :] = 2 (f_m sum_j wt_m[i,j] (z_i - z_j) + f_v sum_j wt_v[i,j] (z_i - z_j)): workgroup = 64 feature columns x 4 row
// groups of 8 rows; the Z column panel and the two weight panels go through LDS in chunks of JB rows, j ascending.
//   f_m = g_mmd2 + g_loss / sqrt(v_c),  f_v = g_var - g_loss mmd2 v_c^(-3/2) / 2 (that term only while var_est >= 1e-8: the
//   clamp's backward), v_c = max(var_est, 1e-8)
constexpr int JB = 64;
__global__ __launch_bounds__(256) void ratio_bwd_kernel(const float* __restrict__ z, int64_t ldz, int m, int D,
                                                        const float* __restrict__ wt_m, const float* __restrict__ wt_v,
                                                        const float* __restrict__ out3, const float* __restrict__ g3,
                                                        float* __restrict__ dz, int64_t lddz) {
  __shared__ float s_z[JB * 64];
  __shared__ __attribute__((aligned(16))) float s_m[JB * 32];      // [j][local row]: a row group's 8 weights = 2 x b128
  __shared__ __attribute__((aligned(16))) float s_v[JB * 32];
  const int M2 = 2 * m;
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + c;
  const int i0 = blockIdx.y * 32;
  float zi[8], am[8], av[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = i0 + rg * 8 + u;
    zi[u] = (i < M2 && d < D) ? z[(int64_t)i * ldz + d] : 0.f;
    am[u] = 0.f;
    av[u] = 0.f;
  }
  for (int j0 = 0; j0 < M2; j0 += JB) {
    __syncthreads();
    for (int j = rg; j < JB; j += 4) s_z[j * 64 + c] = (d < D && j0 + j < M2) ? z[(int64_t)(j0 + j) * ldz + d] : 0.f;
    for (int e = threadIdx.x; e < JB * 32; e += 256) {
      const int r = e / JB, j = e % JB;                            // consecutive threads along j: coalesced reads
      const int i = i0 + r;
      const bool in = i < M2 && j0 + j < M2;
      s_m[j * 32 + r] = in ? wt_m[(int64_t)i * M2 + j0 + j] : 0.f;
      s_v[j * 32 + r] = in ? wt_v[(int64_t)i * M2 + j0 + j] : 0.f;
    }
    __syncthreads();
    const int jn = (M2 - j0) < JB ? (M2 - j0) : JB;
    for (int j = 0; j < jn; ++j) {
      const float zc = s_z[j * 64 + c];
      const float4 m0 = *reinterpret_cast<const float4*>(s_m + j * 32 + rg * 8);
      const float4 m1 = *reinterpret_cast<const float4*>(s_m + j * 32 + rg * 8 + 4);
      const float4 v0 = *reinterpret_cast<const float4*>(s_v + j * 32 + rg * 8);
      const float4 v1 = *reinterpret_cast<const float4*>(s_v + j * 32 + rg * 8 + 4);
      const float wm[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
      const float wv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float df = zi[u] - zc;
        am[u] = fmaf(wm[u], df, am[u]);
        av[u] = fmaf(wv[u], df, av[u]);
      }
    }
  }
  if (d >= D) return;
  const double gl = (double)g3[0], gm = (double)g3[1], gv = (double)g3[2];
  const double mmd2 = (double)out3[1], var = (double)out3[2];
  const double vc = var > 1e-8 ? var : 1e-8;
  const float fm = (float)(2.0 * (gm + gl / sqrt(vc)));
  const float fv = (float)(2.0 * (gv - (out3[2] >= 1e-8f ? 0.5 * gl * mmd2 / (vc * sqrt(vc)) : 0.0)));
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = i0 + rg * 8 + u;
    if (i < M2) dz[(int64_t)i * lddz + d] = fmaf(fv, av[u], fm * am[u]);
  }
}

// ---- linear-time estimators over adjacent rows (model/mmd.py:211-236).  mode 0, linear_mmd2: t_i = <x_i - y_i,
// x_{i+1} - y_{i+1}> -- the product of the differences, not four dot products that cancel.  mode 1, poly_mmd2:
// t_i = kxx^d + kyy^d - kxy^d - kyx^d with kxx = alpha <x_i, x_{i+1}> + c, kxy = alpha <x_i, y_{i+1}> + c,
// kyx = alpha <y_i, x_{i+1}> + c.  value = mean_i t_i over the m - 1 adjacent pairs.
// One wave per pair: fp32 operands, exact products accumulated in fp64 (lane-strided, lane tree); part [m-1] fp64 holds
// t_i, coef [4][m-1] fp32 the derivative factors d alpha k^(d-1) / (m-1) of kxx, kyy, kxy, kyx (mode 1).
__device__ __forceinline__ double ipow(double b, int d) {
  double r = 1.0;
  for (int q = 0; q < d; ++q) r *= b;
  return r;
}

__global__ __launch_bounds__(256) void adjacent_pairs_kernel(const float* __restrict__ x, int64_t ldx,
                                                             const float* __restrict__ y, int64_t ldy, int m, int D, int mode,
                                                             int deg, double alpha, double cc, double* __restrict__ part,
                                                             float* __restrict__ coef) {
  const int lane = threadIdx.x & (WAVE - 1), i = blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE;
  if (i >= m - 1) return;
  const float* x0 = x + (int64_t)i * ldx;
  const float* x1 = x0 + ldx;
  const float* y0 = y + (int64_t)i * ldy;
  const float* y1 = y0 + ldy;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (mode == 0) {
    for (int d = lane; d < D; d += WAVE) s0 += (double)(x0[d] - y0[d]) * (double)(x1[d] - y1[d]);
    s0 = wave_sum_d(s0);
    if (lane == 0) part[i] = s0;
    return;
  }
  for (int d = lane; d < D; d += WAVE) {
    const double a0 = x0[d], a1 = x1[d], b0 = y0[d], b1 = y1[d];
    s0 += a0 * a1;
    s1 += b0 * b1;
    s2 += a0 * b1;
    s3 += b0 * a1;
  }
  s0 = alpha * wave_sum_d(s0) + cc;
  s1 = alpha * wave_sum_d(s1) + cc;
  s2 = alpha * wave_sum_d(s2) + cc;
  s3 = alpha * wave_sum_d(s3) + cc;
  if (lane != 0) return;
  const double p0 = ipow(s0, deg - 1), p1 = ipow(s1, deg - 1), p2 = ipow(s2, deg - 1), p3 = ipow(s3, deg - 1);
  part[i] = p0 * s0 + p1 * s1 - p2 * s2 - p3 * s3;
  if (coef) {
    const double f = (double)deg * alpha / (double)(m - 1);
    coef[i] = (float)(f * p0);
    coef[(m - 1) + i] = (float)(f * p1);
    coef[2 * (m - 1) + i] = (float)(f * p2);
    coef[3 * (m - 1) + i] = (float)(f * p3);
  }
}

__global__ __launch_bounds__(256) void adjacent_fold_kernel(const double* __restrict__ part, int n, float* __restrict__ value) {
  __shared__ double s_red[256 / WAVE];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) value[0] = (float)((((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) / (double)n);
}

// mode 0: dx_i = g / (m-1) (delta_{i-1} + delta_{i+1}), dy_i = -dx_i (delta = x - y; a missing neighbour adds nothing)
// mode 1: dx_i = g (p_i x_{i+1} + p_{i-1} x_{i-1} - s_i y_{i+1} - t_{i-1} y_{i-1}),
//         dy_i = g (q_i y_{i+1} + q_{i-1} y_{i-1} - s_{i-1} x_{i-1} - t_i x_{i+1})   (p, q, s, t: coef rows 0..3)
__global__ __launch_bounds__(256) void adjacent_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ y,
                                                           int64_t ldy, int m, int D, int mode, const float* __restrict__ coef,
                                                           const float* __restrict__ gscale, float* __restrict__ dx,
                                                           int64_t lddx, float* __restrict__ dy, int64_t lddy) {
  const int d = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (d >= D) return;
  const float g = gscale[0];
  const bool lo = i > 0, hi = i < m - 1;
  const float xl = lo ? x[(int64_t)(i - 1) * ldx + d] : 0.f, xh = hi ? x[(int64_t)(i + 1) * ldx + d] : 0.f;
  const float yl = lo ? y[(int64_t)(i - 1) * ldy + d] : 0.f, yh = hi ? y[(int64_t)(i + 1) * ldy + d] : 0.f;
  float gx, gy;
  if (mode == 0) {
    gx = ((xl - yl) + (xh - yh)) / (float)(m - 1);
    gy = -gx;
  } else {
    const int n = m - 1;
    const float p1 = hi ? coef[i] : 0.f, q1 = hi ? coef[n + i] : 0.f, s1 = hi ? coef[2 * n + i] : 0.f, t1 = hi ? coef[3 * n + i] : 0.f;
    const float p0 = lo ? coef[i - 1] : 0.f, q0 = lo ? coef[n + i - 1] : 0.f, s0 = lo ? coef[2 * n + i - 1] : 0.f,
                t0 = lo ? coef[3 * n + i - 1] : 0.f;
    gx = fmaf(p1, xh, p0 * xl) - fmaf(s1, yh, t0 * yl);
    gy = fmaf(q1, yh, q0 * yl) - fmaf(t1, xh, s0 * xl);
  }
  dx[(int64_t)i * lddx + d] = g * gx;
  dy[(int64_t)i * lddy + d] = g * gy;
}

int ratio_shape_ok(const char* who, int m, int D, int64_t ld) {
  SUG_REQUIRE(m >= 2 && m <= SUG_MMD_EST_MAX_ROWS, "%s: m=%d rows per domain (2..%d)", who, m, SUG_MMD_EST_MAX_ROWS);
  SUG_REQUIRE(D >= 1 && D <= SUG_MMD_EST_MAX_D, "%s: D=%d features (1..%d)", who, D, SUG_MMD_EST_MAX_D);
  SUG_REQUIRE(ld >= D, "%s: row stride %lld < D=%d", who, (long long)ld, D);
  return SUG_OK;
}

}  // namespace

extern "C" int sug_mmd_ratio_fwd(const float* z, int64_t ldz, int m, int D, const float* neg_gamma, int nsigma, int biased,
                                 float* K, float* G, double* rows, double* stats, float* out3, float* wt_m, float* wt_v,
                                 void* stream) {
  if (ratio_shape_ok("sug_mmd_ratio_fwd", m, D, ldz) != SUG_OK) return SUG_ERR_ARG;
  SUG_REQUIRE(nsigma >= 1 && nsigma <= SUG_MMD_EST_MAX_SIGMAS, "sug_mmd_ratio_fwd: nsigma=%d (1..%d)", nsigma,
              SUG_MMD_EST_MAX_SIGMAS);
  SUG_REQUIRE(z && neg_gamma && K && G && rows && stats && out3, "sug_mmd_ratio_fwd: null pointer");
  SUG_REQUIRE((wt_m == nullptr) == (wt_v == nullptr), "sug_mmd_ratio_fwd: wt_m and wt_v go together");
  hipStream_t st = (hipStream_t)stream;
  const int M2 = 2 * m;
  const double dm = (double)m, d1 = dm - 1.0;
  RatioCoef k;
  k.c1 = 2.0 / (dm * dm * d1 * d1);
  k.c2 = (4.0 * dm - 6.0) / (dm * dm * dm * d1 * d1 * d1);
  k.c3 = 4.0 * (dm - 2.0) / (dm * dm * dm * d1 * d1);
  k.c4 = 4.0 * (dm - 3.0) / (dm * dm * dm * d1 * d1);
  k.c5 = (8.0 * dm - 12.0) / (dm * dm * dm * dm * dm * d1);
  k.c6 = 8.0 / (dm * dm * dm * d1);
  k.cxx = biased ? 1.0 / (dm * dm) : 1.0 / (dm * d1);
  k.cxy = -2.0 / (dm * dm);
  k.inv_m = 1.0 / dm;
  if (M2 <= 128 && D >= 256) {          // sug_mmd_rbf's own rule: the K_ij are the numbers mix_rbf_mmd2 sums
    hipLaunchKernelGGL(ratio_pairs_small_kernel, dim3(sug_divup(M2, 4), sug_divup(M2, 4)), dim3(256), 0, st, z, ldz, m, D,
                       neg_gamma, nsigma, K, G);
  } else {
    hipLaunchKernelGGL(ratio_pairs_kernel, dim3(sug_divup(M2, TI), sug_divup(M2, TI)), dim3(256), 0, st, z, ldz, m, D,
                       neg_gamma, nsigma, K, G);
  }
  hipLaunchKernelGGL(ratio_rows_kernel, dim3(sug_divup(M2, 256 / WAVE)), dim3(256), 0, st, K, m, rows);
  hipLaunchKernelGGL(ratio_scalars_kernel, dim3(1), dim3(256), 0, st, rows, m, biased ? 1 : 0, k, stats, out3);
  if (wt_m)
    hipLaunchKernelGGL(ratio_coef_kernel, dim3(sug_divup((int64_t)M2 * M2, 256)), dim3(256), 0, st, K, G, rows, stats, m, k,
                       wt_m, wt_v);
  SUG_LAUNCH_CHECK("sug_mmd_ratio_fwd");
  return SUG_OK;
}

extern "C" int sug_mmd_ratio_bwd(const float* z, int64_t ldz, int m, int D, const float* wt_m, const float* wt_v,
                                 const float* out3, const float* g3, float* dz, int64_t lddz, void* stream) {
  if (ratio_shape_ok("sug_mmd_ratio_bwd", m, D, ldz) != SUG_OK) return SUG_ERR_ARG;
  SUG_REQUIRE(lddz >= D, "sug_mmd_ratio_bwd: row stride %lld < D=%d", (long long)lddz, D);
  SUG_REQUIRE(z && wt_m && wt_v && out3 && g3 && dz, "sug_mmd_ratio_bwd: null pointer");
  hipLaunchKernelGGL(ratio_bwd_kernel, dim3(sug_divup(D, 64), sug_divup(2 * m, 32)), dim3(256), 0, (hipStream_t)stream, z, ldz,
                     m, D, wt_m, wt_v, out3, g3, dz, lddz);
  SUG_LAUNCH_CHECK("sug_mmd_ratio_bwd");
  return SUG_OK;
}

extern "C" int sug_mmd_adjacent_fwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int m, int D, int mode, int degree,
                                    double alpha, double c, double* part, float* coef, float* value, void* stream) {
  if (ratio_shape_ok("sug_mmd_adjacent_fwd", m, D, ldx < ldy ? ldx : ldy) != SUG_OK) return SUG_ERR_ARG;
  SUG_REQUIRE(mode == 0 || mode == 1, "sug_mmd_adjacent_fwd: mode %d (0 linear, 1 poly)", mode);
  SUG_REQUIRE(mode == 0 || (degree >= 1 && degree <= SUG_MMD_POLY_MAX_DEGREE), "sug_mmd_adjacent_fwd: degree=%d (1..%d)", degree,
              SUG_MMD_POLY_MAX_DEGREE);
  SUG_REQUIRE(x && y && part && value, "sug_mmd_adjacent_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adjacent_pairs_kernel, dim3(sug_divup(m - 1, 256 / WAVE)), dim3(256), 0, st, x, ldx, y, ldy, m, D, mode,
                     degree, alpha, c, part, mode == 1 ? coef : nullptr);
  hipLaunchKernelGGL(adjacent_fold_kernel, dim3(1), dim3(256), 0, st, part, m - 1, value);
  SUG_LAUNCH_CHECK("sug_mmd_adjacent_fwd");
  return SUG_OK;
}

extern "C" int sug_mmd_adjacent_bwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int m, int D, int mode,
                                    const float* coef, const float* gscale, float* dx, int64_t lddx, float* dy, int64_t lddy,
                                    void* stream) {
  if (ratio_shape_ok("sug_mmd_adjacent_bwd", m, D, ldx < ldy ? ldx : ldy) != SUG_OK) return SUG_ERR_ARG;
  SUG_REQUIRE(lddx >= D && lddy >= D, "sug_mmd_adjacent_bwd: gradient row stride < D=%d", D);
  SUG_REQUIRE(mode == 0 || mode == 1, "sug_mmd_adjacent_bwd: mode %d (0 linear, 1 poly)", mode);
  SUG_REQUIRE(x && y && gscale && dx && dy && (mode == 0 || coef), "sug_mmd_adjacent_bwd: null pointer");
  hipLaunchKernelGGL(adjacent_bwd_kernel, dim3(sug_divup(D, 256), m), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, m, D,
                     mode, coef, gscale, dx, lddx, dy, lddy);
  SUG_LAUNCH_CHECK("sug_mmd_adjacent_bwd");
  return SUG_OK;
}
