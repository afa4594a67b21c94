// The contrastive alignment mode (NAME: CL): the weighted cosine-embedding loss between paired source / target rows.
// Reference: contrastive_loss_weighted, model/mmd.py:80-94, with nn.CosineEmbeddingLoss(margin, reduction='none') as the
// trainer builds it (train_dg_single_gpu.py:236-242).  Per term and row i of m (x_i, y_i fp32 rows of length D):
//   dot = sum x y,  a = sum x x + 1e-12,  b = sum y y + 1e-12,  cos = dot / sqrt(a b)
//   l_i = 1 - cos (label_s[i] == label_t[i]),  max(0, cos - margin) (otherwise);  loss = (1/m) sum_i w_i l_i
// Forward, two launches for all n <= 4 terms (stream order is the only hand-off between them):
//   rows  one workgroup per (row, term): the three sums of the row, fp64 from the per-lane partials on.  Lane t of the 256
//         takes the element quads t, t + 256, ... in ascending order and, of the D % 4 elements behind the last whole quad,
//         element t; lane tree, then the four waves in index order.  A quad is one 16-byte load where the term's base
//         pointer and row stride allow it and four 4-byte loads otherwise: the same elements in the same lanes in the same
//         order either way, so a strided view and its contiguous copy give the same bits
//   fold  one workgroup per term: cos, l_i, the row's backward coefficients, and the mean (thread-strided rows, lane tree,
//         wave order), rounded to fp32 once
// Backward, one launch for all terms: dx_i = g (c1_i y_i - c2_i x_i), dy_i = g (c1_i x_i - c3_i y_i) with
//   c1 = w s / (m sqrt(a b)), c2 = w s cos / (m a), c3 = w s cos / (m b), s = -1 (positive pair), +1 (negative pair with
//   cos > margin), 0 otherwise; formed in fp64 from the saved fp64 coefficients and the upstream scalar on the device,
//   rounded to fp32 at the store.  dx / dy are stored, not accumulated.
// No atomics, no memset, no host read: capturable, and a row's numbers depend on that row alone.
#include "common.h"
#include <cmath>

namespace {

enum { C_XY = 0, C_X, C_Y, C_COS };
static_assert(C_COS + 1 == SUG_CL_LOSS_ROW_FIELDS && C_Y + 1 == SUG_CL_LOSS_SUM_FIELDS, "scratch sizes of include/sug_amd.h");

struct ClTerm {
  const float* x; const float* y; int64_t ldx, ldy;     // features [m, D] of the two domains
  int D;
  int vx, vy, vdx, vdy;                                    // 16-byte access allowed (base pointer and row stride)
  double margin;
  const float* w;                                          // sample weights [m] or null
  double* coef;                                            // [SUG_CL_LOSS_ROW_FIELDS][m] or null (forward only)
  const float* gscale;                                     // backward: upstream gradient (device scalar)
  float* dx; float* dy; int64_t lddx, lddy;                // backward: gradients [m, D], either may be null
};
struct ClMulti {
  ClTerm t[SUG_CL_LOSS_MAX_TERMS];
};

__device__ __forceinline__ float4 load_quad(const float* p, int vec) {
  if (vec) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ void acc3(float xv, float yv, double& sxy, double& sxx, double& syy) {
  const double xd = (double)xv, yd = (double)yv;
  sxy += xd * yd;
  sxx += xd * xd;
  syy += yd * yd;
}

// sums [n][3][m] fp64: <x, y>, <x, x>, <y, y> of every row
__global__ __launch_bounds__(256) void cl_rows_kernel(ClMulti a, int m, double* __restrict__ sums) {
  __shared__ double s_red[256 / WAVE][3];
  const ClTerm& t = a.t[blockIdx.y];
  const int row = blockIdx.x, D = t.D, nq = D >> 2;
  const float* xr = t.x + (int64_t)row * t.ldx;
  const float* yr = t.y + (int64_t)row * t.ldy;
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  for (int q = threadIdx.x; q < nq; q += 256) {
    const float4 xv = load_quad(xr + 4 * (int64_t)q, t.vx);
    const float4 yv = load_quad(yr + 4 * (int64_t)q, t.vy);
    acc3(xv.x, yv.x, sxy, sxx, syy);
    acc3(xv.y, yv.y, sxy, sxx, syy);
    acc3(xv.z, yv.z, sxy, sxx, syy);
    acc3(xv.w, yv.w, sxy, sxx, syy);
  }
  const int e = 4 * nq + (int)threadIdx.x;
  if (threadIdx.x < 3 && e < D) acc3(xr[e], yr[e], sxy, sxx, syy);
  sxy = wave_sum_d(sxy);
  sxx = wave_sum_d(sxx);
  syy = wave_sum_d(syy);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    s_red[threadIdx.x / WAVE][0] = sxy;
    s_red[threadIdx.x / WAVE][1] = sxx;
    s_red[threadIdx.x / WAVE][2] = syy;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int f = threadIdx.x;
    sums[((int64_t)blockIdx.y * 3 + f) * m + row] = ((s_red[0][f] + s_red[1][f]) + s_red[2][f]) + s_red[3][f];
  }
}

__global__ __launch_bounds__(256) void cl_fold_kernel(ClMulti a, int m, const int64_t* __restrict__ ls,
                                                      const int64_t* __restrict__ lt, const double* __restrict__ sums,
                                                      float* __restrict__ values) {
  __shared__ double s_red[256 / WAVE];
  const ClTerm& t = a.t[blockIdx.x];
  const double* sm = sums + (int64_t)blockIdx.x * 3 * m;
  const double inv_m = 1.0 / (double)m;
  double acc = 0.0;
  for (int i = threadIdx.x; i < m; i += 256) {
    const double dot = sm[C_XY * m + i];
    const double na = sm[C_X * m + i] + 1e-12, nb = sm[C_Y * m + i] + 1e-12;       // EPSILON on the squared norms
    const double den = sqrt(na * nb);
    const double c = dot / den;
    const bool pos = ls[i] == lt[i];
    const double w = t.w ? (double)t.w[i] : 1.0;
    double l, s;
    if (pos) {
      l = 1.0 - c;
      s = -1.0;
    } else if (c > t.margin) {
      l = c - t.margin;
      s = 1.0;
    } else {                                                                       // the clamp; a NaN cos stays NaN
      l = (c != c) ? c : 0.0;
      s = 0.0;
    }
    acc += w * l;
    if (t.coef) {
      const double k = w * s * inv_m;
      t.coef[C_XY * m + i] = k / den;
      t.coef[C_X * m + i] = k * c / na;
      t.coef[C_Y * m + i] = k * c / nb;
      t.coef[C_COS * m + i] = c;
    }
  }
  acc = wave_sum_d(acc);
  if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) values[blockIdx.x] = (float)((((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) * inv_m);
}

__device__ __forceinline__ void store_quad(float* p, float4 v, int vec) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = v;
  } else {
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
}

__device__ __forceinline__ float grad1(double g, double ca, float u, double cb, float v) {
  return (float)(g * (ca * (double)u - cb * (double)v));
}

// grid (quads of the longest row / 256, m, live terms): a thread owns one element quad of one row of one term
__global__ __launch_bounds__(256) void cl_bwd_kernel(ClMulti a, int m) {
  const ClTerm& t = a.t[blockIdx.z];
  const int row = blockIdx.y, D = t.D;
  const int64_t e0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  if (e0 >= D) return;
  const double g = (double)t.gscale[0];
  const double c1 = t.coef[C_XY * m + row], c2 = t.coef[C_X * m + row], c3 = t.coef[C_Y * m + row];
  const float* xr = t.x + (int64_t)row * t.ldx + e0;
  const float* yr = t.y + (int64_t)row * t.ldy + e0;
  float* dxr = t.dx ? t.dx + (int64_t)row * t.lddx + e0 : nullptr;
  float* dyr = t.dy ? t.dy + (int64_t)row * t.lddy + e0 : nullptr;
  if (e0 + 4 <= D) {
    const float4 xv = load_quad(xr, t.vx), yv = load_quad(yr, t.vy);
    if (dxr)
      store_quad(dxr, make_float4(grad1(g, c1, yv.x, c2, xv.x), grad1(g, c1, yv.y, c2, xv.y), grad1(g, c1, yv.z, c2, xv.z),
                                  grad1(g, c1, yv.w, c2, xv.w)), t.vdx);
    if (dyr)
      store_quad(dyr, make_float4(grad1(g, c1, xv.x, c3, yv.x), grad1(g, c1, xv.y, c3, yv.y), grad1(g, c1, xv.z, c3, yv.z),
                                  grad1(g, c1, xv.w, c3, yv.w)), t.vdy);
    return;
  }
  const int rest = (int)(D - e0);                                                   // 1 .. 3 elements behind the last whole quad
  for (int j = 0; j < rest; ++j) {
    const float xv = xr[j], yv = yr[j];
    if (dxr) dxr[j] = grad1(g, c1, yv, c2, xv);
    if (dyr) dyr[j] = grad1(g, c1, xv, c3, yv);
  }
}

inline int quad_ok(const void* p, int64_t ld) { return (((uintptr_t)p & 15) == 0 && (ld & 3) == 0) ? 1 : 0; }

int cl_shape_ok(const char* who, int n, int m) {
  SUG_REQUIRE(n >= 1 && n <= SUG_CL_LOSS_MAX_TERMS, "%s: %d terms (1..%d)", who, n, SUG_CL_LOSS_MAX_TERMS);
  SUG_REQUIRE(m >= 1 && m <= SUG_CL_LOSS_MAX_ROWS, "%s: m=%d rows (1..%d)", who, m, SUG_CL_LOSS_MAX_ROWS);
  return SUG_OK;
}

int cl_term_ok(const char* who, int i, const void* x, int64_t ldx, const void* y, int64_t ldy, int D) {
  SUG_REQUIRE(x && y, "%s: null feature pointer of term %d", who, i);
  SUG_REQUIRE(D >= 1 && D <= SUG_CL_LOSS_MAX_D, "%s: D=%d features of term %d (1..%d)", who, D, i, SUG_CL_LOSS_MAX_D);
  SUG_REQUIRE(ldx >= D && ldy >= D, "%s: row stride %lld < D=%d in term %d", who, (long long)(ldx < ldy ? ldx : ldy), D, i);
  return SUG_OK;
}

}  // namespace

extern "C" int sug_cl_loss_fwd(int n, const void* const* x, const int64_t* ldx, const void* const* y, const int64_t* ldy,
                               const int32_t* D, const double* margin, const int64_t* label_s, const int64_t* label_t, int m,
                               const void* const* w, double* sums, void* const* coef, float* values, void* stream) {
  SUG_REQUIRE(x && ldx && y && ldy && D && margin && label_s && label_t && w && sums && coef && values,
              "sug_cl_loss_fwd: null pointer");
  if (cl_shape_ok("sug_cl_loss_fwd", n, m) != SUG_OK) return SUG_ERR_ARG;
  ClMulti a;
  for (int i = 0; i < n; ++i) {
    if (cl_term_ok("sug_cl_loss_fwd", i, x[i], ldx[i], y[i], ldy[i], D[i]) != SUG_OK) return SUG_ERR_ARG;
    SUG_REQUIRE(std::isfinite(margin[i]), "sug_cl_loss_fwd: margin of term %d is not finite", i);
    ClTerm& t = a.t[i];
    t = ClTerm{};
    t.x = (const float*)x[i];
    t.y = (const float*)y[i];
    t.ldx = ldx[i];
    t.ldy = ldy[i];
    t.D = D[i];
    t.vx = quad_ok(x[i], ldx[i]);
    t.vy = quad_ok(y[i], ldy[i]);
    t.margin = margin[i];
    t.w = (const float*)w[i];
    t.coef = (double*)coef[i];
  }
  for (int i = n; i < SUG_CL_LOSS_MAX_TERMS; ++i) a.t[i] = a.t[0];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cl_rows_kernel, dim3(m, n), dim3(256), 0, st, a, m, sums);
  hipLaunchKernelGGL(cl_fold_kernel, dim3(n), dim3(256), 0, st, a, m, label_s, label_t, sums, values);
  SUG_LAUNCH_CHECK("sug_cl_loss_fwd");
  return SUG_OK;
}

extern "C" int sug_cl_loss_bwd(int n, const void* const* x, const int64_t* ldx, const void* const* y, const int64_t* ldy,
                               const int32_t* D, int m, const void* const* coef, const void* const* gscale, void* const* dx,
                               const int64_t* lddx, void* const* dy, const int64_t* lddy, void* stream) {
  SUG_REQUIRE(x && ldx && y && ldy && D && coef && gscale && dx && lddx && dy && lddy, "sug_cl_loss_bwd: null pointer");
  if (cl_shape_ok("sug_cl_loss_bwd", n, m) != SUG_OK) return SUG_ERR_ARG;
  ClMulti a;
  int na = 0, dmax = 0;
  for (int i = 0; i < n; ++i) {
    if (!gscale[i] || (!dx[i] && !dy[i])) continue;                    // a term without a gradient to form: skipped
    if (cl_term_ok("sug_cl_loss_bwd", i, x[i], ldx[i], y[i], ldy[i], D[i]) != SUG_OK) return SUG_ERR_ARG;
    SUG_REQUIRE(coef[i], "sug_cl_loss_bwd: null coefficients of term %d", i);
    SUG_REQUIRE((!dx[i] || lddx[i] >= D[i]) && (!dy[i] || lddy[i] >= D[i]), "sug_cl_loss_bwd: gradient row stride < D=%d in term %d",
                D[i], i);
    ClTerm& t = a.t[na++];
    t = ClTerm{};
    t.x = (const float*)x[i];
    t.y = (const float*)y[i];
    t.ldx = ldx[i];
    t.ldy = ldy[i];
    t.D = D[i];
    t.vx = quad_ok(x[i], ldx[i]);
    t.vy = quad_ok(y[i], ldy[i]);
    t.coef = (double*)coef[i];
    t.gscale = (const float*)gscale[i];
    t.dx = (float*)dx[i];
    t.dy = (float*)dy[i];
    t.lddx = lddx[i];
    t.lddy = lddy[i];
    t.vdx = dx[i] ? quad_ok(dx[i], lddx[i]) : 0;
    t.vdy = dy[i] ? quad_ok(dy[i], lddy[i]) : 0;
    if (D[i] > dmax) dmax = D[i];
  }
  if (na == 0) return SUG_OK;
  for (int i = na; i < SUG_CL_LOSS_MAX_TERMS; ++i) a.t[i] = a.t[0];
  hipLaunchKernelGGL(cl_bwd_kernel, dim3(sug_divup(sug_divup(dmax, 4), 256), m, na), dim3(256), 0, (hipStream_t)stream, a, m);
  SUG_LAUNCH_CHECK("sug_cl_loss_bwd");
  return SUG_OK;
}
