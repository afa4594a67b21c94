// Classifier head of the source-only Point Transformer (PointTransformerCls, model/Ptran_model.py:94-117):
//     logits = L3(relu(L2(relu(L1(mean_P(points))))))      points [B, P, K], L1 K->N1, L2 N1->N2, L3 N2->NC
// for the few rows of a step (B <= 128; K = 512, N1 = 256, N2 = 64 in the model).  The library path is ~20 launches of a
// few us each per forward + backward (mean, three GEMMs with their bias adds and ReLUs, then their backwards); the whole
// arithmetic is ~0.1 GFLOP.  Here:
//   forward   ptcls_fwd1_kernel   mean over P (kept for dW1) and h1 = relu(mean . W1^T + b1);
//             ptcls_fwd2_kernel   h2 = relu(h1 . W2^T + b2) and logits = h2 . W3^T + b3 (h2 stays in LDS between them);
//   backward  ptcls_bwd1_kernel   the row-local chain dz2 = (G . W3) * [h2 > 0], dz1 = (dz2 . W2) * [h1 > 0];
//             ptcls_bwd2_kernel   one wave per 16 x 16 output tile: dpoints = broadcast(dz1 . W1) / P, dW1 = dz1^T . mean,
//                                 dW2 = dz2^T . h1, dW3 = G^T . h2, and the bias gradients (column sums over the rows).
// fp32 on the matrix pipe (v_mfma_f32_16x16x4_f32: an exact fp32 fma chain in k order).  Every output element is summed by
// one wave in one fixed order (no atomics, no split over workgroups), so two runs are bit-identical.
//
// Operand mapping of v_mfma_f32_16x16x4_f32: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15];
// register r of the result holds D[4 (l >> 4) + r][l & 15].  Which four k's a step multiplies is free as long as A and B
// agree: the row-major operands are read as float4 at k = 16 u + 4 q (q = l >> 4), element e of the float4 feeding step e.
#include "common.h"
#include "device_helpers.h"

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int NT = 256;          // threads per workgroup (4 waves)
constexpr int RB = 16;           // rows per workgroup / tile
constexpr int N2F = 64;          // width of the second hidden layer (4 waves x 16 columns in ptcls_fwd2 / ptcls_bwd1)
constexpr int SP = N2F + 4;      // LDS row stride of an [RB][N2F] tile

__device__ __forceinline__ f32x4 zero4() { f32x4 z; z[0] = z[1] = z[2] = z[3] = 0.f; return z; }
__device__ __forceinline__ f32x4 mma4(float4 a, float4 b, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  return acc;
}

// ---------------------------------------------------------------------------------------------------- forward
// Workgroup = rows [r0, r0 + 16) x columns [c0, c0 + 16) of h1.  Wave w sums k in [w K/4, (w + 1) K/4); the four partial
// tiles are added in wave order with the bias.  Workgroups with blockIdx.x == 0 also write the mean rows.
__global__ __launch_bounds__(NT) void ptcls_fwd1_kernel(const float* __restrict__ pts, int B, int P, int K,
                                                        const float* __restrict__ W1, const float* __restrict__ b1, int N1,
                                                        float* __restrict__ mean, float* __restrict__ h1) {
  __shared__ float s_part[4][RB][RB + 1];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.y * RB, c0 = blockIdx.x * RB;
  const int row = min(r0 + i, B - 1);
  const bool wmean = blockIdx.x == 0 && r0 + i < B;
  const float fp = (float)P;
  const float* prow = pts + (int64_t)row * P * K;
  const float* wrow = W1 + (int64_t)(c0 + i) * K;
  const int KW = K >> 2;
  f32x4 acc = zero4();
  for (int u = 0; u < KW; u += 16) {
    const int k = w * KW + u + 4 * q;
    float4 a = ld4(prow + k);
    for (int p = 1; p < P; ++p) {
      const float4 v = ld4(prow + (int64_t)p * K + k);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    a.x /= fp; a.y /= fp; a.z /= fp; a.w /= fp;
    if (wmean) *reinterpret_cast<float4*>(mean + (int64_t)row * K + k) = a;
    acc = mma4(a, ld4(wrow + k), acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) s_part[w][4 * q + r][i] = acc[r];
  __syncthreads();
  const int ii = t >> 4, jj = t & 15;
  if (r0 + ii < B) {
    const float s = ((s_part[0][ii][jj] + s_part[1][ii][jj]) + s_part[2][ii][jj]) + s_part[3][ii][jj] + b1[c0 + jj];
    h1[(int64_t)(r0 + ii) * N1 + c0 + jj] = s > 0.f ? s : 0.f;
  }
}

// Workgroup = rows [r0, r0 + 16): wave w forms columns [16 w, 16 w + 16) of h2 over all N1, the tile goes to LDS, then wave
// w forms logit columns [16 w, 16 w + 16) (waves with 16 w >= NC idle).
__global__ __launch_bounds__(NT) void ptcls_fwd2_kernel(const float* __restrict__ h1, int B, int N1,
                                                        const float* __restrict__ W2, const float* __restrict__ b2,
                                                        const float* __restrict__ W3, const float* __restrict__ b3, int NC,
                                                        float* __restrict__ h2, float* __restrict__ logits) {
  __shared__ __attribute__((aligned(16))) float s_h2[RB * SP];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.x * RB;
  const float* arow = h1 + (int64_t)min(r0 + i, B - 1) * N1;
  const float* wrow = W2 + (int64_t)(16 * w + i) * N1;
  f32x4 acc = zero4();
  for (int u = 0; u < N1; u += 16) acc = mma4(ld4(arow + u + 4 * q), ld4(wrow + u + 4 * q), acc);
  const int col = 16 * w + i;
  const float bias2 = b2[col];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ir = 4 * q + r;
    const float s = acc[r] + bias2;
    const float v = s > 0.f ? s : 0.f;
    s_h2[ir * SP + col] = v;
    if (r0 + ir < B) h2[(int64_t)(r0 + ir) * N2F + col] = v;
  }
  __syncthreads();
  if (16 * w >= NC) return;
  const float* w3row = W3 + (int64_t)min(16 * w + i, NC - 1) * N2F;
  acc = zero4();
#pragma unroll
  for (int u = 0; u < N2F; u += 16)
    acc = mma4(ld4(s_h2 + i * SP + u + 4 * q), ld4(w3row + u + 4 * q), acc);
  if (col < NC) {
    const float bias3 = b3[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ir = 4 * q + r;
      if (r0 + ir < B) logits[(int64_t)(r0 + ir) * NC + col] = acc[r] + bias3;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- backward
// Workgroup = rows [r0, r0 + 16): dz2 (wave w: columns [16 w, 16 w + 16), k over the NC classes, zero-padded to a multiple
// of 4) to LDS and global, then dz1 (wave w: column tiles w, w + 4, ...; k over the 64 columns of dz2).
__global__ __launch_bounds__(NT) void ptcls_bwd1_kernel(const float* __restrict__ G, int B, int NC,
                                                        const float* __restrict__ W3, const float* __restrict__ h2,
                                                        const float* __restrict__ W2, const float* __restrict__ h1, int N1,
                                                        float* __restrict__ dz2, float* __restrict__ dz1) {
  __shared__ __attribute__((aligned(16))) float s_dz2[RB * SP];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.x * RB;
  const int row = min(r0 + i, B - 1);
  const int col = 16 * w + i;
  f32x4 acc = zero4();
  for (int k0 = 0; k0 < NC; k0 += 4) {
    const int k = k0 + q;
    const bool ok = k < NC;
    const float a = ok ? G[(int64_t)row * NC + k] : 0.f;
    const float b = ok ? W3[(int64_t)k * N2F + col] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ir = 4 * q + r;
    const int rr = min(r0 + ir, B - 1);
    const float v = h2[(int64_t)rr * N2F + col] > 0.f ? acc[r] : 0.f;
    s_dz2[ir * SP + col] = v;
    if (r0 + ir < B) dz2[(int64_t)(r0 + ir) * N2F + col] = v;
  }
  __syncthreads();
  for (int ct = w; ct < N1 / 16; ct += 4) {
    const int c = ct * 16 + i;
    acc = zero4();
#pragma unroll 4
    for (int k0 = 0; k0 < N2F; k0 += 4) {
      const int k = k0 + q;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(s_dz2[i * SP + k], W2[(int64_t)k * N1 + c], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ir = 4 * q + r;
      if (r0 + ir < B) {
        const int64_t o = (int64_t)(r0 + ir) * N1 + c;
        dz1[o] = h1[o] > 0.f ? acc[r] : 0.f;
      }
    }
  }
}

struct Bwd2Args {
  const float *G, *mean, *h1, *h2, *dz1, *dz2, *W1;
  float *dpts, *dW1, *db1, *dW2, *db2, *dW3, *db3;
  int B, P, K, N1, NC;
  int n_dx, n_w1, n_w2, n_w3;        // job counts of the tile kinds, in this order, then the bias jobs
};

// C[16 x 16] += A^T B over the B rows (k = batch row, zero-padded to a multiple of 4): A[k][n0 + i] with row stride lda
// (column n0 + i beyond na reads 0), B[k][c0 + j] with row stride ldb.
__device__ __forceinline__ f32x4 tile_atb(const float* A, int lda, int na, int n0, const float* Bm, int ldb, int c0, int rows,
                                          int i, int q) {
  f32x4 acc = zero4();
  const bool oka = n0 + i < na;
  for (int k0 = 0; k0 < rows; k0 += 4) {
    const int k = k0 + q;
    const bool ok = k < rows;
    const float a = (ok && oka) ? A[(int64_t)k * lda + n0 + i] : 0.f;
    const float b = ok ? Bm[(int64_t)k * ldb + c0 + i] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

__global__ __launch_bounds__(NT) void ptcls_bwd2_kernel(Bwd2Args a) {
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  int job = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int B = a.B, K = a.K, N1 = a.N1, NC = a.NC;
  if (job < a.n_dx) {                 // dmean tile (rows r0.., input columns c0..) = dz1 . W1, spread over the P points
    const int ct = job % (K / 16), r0 = (job / (K / 16)) * RB, c0 = ct * 16;
    const float* arow = a.dz1 + (int64_t)min(r0 + i, B - 1) * N1;
    f32x4 acc = zero4();
    for (int k0 = 0; k0 < N1; k0 += 4) {
      const int k = k0 + q;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[k], a.W1[(int64_t)k * K + c0 + i], acc, 0, 0, 0);
    }
    const float fp = (float)a.P;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + 4 * q + r;
      if (row < B) {
        const float v = acc[r] / fp;
        for (int p = 0; p < a.P; ++p) a.dpts[((int64_t)row * a.P + p) * K + c0 + i] = v;
      }
    }
    return;
  }
  job -= a.n_dx;
  if (job < a.n_w1) {                 // dW1 [N1, K] = dz1^T . mean
    const int ct = job % (K / 16), n0 = (job / (K / 16)) * 16, c0 = ct * 16;
    const f32x4 acc = tile_atb(a.dz1, N1, N1, n0, a.mean, K, c0, B, i, q);
#pragma unroll
    for (int r = 0; r < 4; ++r) a.dW1[(int64_t)(n0 + 4 * q + r) * K + c0 + i] = acc[r];
    return;
  }
  job -= a.n_w1;
  if (job < a.n_w2) {                 // dW2 [N2, N1] = dz2^T . h1
    const int ct = job % (N1 / 16), n0 = (job / (N1 / 16)) * 16, c0 = ct * 16;
    const f32x4 acc = tile_atb(a.dz2, N2F, N2F, n0, a.h1, N1, c0, B, i, q);
#pragma unroll
    for (int r = 0; r < 4; ++r) a.dW2[(int64_t)(n0 + 4 * q + r) * N1 + c0 + i] = acc[r];
    return;
  }
  job -= a.n_w2;
  if (job < a.n_w3) {                 // dW3 [NC, N2] = G^T . h2
    const int ct = job % (N2F / 16), n0 = (job / (N2F / 16)) * 16, c0 = ct * 16;
    const f32x4 acc = tile_atb(a.G, NC, NC, n0, a.h2, N2F, c0, B, i, q);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n0 + 4 * q + r < NC) a.dW3[(int64_t)(n0 + 4 * q + r) * N2F + c0 + i] = acc[r];
    return;
  }
  job -= a.n_w3;
  // bias gradients: 64 columns per wave, each the sum over the rows in row order
  const int nb1 = N1 / 64;
  const float* src;
  float* dst;
  int ld, n, c;
  if (job < nb1) { src = a.dz1; dst = a.db1; ld = N1; n = N1; c = job * 64 + lane; }
  else if (job == nb1) { src = a.dz2; dst = a.db2; ld = N2F; n = N2F; c = lane; }
  else if (job == nb1 + 1) { src = a.G; dst = a.db3; ld = NC; n = NC; c = lane; }
  else return;
  if (c >= n) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += src[(int64_t)b * ld + c];
  dst[c] = s;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" int sug_ptcls_head_supported(int B, int P, int K, int N1, int N2, int NC) {
  if (B < 1 || B > 128 || P < 1 || P > 64) return 0;
  if (K < 64 || K > 1024 || K % 64) return 0;            // (four waves, 16 k per step each)
  if (N1 < 64 || N1 > 1024 || N1 % 64) return 0;          // (the bias jobs of ptcls_bwd2 take 64 columns each)
  if (N2 != N2F) return 0;
  if (NC < 2 || NC > 64) return 0;
  return 1;
}

extern "C" int sug_ptcls_head_fwd(const float* points, int B, int P, int K, const float* W1, const float* b1, int N1,
                                  const float* W2, const float* b2, int N2, const float* W3, const float* b3, int NC,
                                  float* mean, float* h1, float* h2, float* logits, void* stream) {
  SUG_REQUIRE(sug_ptcls_head_supported(B, P, K, N1, N2, NC),
              "sug_ptcls_head_fwd: unsupported shape B=%d P=%d K=%d N1=%d N2=%d NC=%d", B, P, K, N1, N2, NC);
  SUG_REQUIRE(points && W1 && b1 && W2 && b2 && W3 && b3 && mean && h1 && h2 && logits, "sug_ptcls_head_fwd: null pointer");
  SUG_REQUIRE(aligned16(points) && aligned16(W1) && aligned16(W2) && aligned16(W3) && aligned16(mean) && aligned16(h1),
              "sug_ptcls_head_fwd: operands must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ptcls_fwd1_kernel, dim3(N1 / RB, sug_divup(B, RB)), dim3(NT), 0, st, points, B, P, K, W1, b1, N1,
                     mean, h1);
  SUG_LAUNCH_CHECK("sug_ptcls_head_fwd");
  hipLaunchKernelGGL(ptcls_fwd2_kernel, dim3(sug_divup(B, RB)), dim3(NT), 0, st, h1, B, N1, W2, b2, W3, b3, NC, h2, logits);
  SUG_LAUNCH_CHECK("sug_ptcls_head_fwd");
  return SUG_OK;
}

extern "C" int sug_ptcls_head_bwd(const float* dlogits, const float* mean, const float* h1, const float* h2, int B, int P,
                                  int K, const float* W1, int N1, const float* W2, int N2, const float* W3, int NC,
                                  float* dz1, float* dz2, float* dpoints, float* dW1, float* db1, float* dW2, float* db2,
                                  float* dW3, float* db3, void* stream) {
  SUG_REQUIRE(sug_ptcls_head_supported(B, P, K, N1, N2, NC),
              "sug_ptcls_head_bwd: unsupported shape B=%d P=%d K=%d N1=%d N2=%d NC=%d", B, P, K, N1, N2, NC);
  SUG_REQUIRE(dlogits && mean && h1 && h2 && W1 && W2 && W3 && dz1 && dz2 && dpoints && dW1 && db1 && dW2 && db2 && dW3 &&
              db3, "sug_ptcls_head_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ptcls_bwd1_kernel, dim3(sug_divup(B, RB)), dim3(NT), 0, st, dlogits, B, NC, W3, h2, W2, h1, N1, dz2,
                     dz1);
  SUG_LAUNCH_CHECK("sug_ptcls_head_bwd");
  Bwd2Args a;
  a.G = dlogits; a.mean = mean; a.h1 = h1; a.h2 = h2; a.dz1 = dz1; a.dz2 = dz2; a.W1 = W1;
  a.dpts = dpoints; a.dW1 = dW1; a.db1 = db1; a.dW2 = dW2; a.db2 = db2; a.dW3 = dW3; a.db3 = db3;
  a.B = B; a.P = P; a.K = K; a.N1 = N1; a.NC = NC;
  a.n_dx = sug_divup(B, RB) * (K / 16);
  a.n_w1 = (N1 / 16) * (K / 16);
  a.n_w2 = (N2F / 16) * (N1 / 16);
  a.n_w3 = sug_divup(NC, 16) * (N2F / 16);
  const int jobs = a.n_dx + a.n_w1 + a.n_w2 + a.n_w3 + N1 / 64 + 2;
  hipLaunchKernelGGL(ptcls_bwd2_kernel, dim3(sug_divup(jobs, 4)), dim3(NT), 0, st, a);
  SUG_LAUNCH_CHECK("sug_ptcls_head_bwd");
  return SUG_OK;
}
