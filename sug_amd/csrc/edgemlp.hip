// Two-layer EdgeConv block: the EdgeConv blocks of the DGCNN part-segmentation network and the DGCNN form of the T-Net
// (model/model_utils.py:70-77 with DGCNN_Flag) put TWO 1x1 convolutions in front of the max over the k neighbours:
//     y1 = P[idx] + Q,  a1 = act1(bn1(y1)),  y2 = a1 . W^T (+ b),  out = act2(bn2(ext_j y2))
// The first layer is not monotone into the max, so y1 has to exist per edge; what never exists is the [B,N,k,2C] edge
// feature, y2 and a2.
//
//   edge_expand_kernel      y1 [B*N*k, 64] from [P | Q] and the lists, with the BatchNorm sums of y1 from the same pass
//   edgemlp_max_kernel      the short-segment sibling of pointmlp_max_kernel<64, XF>: bn1 + act1 on the way into LDS (a1
//                           written once for the backward), 32-row MFMA tiles, bn2 sums, extreme + arg per k-row segment
//   edge_expand_bwd_kernel  dY1 -> [dP | dQ] over the reverse lists, fixed order
//
// Segments of k rows (2 <= k <= 32) do not line up with the 32-row tiles: a tile holds several, or one straddles two.
// The accumulator tile (sign-folded y2) therefore goes through LDS once and one thread per channel walks its 32 rows in
// ascending order with the running extreme, its j and the segment counter in registers: they reset where a segment ends,
// wherever in a tile that is.  A workgroup owns whole segments, so nothing is carried between workgroups.
#include "common.h"
#include "mfma_tile.h"

namespace {
using namespace sug_tile;

constexpr int EC = 64;                 // C1: channels of y1 / a1 = K of the second layer
constexpr int ECH = EC / 4;            // float4 chunks per row

__global__ __launch_bounds__(256) void edge_expand_kernel(const float* __restrict__ pq, int64_t ldpq,
                                                          const int32_t* __restrict__ idx, int N, int k, int E, int per_wg,
                                                          float* __restrict__ y1, float* __restrict__ ws) {
  __shared__ double s_a[16][EC], s_b[16][EC];
  const int c4 = threadIdx.x & (ECH - 1), rs = threadIdx.x >> 4;
  auto edge = [&](int e) {
    const int p = e / k, b = p / N;
    int m = idx[e];
    m = m < 0 ? 0 : (m >= N ? N - 1 : m);
    const float4 pv = *reinterpret_cast<const float4*>(pq + ((int64_t)b * N + m) * ldpq + c4 * 4);
    const float4 qv = *reinterpret_cast<const float4*>(pq + (int64_t)p * ldpq + EC + c4 * 4);
    return make_float4(__fadd_rn(pv.x, qv.x), __fadd_rn(pv.y, qv.y), __fadd_rn(pv.z, qv.z), __fadd_rn(pv.w, qv.w));
  };
  const float4 pvt = edge(0);                               // pivot of the BatchNorm sums: y1 of the launch's first edge
  if (blockIdx.x == 0 && rs == 0) *reinterpret_cast<float4*>(ws + SUG_PIVOT_OFFSET(EC) + c4 * 4) = pvt;
  // per-thread sums in fp64 (the pass is bound by memory): the only fp32 rounding of the sums is that of the partial row
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  const int e0 = blockIdx.x * per_wg;
  const int e1 = (E - e0 < per_wg) ? E : e0 + per_wg;
  for (int e = e0 + rs; e < e1; e += 16) {
    const float4 y = edge(e);
    *reinterpret_cast<float4*>(y1 + (int64_t)e * EC + c4 * 4) = y;
    const double v[4] = {(double)(y.x - pvt.x), (double)(y.y - pvt.y), (double)(y.z - pvt.z), (double)(y.w - pvt.w)};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      s1[u] += v[u];
      s2[u] = fma(v[u], v[u], s2[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    s_a[rs][c4 * 4 + u] = s1[u];
    s_b[rs][c4 * 4 + u] = s2[u];
  }
  __syncthreads();
  if (threadIdx.x < 2 * EC) {                               // the 16 row slots in ascending order
    const int c = threadIdx.x & (EC - 1);
    const bool sq = threadIdx.x >= EC;
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += sq ? s_b[i][c] : s_a[i][c];
    ws[(size_t)blockIdx.x * 2 * EC + threadIdx.x] = (float)t;
  }
}

template <int CO>
__global__ __launch_bounds__(2 * CO) void edgemlp_max_kernel(
    const float* __restrict__ x, int64_t ldx, int R, const float* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ gamma, int k, int rows_per_wg, float* __restrict__ zext, int32_t* __restrict__ arg,
    float* __restrict__ ws, const float* __restrict__ xcoef, float xslope, float* __restrict__ zout, int64_t ldz) {
  constexpr int CP = EC, NT = 2 * CO;
  constexpr int RS = CP + 4, HALF = CP / 2, CH = CP / 8, YS = CO + 1;
  __shared__ __attribute__((aligned(16))) float s_tile[TJ * RS];
  __shared__ float s_y[TJ * YS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cj = lane & 31, h = lane >> 5;
  const int col = wv * 32 + cj;
  const int rb = blockIdx.x;
  const int row_begin = rb * rows_per_wg;
  const int nrows = (R - row_begin < rows_per_wg) ? R - row_begin : rows_per_wg;
  const float* xb = x + (int64_t)row_begin * ldx;

  // B operand, sign of gamma folded in, pivot: as pointmlp_max_kernel
  float bq[HALF];
  {
    const float* wr = W + (int64_t)col * CP;
#pragma unroll
    for (int g = 0; g < CP / 8; ++g) {
      const float4 lo = *reinterpret_cast<const float4*>(wr + 8 * g);
      const float4 hi = *reinterpret_cast<const float4*>(wr + 8 * g + 4);
      bq[4 * g + 0] = h ? lo.y : lo.x;
      bq[4 * g + 1] = h ? lo.w : lo.z;
      bq[4 * g + 2] = h ? hi.y : hi.x;
      bq[4 * g + 3] = h ? hi.w : hi.z;
    }
  }
  float xsc[8], xsh[8];
  {
    const int c8 = tid % CH;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xsc[e] = xcoef[c8 * 8 + e];
      xsh[e] = xcoef[CP + c8 * 8 + e];
    }
  }
  auto xf1 = [&](float v, float sc, float sh) {
    const float t = fmaf(v, sc, sh);
    return t > 0.f ? t : xslope * t;
  };
  float* zb = zout != nullptr ? zout + (int64_t)row_begin * ldz : nullptr;
  auto xform = [&](TileRegs<CP, NT>& t, int row0) {
#pragma unroll
    for (int u = 0; u < TileRegs<CP, NT>::NV; ++u) {
      float4 a = t.lo[u], b = t.hi[u];
      a.x = xf1(a.x, xsc[0], xsh[0]); a.y = xf1(a.y, xsc[1], xsh[1]); a.z = xf1(a.z, xsc[2], xsh[2]); a.w = xf1(a.w, xsc[3], xsh[3]);
      b.x = xf1(b.x, xsc[4], xsh[4]); b.y = xf1(b.y, xsc[5], xsh[5]); b.z = xf1(b.z, xsc[6], xsh[6]); b.w = xf1(b.w, xsc[7], xsh[7]);
      t.lo[u] = a;
      t.hi[u] = b;
      if (zb != nullptr) {
        const int item = tid + u * NT;
        const int r = row0 + item / CH;
        if (r < nrows) {
          float* d = zb + (int64_t)r * ldz + (item % CH) * 8;
          *reinterpret_cast<float4*>(d) = a;
          *reinterpret_cast<float4*>(d + 4) = b;
        }
      }
    }
  };
  const float sgn = gamma[col] >= 0.f ? 1.f : -1.f;
#pragma unroll
  for (int e = 0; e < HALF; ++e) bq[e] *= sgn;
  const float bj = bias ? sgn * bias[col] : 0.f;
  float pvt;
  {
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < HALF; ++e) d = fmaf(xf1(x[2 * e + h], xcoef[2 * e + h], xcoef[CP + 2 * e + h]), bq[e], d);
    pvt = __fadd_rn(d + __shfl_xor(d, 32), bj);            // sgn * (y2 of the launch's first row)
    if (rb == 0 && h == 0) ws[SUG_PIVOT_OFFSET(CO) + col] = sgn * pvt;
  }

  double s1 = 0.0, s2 = 0.0;                                  // (the epilogue is a sliver of the tile's MFMA time)
  // the walker of channel tid (tid < CO): running extreme of the open segment, its j, the segment's index
  const float wsgn = (tid < CO && gamma[tid < CO ? tid : 0] < 0.f) ? -1.f : 1.f;
  float best = -INFINITY;
  int barg = 0, j = 0;
  int64_t seg = row_begin / k;
  const int ntile = (nrows + TJ - 1) / TJ;
  const float* arow = s_tile + cj * RS + h * HALF;

  TileRegs<CP, NT> tr;
  tile_load<CP, NT>(tr, xb, ldx, nrows, 0);
  for (int t = 0; t < ntile; ++t) {
    xform(tr, t * TJ);
    tile_store<CP, false, NT>(tr, s_tile, nullptr, nrows, t * TJ);
    __syncthreads();
    if (t + 1 < ntile) tile_load<CP, NT>(tr, xb, ldx, nrows, (t + 1) * TJ);     // in flight under the chain
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int g = 0; g < HALF / 4; ++g) {
      const float4 a4 = *reinterpret_cast<const float4*>(arow + 4 * g);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, bq[4 * g + 0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, bq[4 * g + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, bq[4 * g + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, bq[4 * g + 3], acc, 0, 0, 0);
    }
    const int lim = nrows - t * TJ - 4 * h;                  // rows of a partial last tile stay out of the sums
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int rt = (c & 3) + 8 * (c >> 2);
      const float y = __fadd_rn(acc[c], bj);
      if (rt < lim) {
        const double yv = (double)(y - pvt);
        s1 += yv;
        s2 = fma(yv, yv, s2);
      }
      s_y[(rt + 4 * h) * YS + col] = y;
    }
    __syncthreads();
    if (tid < CO) {
      const int nr = (nrows - t * TJ < TJ) ? nrows - t * TJ : TJ;
      for (int r = 0; r < nr; ++r) {
        const float v = s_y[r * YS + tid];
        const bool up = v > best;                            // strict: the lowest j wins a tie
        best = up ? v : best;
        barg = up ? j : barg;
        if (++j == k) {
          zext[seg * CO + tid] = wsgn * best;
          arg[seg * CO + tid] = barg;
          best = -INFINITY;
          barg = 0;
          j = 0;
          ++seg;
        }
      }
    }
  }
  s1 += __shfl_xor(s1, 32);
  s2 += __shfl_xor(s2, 32);
  if (h == 0) {
    ws[(size_t)rb * 2 * CO + col] = sgn * (float)s1;
    ws[(size_t)rb * 2 * CO + CO + col] = (float)s2;
  }
}

__global__ __launch_bounds__(256) void edge_expand_bwd_kernel(const float* __restrict__ dy, const int32_t* __restrict__ rev_off,
                                                              const int32_t* __restrict__ rev_ent, int BN, int N, int k,
                                                              float* __restrict__ dpq, int64_t ld) {
  const int c4 = threadIdx.x & (ECH - 1);
  const int p = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (p >= BN) return;
  const int b = p / N, m = p - b * N;
  const int E = N * k;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f), a = q;
  const float* own = dy + (int64_t)p * k * EC + c4 * 4;
  for (int j = 0; j < k; ++j) {                              // dQ: ascending j
    const float4 v = *reinterpret_cast<const float4*>(own + j * EC);
    q.x += v.x; q.y += v.y; q.z += v.z; q.w += v.w;
  }
  const int32_t* off = rev_off + (int64_t)b * (N + 1);
  const int32_t* ent = rev_ent + (int64_t)b * E;
  int u0 = off[m], u1 = off[m + 1];
  u0 = u0 < 0 ? 0 : u0;
  u1 = u1 > E ? E : u1;
  const float* cloud = dy + (int64_t)b * E * EC + c4 * 4;
  for (int u = u0; u < u1; ++u) {                            // dP: the entries that name this point, ascending e
    int e = ent[u];
    e = e < 0 ? 0 : (e >= E ? E - 1 : e);
    const float4 v = *reinterpret_cast<const float4*>(cloud + (int64_t)e * EC);
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  float* d = dpq + (int64_t)p * ld + c4 * 4;
  *reinterpret_cast<float4*>(d) = a;
  *reinterpret_cast<float4*>(d + EC) = q;
}

}  // namespace

extern "C" int sug_edgemlp_supported(int k, int C1, int Co) {
  return (k >= 2 && k <= 32 && C1 == EC && (Co == 64 || Co == 128)) ? 1 : 0;
}

extern "C" int sug_edge_expand_fwd(const float* pq, int64_t ldpq, const int32_t* idx, int B, int N, int k, int C1,
                                   const float* gamma, const float* beta, int training, float eps, float momentum,
                                   float* running_mean, float* running_var, float* y1, float* coef, float* ws,
                                   void* stream) {
  SUG_REQUIRE(pq && idx && y1 && coef && ws, "sug_edge_expand_fwd: null pointer");
  SUG_REQUIRE(C1 == EC, "sug_edge_expand_fwd: C1=%d (64 channels)", C1);
  SUG_REQUIRE(B > 0 && N > 0 && k >= 1 && k <= 32 && (int64_t)B * N * k < (1ll << 31), "sug_edge_expand_fwd: bad shape");
  SUG_REQUIRE(ldpq >= 2 * EC && ldpq % 4 == 0 && ((uintptr_t)pq % 16) == 0 && ((uintptr_t)y1 % 16) == 0,
              "sug_edge_expand_fwd: pq / y1 must be 16-byte aligned, ldpq a multiple of 4 and >= 2*C1");
  SUG_REQUIRE(!training || (gamma && beta), "sug_edge_expand_fwd: null BatchNorm parameters");
  const int E = B * N * k;
  int per_wg = sug_divup(E, SUG_STATS_ROWS);
  if (per_wg < 256) per_wg = 256;
  per_wg = (per_wg + 15) / 16 * 16;
  const int nwg = sug_divup(E, per_wg);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(edge_expand_kernel, dim3(nwg), dim3(256), 0, st, pq, ldpq, idx, N, k, E, per_wg, y1, ws);
  SUG_LAUNCH_CHECK("sug_edge_expand_fwd");
  if (training)
    return sug_stats_finalize(ws, nwg, EC, gamma, beta, (double)E, eps, momentum, running_mean, running_var, coef, st,
                              ws + SUG_PIVOT_OFFSET(EC));
  return SUG_OK;
}

extern "C" int sug_edgemlp_max_layer_fwd_xf(const float* y, int64_t ldy, int64_t rows, int K, const float* xcoef, float xslope,
                                            float* zout, int64_t ldz, const float* w, const float* bias, const float* gamma,
                                            const float* beta, int Co, int seg, int groups, int training, float eps,
                                            float momentum, float slope, float* running_mean, float* running_var,
                                            float* zext, int32_t* arg, float* coef, float* out, int64_t ldo, float* ws,
                                            void* stream) {
  SUG_REQUIRE(y && xcoef && w && gamma && beta && zext && arg && coef && out && ws, "sug_edgemlp_max_layer_fwd_xf: null pointer");
  SUG_REQUIRE(sug_edgemlp_supported(seg, K, Co), "sug_edgemlp_max_layer_fwd_xf: seg=%d K=%d Co=%d (2 <= seg <= 32, K = 64, Co 64 or 128)",
              seg, K, Co);
  SUG_REQUIRE(groups == 1, "sug_edgemlp_max_layer_fwd_xf: %d domain groups (one)", groups);
  SUG_REQUIRE(rows > 0 && rows % seg == 0 && rows < (1ll << 31), "sug_edgemlp_max_layer_fwd_xf: %lld rows are not whole segments of %d",
              (long long)rows, seg);
  SUG_REQUIRE(ldy >= K && ldy % 4 == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)w % 16) == 0 && ldo >= Co,
              "sug_edgemlp_max_layer_fwd_xf: y / w must be 16-byte aligned with row strides in multiples of 4");
  SUG_REQUIRE(!zout || (ldz >= K && ldz % 4 == 0 && ((uintptr_t)zout % 16) == 0), "sug_edgemlp_max_layer_fwd_xf: bad zout / ldz");
  // whole segments per workgroup; as many workgroups as the statistics workspace has rows for, 8 tiles or more each
  int64_t rpw = (rows + SUG_STATS_ROWS - 1) / SUG_STATS_ROWS;
  if (rpw < 256) rpw = 256;
  rpw = (rpw + seg - 1) / seg * seg;
  const int nrb = sug_divup(rows, rpw);
  hipStream_t st = (hipStream_t)stream;
  if (Co == 128)
    hipLaunchKernelGGL((edgemlp_max_kernel<128>), dim3(nrb), dim3(256), 0, st, y, ldy, (int)rows, w, bias, gamma, seg, (int)rpw,
                       zext, arg, ws, xcoef, xslope, zout, ldz);
  else
    hipLaunchKernelGGL((edgemlp_max_kernel<64>), dim3(nrb), dim3(128), 0, st, y, ldy, (int)rows, w, bias, gamma, seg, (int)rpw,
                       zext, arg, ws, xcoef, xslope, zout, ldz);
  SUG_LAUNCH_CHECK("sug_edgemlp_max_layer_fwd_xf");
  if (training) {
    int rc = sug_stats_finalize(ws, nrb, Co, gamma, beta, (double)rows, eps, momentum, running_mean, running_var, coef, st,
                                ws + SUG_PIVOT_OFFSET(Co));
    if (rc != SUG_OK) return rc;
  }
  return sug_affine_act(zext, Co, coef, rows / seg, Co, slope, out, ldo, stream);
}

extern "C" int sug_edge_expand_bwd(const float* dy1, const int32_t* rev_off, const int32_t* rev_ent, int B, int N, int k,
                                   int C1, float* dpq, int64_t lddpq, void* stream) {
  SUG_REQUIRE(dy1 && rev_off && rev_ent && dpq, "sug_edge_expand_bwd: null pointer");
  SUG_REQUIRE(C1 == EC, "sug_edge_expand_bwd: C1=%d (64 channels)", C1);
  SUG_REQUIRE(B > 0 && N > 0 && k >= 1 && k <= 32 && (int64_t)B * N * k < (1ll << 31), "sug_edge_expand_bwd: bad shape");
  SUG_REQUIRE(lddpq >= 2 * EC && lddpq % 4 == 0 && ((uintptr_t)dpq % 16) == 0 && ((uintptr_t)dy1 % 16) == 0,
              "sug_edge_expand_bwd: dy1 / dpq must be 16-byte aligned, lddpq a multiple of 4 and >= 2*C1");
  const int BN = B * N;
  hipLaunchKernelGGL(edge_expand_bwd_kernel, dim3(sug_divup(BN, 16)), dim3(256), 0, (hipStream_t)stream, dy1, rev_off, rev_ent,
                     BN, N, k, dpq, lddpq);
  SUG_LAUNCH_CHECK("sug_edge_expand_bwd");
  return SUG_OK;
}
