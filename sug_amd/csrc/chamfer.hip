// ChamferDistance as an op of its own: per-point squared distances, nearest-neighbour indices and the gradients to both
// clouds (the contract of the third-party op that the reference's model/mmd.py imports; cd_distance, model/mmd.py:169-175).
// sug_chamfer (mmd.hip) keeps serving the detached per-pair scalar of the SDA geometric weights.
//
// Forward: one launch, both directions (the first nbn workgroups of a cloud pair answer a -> b, the others b -> a).  Four
// lanes per query point, each over a quarter of the candidates in two chains, the candidates through LDS in tiles of
// CH_TILE points.  Every chain sees its candidates in ascending j and replaces its best on a strictly smaller distance
// only, so it holds the lowest j of its own minimum; chains and lanes are then merged by (distance, index) -- the lowest
// index of the minimum, however the candidates were split.  d = sq3(x - cx, y - cy, z - cz): reproducible in fp32 on a CPU.
//
// Backward: one launch, both sides.  Four lanes per TARGET point scan the other cloud's index array from LDS (b128
// broadcast reads, four indices per read) and add 2 g_j (t_i - s_j) for every j that names the point: lane c takes the
// index quadruples q = c, c + 4, ... in ascending order (lane 0 starts from the point's own term 2 g_i (t_i - s_idx[i])),
// and the four partial sums are added as ((p0 + p1) + p2) + p3.  No atomics, no list build; the order is a function of
// the point's and the contributors' indices inside the cloud alone.  O(N M) like the forward.
// Algorithmic bytes: forward 12 B (N + M) in, 8 B (N + M) out; FLOPs 2 * 8 B N M.
#include <limits.h>
#include "common.h"

namespace {

constexpr int CH_TILE = 1024;   // candidate points per LDS tile: 16 KB forward, 20 KB backward (a multiple of 16)

// dist[b][i] = min_j d(q_i, c_j), idx[b][i] = the lowest j attaining it; blockIdx.x < nbn: q = a (N), c = b (M); else swapped
__global__ __launch_bounds__(256) void chamfer_nn_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int M,
                                                         int nbn, float* __restrict__ dist1, float* __restrict__ dist2,
                                                         int32_t* __restrict__ idx1, int32_t* __restrict__ idx2) {
  __shared__ __attribute__((aligned(16))) float s_p[CH_TILE * 4];   // (x, y, z, pad): one b128 broadcast read per candidate
  const bool rev = (int)blockIdx.x >= nbn;
  const int blk = rev ? blockIdx.x - nbn : blockIdx.x;
  const int cloud = blockIdx.y;
  const int nq = rev ? M : N, nc = rev ? N : M;
  const float* qp = (rev ? b : a) + (int64_t)cloud * nq * 3;
  const float* cp = (rev ? a : b) + (int64_t)cloud * nc * 3;
  const int t = blk * 256 + threadIdx.x;
  const int i = t >> 2, cl = t & 3;
  float x = 0.f, y = 0.f, zc = 0.f;
  if (i < nq) { x = qp[3 * i]; y = qp[3 * i + 1]; zc = qp[3 * i + 2]; }
  float b0 = INFINITY, b1 = INFINITY;
  int k0 = INT_MAX, k1 = INT_MAX;              // "no candidate yet": loses every tie against a real index
  for (int c0 = 0; c0 < nc; c0 += CH_TILE) {
    const int cnt = (nc - c0) < CH_TILE ? (nc - c0) : CH_TILE;
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * 3; e += 256) s_p[(e / 3) * 4 + e % 3] = cp[(int64_t)c0 * 3 + e];
    __syncthreads();
    if (i < nq) {
      int j = cl;
      for (; j + 4 < cnt; j += 8) {
        const float4 c0v = *reinterpret_cast<const float4*>(s_p + 4 * j), c1v = *reinterpret_cast<const float4*>(s_p + 4 * j + 16);
        const float d0 = sq3(x - c0v.x, y - c0v.y, zc - c0v.z), d1 = sq3(x - c1v.x, y - c1v.y, zc - c1v.z);
        if (d0 < b0) { b0 = d0; k0 = c0 + j; }
        if (d1 < b1) { b1 = d1; k1 = c0 + j + 4; }
      }
      for (; j < cnt; j += 4) {
        const float4 c = *reinterpret_cast<const float4*>(s_p + 4 * j);
        const float d = sq3(x - c.x, y - c.y, zc - c.z);
        if (d < b0) { b0 = d; k0 = c0 + j; }
      }
    }
  }
  // the two chains, then the point's four lanes: the smaller distance, on equal distances the smaller index
  float best = b0;
  int k = k0;
  if (b1 < best || (b1 == best && k1 < k)) { best = b1; k = k1; }
#pragma unroll
  for (int o = 1; o <= 2; o <<= 1) {
    const float ob = __shfl_xor(best, o);
    const int ok = __shfl_xor(k, o);
    if (ob < best || (ob == best && ok < k)) { best = ob; k = ok; }
  }
  if (k == INT_MAX) k = 0;                     // every distance overflowed to +inf: candidate 0 is the lowest of the minimum
  if (cl == 0 && i < nq) {
    (rev ? dist2 : dist1)[(int64_t)cloud * nq + i] = best;
    (rev ? idx2 : idx1)[(int64_t)cloud * nq + i] = k;
  }
}

// gt[b][i] = 2 gT_i (t_i - s_{idxT[i]}) + sum over j ascending with idxS[j] == i of 2 gS_j (t_i - s_j)
// blockIdx.x < nba: target = a (N), source = b (M), gT = g1, idxT = idx1, gS = g2, idxS = idx2, out = ga; else swapped.
// An index outside the other cloud (never produced by the forward) is not followed: that point's gradient is NaN.
__global__ __launch_bounds__(256) void chamfer_nn_bwd_kernel(const float* __restrict__ g1, const float* __restrict__ g2,
                                                             const float* __restrict__ a, const float* __restrict__ b,
                                                             const int32_t* __restrict__ idx1, const int32_t* __restrict__ idx2,
                                                             int N, int M, int nba, float* __restrict__ ga,
                                                             float* __restrict__ gb) {
  __shared__ __attribute__((aligned(16))) float s_p[CH_TILE * 4];   // source point and its doubled upstream gradient: (x, y, z, 2 g)
  __shared__ __attribute__((aligned(16))) int s_i[CH_TILE];         // the source points' indices into the target cloud; -1 behind the end
  const bool rev = (int)blockIdx.x >= nba;
  const int blk = rev ? blockIdx.x - nba : blockIdx.x;
  const int cloud = blockIdx.y;
  const int nt = rev ? M : N, ns = rev ? N : M;
  const float* tp = (rev ? b : a) + (int64_t)cloud * nt * 3;
  const float* sp = (rev ? a : b) + (int64_t)cloud * ns * 3;
  const float* gT = (rev ? g2 : g1) + (int64_t)cloud * nt;
  const float* gS = (rev ? g1 : g2) + (int64_t)cloud * ns;
  const int32_t* iT = (rev ? idx2 : idx1) + (int64_t)cloud * nt;
  const int32_t* iS = (rev ? idx1 : idx2) + (int64_t)cloud * ns;
  float* out = (rev ? gb : ga) + (int64_t)cloud * nt * 3;
  const int t = blk * 256 + threadIdx.x;
  const int i = t >> 2, cl = t & 3;
  const bool live = i < nt;
  const int want = live ? i : -2;              // a lane without a point matches nothing (-1 pads the index tile)
  float x = 0.f, y = 0.f, zc = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
  if (live) {
    x = tp[3 * i]; y = tp[3 * i + 1]; zc = tp[3 * i + 2];
    if (cl == 0) {                             // the point's own term
      const int k = iT[i];
      if ((unsigned)k < (unsigned)ns) {
        const float w = 2.0f * gT[i];
        ax = w * (x - sp[3 * k]); ay = w * (y - sp[3 * k + 1]); az = w * (zc - sp[3 * k + 2]);
      } else {
        ax = ay = az = NAN;
      }
    }
  }
  for (int c0 = 0; c0 < ns; c0 += CH_TILE) {
    const int cnt = (ns - c0) < CH_TILE ? (ns - c0) : CH_TILE;
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * 3; e += 256) s_p[(e / 3) * 4 + e % 3] = sp[(int64_t)c0 * 3 + e];
    for (int e = threadIdx.x; e < CH_TILE; e += 256) {
      if (e < cnt) { s_p[4 * e + 3] = 2.0f * gS[c0 + e]; s_i[e] = iS[c0 + e]; }
      else s_i[e] = -1;
    }
    __syncthreads();
    const int nq4 = (cnt + 3) >> 2;
    for (int q = cl; q < nq4; q += 4) {
      const int4 v = *reinterpret_cast<const int4*>(s_i + 4 * q);
      const int vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (vv[u] == want) {
          const float4 c = *reinterpret_cast<const float4*>(s_p + 4 * (4 * q + u));
          ax += c.w * (x - c.x); ay += c.w * (y - c.y); az += c.w * (zc - c.z);
        }
      }
    }
  }
  // ((p0 + p1) + p2) + p3 in lane 0 of the point's four lanes
  const float x1 = __shfl_xor(ax, 1), y1 = __shfl_xor(ay, 1), z1 = __shfl_xor(az, 1);     // lane 0 <- 1, lane 2 <- 3
  const float x2 = __shfl_down(ax, 2), y2 = __shfl_down(ay, 2), z2 = __shfl_down(az, 2);   // lane 0 <- 2
  const float x3 = __shfl_down(ax, 3), y3 = __shfl_down(ay, 3), z3 = __shfl_down(az, 3);   // lane 0 <- 3
  if (cl == 0 && live) {
    out[3 * i] = ((ax + x1) + x2) + x3;
    out[3 * i + 1] = ((ay + y1) + y2) + y3;
    out[3 * i + 2] = ((az + z1) + z2) + z3;
  }
}

}  // namespace

extern "C" int sug_chamfer_nn(const float* a, const float* b, int B, int N, int M, float* dist1, float* dist2, int32_t* idx1,
                              int32_t* idx2, void* stream) {
  SUG_REQUIRE(a && b && dist1 && dist2 && idx1 && idx2, "sug_chamfer_nn: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && M > 0 && N <= SUG_CHAMFER_MAX_POINTS && M <= SUG_CHAMFER_MAX_POINTS && B <= 65535,
              "sug_chamfer_nn: bad shape B=%d N=%d M=%d (1..65535 pairs of 1..%d points)", B, N, M, SUG_CHAMFER_MAX_POINTS);
  const int nbn = sug_divup(4 * N, 256), nbm = sug_divup(4 * M, 256);
  hipLaunchKernelGGL(chamfer_nn_kernel, dim3(nbn + nbm, B), dim3(256), 0, (hipStream_t)stream, a, b, N, M, nbn, dist1, dist2,
                     idx1, idx2);
  SUG_LAUNCH_CHECK("sug_chamfer_nn");
  return SUG_OK;
}

extern "C" int sug_chamfer_nn_bwd(const float* g1, const float* g2, const float* a, const float* b, const int32_t* idx1,
                                  const int32_t* idx2, int B, int N, int M, float* ga, float* gb, void* stream) {
  SUG_REQUIRE(g1 && g2 && a && b && idx1 && idx2, "sug_chamfer_nn_bwd: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && M > 0 && N <= SUG_CHAMFER_MAX_POINTS && M <= SUG_CHAMFER_MAX_POINTS && B <= 65535,
              "sug_chamfer_nn_bwd: bad shape B=%d N=%d M=%d (1..65535 pairs of 1..%d points)", B, N, M, SUG_CHAMFER_MAX_POINTS);
  if (!ga && !gb) return SUG_OK;                                   // neither cloud takes a gradient
  const int nba = ga ? sug_divup(4 * N, 256) : 0, nbb = gb ? sug_divup(4 * M, 256) : 0;
  hipLaunchKernelGGL(chamfer_nn_bwd_kernel, dim3(nba + nbb, B), dim3(256), 0, (hipStream_t)stream, g1, g2, a, b, idx1, idx2, N, M,
                     nba, ga, gb);
  SUG_LAUNCH_CHECK("sug_chamfer_nn_bwd");
  return SUG_OK;
}
