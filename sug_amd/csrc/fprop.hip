// PointNet++ multi-scale grouping and feature propagation: the ball query for several radii in one pass over the
// distances, the 3-NN selection on the direct-form distance, and the inverse-distance interpolation of
// PointNetFeaturePropagation.forward (model/pointnet2_utils.py:84-104, :301-308; model/PTran_utils.py:36, :292-299).
#include "common.h"

namespace {

// ---------------------------------------------------------------------------
// Ball query for R <= 4 radii: one wave per query, 64 candidates per step.  The distance of a (query, point) pair is
// computed once, in sug_ball_query's operation order, and tested against every radius whose list is not yet full; a
// list's ballot + prefix popcount gives the ascending-index order, exactly as ball_query_kernel does for one radius.
// The scan ends when every list is full.
// ---------------------------------------------------------------------------
struct BallMulti {
  float r2[4];
  int ns[4];
  int32_t* out[4];
};

template <bool LDS>
__global__ __launch_bounds__(256) void ball_query_multi_kernel(const float* __restrict__ xyz,
                                                               const float* __restrict__ qry, int N, int S, int R,
                                                               BallMulti a, int qpw) {
  extern __shared__ __attribute__((aligned(16))) float s_pts[];             // [N*3] when LDS
  const int b = blockIdx.y;
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const float* pb = xyz + (int64_t)b * N * 3;
  if (LDS) {
    for (int i = threadIdx.x; i < 3 * N; i += 256) s_pts[i] = pb[i];
    __syncthreads();
  }
  for (int qi = 0; qi < qpw; ++qi) {
    const int s = (blockIdx.x * (256 / WAVE) + wv) * qpw + qi;
    if (s >= S) break;  // whole wave exits together
    const float* q = qry + ((int64_t)b * S + s) * 3;
    const float qx = q[0], qy = q[1], qz = q[2];
    const float nq = sq3(qx, qy, qz);
    int cnt[4] = {0, 0, 0, 0}, first[4] = {N, N, N, N};
    for (int j0 = 0; j0 < N; j0 += WAVE) {
      bool open = false;
#pragma unroll
      for (int r = 0; r < 4; ++r) open = open || (r < R && cnt[r] < a.ns[r]);
      if (!open) break;
      const int j = j0 + lane;
      float d = INFINITY;                                     // !(inf > r2) is false: lanes past N never hit
      if (j < N) {
        const float x = LDS ? s_pts[j * 3 + 0] : pb[j * 3 + 0], y = LDS ? s_pts[j * 3 + 1] : pb[j * 3 + 1],
                    z = LDS ? s_pts[j * 3 + 2] : pb[j * 3 + 2];
        d = sqdist_expanded(dot3(qx, qy, qz, x, y, z), nq, sq3(x, y, z));
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r < R && cnt[r] < a.ns[r]) {                      // uniform over the wave
          const bool hit = j < N && !(d > a.r2[r]);
          const unsigned long long m = __ballot(hit);
          if (m) {
            if (cnt[r] == 0) first[r] = j0 + __builtin_ctzll(m);
            const int pos = cnt[r] + __builtin_popcountll(m & ((1ull << lane) - 1ull));
            if (hit && pos < a.ns[r]) a.out[r][((int64_t)b * S + s) * a.ns[r] + pos] = j;
            cnt[r] += __builtin_popcountll(m);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r < R) {
        const int c = cnt[r] > a.ns[r] ? a.ns[r] : cnt[r];
        for (int p = c + lane; p < a.ns[r]; p += WAVE) a.out[r][((int64_t)b * S + s) * a.ns[r] + p] = first[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// 3 nearest of S candidates (LDS-resident) for every point of the dense cloud on the direct-form distance
// ((q-c)_x^2 + (q-c)_y^2) + (q-c)_z^2 (model/PTran_utils.py:36); ascending d, ties -> lowest index.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void three_nn_direct_kernel(const float* __restrict__ qry,
                                                              const float* __restrict__ cand, int N, int S,
                                                              int32_t* __restrict__ idx3, float* __restrict__ dist3) {
  extern __shared__ float s_c[];  // S*3
  const int b = blockIdx.y;
  const float* cb = cand + (int64_t)b * S * 3;
  for (int j = threadIdx.x; j < S * 3; j += 256) s_c[j] = cb[j];
  __syncthreads();
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float* q = qry + ((int64_t)b * N + n) * 3;
  const float qx = q[0], qy = q[1], qz = q[2];
  float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
  int i0 = 0, i1 = 0, i2 = 0;
  for (int j = 0; j < S; ++j) {
    const float d = sq3(__fsub_rn(qx, s_c[j * 3 + 0]), __fsub_rn(qy, s_c[j * 3 + 1]), __fsub_rn(qz, s_c[j * 3 + 2]));
    if (d < d2) {
      if (d < d1) {
        d2 = d1; i2 = i1;
        if (d < d0) {
          d1 = d0; i1 = i0;
          d0 = d; i0 = j;
        } else {
          d1 = d; i1 = j;
        }
      } else {
        d2 = d; i2 = j;
      }
    }
  }
  const int64_t o = ((int64_t)b * N + n) * 3;
  idx3[o + 0] = i0; idx3[o + 1] = i1; idx3[o + 2] = i2;
  dist3[o + 0] = d0; dist3[o + 1] = d1; dist3[o + 2] = d2;
}

// ---------------------------------------------------------------------------
// Feature propagation's interpolation, forward: 16 lanes per dense point, V channels per lane and step.
//   r_t = 1 / (d_t + 1e-8)   (no clamp: a negative rounding residue of the expanded form goes through as it does in
//   the reference),  w_t = r_t / ((r_0 + r_1) + r_2),  out[n, :] = (w_0 src[i_0] + w_1 src[i_1]) + w_2 src[i_2].
// The three weights are kept ([B,N,3]) for the backward.
// ---------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void fp_interp_fwd_kernel(const float* __restrict__ src, int64_t lds,
                                                            const int32_t* __restrict__ idx3,
                                                            const float* __restrict__ d3, int N, int S, int D,
                                                            int64_t BN, float* __restrict__ out, int64_t ldo,
                                                            float* __restrict__ w3) {
  const int64_t p = (int64_t)blockIdx.x * 16 + threadIdx.x / 16;
  if (p >= BN) return;
  const int lane = threadIdx.x & 15;
  const int64_t b = p / N;
  const float r0 = 1.0f / (d3[p * 3 + 0] + 1e-8f), r1 = 1.0f / (d3[p * 3 + 1] + 1e-8f),
              r2 = 1.0f / (d3[p * 3 + 2] + 1e-8f);
  const float R = (r0 + r1) + r2;
  const float w0 = r0 / R, w1 = r1 / R, w2 = r2 / R;
  if (lane < 3) w3[p * 3 + lane] = lane == 0 ? w0 : (lane == 1 ? w1 : w2);
  int j0 = idx3[p * 3 + 0], j1 = idx3[p * 3 + 1], j2 = idx3[p * 3 + 2];
  j0 = min(max(j0, 0), S - 1); j1 = min(max(j1, 0), S - 1); j2 = min(max(j2, 0), S - 1);      // never read outside src
  const float* n0 = src + (b * S + j0) * lds;
  const float* n1 = src + (b * S + j1) * lds;
  const float* n2 = src + (b * S + j2) * lds;
  float* o = out + p * ldo;
  for (int c = lane * V; c < D; c += 16 * V) {
    if (V == 4) {
      const float4 a = *reinterpret_cast<const float4*>(n0 + c), bq = *reinterpret_cast<const float4*>(n1 + c),
                   cq = *reinterpret_cast<const float4*>(n2 + c);
      float4 v;      // torch.sum(sel * w, dim=2): ((a*w0 + b*w1) + c*w2)
      v.x = (a.x * w0 + bq.x * w1) + cq.x * w2; v.y = (a.y * w0 + bq.y * w1) + cq.y * w2;
      v.z = (a.z * w0 + bq.z * w1) + cq.z * w2; v.w = (a.w * w0 + bq.w * w1) + cq.w * w2;
      *reinterpret_cast<float4*>(o + c) = v;
    } else {
      o[c] = (n0[c] * w0 + n1[c] * w1) + n2[c] * w2;
    }
  }
}

// Backward by destination row: dsrc[b, s, :] = sum over the entries e = 3n + t of s's reverse list (sug_reverse_lists, sorted:
// ascending e) of w3[b, e] * g[b, n, :].  Every row of dsrc is written once (zero for an empty list); no atomics, one order.
template <int V>
__global__ __launch_bounds__(256) void fp_interp_bwd_kernel(const float* __restrict__ g, int64_t ldg,
                                                            const float* __restrict__ w3,
                                                            const int32_t* __restrict__ rev_off,
                                                            const int32_t* __restrict__ rev_ent, int N, int S, int D,
                                                            int64_t total, float* __restrict__ dsrc, int64_t ldd) {
  const int DV = D / V;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int c = (int)(t % DV) * V;
    const int64_t row = t / DV;        // b*S + s
    const int64_t b = row / S;
    const int s = (int)(row - b * S);
    const int32_t* off = rev_off + b * (S + 1) + s;
    const int e0 = off[0], e1 = off[1];
    const int32_t* ent = rev_ent + b * 3 * N;
    const float* wb = w3 + b * 3 * N;
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
    for (int i = e0; i < e1; ++i) {
      const int e = ent[i];
      const float w = wb[e];
      const float* gr = g + (b * N + e / 3) * ldg + c;
      if (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(gr);
        acc[0] += w * q.x; acc[1] += w * q.y; acc[2] += w * q.z; acc[3] += w * q.w;
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += w * gr[v];
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) dsrc[row * ldd + c + v] = acc[v];
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int sug_ball_query_multi(const float* xyz, const float* query, int B, int N, int S, int R, const float* r2,
                                    const int32_t* nsample, int32_t* const* out, void* stream) {
  SUG_REQUIRE(xyz && query && r2 && nsample && out, "sug_ball_query_multi: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && S > 0, "sug_ball_query_multi: bad shape");
  SUG_REQUIRE(R >= 1 && R <= 4, "sug_ball_query_multi: need 1 <= R <= 4 radii, got %d", R);
  SUG_REQUIRE(B <= 65535, "sug_ball_query_multi: B too large");
  BallMulti a;
  for (int r = 0; r < 4; ++r) {
    const int q = r < R ? r : 0;
    SUG_REQUIRE(out[q] && nsample[q] > 0, "sug_ball_query_multi: list %d: null pointer or nsample <= 0", q);
    a.r2[r] = r2[q];
    a.ns[r] = nsample[q];
    a.out[r] = out[q];
  }
  hipStream_t st = (hipStream_t)stream;
  if (N <= 4096) {
    int qpw = 1;                  // as sug_ball_query: plenty of workgroups first, then up to 4 queries per staging
    while (qpw < 4 && (int64_t)B * sug_divup(S, 4 * 2 * qpw) >= 2048) qpw *= 2;
    dim3 grid(sug_divup(S, (256 / WAVE) * qpw), B);
    hipLaunchKernelGGL((ball_query_multi_kernel<true>), grid, dim3(256), (size_t)3 * N * sizeof(float), st, xyz, query, N, S,
                       R, a, qpw);
  } else {
    dim3 grid(sug_divup(S, 256 / WAVE), B);
    hipLaunchKernelGGL((ball_query_multi_kernel<false>), grid, dim3(256), 0, st, xyz, query, N, S, R, a, 1);
  }
  SUG_LAUNCH_CHECK("sug_ball_query_multi");
  return SUG_OK;
}

extern "C" int sug_three_nn_direct(const float* query, const float* cand, int B, int N, int S, int32_t* idx3,
                                   float* dist3, void* stream) {
  SUG_REQUIRE(query && cand && idx3 && dist3, "sug_three_nn_direct: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && S >= 3, "sug_three_nn_direct: bad shape (S=%d must be >= 3)", S);
  SUG_REQUIRE(S <= 2048, "sug_three_nn_direct: S=%d > 2048", S);
  SUG_REQUIRE(B <= 65535, "sug_three_nn_direct: B too large");
  dim3 grid(sug_divup(N, 256), B);
  hipLaunchKernelGGL(three_nn_direct_kernel, grid, dim3(256), (size_t)S * 3 * sizeof(float), (hipStream_t)stream, query,
                     cand, N, S, idx3, dist3);
  SUG_LAUNCH_CHECK("sug_three_nn_direct");
  return SUG_OK;
}

extern "C" int sug_fp_interp_fwd(const float* src, int64_t lds, const int32_t* idx3, const float* d3, int B, int N, int S,
                                 int D, float* out, int64_t ldo, float* w3, void* stream) {
  SUG_REQUIRE(src && idx3 && d3 && out && w3, "sug_fp_interp_fwd: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && S >= 3 && D > 0 && lds >= D && ldo >= D, "sug_fp_interp_fwd: bad shape B=%d N=%d S=%d D=%d", B, N, S,
              D);
  const int64_t BN = (int64_t)B * N;
  const bool v4 = D % 4 == 0 && lds % 4 == 0 && ldo % 4 == 0 && aligned16(src) && aligned16(out);
  if (v4)
    hipLaunchKernelGGL((fp_interp_fwd_kernel<4>), dim3(sug_divup(BN, 16)), dim3(256), 0, (hipStream_t)stream, src, lds, idx3, d3,
                       N, S, D, BN, out, ldo, w3);
  else
    hipLaunchKernelGGL((fp_interp_fwd_kernel<1>), dim3(sug_divup(BN, 16)), dim3(256), 0, (hipStream_t)stream, src, lds, idx3, d3,
                       N, S, D, BN, out, ldo, w3);
  SUG_LAUNCH_CHECK("sug_fp_interp_fwd");
  return SUG_OK;
}

extern "C" int sug_fp_interp_bwd(const float* g, int64_t ldg, const int32_t* idx3, const float* w3, int B, int N, int S, int D,
                                 int32_t* rev_off, int32_t* rev_ent, float* dsrc, int64_t ldd, void* stream) {
  SUG_REQUIRE(g && idx3 && w3 && dsrc && rev_off && rev_ent, "sug_fp_interp_bwd: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && S >= 3 && D > 0 && ldg >= D && ldd >= D, "sug_fp_interp_bwd: bad shape B=%d N=%d S=%d D=%d", B, N, S,
              D);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = sug_reverse_lists(idx3, B, 3 * N, S, 1, rev_off, rev_ent, st)) return rc;
  const bool v4 = D % 4 == 0 && ldg % 4 == 0 && ldd % 4 == 0 && aligned16(g) && aligned16(dsrc);
  const int64_t total = (int64_t)B * S * (v4 ? D / 4 : D);
  const int grid = (int)((total + 255) / 256 < 65536 * 16 ? (total + 255) / 256 : 65536 * 16);
  if (v4)
    hipLaunchKernelGGL((fp_interp_bwd_kernel<4>), dim3(grid), dim3(256), 0, st, g, ldg, w3, rev_off, rev_ent, N, S, D, total, dsrc,
                       ldd);
  else
    hipLaunchKernelGGL((fp_interp_bwd_kernel<1>), dim3(grid), dim3(256), 0, st, g, ldg, w3, rev_off, rev_ent, N, S, D, total, dsrc,
                       ldd);
  SUG_LAUNCH_CHECK("sug_fp_interp_bwd");
  return SUG_OK;
}
