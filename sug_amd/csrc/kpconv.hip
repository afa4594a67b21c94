// KPConv backbone (model/KPConv_model.py, model/KPConv_blocks.py): the preprocessing pyramid (grid subsampling, radius
// neighbours and their reverse lists) and the rigid / linear-influence / sum-aggregation kernel point convolution with
// the per-cloud instance norm, max pooling and global average around it.
//
// ROW LAYOUT.  Clouds are PACKED: level l owns a buffer of C_l rows, of which rows [0, off[B]) are
// valid -- the clouds back to back at the device offsets off[B+1] -- and rows [off[B], C_l) are dead.  Neighbour tables
// [C_q, H] hold global support indices; a missing slot holds the shadow index, the row count C_s of the support buffer (as
// the reference pads them).  Every reduction has one fixed order, no float atomics: the backward scatters go through the
// sorted reverse lists of sug_radius_reverse, so the backbone is reproducible bit for bit from run to run.  Invariants:
//   1. every dead row of every level tensor is exactly zero: coordinates, activations, and the gradients of both;
//   2. every slot of a dead query's table row is the shadow index;
//   3. the reverse list of a dead support is empty (lo == hi);
//   4. a kernel of this file never reads a dead row of an input, and writes zeros to the dead rows of each output,
//      forward and backward.  The library GEMMs run on all C_l rows; their weight gradients stay right because the
//      dead rows of both operands are zero (a NaN in a dead row would poison dW);
//   5. no buffer, no grid and no host branch depends on a value in device memory, and nothing is copied to the host.
// The kernels take the valid count from device memory (off[B], by pointer) and the row count by value.  EXACT SIZES are
// the case C_l == off[B]: no dead rows, so 1. to 4. hold trivially and the dead-row branches below run over nothing (the
// exact-size pyramid gives up 5.: it reads the level totals once to slice its buffers).  With level caps C_0 = B*N and
// C_l = min(C_{l-1}, 64*ceil(B*caps[l-1]/64)) are constants of the launch sequence.  sug_kpconv_bwd,
// sug_seg_max_pool_fwd and sug_seg_max_pool_bwd hold under 2. and 3. as they are: a dead support's empty list sums to 0,
// a dead query's all-shadow row reads only the zero shadow.
// Overflow (a level total above C_l): the pack step clamps the offsets to C_l and drops the rows past it -- the tail of
// the last clouds, a cloud may become empty (an empty cloud normalises nothing; its mean row and pooled feature are 0).
// The unclamped total is folded into a small device record (sug_grid_subsample).
#include "common.h"

namespace {

constexpr int SUB_BLOCK = 1024;        // one workgroup per cloud in the subsample / reverse-list kernels
constexpr int KP_MAX_K = 16;           // kernel points
constexpr int KP_MAX_H = 64;           // neighbour slots
constexpr int KP_QB = 8;               // queries per workgroup of sug_kpconv_fwd
constexpr float LEAKY = 0.1f;

__device__ __forceinline__ int cloud_of(const int32_t* off, int B, int i) {
  int b = 0;
  while (b + 1 < B && off[b + 1] <= i) ++b;
  return b;
}

// Exclusive scan of n ints in LDS v[] in place by a SUB_BLOCK-thread workgroup (part: SUB_BLOCK ints of LDS); returns
// the total.  Each thread owns a contiguous chunk, so the result does not depend on timing.
__device__ int block_exclusive_scan(int* v, int n, int* part) {
  const int t = threadIdx.x;
  const int per = (n + SUB_BLOCK - 1) / SUB_BLOCK;
  const int lo = min(n, t * per), hi = min(n, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += v[i];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < SUB_BLOCK; o <<= 1) {
    int a = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += a;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int i = lo; i < hi; ++i) {
    int c = v[i];
    v[i] = run;
    run += c;
  }
  int total = part[SUB_BLOCK - 1];
  __syncthreads();
  return total;
}

// One cloud per workgroup: voxel key floor(p / dl) per axis (true fp32 division), voxels in order of their first point,
// each voxel's point = fp32 sum of its points in point order divided once by the count.
__global__ void __launch_bounds__(SUB_BLOCK) grid_subsample_kernel(const float* __restrict__ pts,
                                                                   const int32_t* __restrict__ off, float dl, int cap,
                                                                   float* __restrict__ out_pad, int32_t* __restrict__ cnt) {
  extern __shared__ int lds[];
  const int b = blockIdx.x;
  const int p0 = off[b], n = off[b + 1] - p0;
  int* kx = lds;
  int* ky = kx + cap;
  int* kz = ky + cap;
  int* first = kz + cap;
  int* ord = first + cap;
  int* part = ord + cap;
  if (n > cap) {      // the host sized cap from the previous level's total; a longer cloud cannot occur
    if (threadIdx.x == 0) cnt[b] = 0;
    return;
  }
  for (int i = threadIdx.x; i < n; i += SUB_BLOCK) {
    const float* p = pts + (size_t)(p0 + i) * 3;
    kx[i] = (int)floorf(__fdiv_rn(p[0], dl));
    ky[i] = (int)floorf(__fdiv_rn(p[1], dl));
    kz[i] = (int)floorf(__fdiv_rn(p[2], dl));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += SUB_BLOCK) {
    const int a = kx[i], c = ky[i], d = kz[i];
    int f = i;
    for (int j = 0; j < i; ++j)
      if (kx[j] == a && ky[j] == c && kz[j] == d) {
        f = j;
        break;
      }
    first[i] = f;
    ord[i] = (f == i) ? 1 : 0;
  }
  __syncthreads();
  const int nv = block_exclusive_scan(ord, n, part);
  for (int i = threadIdx.x; i < n; i += SUB_BLOCK) {
    if (first[i] != i) continue;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int m = 0;
    for (int j = i; j < n; ++j)
      if (first[j] == i) {
        const float* p = pts + (size_t)(p0 + j) * 3;
        sx = __fadd_rn(sx, p[0]);
        sy = __fadd_rn(sy, p[1]);
        sz = __fadd_rn(sz, p[2]);
        ++m;
      }
    const float fm = (float)m;
    float* o = out_pad + ((size_t)b * cap + ord[i]) * 3;
    o[0] = __fdiv_rn(sx, fm);
    o[1] = __fdiv_rn(sy, fm);
    o[2] = __fdiv_rn(sz, fm);
  }
  if (threadIdx.x == 0) cnt[b] = nv;
}

// padded [B, cap, 3] -> packed rows of out [C, 3], offsets from the counts (out_off [B+1]).  Offsets are clamped to C (rows
// past C are dropped) and the dead rows [min(total, C), C) are zero-filled.  With a record rec (int32
// [SUG_KPCONV_RECORD_INTS]; may be null) the unclamped total is folded into it: rec[level] = max(rec[level], total);
// rec[4] counts the forwards with an overflow at any level (rec[5] = this forward has been counted; cleared by the
// level-0 call) -- one lane, plain stores.  Grid covers B*cap >= C threads.
__global__ void pack_kernel(const float* __restrict__ pad, int cap, const int32_t* __restrict__ cnt, int B, int C,
                            float* __restrict__ out, int32_t* __restrict__ out_off, int32_t* __restrict__ rec, int level) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < B * cap) {
    const int b = t / cap, i = t - b * cap;
    if (i < cnt[b]) {
      int o = 0;
      for (int j = 0; j < b; ++j) o += cnt[j];
      if (o + i < C)
        for (int a = 0; a < 3; ++a) out[(size_t)(o + i) * 3 + a] = pad[(size_t)t * 3 + a];
    }
  }
  if (t < C) {
    int total = 0;
    for (int j = 0; j < B; ++j) total += cnt[j];
    if (t >= total)
      for (int a = 0; a < 3; ++a) out[(size_t)t * 3 + a] = 0.f;
  }
  if (t == 0) {
    int o = 0;
    out_off[0] = 0;
    for (int j = 0; j < B; ++j) out_off[j + 1] = min(o += cnt[j], C);
    if (rec) {
      if (o > rec[level]) rec[level] = o;
      int counted = level == 0 ? 0 : rec[5];
      if (o > C && !counted) {
        rec[4] += 1;
        counted = 1;
      }
      rec[5] = counted;
    }
  }
}

// One query per thread: the first `limit` supports of its cloud, in support order, with d^2 < r^2; shadow-padded.
// A dead query (i >= qoff[B]) gets an all-shadow row and reads nothing.
__global__ void radius_kernel(const float* __restrict__ q, const int32_t* __restrict__ qoff, const float* __restrict__ s,
                              const int32_t* __restrict__ soff, int B, int Nq, int Ns, float r2, int limit,
                              int32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Nq) return;
  int32_t* o = out + (size_t)i * limit;
  int m = 0;
  if (i >= qoff[B]) {
    for (; m < limit; ++m) o[m] = Ns;
    return;
  }
  const int b = cloud_of(qoff, B, i);
  const int s0 = soff[b], s1 = min(soff[b + 1], Ns);
  const float qx = q[(size_t)i * 3], qy = q[(size_t)i * 3 + 1], qz = q[(size_t)i * 3 + 2];
  for (int j = s0; j < s1 && m < limit; ++j) {
    const float dx = __fsub_rn(s[(size_t)j * 3], qx), dy = __fsub_rn(s[(size_t)j * 3 + 1], qy),
                dz = __fsub_rn(s[(size_t)j * 3 + 2], qz);
    const float d2 = sq3(dx, dy, dz);
    if (d2 < r2) o[m++] = j;
  }
  for (; m < limit; ++m) o[m] = Ns;
}

// One cloud per workgroup: the entries e = q*H + h of the cloud's queries that name support s, ascending, at
// rev_ent[rev_be[s][0] .. rev_be[s][1]) (inside the cloud's own range [q0*H, q1*H) of rev_ent).
// One more workgroup (blockIdx.x == B) gives the dead supports [soff[B], Ns) their empty lists.
__global__ void __launch_bounds__(SUB_BLOCK) radius_reverse_kernel(const int32_t* __restrict__ nbr,
                                                                   const int32_t* __restrict__ qoff,
                                                                   const int32_t* __restrict__ soff, int H, int Ns,
                                                                   int cap, int32_t* __restrict__ rev_be,
                                                                   int32_t* __restrict__ rev_ent) {
  extern __shared__ int lds[];
  int* cnt = lds;
  int* cur = cnt + cap;
  int* part = cur + cap;
  const int b = blockIdx.x;
  if (b == (int)gridDim.x - 1) {      // uniform: before the first barrier
    for (int i = soff[b] + threadIdx.x; i < Ns; i += SUB_BLOCK) rev_be[(size_t)i * 2] = rev_be[(size_t)i * 2 + 1] = 0;
    return;
  }
  const int q0 = qoff[b], q1 = qoff[b + 1], s0 = soff[b], ns = soff[b + 1] - s0;
  if (ns > cap) return;
  const int e0 = q0 * H, e1 = q1 * H;
  for (int i = threadIdx.x; i < ns; i += SUB_BLOCK) cnt[i] = 0;
  __syncthreads();
  for (int e = e0 + threadIdx.x; e < e1; e += SUB_BLOCK) {
    const int s = nbr[e] - s0;
    if (s >= 0 && s < ns && s + s0 < Ns) atomicAdd(&cnt[s], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ns; i += SUB_BLOCK) cur[i] = cnt[i];
  __syncthreads();
  block_exclusive_scan(cur, ns, part);
  for (int i = threadIdx.x; i < ns; i += SUB_BLOCK) {
    rev_be[(size_t)(s0 + i) * 2] = e0 + cur[i];
    rev_be[(size_t)(s0 + i) * 2 + 1] = e0 + cur[i] + cnt[i];
  }
  __syncthreads();
  for (int e = e0 + threadIdx.x; e < e1; e += SUB_BLOCK) {
    const int s = nbr[e] - s0;
    if (s >= 0 && s < ns && s + s0 < Ns) rev_ent[e0 + atomicAdd(&cur[s], 1)] = e;
  }
  __threadfence_block();
  __syncthreads();
  // placement order above depends on timing: sort each list (short, insertion sort) to the ascending (q, h) order
  for (int i = threadIdx.x; i < ns; i += SUB_BLOCK) {
    const int lo = rev_be[(size_t)(s0 + i) * 2], hi = rev_be[(size_t)(s0 + i) * 2 + 1];
    for (int a = lo + 1; a < hi; ++a) {
      const int v = rev_ent[a];
      int c = a - 1;
      while (c >= lo && rev_ent[c] > v) {
        rev_ent[c + 1] = rev_ent[c];
        --c;
      }
      rev_ent[c + 1] = v;
    }
  }
}

// KPConv aggregation: KP_QB queries per workgroup.  Phase 1 (all threads over the QB x H slots): influences
// w[k,h] = max(0, 1 - |(s_h - q) - kp_k| / extent) into LDS and out to w_out [Nq, H, K]; the positive-sum flags of the
// neighbour rows.  Phase 2 (threads over QB x Cin): wf[q, k, c] = sum_h w[k,h] x[s_h, c], divided by
// max(1, #positive rows); written as [Nq, K*Cin] for the GEMM against W viewed as [K*Cin, Cout].
// *nq_valid: the valid queries of the Nq; dead queries get zero wf / w rows and cnt 1.
__global__ void __launch_bounds__(256) kpconv_fwd_kernel(const float* __restrict__ q, const float* __restrict__ s,
                                                         const int32_t* __restrict__ nbr,
                                                         const int32_t* __restrict__ nq_valid, int Nq, int H, int Ns,
                                                         const float* __restrict__ kp, int K, float extent,
                                                         const float* __restrict__ x, int Cin, float* __restrict__ wf,
                                                         float* __restrict__ w_out, float* __restrict__ cnt_out) {
  __shared__ float w[KP_QB][KP_MAX_K][KP_MAX_H];
  __shared__ int nid[KP_QB][KP_MAX_H];
  __shared__ int pos[KP_QB][KP_MAX_H];
  __shared__ float cnt[KP_QB];
  const int qb0 = blockIdx.x * KP_QB;
  const int nv = min(*nq_valid, Nq);
  if (qb0 >= nv) {      // a wholly dead tile (blockIdx and a uniform load only): zeros, before the first barrier
    const int rows = min(KP_QB, Nq - qb0);
    for (int t = threadIdx.x; t < rows * K * Cin; t += blockDim.x) wf[(size_t)qb0 * K * Cin + t] = 0.f;
    for (int t = threadIdx.x; t < rows * H * K; t += blockDim.x) w_out[(size_t)qb0 * H * K + t] = 0.f;
    if ((int)threadIdx.x < rows) cnt_out[qb0 + threadIdx.x] = 1.f;
    return;
  }
  for (int t = threadIdx.x; t < KP_QB * H; t += blockDim.x) {
    const int qi = t / H, h = t - qi * H, qq = qb0 + qi;
    int sid = -1, p = 0;
    if (qq < nv) {
      const int sv = nbr[(size_t)qq * H + h];
      if (sv >= 0 && sv < Ns) sid = sv;
    }
    if (sid >= 0) {
      const float dx = __fsub_rn(s[(size_t)sid * 3], q[(size_t)qq * 3]);
      const float dy = __fsub_rn(s[(size_t)sid * 3 + 1], q[(size_t)qq * 3 + 1]);
      const float dz = __fsub_rn(s[(size_t)sid * 3 + 2], q[(size_t)qq * 3 + 2]);
      for (int k = 0; k < K; ++k) {
        const float ex = __fsub_rn(dx, kp[k * 3]), ey = __fsub_rn(dy, kp[k * 3 + 1]), ez = __fsub_rn(dz, kp[k * 3 + 2]);
        const float v = fmaxf(0.f, __fsub_rn(1.f, __fdiv_rn(sqrtf(sq3(ex, ey, ez)), extent)));
        w[qi][k][h] = v;
        w_out[((size_t)qq * H + h) * K + k] = v;
      }
      float sum = 0.f;
      for (int c = 0; c < Cin; ++c) sum = __fadd_rn(sum, x[(size_t)sid * Cin + c]);
      p = sum > 0.f;
    } else {
      for (int k = 0; k < K; ++k) {
        w[qi][k][h] = 0.f;
        if (qq < Nq) w_out[((size_t)qq * H + h) * K + k] = 0.f;
      }
    }
    nid[qi][h] = sid;
    pos[qi][h] = p;
  }
  __syncthreads();
  if (threadIdx.x < KP_QB) {
    int m = 0;
    for (int h = 0; h < H; ++h) m += pos[threadIdx.x][h];
    cnt[threadIdx.x] = (float)max(m, 1);
    if (qb0 + (int)threadIdx.x < Nq) cnt_out[qb0 + threadIdx.x] = (float)max(m, 1);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < KP_QB * Cin; t += blockDim.x) {
    const int qi = t / Cin, c = t - qi * Cin, qq = qb0 + qi;
    if (qq >= Nq) continue;
    float acc[KP_MAX_K];
#pragma unroll
    for (int k = 0; k < KP_MAX_K; ++k) acc[k] = 0.f;
    for (int h = 0; h < H; ++h) {
      const int sid = nid[qi][h];
      if (sid < 0) continue;
      const float xv = x[(size_t)sid * Cin + c];
#pragma unroll
      for (int k = 0; k < KP_MAX_K; ++k)
        if (k < K) acc[k] = fmaf(w[qi][k][h], xv, acc[k]);
    }
    float* o = wf + (size_t)qq * K * Cin + c;
#pragma unroll
    for (int k = 0; k < KP_MAX_K; ++k)
      if (k < K) o[(size_t)k * Cin] = __fdiv_rn(acc[k], cnt[qi]);
  }
}

// dx[s, c] = sum over s's reverse entries (q, h), ascending, of (sum_k w[q,h,k] dwf[q,k,c]) / cnt[q]
__global__ void kpconv_bwd_kernel(const int32_t* __restrict__ rev_be, const int32_t* __restrict__ rev_ent, int H, int K,
                                  const float* __restrict__ w, const float* __restrict__ cnt,
                                  const float* __restrict__ dwf, int Ns, int Cin, float* __restrict__ dx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)Ns * Cin) return;
  const int sid = (int)(t / Cin), c = (int)(t - (int64_t)sid * Cin);
  const int lo = rev_be[(size_t)sid * 2], hi = rev_be[(size_t)sid * 2 + 1];
  float acc = 0.f;
  for (int a = lo; a < hi; ++a) {
    const int e = rev_ent[a], qq = e / H;
    const float* we = w + (size_t)e * K;
    const float* g = dwf + (size_t)qq * K * Cin + c;
    float v = 0.f;
    for (int k = 0; k < K; ++k) v = fmaf(we[k], g[(size_t)k * Cin], v);
    acc = __fadd_rn(acc, __fdiv_rn(v, cnt[qq]));
  }
  dx[t] = acc;
}

// Segmented statistics: one workgroup per (cloud, 64-channel chunk), 256 threads = 4 row lanes x 64 channels; each lane
// sums its rows in order (fp64), the four lanes are combined in lane order.
__device__ __forceinline__ double seg_combine(double v, double* red) {
  const int c = threadIdx.x & 63, l = threadIdx.x >> 6;
  red[l * 64 + c] = v;
  __syncthreads();
  const double r = ((red[c] + red[64 + c]) + red[128 + c]) + red[192 + c];
  __syncthreads();
  return r;
}

// x / y have N rows: workgroup blockIdx.x == B zero-fills the dead rows [off[B], N) of y; an empty cloud writes
// mean = rstd = 0 and normalises nothing.  Both leave before the first barrier, on uniform values only.
__global__ void __launch_bounds__(256) seg_instnorm_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ off,
                                                               int N, int C, float eps, int mode,
                                                               const float* __restrict__ sc, float* __restrict__ y,
                                                               float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  __shared__ double red[256];
  const int b = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), l = threadIdx.x >> 6;
  const bool on = c < C;
  if (b == (int)gridDim.x - 1) {
    if (on)
      for (int r = off[b] + l; r < N; r += 4) y[(size_t)r * C + c] = 0.f;
    return;
  }
  const int r0 = off[b], r1 = off[b + 1];
  if (r1 <= r0) {
    if (on && l == 0) mean_out[(size_t)b * C + c] = rstd_out[(size_t)b * C + c] = 0.f;
    return;
  }
  const double n = (double)(r1 - r0);
  double s1 = 0.0;
  if (on)
    for (int r = r0 + l; r < r1; r += 4) s1 += (double)x[(size_t)r * C + c];
  const double mean = seg_combine(s1, red) / n;
  double s2 = 0.0;
  if (on)
    for (int r = r0 + l; r < r1; r += 4) {
      const double d = (double)x[(size_t)r * C + c] - mean;
      s2 += d * d;
    }
  const double var = seg_combine(s2, red) / n;
  if (!on) return;
  const float m = (float)mean, rs = (float)(1.0 / sqrt(var + (double)eps));
  if (l == 0) {
    mean_out[(size_t)b * C + c] = m;
    rstd_out[(size_t)b * C + c] = rs;
  }
  for (int r = r0 + l; r < r1; r += 4) {
    const size_t i = (size_t)r * C + c;
    float v = __fmul_rn(__fsub_rn(x[i], m), rs);
    if (mode == 2) v = __fadd_rn(v, sc[i]);
    if (mode >= 1) v = v > 0.f ? v : __fmul_rn(v, LEAKY);
    y[i] = v;
  }
}

// gp = g * act'(out); dsc = gp (mode 2); dx = rstd (gp - mean(gp) - xhat mean(gp xhat)), xhat = (x - mean) rstd
__global__ void __launch_bounds__(256) seg_instnorm_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                               const float* __restrict__ x, const float* __restrict__ mean_in,
                                                               const float* __restrict__ rstd_in,
                                                               const int32_t* __restrict__ off, int N, int C, int mode,
                                                               float* __restrict__ dx, float* __restrict__ dsc) {
  __shared__ double red[256];
  const int b = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), l = threadIdx.x >> 6;
  const bool on = c < C;
  if (b == (int)gridDim.x - 1) {      // the dead rows of dx (and dsc): zeros
    if (on)
      for (int r = off[b] + l; r < N; r += 4) {
        dx[(size_t)r * C + c] = 0.f;
        if (mode == 2) dsc[(size_t)r * C + c] = 0.f;
      }
    return;
  }
  const int r0 = off[b], r1 = off[b + 1];
  if (r1 <= r0) return;                       // an empty cloud has no rows to write
  const double n = (double)(r1 - r0);
  const float m = on ? mean_in[(size_t)b * C + c] : 0.f, rs = on ? rstd_in[(size_t)b * C + c] : 0.f;
  double s1 = 0.0, s2 = 0.0;
  if (on)
    for (int r = r0 + l; r < r1; r += 4) {
      const size_t i = (size_t)r * C + c;
      float gp = g[i];
      if (mode >= 1 && !(y[i] > 0.f)) gp = __fmul_rn(gp, LEAKY);
      const float xh = __fmul_rn(__fsub_rn(x[i], m), rs);
      s1 += (double)gp;
      s2 += (double)gp * (double)xh;
    }
  const double mg = seg_combine(s1, red) / n;
  const double mgx = seg_combine(s2, red) / n;
  if (!on) return;
  for (int r = r0 + l; r < r1; r += 4) {
    const size_t i = (size_t)r * C + c;
    float gp = g[i];
    if (mode >= 1 && !(y[i] > 0.f)) gp = __fmul_rn(gp, LEAKY);
    if (mode == 2) dsc[i] = gp;
    const double xh = (double)__fmul_rn(__fsub_rn(x[i], m), rs);
    dx[i] = (float)((double)rs * ((double)gp - mg - xh * mgx));
  }
}

// out[q, c] = max over the H slots of x[slot, c], a shadow slot reading 0; first maximum (lowest h) wins
__global__ void max_pool_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ nbr, int Nq, int H, int Ns,
                                    int C, float* __restrict__ y, int32_t* __restrict__ arg) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)Nq * C) return;
  const int qq = (int)(t / C), c = (int)(t - (int64_t)qq * C);
  float best = 0.f;
  int a = -1;
  for (int h = 0; h < H; ++h) {
    const int sid = nbr[(size_t)qq * H + h];
    const float v = (sid >= 0 && sid < Ns) ? x[(size_t)sid * C + c] : 0.f;
    if (a < 0 || v > best) {
      best = v;
      a = h;
    }
  }
  y[t] = best;
  arg[t] = a;
}

// dx[s, c] = sum over s's reverse entries (q, h), ascending, with arg[q, c] == h of g[q, c]
__global__ void max_pool_bwd_kernel(const float* __restrict__ g, const int32_t* __restrict__ arg,
                                    const int32_t* __restrict__ rev_be, const int32_t* __restrict__ rev_ent, int H,
                                    int Ns, int C, float* __restrict__ dx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)Ns * C) return;
  const int sid = (int)(t / C), c = (int)(t - (int64_t)sid * C);
  const int lo = rev_be[(size_t)sid * 2], hi = rev_be[(size_t)sid * 2 + 1];
  float acc = 0.f;
  for (int a = lo; a < hi; ++a) {
    const int e = rev_ent[a], qq = e / H, h = e - qq * H;
    if (arg[(size_t)qq * C + c] == h) acc = __fadd_rn(acc, g[(size_t)qq * C + c]);
  }
  dx[t] = acc;
}

__global__ void __launch_bounds__(256) seg_mean_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ off,
                                                           int C, float* __restrict__ y) {
  __shared__ double red[256];
  const int b = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), l = threadIdx.x >> 6;
  const int r0 = off[b], r1 = off[b + 1];
  if (r1 <= r0) {                     // an empty cloud's pooled row is 0 (uniform: before the barrier)
    if (c < C && l == 0) y[(size_t)b * C + c] = 0.f;
    return;
  }
  double s = 0.0;
  if (c < C)
    for (int r = r0 + l; r < r1; r += 4) s += (double)x[(size_t)r * C + c];
  s = seg_combine(s, red);
  if (c < C && l == 0) y[(size_t)b * C + c] = (float)(s / (double)(r1 - r0));
}

__global__ void seg_mean_bwd_kernel(const float* __restrict__ g, const int32_t* __restrict__ off, int B, int N, int C,
                                    float* __restrict__ dx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)N * C) return;
  const int r = (int)(t / C), c = (int)(t - (int64_t)r * C);
  if (r >= off[B]) {                          // a dead row
    dx[t] = 0.f;
    return;
  }
  const int b = cloud_of(off, B, r);
  dx[t] = __fdiv_rn(g[(size_t)b * C + c], (float)(off[b + 1] - off[b]));
}

// sample_tensor_slices from device offsets: out[b, j, :] = x[off[b] + idx(j, n), :], n = off[b+1] - off[b],
// idx = j * (n / S) for n >= S and j mod n below that; zeros for n == 0.  One thread per output element.
__global__ void sample_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ off, int B, int S, int D,
                                   float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * S * D) return;
  const int d = (int)(t % D), j = (int)((t / D) % S), b = (int)(t / ((int64_t)D * S));
  const int r0 = off[b], n = off[b + 1] - r0;
  float v = 0.f;
  if (n > 0) {
    const int idx = n >= S ? j * (n / S) : j % n;
    v = x[(size_t)(r0 + idx) * D + d];
  }
  out[t] = v;
}

}  // namespace

extern "C" int sug_grid_subsample(const float* pts, const int32_t* off, int B, int cap, float dl, int C, int level,
                                  float* out_pad, int32_t* cnt, float* out, int32_t* out_off, int32_t* record,
                                  void* stream) {
  SUG_REQUIRE(pts && off && out_pad && cnt && out && out_off, "sug_grid_subsample: null pointer");
  SUG_REQUIRE(B > 0 && cap > 0 && cap <= SUG_KPCONV_MAX_CLOUD, "sug_grid_subsample: cap %d outside (0, %d]", cap,
              SUG_KPCONV_MAX_CLOUD);
  SUG_REQUIRE(C > 0 && (int64_t)C <= (int64_t)B * cap && (!record || (level >= 0 && level < 4)),
              "sug_grid_subsample: capacity %d outside (0, B*cap] or level %d outside [0, 4)", C, level);
  SUG_REQUIRE(dl > 0.f, "sug_grid_subsample: dl must be positive");
  hipStream_t st = (hipStream_t)stream;
  const int sh = (5 * cap + SUB_BLOCK) * (int)sizeof(int);
  static SugLdsOptIn note;
  if (int rc = sug_allow_dynamic_lds(note, &grid_subsample_kernel, (5 * SUG_KPCONV_MAX_CLOUD + SUB_BLOCK) * 4,
                                     "sug_grid_subsample"))
    return rc;
  hipLaunchKernelGGL(grid_subsample_kernel, dim3(B), dim3(SUB_BLOCK), sh, st, pts, off, dl, cap, out_pad, cnt);
  SUG_LAUNCH_CHECK("sug_grid_subsample");
  hipLaunchKernelGGL(pack_kernel, dim3(sug_divup((int64_t)B * cap, 256)), dim3(256), 0, st, out_pad, cap, cnt, B, C, out,
                     out_off, record, level);
  SUG_LAUNCH_CHECK("sug_grid_subsample/pack");
  return SUG_OK;
}

extern "C" int sug_radius_neighbors(const float* q, const int32_t* qoff, int Nq, const float* s, const int32_t* soff,
                                    int Ns, int B, float radius, int limit, int32_t* out, void* stream) {
  SUG_REQUIRE(q && qoff && s && soff && out, "sug_radius_neighbors: null pointer");
  SUG_REQUIRE(B > 0 && Nq > 0 && Ns > 0 && limit > 0 && limit <= KP_MAX_H, "sug_radius_neighbors: bad shape");
  const float r2 = radius * radius;       // fp32(r) * fp32(r), rounded once
  hipLaunchKernelGGL(radius_kernel, dim3(sug_divup(Nq, 256)), dim3(256), 0, (hipStream_t)stream, q, qoff, s, soff, B, Nq,
                     Ns, r2, limit, out);
  SUG_LAUNCH_CHECK("sug_radius_neighbors");
  return SUG_OK;
}

extern "C" int sug_radius_reverse(const int32_t* nbr, const int32_t* qoff, const int32_t* soff, int B, int H, int Ns,
                                  int cap, int32_t* rev_be, int32_t* rev_ent, void* stream) {
  SUG_REQUIRE(nbr && qoff && soff && rev_be && rev_ent, "sug_radius_reverse: null pointer");
  SUG_REQUIRE(B > 0 && H > 0 && Ns > 0 && cap > 0 && cap <= SUG_KPCONV_MAX_CLOUD,
              "sug_radius_reverse: bad shape (cap %d, at most %d supports per cloud)", cap, SUG_KPCONV_MAX_CLOUD);
  const int sh = (2 * cap + SUB_BLOCK) * (int)sizeof(int);
  hipLaunchKernelGGL(radius_reverse_kernel, dim3(B + 1), dim3(SUB_BLOCK), sh, (hipStream_t)stream, nbr, qoff, soff, H, Ns,
                     cap, rev_be, rev_ent);
  SUG_LAUNCH_CHECK("sug_radius_reverse");
  return SUG_OK;
}

extern "C" int sug_kpconv_fwd(const float* q, const float* s, const int32_t* nbr, const int32_t* nq_valid, int Nq, int H,
                              int Ns, const float* kp, int K, float extent, const float* x, int Cin, float* wf, float* w,
                              float* cnt, void* stream) {
  SUG_REQUIRE(q && s && nbr && nq_valid && kp && x && wf && w && cnt, "sug_kpconv_fwd: null pointer");
  SUG_REQUIRE(Nq > 0 && Ns > 0 && Cin > 0 && H > 0 && H <= KP_MAX_H && K > 0 && K <= KP_MAX_K && extent > 0.f,
              "sug_kpconv_fwd: bad shape (H %d <= %d, K %d <= %d)", H, KP_MAX_H, K, KP_MAX_K);
  hipLaunchKernelGGL(kpconv_fwd_kernel, dim3(sug_divup(Nq, KP_QB)), dim3(256), 0, (hipStream_t)stream, q, s, nbr, nq_valid,
                     Nq, H, Ns, kp, K, extent, x, Cin, wf, w, cnt);
  SUG_LAUNCH_CHECK("sug_kpconv_fwd");
  return SUG_OK;
}

extern "C" int sug_kpconv_bwd(const int32_t* rev_be, const int32_t* rev_ent, int H, int K, const float* w,
                              const float* cnt, const float* dwf, int Ns, int Cin, float* dx, void* stream) {
  SUG_REQUIRE(rev_be && rev_ent && w && cnt && dwf && dx, "sug_kpconv_bwd: null pointer");
  SUG_REQUIRE(H > 0 && K > 0 && Ns > 0 && Cin > 0, "sug_kpconv_bwd: bad shape");
  hipLaunchKernelGGL(kpconv_bwd_kernel, dim3(sug_divup((int64_t)Ns * Cin, 256)), dim3(256), 0, (hipStream_t)stream, rev_be,
                     rev_ent, H, K, w, cnt, dwf, Ns, Cin, dx);
  SUG_LAUNCH_CHECK("sug_kpconv_bwd");
  return SUG_OK;
}

extern "C" int sug_seg_instnorm_fwd(const float* x, const int32_t* off, int B, int N, int C, float eps, int mode,
                                    const float* sc, float* y, float* mean, float* rstd, void* stream) {
  SUG_REQUIRE(x && off && y && mean && rstd && (mode != 2 || sc), "sug_seg_instnorm_fwd: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && C > 0 && mode >= 0 && mode <= 2, "sug_seg_instnorm_fwd: bad shape / mode");
  hipLaunchKernelGGL(seg_instnorm_fwd_kernel, dim3(B + 1, sug_divup(C, 64)), dim3(256), 0, (hipStream_t)stream, x, off, N,
                     C, eps, mode, sc, y, mean, rstd);
  SUG_LAUNCH_CHECK("sug_seg_instnorm_fwd");
  return SUG_OK;
}

extern "C" int sug_seg_instnorm_bwd(const float* g, const float* y, const float* x, const float* mean, const float* rstd,
                                    const int32_t* off, int B, int N, int C, int mode, float* dx, float* dsc,
                                    void* stream) {
  SUG_REQUIRE(g && y && x && mean && rstd && off && dx && (mode != 2 || dsc), "sug_seg_instnorm_bwd: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && C > 0 && mode >= 0 && mode <= 2, "sug_seg_instnorm_bwd: bad shape / mode");
  hipLaunchKernelGGL(seg_instnorm_bwd_kernel, dim3(B + 1, sug_divup(C, 64)), dim3(256), 0, (hipStream_t)stream, g, y, x,
                     mean, rstd, off, N, C, mode, dx, dsc);
  SUG_LAUNCH_CHECK("sug_seg_instnorm_bwd");
  return SUG_OK;
}

extern "C" int sug_seg_max_pool_fwd(const float* x, const int32_t* nbr, int Nq, int H, int Ns, int C, float* y,
                                    int32_t* arg, void* stream) {
  SUG_REQUIRE(x && nbr && y && arg, "sug_seg_max_pool_fwd: null pointer");
  SUG_REQUIRE(Nq > 0 && H > 0 && Ns > 0 && C > 0, "sug_seg_max_pool_fwd: bad shape");
  hipLaunchKernelGGL(max_pool_fwd_kernel, dim3(sug_divup((int64_t)Nq * C, 256)), dim3(256), 0, (hipStream_t)stream, x, nbr,
                     Nq, H, Ns, C, y, arg);
  SUG_LAUNCH_CHECK("sug_seg_max_pool_fwd");
  return SUG_OK;
}

extern "C" int sug_seg_max_pool_bwd(const float* g, const int32_t* arg, const int32_t* rev_be, const int32_t* rev_ent,
                                    int H, int Ns, int C, float* dx, void* stream) {
  SUG_REQUIRE(g && arg && rev_be && rev_ent && dx, "sug_seg_max_pool_bwd: null pointer");
  SUG_REQUIRE(H > 0 && Ns > 0 && C > 0, "sug_seg_max_pool_bwd: bad shape");
  hipLaunchKernelGGL(max_pool_bwd_kernel, dim3(sug_divup((int64_t)Ns * C, 256)), dim3(256), 0, (hipStream_t)stream, g, arg,
                     rev_be, rev_ent, H, Ns, C, dx);
  SUG_LAUNCH_CHECK("sug_seg_max_pool_bwd");
  return SUG_OK;
}

extern "C" int sug_seg_mean_fwd(const float* x, const int32_t* off, int B, int C, float* y, void* stream) {
  SUG_REQUIRE(x && off && y, "sug_seg_mean_fwd: null pointer");
  SUG_REQUIRE(B > 0 && C > 0, "sug_seg_mean_fwd: bad shape");
  hipLaunchKernelGGL(seg_mean_fwd_kernel, dim3(B, sug_divup(C, 64)), dim3(256), 0, (hipStream_t)stream, x, off, C, y);
  SUG_LAUNCH_CHECK("sug_seg_mean_fwd");
  return SUG_OK;
}

extern "C" int sug_seg_mean_bwd(const float* g, const int32_t* off, int B, int N, int C, float* dx, void* stream) {
  SUG_REQUIRE(g && off && dx, "sug_seg_mean_bwd: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && C > 0, "sug_seg_mean_bwd: bad shape");
  hipLaunchKernelGGL(seg_mean_bwd_kernel, dim3(sug_divup((int64_t)N * C, 256)), dim3(256), 0, (hipStream_t)stream, g, off, B,
                     N, C, dx);
  SUG_LAUNCH_CHECK("sug_seg_mean_bwd");
  return SUG_OK;
}

extern "C" int sug_kp_sample_rows(const float* x, const int32_t* off, int B, int S, int D, float* out, void* stream) {
  SUG_REQUIRE(x && off && out, "sug_kp_sample_rows: null pointer");
  SUG_REQUIRE(B > 0 && S > 0 && D > 0, "sug_kp_sample_rows: bad shape");
  hipLaunchKernelGGL(sample_rows_kernel, dim3(sug_divup((int64_t)B * S * D, 256)), dim3(256), 0, (hipStream_t)stream, x, off, B,
                     S, D, out);
  SUG_LAUNCH_CHECK("sug_kp_sample_rows");
  return SUG_OK;
}
