// Device-resident data pipeline: what UnifiedPointDG.__getitem__ (data/dataloader.py:302-327) does per cloud -- normal_pc,
// the fixed pre-rotation, the random z-rotation, the clipped jitter, zero padding or a random ordered subset, the transpose
// -- for a whole batch in one launch, one workgroup per cloud.  sug_prepare_batch_aug adds the three augmentations that
// pc_augment lists but leaves switched off (random scale, rotation perturbation, shift), behind the jitter in its line order.
// Counter layout of the in-kernel draws: include/sug_amd.h.
#include "common.h"

namespace {

constexpr int PREP_MAX_P = SUG_PREP_MAX_POINTS;
constexpr int PREP_MAX_WAVES = 16;

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key k[2]
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__device__ __forceinline__ float u24(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }              // [0, 1)
__device__ __forceinline__ float u24_open(uint32_t w) { return (float)((w >> 8) + 1u) * 5.9604644775390625e-8f; }  // (0, 1]

// one compare-exchange of a bitonic stage: slots i and i + j, ascending where (i & k) == 0
__device__ __forceinline__ void sort_pair(unsigned long long* key, int i, int j, int k) {
  const unsigned long long x = key[i], y = key[i + j];
  if ((x > y) == ((i & k) == 0)) { key[i] = y; key[i + j] = x; }
}

struct PrepArgs {
  const float* pts;         // [M, P, 3]
  const int32_t* idx;       // [B]
  const float* angles;      // [B] or null
  const float* noise;       // [B, P, 3] or null
  const int32_t* sel;       // [B, N] or null
  const uint64_t* counter;  // [1] or null (only when nothing is drawn in the kernel)
  float* out;               // [B, 3, N]
  float* angles_out;        // [B] or null
  float* noise_out;         // [B, N, 3] or null
  int32_t* sel_out;         // [B, N] or null
  float pre[9];             // pre-rotation, row-major (used when has_pre)
  uint64_t seed;
  int M, P, N, P2;
  int stages, has_pre, sort;
  float sigma, clip;
  // sug_prepare_batch_aug only (SUG_PREP_SCALE / _PERTURB / _SHIFT); the draws are per cloud
  const float* scales;      // [B] or null
  const float* perturb;     // [B, 3] standard normals, or null
  const float* shifts;      // [B, 3] or null
  float* scales_out;        // [B] or null
  float* perturb_out;       // [B, 3] or null
  float* shifts_out;        // [B, 3] or null
  float scale_low, scale_high, shift_range, angle_sigma, angle_clip;
};

constexpr int PREP_AUG_STAGES = SUG_PREP_SCALE | SUG_PREP_PERTURB | SUG_PREP_SHIFT;

__global__ __launch_bounds__(1024) void prepare_batch_kernel(const PrepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  float* s_xyz = reinterpret_cast<float*>(s_raw);                                            // [P, 3]
  unsigned long long* s_key = reinterpret_cast<unsigned long long*>(s_raw + (((size_t)a.P * 12 + 15) & ~(size_t)15));  // [P2] when sort
  __shared__ double s_sum[PREP_MAX_WAVES][3];
  __shared__ float s_max[PREP_MAX_WAVES];
  __shared__ float s_aug[13];           // per cloud: the scale, the perturbation matrix (row-major), the shift

  const int b = blockIdx.x, t = threadIdx.x, T = blockDim.x;
  const int lane = t & (WAVE - 1), wv = t / WAVE, nw = T / WAVE;
  const int P = a.P, N = a.N;
  float* ob = a.out + (int64_t)b * 3 * N;
  const int ci = a.idx[b];
  if (ci < 0 || ci >= a.M) {            // an index outside the dataset: never read there, mark the cloud (uniform over the block)
    for (int i = t; i < 3 * N; i += T) ob[i] = NAN;
    return;
  }
  const float* pb = a.pts + (int64_t)ci * P * 3;
  for (int i = t; i < 3 * P; i += T) s_xyz[i] = pb[i];

  uint32_t c0 = 0, c1 = 0;
  if (a.counter) {
    const uint64_t c = *a.counter;
    c0 = (uint32_t)c; c1 = (uint32_t)(c >> 32);
  }
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  if (t == 0 && ((a.stages & PREP_AUG_STAGES) || a.scales_out || a.perturb_out || a.shifts_out)) {
    // the per-cloud draws of the three extra stages, by one lane; every lane reads them behind the barrier below
    float sc = 1.0f, g[3] = {0.0f, 0.0f, 0.0f}, sh[3] = {0.0f, 0.0f, 0.0f};
    if (a.stages & SUG_PREP_SCALE) {
      if (a.scales) {
        sc = a.scales[b];
      } else {
        uint32_t w[4];
        philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_SCALE, k0, k1, w);
        sc = a.scale_low + u24(w[0]) * (a.scale_high - a.scale_low);
      }
    }
    if (a.stages & SUG_PREP_PERTURB) {
      if (a.perturb) {
        g[0] = a.perturb[3 * b + 0]; g[1] = a.perturb[3 * b + 1]; g[2] = a.perturb[3 * b + 2];
      } else {                                  // the jitter's Box-Muller
        uint32_t w[4];
        philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_PERTURB, k0, k1, w);
        const float r0 = sqrtf(-2.0f * logf(u24_open(w[0]))), r1 = sqrtf(-2.0f * logf(u24_open(w[2])));
        float s0, q0, s1, q1;
        sincosf(6.28318530717958647692f * u24(w[1]), &s0, &q0);
        sincosf(6.28318530717958647692f * u24(w[3]), &s1, &q1);
        g[0] = r0 * q0; g[1] = r0 * s0; g[2] = r1 * q1;
      }
      // R = Rz (Ry Rx) of rotate_perturbation_point_cloud, formed in fp64 from the fp32 normals and rounded once
      const double lim = (double)a.angle_clip;
      double sx, cx, sy, cy, sz, cz;
      sincos(fmin(fmax((double)a.angle_sigma * (double)g[0], -lim), lim), &sx, &cx);
      sincos(fmin(fmax((double)a.angle_sigma * (double)g[1], -lim), lim), &sy, &cy);
      sincos(fmin(fmax((double)a.angle_sigma * (double)g[2], -lim), lim), &sz, &cz);
      const double m0[3] = {cy, sy * sx, sy * cx}, m1[3] = {0.0, cx, -sx}, m2[3] = {-sy, cy * sx, cy * cx};   // Ry Rx
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        s_aug[1 + j] = (float)(cz * m0[j] - sz * m1[j]);
        s_aug[4 + j] = (float)(sz * m0[j] + cz * m1[j]);
        s_aug[7 + j] = (float)m2[j];
      }
    }
    if (a.stages & SUG_PREP_SHIFT) {
      if (a.shifts) {
        sh[0] = a.shifts[3 * b + 0]; sh[1] = a.shifts[3 * b + 1]; sh[2] = a.shifts[3 * b + 2];
      } else {
        uint32_t w[4];
        philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_SHIFT, k0, k1, w);
#pragma unroll
        for (int j = 0; j < 3; ++j) sh[j] = (2.0f * u24(w[j]) - 1.0f) * a.shift_range;
      }
    }
    s_aug[0] = sc; s_aug[10] = sh[0]; s_aug[11] = sh[1]; s_aug[12] = sh[2];
    if (a.scales_out) a.scales_out[b] = sc;
    if (a.perturb_out) { a.perturb_out[3 * b + 0] = g[0]; a.perturb_out[3 * b + 1] = g[1]; a.perturb_out[3 * b + 2] = g[2]; }
    if (a.shifts_out) { a.shifts_out[3 * b + 0] = sh[0]; a.shifts_out[3 * b + 1] = sh[1]; a.shifts_out[3 * b + 2] = sh[2]; }
  }
  if (a.sort) {                         // subset keys: Philox block q -> points 4q .. 4q+3; past P: last in the order
    for (int q = t; q < a.P2 / 4; q += T) {
      uint32_t w[4];
      philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_SUBSET | (uint32_t)q, k0, k1, w);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = 4 * q + j;
        s_key[p] = p < P ? ((unsigned long long)w[j] << 32) | (unsigned)p : ~0ull;
      }
    }
  }
  __syncthreads();

  float den = 1.0f;                     // max norm; the points are divided by it, as in the reference
  if (a.stages & SUG_PREP_NORMALIZE) {
    // mean over all P points: fp64 partial sums, lanes by xor-shuffle, waves in index order -- one fixed order
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int p = t; p < P; p += T) {
      sx += (double)s_xyz[3 * p + 0]; sy += (double)s_xyz[3 * p + 1]; sz += (double)s_xyz[3 * p + 2];
    }
    sx = wave_sum_d(sx); sy = wave_sum_d(sy); sz = wave_sum_d(sz);
    if (lane == 0) { s_sum[wv][0] = sx; s_sum[wv][1] = sy; s_sum[wv][2] = sz; }
    __syncthreads();
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int w = 0; w < nw; ++w) { mx += s_sum[w][0]; my += s_sum[w][1]; mz += s_sum[w][2]; }
    mx /= (double)P; my /= (double)P; mz /= (double)P;
    float m2 = 0.0f;
    for (int p = t; p < P; p += T) {
      const float x = (float)((double)s_xyz[3 * p + 0] - mx), y = (float)((double)s_xyz[3 * p + 1] - my),
                  z = (float)((double)s_xyz[3 * p + 2] - mz);
      s_xyz[3 * p + 0] = x; s_xyz[3 * p + 1] = y; s_xyz[3 * p + 2] = z;
      m2 = fmaxf(m2, sq3(x, y, z));
    }
    m2 = wave_max_f(m2);
    if (lane == 0) s_max[wv] = m2;
    __syncthreads();
    m2 = s_max[0];
    for (int w = 1; w < nw; ++w) m2 = fmaxf(m2, s_max[w]);
    den = sqrtf(m2);
  }

  if (a.sort) {
    // Bitonic sort of (word, point) over P2 >= 128 slots, one compare-exchange per lane and stage on the pair (i, i + j).
    // Strides j <= 64 stay inside an aligned 128-slot chunk, which one wave owns: those stages (56 of the 66 at P2 = 2048)
    // need wave-level ordering only; a stride above 64 crosses chunks and takes a workgroup barrier.
    const int chunks = a.P2 / 128;
    for (int k = 2; k <= a.P2; k <<= 1) {
      int j = k >> 1;
      for (; j > 64; j >>= 1) {
        for (int q = t; q < a.P2 / 2; q += T) sort_pair(s_key, ((q & ~(j - 1)) << 1) | (q & (j - 1)), j, k);
        __syncthreads();
      }
      for (int c = wv; c < chunks; c += nw) {
        for (int jj = j; jj > 0; jj >>= 1) {
          sort_pair(s_key, c * 128 + (((lane & ~(jj - 1)) << 1) | (lane & (jj - 1))), jj, k);
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      }
      if (k >= 128) __syncthreads();      // the next k starts with a stride across chunks (or the sort is done)
    }
  }

  float ang = 0.0f, cs = 1.0f, sn = 0.0f;
  if (a.stages & SUG_PREP_ROTATE_Z) {
    if (a.angles) {
      ang = a.angles[b];
    } else {
      uint32_t w[4];
      philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_ANGLE, k0, k1, w);
      ang = u24(w[0]) * 6.28318530717958647692f;
    }
    sincosf(ang, &sn, &cs);
  }
  if (a.angles_out && t == 0) a.angles_out[b] = ang;

  const bool jit = (a.stages & SUG_PREP_JITTER) != 0;
  for (int n = t; n < N; n += T) {
    int src;
    if (a.sel) src = a.sel[(int64_t)b * N + n];
    else if (a.sort) src = (int)(unsigned)s_key[n];
    else src = n < P ? n : -1;
    float x = 0.0f, y = 0.0f, z = 0.0f, g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    if (src >= P || (a.sel && src < 0)) {       // a supplied index outside the cloud
      x = y = z = NAN;
    } else if (src >= 0) {
      x = s_xyz[3 * src + 0]; y = s_xyz[3 * src + 1]; z = s_xyz[3 * src + 2];
      if (a.stages & SUG_PREP_NORMALIZE) { x = x / den; y = y / den; z = z / den; }
      if (a.has_pre) {                          // x.dot(R): out_j = (x R_0j + y R_1j) + z R_2j
        const float u = (x * a.pre[0] + y * a.pre[3]) + z * a.pre[6], v = (x * a.pre[1] + y * a.pre[4]) + z * a.pre[7],
                    w = (x * a.pre[2] + y * a.pre[5]) + z * a.pre[8];
        x = u; y = v; z = w;
      }
      if (a.stages & SUG_PREP_ROTATE_Z) {       // [[c, -s, 0], [s, c, 0], [0, 0, 1]], row vector on the left
        const float u = x * cs + y * sn, v = y * cs - x * sn;
        x = u; y = v;
      }
      if (jit) {
        if (a.noise) {
          const float* nb = a.noise + ((int64_t)b * P + src) * 3;
          g0 = nb[0]; g1 = nb[1]; g2 = nb[2];
        } else {                                // Box-Muller: words 0, 1 -> two normals, words 2, 3 -> the third
          uint32_t w[4];
          philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_NOISE | (uint32_t)n, k0, k1, w);
          const float r0 = sqrtf(-2.0f * logf(u24_open(w[0]))), r1 = sqrtf(-2.0f * logf(u24_open(w[2])));
          float s0, q0, s1, q1;
          sincosf(6.28318530717958647692f * u24(w[1]), &s0, &q0);
          sincosf(6.28318530717958647692f * u24(w[3]), &s1, &q1);
          g0 = r0 * q0; g1 = r0 * s0; g2 = r1 * q1;
        }
        x += fminf(fmaxf(a.sigma * g0, -a.clip), a.clip);
        y += fminf(fmaxf(a.sigma * g1, -a.clip), a.clip);
        z += fminf(fmaxf(a.sigma * g2, -a.clip), a.clip);
      }
      if (a.stages & SUG_PREP_SCALE) {
        const float sc = s_aug[0];
        x *= sc; y *= sc; z *= sc;
      }
      if (a.stages & SUG_PREP_PERTURB) {        // p . R, as the pre-rotation
        const float u = (x * s_aug[1] + y * s_aug[4]) + z * s_aug[7], v = (x * s_aug[2] + y * s_aug[5]) + z * s_aug[8],
                    w = (x * s_aug[3] + y * s_aug[6]) + z * s_aug[9];
        x = u; y = v; z = w;
      }
      if (a.stages & SUG_PREP_SHIFT) { x += s_aug[10]; y += s_aug[11]; z += s_aug[12]; }
    }
    ob[n] = x; ob[N + n] = y; ob[2 * N + n] = z;              // [3, N]: coalesced along N
    if (a.sel_out) a.sel_out[(int64_t)b * N + n] = src;
    if (a.noise_out) {
      float* no = a.noise_out + ((int64_t)b * N + n) * 3;
      no[0] = g0; no[1] = g1; no[2] = g2;
    }
  }
}

// ---- sug_prepare_seg_batch: the part-segmentation batch (points with extra channels, per-point labels, category) ----------
struct SegArgs {
  PrepArgs p;                   // prepare_batch_kernel's fields; out is [B, 3 + E, N]; P2 and sort are decided in the kernel
  const float* extra;           // [M, P, E] or null (E == 0)
  const uint8_t* point_label;   // [M, P]
  const int64_t* category;      // [M] or null
  const int32_t* lengths;       // [M] or null: every cloud has P points
  int64_t* label_out;           // [B, N]
  int64_t* category_out;        // [B] or null
  int E;
};

// three standard normals from one Philox block: words 0, 1 -> two, words 2, 3 -> the third (the jitter's Box-Muller)
__device__ __forceinline__ void box_muller3(const uint32_t w[4], float& g0, float& g1, float& g2) {
  const float r0 = sqrtf(-2.0f * logf(u24_open(w[0]))), r1 = sqrtf(-2.0f * logf(u24_open(w[2])));
  float s0, q0, s1, q1;
  sincosf(6.28318530717958647692f * u24(w[1]), &s0, &q0);
  sincosf(6.28318530717958647692f * u24(w[3]), &s1, &q1);
  g0 = r0 * q0; g1 = r0 * s0; g2 = r1 * q1;
}

// The per-cloud draws of the scale, perturbation and shift stages, by one lane, into s_aug[13] (the scale, the matrix
// row-major, the shift) and the debug outputs: prepare_batch_kernel's block, operation for operation.
__device__ __forceinline__ void seg_cloud_draws(const PrepArgs& a, int b, uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1,
                                                float* s_aug) {
  float sc = 1.0f, g[3] = {0.0f, 0.0f, 0.0f}, sh[3] = {0.0f, 0.0f, 0.0f};
  if (a.stages & SUG_PREP_SCALE) {
    if (a.scales) {
      sc = a.scales[b];
    } else {
      uint32_t w[4];
      philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_SCALE, k0, k1, w);
      sc = a.scale_low + u24(w[0]) * (a.scale_high - a.scale_low);
    }
  }
  if (a.stages & SUG_PREP_PERTURB) {
    if (a.perturb) {
      g[0] = a.perturb[3 * b + 0]; g[1] = a.perturb[3 * b + 1]; g[2] = a.perturb[3 * b + 2];
    } else {
      uint32_t w[4];
      philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_PERTURB, k0, k1, w);
      box_muller3(w, g[0], g[1], g[2]);
    }
    // R = Rz (Ry Rx) of rotate_perturbation_point_cloud, formed in fp64 from the fp32 normals and rounded once
    const double lim = (double)a.angle_clip;
    double sx, cx, sy, cy, sz, cz;
    sincos(fmin(fmax((double)a.angle_sigma * (double)g[0], -lim), lim), &sx, &cx);
    sincos(fmin(fmax((double)a.angle_sigma * (double)g[1], -lim), lim), &sy, &cy);
    sincos(fmin(fmax((double)a.angle_sigma * (double)g[2], -lim), lim), &sz, &cz);
    const double m0[3] = {cy, sy * sx, sy * cx}, m1[3] = {0.0, cx, -sx}, m2[3] = {-sy, cy * sx, cy * cx};   // Ry Rx
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      s_aug[1 + j] = (float)(cz * m0[j] - sz * m1[j]);
      s_aug[4 + j] = (float)(sz * m0[j] + cz * m1[j]);
      s_aug[7 + j] = (float)m2[j];
    }
  }
  if (a.stages & SUG_PREP_SHIFT) {
    if (a.shifts) {
      sh[0] = a.shifts[3 * b + 0]; sh[1] = a.shifts[3 * b + 1]; sh[2] = a.shifts[3 * b + 2];
    } else {
      uint32_t w[4];
      philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_SHIFT, k0, k1, w);
#pragma unroll
      for (int j = 0; j < 3; ++j) sh[j] = (2.0f * u24(w[j]) - 1.0f) * a.shift_range;
    }
  }
  s_aug[0] = sc; s_aug[10] = sh[0]; s_aug[11] = sh[1]; s_aug[12] = sh[2];
  if (a.scales_out) a.scales_out[b] = sc;
  if (a.perturb_out) { a.perturb_out[3 * b + 0] = g[0]; a.perturb_out[3 * b + 1] = g[1]; a.perturb_out[3 * b + 2] = g[2]; }
  if (a.shifts_out) { a.shifts_out[3 * b + 0] = sh[0]; a.shifts_out[3 * b + 1] = sh[1]; a.shifts_out[3 * b + 2] = sh[2]; }
}

// One workgroup per cloud, as prepare_batch_kernel, on the cloud's first L = lengths[idx[b]] points.  Whether the cloud sorts
// (L > N, or SUG_PREP_SHUFFLE) and how many slots (the power of two >= max(L, 128)) is decided here from L, uniformly over
// the workgroup: the host sizes the LDS for P and never waits for a length.  Only xyz and the keys are staged; the extra
// channels and the labels are gathered from HBM by the source index in the output loop.
__global__ __launch_bounds__(1024) void prepare_seg_batch_kernel(const SegArgs s) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const PrepArgs& a = s.p;
  float* s_xyz = reinterpret_cast<float*>(s_raw);                                            // [P, 3], L rows filled
  unsigned long long* s_key = reinterpret_cast<unsigned long long*>(s_raw + (((size_t)a.P * 12 + 15) & ~(size_t)15));  // [P2(P)], no sel
  __shared__ double s_sum[PREP_MAX_WAVES][3];
  __shared__ float s_max[PREP_MAX_WAVES];
  __shared__ float s_aug[13];

  const int b = blockIdx.x, t = threadIdx.x, T = blockDim.x;
  const int lane = t & (WAVE - 1), wv = t / WAVE, nw = T / WAVE;
  const int P = a.P, N = a.N, E = s.E, C = 3 + s.E;
  float* ob = a.out + (int64_t)b * C * N;
  int64_t* lb = s.label_out + (int64_t)b * N;
  const int ci = a.idx[b];
  int L = 0;
  if (ci >= 0 && ci < a.M) L = s.lengths ? s.lengths[ci] : P;
  if (L < 1 || L > P) {
    // an index outside the dataset or a length outside [1, P]: never read there; the cloud is NaN, its labels and its category
    // -1, the debug outputs those of a launch with every stage off (uniform over the block)
    for (int i = t; i < C * N; i += T) ob[i] = NAN;
    for (int n = t; n < N; n += T) {
      lb[n] = -1;
      if (a.sel_out) a.sel_out[(int64_t)b * N + n] = -1;
      if (a.noise_out) {
        float* no = a.noise_out + ((int64_t)b * N + n) * 3;
        no[0] = 0.0f; no[1] = 0.0f; no[2] = 0.0f;
      }
    }
    if (t == 0) {
      if (s.category_out) s.category_out[b] = -1;
      if (a.angles_out) a.angles_out[b] = 0.0f;
      if (a.scales_out) a.scales_out[b] = 1.0f;
      if (a.perturb_out) { a.perturb_out[3 * b + 0] = 0.0f; a.perturb_out[3 * b + 1] = 0.0f; a.perturb_out[3 * b + 2] = 0.0f; }
      if (a.shifts_out) { a.shifts_out[3 * b + 0] = 0.0f; a.shifts_out[3 * b + 1] = 0.0f; a.shifts_out[3 * b + 2] = 0.0f; }
    }
    return;
  }
  const float* pb = a.pts + (int64_t)ci * P * 3;
  for (int i = t; i < 3 * L; i += T) s_xyz[i] = pb[i];

  uint32_t c0 = 0, c1 = 0;
  if (a.counter) {
    const uint64_t c = *a.counter;
    c0 = (uint32_t)c; c1 = (uint32_t)(c >> 32);
  }
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  if (t == 0) {
    if ((a.stages & PREP_AUG_STAGES) || a.scales_out || a.perturb_out || a.shifts_out) seg_cloud_draws(a, b, c0, c1, k0, k1, s_aug);
    if (s.category_out) s.category_out[b] = s.category[ci];
  }
  const bool sort = !a.sel && (L > N || (a.stages & SUG_PREP_SHUFFLE));
  int P2 = 128;                         // sort slots: a power of two, whole 128-slot chunks
  while (P2 < L) P2 <<= 1;
  if (sort) {                           // subset keys: Philox block q -> points 4q .. 4q+3; past L: last in the order
    for (int q = t; q < P2 / 4; q += T) {
      uint32_t w[4];
      philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_SUBSET | (uint32_t)q, k0, k1, w);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = 4 * q + j;
        s_key[p] = p < L ? ((unsigned long long)w[j] << 32) | (unsigned)p : ~0ull;
      }
    }
  }
  __syncthreads();

  float den = 1.0f;
  if (a.stages & SUG_PREP_NORMALIZE) {
    // prepare_batch_kernel's normal_pc with L in place of P: the same partial sums in the same order
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int p = t; p < L; p += T) {
      sx += (double)s_xyz[3 * p + 0]; sy += (double)s_xyz[3 * p + 1]; sz += (double)s_xyz[3 * p + 2];
    }
    sx = wave_sum_d(sx); sy = wave_sum_d(sy); sz = wave_sum_d(sz);
    if (lane == 0) { s_sum[wv][0] = sx; s_sum[wv][1] = sy; s_sum[wv][2] = sz; }
    __syncthreads();
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int w = 0; w < nw; ++w) { mx += s_sum[w][0]; my += s_sum[w][1]; mz += s_sum[w][2]; }
    mx /= (double)L; my /= (double)L; mz /= (double)L;
    float m2 = 0.0f;
    for (int p = t; p < L; p += T) {
      const float x = (float)((double)s_xyz[3 * p + 0] - mx), y = (float)((double)s_xyz[3 * p + 1] - my),
                  z = (float)((double)s_xyz[3 * p + 2] - mz);
      s_xyz[3 * p + 0] = x; s_xyz[3 * p + 1] = y; s_xyz[3 * p + 2] = z;
      m2 = fmaxf(m2, sq3(x, y, z));
    }
    m2 = wave_max_f(m2);
    if (lane == 0) s_max[wv] = m2;
    __syncthreads();
    m2 = s_max[0];
    for (int w = 1; w < nw; ++w) m2 = fmaxf(m2, s_max[w]);
    den = sqrtf(m2);
  }

  if (sort) {                           // prepare_batch_kernel's bitonic sort, over this cloud's P2 slots
    const int chunks = P2 / 128;
    for (int k = 2; k <= P2; k <<= 1) {
      int j = k >> 1;
      for (; j > 64; j >>= 1) {
        for (int q = t; q < P2 / 2; q += T) sort_pair(s_key, ((q & ~(j - 1)) << 1) | (q & (j - 1)), j, k);
        __syncthreads();
      }
      for (int c = wv; c < chunks; c += nw) {
        for (int jj = j; jj > 0; jj >>= 1) {
          sort_pair(s_key, c * 128 + (((lane & ~(jj - 1)) << 1) | (lane & (jj - 1))), jj, k);
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      }
      if (k >= 128) __syncthreads();
    }
  }

  float ang = 0.0f, cs = 1.0f, sn = 0.0f;
  if (a.stages & SUG_PREP_ROTATE_Z) {
    if (a.angles) {
      ang = a.angles[b];
    } else {
      uint32_t w[4];
      philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_ANGLE, k0, k1, w);
      ang = u24(w[0]) * 6.28318530717958647692f;
    }
    sincosf(ang, &sn, &cs);
  }
  if (a.angles_out && t == 0) a.angles_out[b] = ang;

  const bool jit = (a.stages & SUG_PREP_JITTER) != 0, turn = (a.stages & SUG_PREP_NORMALS) != 0;
  const float* eb = E ? s.extra + (int64_t)ci * P * E : nullptr;
  const uint8_t* pl = s.point_label + (int64_t)ci * P;
  for (int n = t; n < N; n += T) {
    int src;
    if (a.sel) {
      src = a.sel[(int64_t)b * N + n];
    } else if (n < L) {
      src = sort ? (int)(unsigned)s_key[n] : n;
    } else {                                    // L <= N: row n is drawn with replacement, word (n - L) % 4 of block (n - L) / 4
      uint32_t w[4];
      const int f = n - L;
      philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_FILL | (uint32_t)(f >> 2), k0, k1, w);
      const int j = f & 3;
      src = (int)__umulhi(j == 0 ? w[0] : (j == 1 ? w[1] : (j == 2 ? w[2] : w[3])), (uint32_t)L);   // (word * L) >> 32
    }
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    if ((unsigned)src >= (unsigned)L) {         // a supplied index outside the cloud: the row is NaN, its label -1
      for (int c = 0; c < C; ++c) ob[(int64_t)c * N + n] = NAN;
      lb[n] = -1;
    } else {
      float x = s_xyz[3 * src + 0], y = s_xyz[3 * src + 1], z = s_xyz[3 * src + 2];
      if (a.stages & SUG_PREP_NORMALIZE) { x = x / den; y = y / den; z = z / den; }
      if (a.has_pre) {                          // x.dot(R): out_j = (x R_0j + y R_1j) + z R_2j
        const float u = (x * a.pre[0] + y * a.pre[3]) + z * a.pre[6], v = (x * a.pre[1] + y * a.pre[4]) + z * a.pre[7],
                    w = (x * a.pre[2] + y * a.pre[5]) + z * a.pre[8];
        x = u; y = v; z = w;
      }
      if (a.stages & SUG_PREP_ROTATE_Z) {
        const float u = x * cs + y * sn, v = y * cs - x * sn;
        x = u; y = v;
      }
      if (jit) {
        if (a.noise) {
          const float* nb = a.noise + ((int64_t)b * P + src) * 3;
          g0 = nb[0]; g1 = nb[1]; g2 = nb[2];
        } else {
          uint32_t w[4];
          philox4x32_10(c0, c1, (uint32_t)b, SUG_PREP_DRAW_NOISE | (uint32_t)n, k0, k1, w);
          box_muller3(w, g0, g1, g2);
        }
        x += fminf(fmaxf(a.sigma * g0, -a.clip), a.clip);
        y += fminf(fmaxf(a.sigma * g1, -a.clip), a.clip);
        z += fminf(fmaxf(a.sigma * g2, -a.clip), a.clip);
      }
      if (a.stages & SUG_PREP_SCALE) {
        const float sc = s_aug[0];
        x *= sc; y *= sc; z *= sc;
      }
      if (a.stages & SUG_PREP_PERTURB) {
        const float u = (x * s_aug[1] + y * s_aug[4]) + z * s_aug[7], v = (x * s_aug[2] + y * s_aug[5]) + z * s_aug[8],
                    w = (x * s_aug[3] + y * s_aug[6]) + z * s_aug[9];
        x = u; y = v; z = w;
      }
      if (a.stages & SUG_PREP_SHIFT) { x += s_aug[10]; y += s_aug[11]; z += s_aug[12]; }
      ob[n] = x; ob[N + n] = y; ob[2 * N + n] = z;            // [3 + E, N]: coalesced along N
      const float* er = eb + (int64_t)src * E;
      int e = 0;
      if (turn) {                               // a direction: the three rotations of the coordinates, nothing else
        float p = er[0], q = er[1], r = er[2];
        if (a.has_pre) {
          const float u = (p * a.pre[0] + q * a.pre[3]) + r * a.pre[6], v = (p * a.pre[1] + q * a.pre[4]) + r * a.pre[7],
                      w = (p * a.pre[2] + q * a.pre[5]) + r * a.pre[8];
          p = u; q = v; r = w;
        }
        if (a.stages & SUG_PREP_ROTATE_Z) {
          const float u = p * cs + q * sn, v = q * cs - p * sn;
          p = u; q = v;
        }
        if (a.stages & SUG_PREP_PERTURB) {
          const float u = (p * s_aug[1] + q * s_aug[4]) + r * s_aug[7], v = (p * s_aug[2] + q * s_aug[5]) + r * s_aug[8],
                      w = (p * s_aug[3] + q * s_aug[6]) + r * s_aug[9];
          p = u; q = v; r = w;
        }
        ob[3 * (int64_t)N + n] = p; ob[4 * (int64_t)N + n] = q; ob[5 * (int64_t)N + n] = r;
        e = 3;
      }
      for (; e < E; ++e) ob[(int64_t)(3 + e) * N + n] = er[e];
      lb[n] = (int64_t)pl[src];
    }
    if (a.sel_out) a.sel_out[(int64_t)b * N + n] = src;
    if (a.noise_out) {
      float* no = a.noise_out + ((int64_t)b * N + n) * 3;
      no[0] = g0; no[1] = g1; no[2] = g2;
    }
  }
}

}  // namespace

// The parameters of the scale, perturbation and shift stages from the host array `aug` into `a`, checked; all three
// launchers' rule.
static int prep_aug_params(const char* fn, int stages, const float* aug, PrepArgs& a) {
  a.scale_low = a.scale_high = 1.f; a.shift_range = a.angle_sigma = a.angle_clip = 0.f;
  if (stages & PREP_AUG_STAGES) {
    SUG_REQUIRE(aug, "%s: null aug_params: the scale, perturbation and shift stages need their %d parameters", fn,
                SUG_PREP_AUG_PARAMS);
    a.scale_low = aug[SUG_PREP_AUG_SCALE_LOW]; a.scale_high = aug[SUG_PREP_AUG_SCALE_HIGH];
    a.shift_range = aug[SUG_PREP_AUG_SHIFT_RANGE];
    a.angle_sigma = aug[SUG_PREP_AUG_ANGLE_SIGMA]; a.angle_clip = aug[SUG_PREP_AUG_ANGLE_CLIP];
    SUG_REQUIRE(std::isfinite(a.scale_low) && std::isfinite(a.scale_high) && a.scale_low > 0.f && a.scale_low <= a.scale_high,
                "%s: scale_low=%g, scale_high=%g: need finite 0 < scale_low <= scale_high", fn, a.scale_low, a.scale_high);
    SUG_REQUIRE(a.shift_range >= 0.f && std::isfinite(a.shift_range), "%s: shift_range=%g must be finite and not negative", fn,
                a.shift_range);
    SUG_REQUIRE(a.angle_sigma >= 0.f && std::isfinite(a.angle_sigma), "%s: angle_sigma=%g must be finite and not negative", fn,
                a.angle_sigma);
    SUG_REQUIRE(a.angle_clip >= 0.f && std::isfinite(a.angle_clip), "%s: angle_clip=%g must be finite and not negative", fn,
                a.angle_clip);
  }
  return SUG_OK;
}

// sort slots for P points (a power of two, whole 128-slot chunks) and the workgroup size: shared by the two kernels
static int prep_sort_slots(int P) {
  int P2 = 128;
  while (P2 < P) P2 <<= 1;
  return P2;
}
static int prep_threads(int P) { return P <= 256 ? 256 : (P <= 1024 ? 512 : 1024); }

// The checks and the launch of both entry points; `fn` names the caller in the messages, `known` are its stage bits.
static int prepare_launch(const char* fn, int known, const float* pts, int M, int P, const int32_t* idx, int B, int N, int stages,
                          const float* pre_rot, const float* angles, const float* noise, const int32_t* sel, const float* scales,
                          const float* perturb, const float* shifts, uint64_t seed, const uint64_t* counter, float sigma,
                          float clip, const float* aug, float* out, float* angles_out, float* noise_out, int32_t* sel_out,
                          float* scales_out, float* perturb_out, float* shifts_out, void* stream) {
  SUG_REQUIRE(pts && idx && out, "%s: null pointer (pts, idx and out are required)", fn);
  SUG_REQUIRE(B > 0, "%s: B=%d: an empty batch", fn, B);
  SUG_REQUIRE(M > 0 && P > 0 && N > 0, "%s: bad shape M=%d P=%d N=%d", fn, M, P, N);
  SUG_REQUIRE(P <= PREP_MAX_P, "%s: P=%d > %d points per cloud", fn, P, PREP_MAX_P);
  SUG_REQUIRE(2 * (int64_t)N <= 3 * (int64_t)P, "%s: too few points: N=%d > 1.5 * P=%d", fn, N, P);
  SUG_REQUIRE((stages & ~known) == 0, "%s: unknown bits in stages=%d", fn, stages);
  SUG_REQUIRE(!sel || N <= P, "%s: sel given but N=%d > P=%d (padding rows have no source point)", fn, N, P);
  const bool sort = !sel && (P > N || (P == N && (stages & SUG_PREP_SHUFFLE)));
  const bool draws = sort || ((stages & SUG_PREP_ROTATE_Z) && !angles) || ((stages & SUG_PREP_JITTER) && !noise) ||
                     ((stages & SUG_PREP_SCALE) && !scales) || ((stages & SUG_PREP_PERTURB) && !perturb) ||
                     ((stages & SUG_PREP_SHIFT) && !shifts);
  SUG_REQUIRE(!draws || counter, "%s: null counter: in-kernel draws need the device batch counter", fn);
  SUG_REQUIRE(sigma >= 0.f && clip >= 0.f, "%s: sigma and clip must not be negative", fn);
  PrepArgs a;
  if (int rc = prep_aug_params(fn, stages, aug, a)) return rc;
  a.pts = pts; a.idx = idx; a.angles = angles; a.noise = noise; a.sel = sel; a.counter = draws ? counter : nullptr;
  a.out = out; a.angles_out = angles_out; a.noise_out = noise_out; a.sel_out = sel_out;
  a.scales = scales; a.perturb = perturb; a.shifts = shifts;
  a.scales_out = scales_out; a.perturb_out = perturb_out; a.shifts_out = shifts_out;
  for (int i = 0; i < 9; ++i) a.pre[i] = pre_rot ? pre_rot[i] : (i % 4 == 0 ? 1.f : 0.f);
  a.seed = seed; a.M = M; a.P = P; a.N = N;
  const int P2 = prep_sort_slots(P);
  a.P2 = P2; a.stages = stages; a.has_pre = pre_rot != nullptr; a.sort = sort;
  a.sigma = sigma; a.clip = clip;
  const size_t sh = (((size_t)P * 12 + 15) & ~(size_t)15) + (sort ? (size_t)P2 * 8 : 0);
  if (sh > 64 * 1024) {
    static SugLdsOptIn note;
    if (int rc = sug_allow_dynamic_lds(note, &prepare_batch_kernel, 96 * 1024, fn)) return rc;
  }
  hipLaunchKernelGGL(prepare_batch_kernel, dim3(B), dim3(prep_threads(P)), sh, (hipStream_t)stream, a);
  SUG_LAUNCH_CHECK(fn);
  return SUG_OK;
}

extern "C" int sug_prepare_batch(const float* pts, int M, int P, const int32_t* idx, int B, int N, int stages,
                                 const float* pre_rot, const float* angles, const float* noise, const int32_t* sel,
                                 uint64_t seed, const uint64_t* counter, float sigma, float clip, float* out,
                                 float* angles_out, float* noise_out, int32_t* sel_out, void* stream) {
  return prepare_launch("sug_prepare_batch", SUG_PREP_NORMALIZE | SUG_PREP_ROTATE_Z | SUG_PREP_JITTER | SUG_PREP_SHUFFLE, pts, M, P,
                        idx, B, N, stages, pre_rot, angles, noise, sel, nullptr, nullptr, nullptr, seed, counter, sigma, clip,
                        nullptr, out, angles_out, noise_out, sel_out, nullptr, nullptr, nullptr, stream);
}

extern "C" int sug_prepare_batch_aug(const float* pts, int M, int P, const int32_t* idx, int B, int N, int stages,
                                     const float* pre_rot, const float* angles, const float* noise, const int32_t* sel,
                                     const float* scales, const float* perturb, const float* shifts, uint64_t seed,
                                     const uint64_t* counter, float sigma, float clip, const float* aug_params, float* out,
                                     float* angles_out, float* noise_out, int32_t* sel_out, float* scales_out,
                                     float* perturb_out, float* shifts_out, void* stream) {
  return prepare_launch("sug_prepare_batch_aug",
                        SUG_PREP_NORMALIZE | SUG_PREP_ROTATE_Z | SUG_PREP_JITTER | SUG_PREP_SHUFFLE | PREP_AUG_STAGES, pts, M, P, idx,
                        B, N, stages, pre_rot, angles, noise, sel, scales, perturb, shifts, seed, counter, sigma, clip, aug_params,
                        out, angles_out, noise_out, sel_out, scales_out, perturb_out, shifts_out, stream);
}

extern "C" int sug_prepare_seg_batch(const float* pts, const float* extra, const uint8_t* point_label, const int64_t* category,
                                     const int32_t* lengths, int M, int P, int E, const int32_t* idx, int B, int N, int stages,
                                     const float* pre_rot, const float* angles, const float* noise, const int32_t* sel,
                                     const float* scales, const float* perturb, const float* shifts, uint64_t seed,
                                     const uint64_t* counter, float sigma, float clip, const float* aug_params, float* out,
                                     int64_t* label_out, int64_t* category_out, float* angles_out, float* noise_out,
                                     int32_t* sel_out, float* scales_out, float* perturb_out, float* shifts_out, void* stream) {
  const char* fn = "sug_prepare_seg_batch";
  const int known = SUG_PREP_NORMALIZE | SUG_PREP_ROTATE_Z | SUG_PREP_JITTER | SUG_PREP_SHUFFLE | PREP_AUG_STAGES | SUG_PREP_NORMALS;
  SUG_REQUIRE(pts && idx && out && label_out && point_label,
              "%s: null pointer (pts, point_label, idx, out and label_out are required)", fn);
  SUG_REQUIRE(E >= 0 && E <= SUG_PREP_SEG_MAX_EXTRA, "%s: E=%d extra channels outside [0, %d]", fn, E, SUG_PREP_SEG_MAX_EXTRA);
  SUG_REQUIRE(E == 0 || extra, "%s: null extra with E=%d", fn, E);
  SUG_REQUIRE(!category_out || category, "%s: category_out given but category is null", fn);
  SUG_REQUIRE(B > 0, "%s: B=%d: an empty batch", fn, B);
  SUG_REQUIRE(M > 0 && P > 0 && N > 0, "%s: bad shape M=%d P=%d N=%d", fn, M, P, N);
  SUG_REQUIRE(P <= PREP_MAX_P, "%s: P=%d > %d points per cloud", fn, P, PREP_MAX_P);
  SUG_REQUIRE(N <= PREP_MAX_P, "%s: N=%d > %d output rows per cloud", fn, N, PREP_MAX_P);
  SUG_REQUIRE((stages & ~known) == 0, "%s: unknown bits in stages=%d", fn, stages);
  SUG_REQUIRE(!(stages & SUG_PREP_NORMALS) || E >= 3, "%s: SUG_PREP_NORMALS needs E >= 3 extra channels (E=%d)", fn, E);
  // without sel the subset keys or the fill rows are drawn, whichever the cloud's length asks for
  const bool draws = !sel || ((stages & SUG_PREP_ROTATE_Z) && !angles) || ((stages & SUG_PREP_JITTER) && !noise) ||
                     ((stages & SUG_PREP_SCALE) && !scales) || ((stages & SUG_PREP_PERTURB) && !perturb) ||
                     ((stages & SUG_PREP_SHIFT) && !shifts);
  SUG_REQUIRE(!draws || counter, "%s: null counter: in-kernel draws need the device batch counter", fn);
  SUG_REQUIRE(sigma >= 0.f && clip >= 0.f, "%s: sigma and clip must not be negative", fn);
  SegArgs s;
  PrepArgs& a = s.p;
  if (int rc = prep_aug_params(fn, stages, aug_params, a)) return rc;
  a.pts = pts; a.idx = idx; a.angles = angles; a.noise = noise; a.sel = sel; a.counter = draws ? counter : nullptr;
  a.out = out; a.angles_out = angles_out; a.noise_out = noise_out; a.sel_out = sel_out;
  a.scales = scales; a.perturb = perturb; a.shifts = shifts;
  a.scales_out = scales_out; a.perturb_out = perturb_out; a.shifts_out = shifts_out;
  for (int i = 0; i < 9; ++i) a.pre[i] = pre_rot ? pre_rot[i] : (i % 4 == 0 ? 1.f : 0.f);
  a.seed = seed; a.M = M; a.P = P; a.N = N;
  a.P2 = prep_sort_slots(P); a.sort = 0;        // not read: the kernel decides both from the cloud's length; P2 bounds the LDS
  a.stages = stages; a.has_pre = pre_rot != nullptr;
  a.sigma = sigma; a.clip = clip;
  s.extra = extra; s.point_label = point_label; s.category = category; s.lengths = lengths;
  s.label_out = label_out; s.category_out = category_out; s.E = E;
  const size_t sh = (((size_t)P * 12 + 15) & ~(size_t)15) + (sel ? 0 : (size_t)a.P2 * 8);
  if (sh > 64 * 1024) {
    static SugLdsOptIn note;
    if (int rc = sug_allow_dynamic_lds(note, &prepare_seg_batch_kernel, 96 * 1024, fn)) return rc;
  }
  hipLaunchKernelGGL(prepare_seg_batch_kernel, dim3(B), dim3(prep_threads(P)), sh, (hipStream_t)stream, s);
  SUG_LAUNCH_CHECK(fn);
  return SUG_OK;
}
