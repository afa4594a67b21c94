// The scalar tail of a SUG step (train_dg_single_gpu.py:269-292, :314-324) as two launches each way instead of ~25:
//   * cross entropy of BOTH classifier heads on the source rows of the paired logits:
//       loss_cls = w * (CE(pred_s1, label) + CE(pred_s2, label)),  CE = nn.CrossEntropyLoss() (mean over the batch),
//     w = 0.5 * SRC_LOSS_WEIGHT * CLS_WEIGHT folded on the host; forward: log-softmax + NLL + mean + weight in one
//     single-workgroup kernel (torch: 2 x log_softmax, 2 x nll_loss, add, mul); backward: w * g * (softmax - onehot) / M
//     for the source rows and ZEROS for the target rows of the paired [2B, C] logits, so that no torch.stack / zero fill
//     rebuilds the pair's gradient;
//   * total = loss_cls + wg * v_geo + ws * (v_sem1 + v_sem2) with the reported parts wg*v_geo and ws*(v_sem1+v_sem2)
//     (the five scalar launches of the loss sum and their backward).
// fp32, fixed summation order (one workgroup; rows summed by thread 0 in order).
#include "common.h"

namespace {
constexpr int CE_MAXC = SUG_CE_PAIR_MAX_CLASSES;    // classes
constexpr int CE_MAXROWS = SUG_CE_PAIR_MAX_ROWS;    // source rows x 2 heads

__global__ __launch_bounds__(512) void ce_pair_fwd_kernel(const float* __restrict__ l1, const float* __restrict__ l2, int64_t ld,
                                                          const int64_t* __restrict__ label, int M, int C, float w,
                                                          int64_t ignore_index, float* __restrict__ loss,
                                                          float* __restrict__ lse) {
  __shared__ float s_nll[CE_MAXROWS];
  const int t = threadIdx.x;
  if (t < 2 * M) {
    const int hd = t / M, i = t % M;
    const float* row = (hd ? l2 : l1) + (int64_t)i * ld;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, row[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(row[c] - mx);
    const float l = mx + logf(s);                    // logsumexp of the row
    lse[t] = l;
    // nn.CrossEntropyLoss semantics: a row whose label is `ignore_index` contributes nothing and does not count in the
    // mean; any other label outside [0, C) is an error -- torch raises (a device-side assert); a kernel cannot, so the row
    // poisons the loss with NaN instead of being scored as some class (round 4 clamped such labels silently)
    const int64_t y = label[i];
    s_nll[t] = (y == ignore_index) ? 0.f : ((y < 0 || y >= C) ? NAN : l - row[y]);       // -log_softmax(row)[y]
  }
  __syncthreads();
  if (t == 0) {
    float a = 0.f, b = 0.f;
    int cnt = 0;
    for (int i = 0; i < M; ++i) cnt += label[i] != ignore_index;
    for (int i = 0; i < M; ++i) a += s_nll[i];
    for (int i = 0; i < M; ++i) b += s_nll[M + i];
    lse[2 * M] = (float)cnt;                         // rows that count: the backward divides by it (0 rows -> NaN, as torch)
    loss[0] = w * (a / (float)cnt + b / (float)cnt);
  }
}

__global__ __launch_bounds__(256) void ce_pair_bwd_kernel(const float* __restrict__ l1, const float* __restrict__ l2, int64_t ld,
                                                          const int64_t* __restrict__ label, int M, int Mtot, int C, float w,
                                                          int64_t ignore_index, const float* __restrict__ g,
                                                          const float* __restrict__ lse, float* __restrict__ d1,
                                                          float* __restrict__ d2) {
  const int64_t n = (int64_t)2 * Mtot * C;
  const float f = w * g[0] / lse[2 * M];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int hd = (int)(e / ((int64_t)Mtot * C));
    const int r = (int)((e / C) % Mtot), c = (int)(e % C);
    float v = 0.f;
    if (r < M) {
      const float x = (hd ? l2 : l1)[(int64_t)r * ld + c];
      const int64_t y = label[r];
      v = (y == ignore_index) ? 0.f : ((y < 0 || y >= C) ? NAN : f * (expf(x - lse[hd * M + r]) - (c == y ? 1.f : 0.f)));
    }
    (hd ? d2 : d1)[(int64_t)r * C + c] = v;
  }
}

__global__ void loss_combine_fwd_kernel(const float* __restrict__ lcls, const float* __restrict__ v0, const float* __restrict__ v1,
                                        const float* __restrict__ v2, float wg, float ws, float* __restrict__ out) {
  if (threadIdx.x == 0) {
    const float geo = v0 ? wg * v0[0] : 0.f;
    const float sem = v1 ? ws * (v1[0] + (v2 ? v2[0] : 0.f)) : 0.f;
    float tot = lcls[0];
    if (v0) tot += geo;                              // (loss_cls + loss_geo) + loss_sem, the step's own order
    if (v1) tot += sem;
    out[0] = tot; out[1] = geo; out[2] = sem;
  }
}
__global__ void loss_combine_bwd_kernel(const float* __restrict__ g, float wg, float ws, float* __restrict__ out) {
  if (threadIdx.x == 0) {
    const float gv = g[0];
    out[0] = gv; out[1] = wg * gv; out[2] = ws * gv; out[3] = ws * gv;
  }
}
// ---- single-head cross entropy of the source-only loop (train_source.py:120, :130-131) ----------------------------------
// One workgroup of up to 16 waves: a WAVE per row, a LANE per class (C <= 64), so a row is one coalesced load and its max /
// sum are cross-lane reductions of one fixed shape (DPP max, xor butterfly); the rows' terms meet in LDS and wave 0 folds them
// in fp64 -- lane l takes rows l, l + 64, ... in order, then the butterfly -- an order that does not depend on the number of
// waves launched.  Thread 0 writes the loss and keeps the epoch's books (plain fp64 read-modify-write: one workgroup, stream
// order).
constexpr int CE1_MAXC = SUG_CE_MAX_CLASSES;
constexpr int CE1_MAXROWS = SUG_CE_MAX_ROWS;

__global__ __launch_bounds__(1024) void ce_fwd_kernel(const float* __restrict__ logits, int64_t ld,
                                                      const int64_t* __restrict__ label, int M, int C, int64_t ignore_index,
                                                      float eps, float* __restrict__ loss, float* __restrict__ lse,
                                                      double* __restrict__ totals) {
  __shared__ float s_term[CE1_MAXROWS];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, nwave = blockDim.x / WAVE;
  for (int r = wave; r < M; r += nwave) {                 // wave-uniform trip count
    const float* row = logits + (int64_t)r * ld;
    const bool in = lane < C;
    const float z = in ? row[lane] : -INFINITY;
    const float mx = wave_max_f(z);
    const float l = mx + logf(wave_sum_f(in ? expf(z - mx) : 0.f));     // logsumexp of the row
    // label contract of sug_ce_pair_fwd: ignore_index rows count for nothing, any other label outside [0, C) poisons the loss
    const int64_t y = label[r];
    float term = 0.f;
    if (y != ignore_index) {
      term = (y < 0 || y >= C) ? NAN : l - row[y];                      // -log_softmax(row)[y]
      if (eps > 0.f) term = (1.f - eps) * term + (eps / (float)C) * wave_sum_f(in ? l - z : 0.f);
    }
    if (lane == 0) {
      lse[r] = l;
      s_term[r] = term;
    }
  }
  __syncthreads();
  if (wave == 0) {
    double a = 0.0;
    int cnt = 0;
    for (int i = lane; i < M; i += WAVE) {
      a += (double)s_term[i];
      cnt += label[i] != ignore_index;
    }
    a = wave_sum_d(a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) {
      const float v = (float)(a / (double)cnt);           // no row counts -> 0 / 0 = NaN, as torch
      lse[M] = (float)cnt;                                // the backward divides by it
      loss[0] = v;
      if (totals) {                                       // loss_total += loss.item() * data.size(0); data_total += data.size(0)
        totals[0] += (double)v * (double)M;
        totals[1] += (double)M;
      }
    }
  }
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ label,
                                                     int M, int C, int64_t ignore_index, float eps, const float* __restrict__ g,
                                                     const float* __restrict__ lse, float* __restrict__ d) {
  const int n = M * C;                                    // <= 65536
  const float f = g[0] / lse[M], on = 1.f - eps + eps / (float)C, off = eps / (float)C;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    const int r = e / C, c = e - r * C;
    const int64_t y = label[r];
    float v = 0.f;
    if (y != ignore_index)
      v = (y < 0 || y >= C) ? NAN : f * (expf(logits[(int64_t)r * ld + c] - lse[r]) - (c == y ? on : off));
    d[e] = v;
  }
}
// ---- phase-1 loss of the two-phase UDA step (train_uda.py:149-160, train_dg_naive_mmd.py:225-241) ------------------------
//   loss = a_s * (CE(ys1) + CE(ys2)) + a_t * (CE(yt1) + CE(yt2)) - mean |softmax(yt1) - softmax(yt2)|
// in one launch each way instead of ~30.  The shape of ce_fwd_kernel: one workgroup, a WAVE per row, a LANE per class
// (C <= 64); a row of both heads is two coalesced loads, its max / sums are cross-lane reductions of one fixed shape; the
// rows' terms meet in LDS and wave 0 folds them in fp64 -- lane l takes rows l, l + 64, ... in order, then the butterfly -- an
// order that does not depend on the number of waves launched.  Thread 0 writes the four scalars and keeps the epoch's books
// (plain fp64 read-modify-write: one workgroup, stream order).  Labels outside [0, C) poison the loss with NaN.
constexpr int MCD_MAXROWS = SUG_MCD_MAX_ROWS;

__device__ __forceinline__ float row_lse(float z, bool in) {
  const float mx = wave_max_f(z);
  return mx + logf(wave_sum_f(in ? expf(z - mx) : 0.f));
}

__global__ __launch_bounds__(1024) void mcd_loss_fwd_kernel(const float* __restrict__ ys1, const float* __restrict__ ys2,
                                                            const float* __restrict__ yt1, const float* __restrict__ yt2, int64_t ld,
                                                            const int64_t* __restrict__ label, const int64_t* __restrict__ label_t,
                                                            int Ms, int Mt, int C, float a_s, float a_t, float r_s,
                                                            float* __restrict__ out, float* __restrict__ lse,
                                                            double* __restrict__ totals) {
  __shared__ float s_ces[MCD_MAXROWS], s_cet[MCD_MAXROWS], s_dis[MCD_MAXROWS];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, nwave = blockDim.x / WAVE;
  const bool in = lane < C;
  for (int r = wave; r < Ms; r += nwave) {                // source rows: the cross entropy of both heads (wave-uniform trips)
    const float *r1 = ys1 + (int64_t)r * ld, *r2 = ys2 + (int64_t)r * ld;
    const float l1 = row_lse(in ? r1[lane] : -INFINITY, in), l2 = row_lse(in ? r2[lane] : -INFINITY, in);
    if (lane == 0) {
      const int64_t y = label[r];
      lse[r] = l1;
      lse[Ms + r] = l2;
      s_ces[r] = (y < 0 || y >= C) ? NAN : (l1 - r1[y]) + (l2 - r2[y]);
    }
  }
  for (int r = wave; r < Mt; r += nwave) {                // target rows: the discrepancy, and the cross entropy when a_t != 0
    const float *r1 = yt1 + (int64_t)r * ld, *r2 = yt2 + (int64_t)r * ld;
    const float z1 = in ? r1[lane] : -INFINITY, z2 = in ? r2[lane] : -INFINITY;
    const float l1 = row_lse(z1, in), l2 = row_lse(z2, in);
    const float d = wave_sum_f(in ? fabsf(expf(z1 - l1) - expf(z2 - l2)) : 0.f);
    if (lane == 0) {
      lse[2 * Ms + r] = l1;
      lse[2 * Ms + Mt + r] = l2;
      s_dis[r] = d;
      float t = 0.f;
      if (a_t != 0.f) {
        const int64_t y = label_t[r];
        t = (y < 0 || y >= C) ? NAN : (l1 - r1[y]) + (l2 - r2[y]);
      }
      s_cet[r] = t;
    }
  }
  __syncthreads();
  if (wave == 0) {
    double a = 0.0, b = 0.0, d = 0.0;
    for (int i = lane; i < Ms; i += WAVE) a += (double)s_ces[i];
    for (int i = lane; i < Mt; i += WAVE) {
      b += (double)s_cet[i];
      d += (double)s_dis[i];
    }
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    d = wave_sum_d(d);
    if (lane == 0) {
      const float ces = (float)(a / (double)Ms), cet = (float)(b / (double)Mt);
      const float adv = -(float)(d / ((double)Mt * (double)C));
      float loss = a_s * ces + adv;                       // args.weight * loss_s + loss_adv (+ 0.5 * TARGET_LOSS * loss_t)
      const float lt = a_t != 0.f ? a_t * cet : 0.f;
      if (a_t != 0.f) loss += lt;
      const float ls = r_s * ces;
      out[0] = loss; out[1] = ls; out[2] = adv; out[3] = lt;
      if (totals) {                                       // train_uda.py:180-184
        totals[0] += (double)ls * (double)Ms;
        totals[1] += (double)adv * (double)Ms;
        totals[2] += (double)Ms;
        totals[3] += (double)Mt;
      }
    }
  }
}

// A wave per row of the Ms + Mt rows (source rows first), a lane per class; the four gradient blocks are dense [rows, C].
__global__ __launch_bounds__(256) void mcd_loss_bwd_kernel(const float* __restrict__ ys1, const float* __restrict__ ys2,
                                                           const float* __restrict__ yt1, const float* __restrict__ yt2, int64_t ld,
                                                           const int64_t* __restrict__ label, const int64_t* __restrict__ label_t,
                                                           int Ms, int Mt, int C, float a_s, float a_t, const float* __restrict__ g,
                                                           const float* __restrict__ lse, float* __restrict__ ds1,
                                                           float* __restrict__ ds2, float* __restrict__ dt1, float* __restrict__ dt2) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int R = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;      // wave-uniform
  if (R >= Ms + Mt) return;
  const bool in = lane < C;
  const float gv = g[0];
  if (R < Ms) {
    const int64_t o = (int64_t)R * ld + lane, y = label[R];
    const float f = gv * a_s / (float)Ms;
    const bool bad = y < 0 || y >= C;
    if (in) {
      const float hot = lane == y ? 1.f : 0.f;
      ds1[(int64_t)R * C + lane] = bad ? NAN : f * (expf(ys1[o] - lse[R]) - hot);
      ds2[(int64_t)R * C + lane] = bad ? NAN : f * (expf(ys2[o] - lse[Ms + R]) - hot);
    }
    return;
  }
  const int r = R - Ms;
  const int64_t o = (int64_t)r * ld + lane;
  const float p1 = in ? expf(yt1[o] - lse[2 * Ms + r]) : 0.f, p2 = in ? expf(yt2[o] - lse[2 * Ms + Mt + r]) : 0.f;
  const float df = p1 - p2;
  const float s = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);                 // sign(0) = 0, as the backward of torch.abs
  // s_j - <s,p> written as sum_c p_c (s_j - s_c) (sum_c p_c = 1): for s_j = +-1 every term has one sign, so a class whose
  // probability is close to 1 does not lose its factor 1 - p_j to cancellation.  With P+ / P0 / P- the probability mass of the
  // classes with s = +1 / 0 / -1:  s_j = +1 -> P0 + 2 P-,  s_j = -1 -> -(P0 + 2 P+),  s_j = 0 -> P- - P+.
  const float up1 = wave_sum_f(s > 0.f ? p1 : 0.f), eq1 = wave_sum_f(s == 0.f ? p1 : 0.f), dn1 = wave_sum_f(s < 0.f ? p1 : 0.f);
  const float up2 = wave_sum_f(s > 0.f ? p2 : 0.f), eq2 = wave_sum_f(s == 0.f ? p2 : 0.f), dn2 = wave_sum_f(s < 0.f ? p2 : 0.f);
  const float t1 = s > 0.f ? eq1 + 2.f * dn1 : (s < 0.f ? -(eq1 + 2.f * up1) : dn1 - up1);
  const float t2 = s > 0.f ? eq2 + 2.f * dn2 : (s < 0.f ? -(eq2 + 2.f * up2) : dn2 - up2);
  const float k = gv / ((float)Mt * (float)C);
  float v1 = -k * (p1 * t1), v2 = k * (p2 * t2);
  if (a_t != 0.f) {
    const int64_t y = label_t[r];
    const float f = gv * a_t / (float)Mt, hot = lane == y ? 1.f : 0.f;
    const bool bad = y < 0 || y >= C;
    v1 = bad ? NAN : v1 + f * (p1 - hot);
    v2 = bad ? NAN : v2 + f * (p2 - hot);
  }
  if (in) {
    dt1[(int64_t)r * C + lane] = v1;
    dt2[(int64_t)r * C + lane] = v2;
  }
}
// ---- classification loss of the shipped configurations (train_dg_single_gpu.py:163-180, :269-292; train_dg_naive_mmd.py:156-165,
// :225-241): focal / class-weighted loss of both heads on source and target rows and the heads' discrepancy ---------------------
//   L(z, y) = alpha[y] * m(q) * (-log p_y),  p = softmax(z),  q = 1 - p_y,  m(q) = 1 (gamma == 0) or q^gamma
//   loss = a_s * (R(L(ys1)) + R(L(ys2))) + a_t * (R(L(yt1)) + R(L(yt2))) - a_d * mean |softmax(yt1) - softmax(yt2)|
// (R: mean over the rows, or their sum) in one launch each way.  The shape of mcd_loss_fwd_kernel: one workgroup, a WAVE per row,
// a LANE per class; the rows' terms meet in LDS, wave 0 folds them in fp64 in one fixed order, thread 0 writes the four scalars and
// keeps the books.  Numerics: p = exp(z - max) / sum; q is the SUM OF THE OTHER classes' probabilities (1 - p_y cancels once
// p_y rounds to 1, which is the normal state of a trained row); log p_y = (z_y - max) - log(sum).  alpha == null: alpha = 1, and
// with gamma == 0 that is nn.CrossEntropyLoss, ignore_index honoured as ce_pair_fwd_kernel does (`ign`).
struct ClsRow {
  float mx, sum, e, q, logp;       // row max, sum of exp(z - max), this lane's exp(z - max), 1 - p_y, log p_y
};

__device__ __forceinline__ ClsRow cls_row(float z, bool in, int lane, int yi) {
  ClsRow r;
  r.mx = wave_max_f(z);
  r.e = in ? expf(z - r.mx) : 0.f;
  r.sum = wave_sum_f(r.e);
  r.q = wave_sum_f(lane != yi ? r.e : 0.f) / r.sum;
  r.logp = (__shfl(z, yi) - r.mx) - logf(r.sum);
  return r;
}
__device__ __forceinline__ ClsRow cls_row_saved(float z, bool in, int lane, int yi, float mx, float sum) {
  ClsRow r;
  r.mx = mx;
  r.sum = sum;
  r.e = in ? expf(z - mx) : 0.f;
  r.q = wave_sum_f(lane != yi ? r.e : 0.f) / sum;
  r.logp = (__shfl(z, yi) - mx) - logf(sum);
  return r;
}
__device__ __forceinline__ float cls_term(const ClsRow& r, float gamma) {
  return (gamma == 0.f ? 1.f : powf(r.q, gamma)) * (-r.logp);
}
// d L / d z_j over alpha_y: [m(q) - gamma q^(gamma-1) p_y log p_y] * (p_j - delta_jy), with p_y - 1 = -q; the second term is
// dropped for gamma == 0 (torch's pow backward returns zero for exponent 0)
__device__ __forceinline__ float cls_grad(const ClsRow& r, float gamma, int lane, int yi) {
  float c = 1.f;
  if (gamma != 0.f) c = powf(r.q, gamma - 1.f) * (r.q - gamma * (__shfl(r.e, yi) / r.sum) * r.logp);
  return c * (lane == yi ? -r.q : r.e / r.sum);
}

// save: [2R] floats for the R = 2*Ms + 2*Mt rows in the order ys1, ys2, yt1, yt2 -- the rows' max, then their sums -- and the two
// divisors of the reduction (source, target) behind them.
__global__ __launch_bounds__(1024) void cls_loss_fwd_kernel(const float* __restrict__ ys1, const float* __restrict__ ys2,
                                                            const float* __restrict__ yt1, const float* __restrict__ yt2, int64_t ld,
                                                            const int64_t* __restrict__ label, const int64_t* __restrict__ label_t,
                                                            int Ms, int Mt, int C, const float* __restrict__ alpha, float gamma,
                                                            int reduce_sum, int ign, int64_t ignore_index, float a_s, float a_t,
                                                            float a_d, float r_s, float* __restrict__ out, float* __restrict__ save,
                                                            double* __restrict__ totals) {
  __shared__ float s_ls[MCD_MAXROWS], s_lt[MCD_MAXROWS], s_dis[MCD_MAXROWS];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, nwave = blockDim.x / WAVE;
  const bool in = lane < C;
  const int R = 2 * Ms + 2 * Mt;
  const bool target = a_t != 0.f || a_d != 0.f;
  for (int r = wave; r < Ms; r += nwave) {                // source rows (wave-uniform trips)
    const int64_t y = label[r];
    const bool skip = ign && y == ignore_index, bad = !skip && (y < 0 || y >= C);
    const int yi = (skip || bad) ? 0 : (int)y;
    const ClsRow r1 = cls_row(in ? ys1[(int64_t)r * ld + lane] : -INFINITY, in, lane, yi);
    const ClsRow r2 = cls_row(in ? ys2[(int64_t)r * ld + lane] : -INFINITY, in, lane, yi);
    if (lane == 0) {
      save[r] = r1.mx;
      save[Ms + r] = r2.mx;
      save[R + r] = r1.sum;
      save[R + Ms + r] = r2.sum;
      float t = 0.f;
      if (!skip) t = bad ? NAN : (alpha ? alpha[yi] : 1.f) * (cls_term(r1, gamma) + cls_term(r2, gamma));
      s_ls[r] = t;
    }
  }
  for (int r = wave; r < Mt && target; r += nwave) {      // target rows: the discrepancy, and the loss when a_t != 0
    const int64_t y = a_t != 0.f ? label_t[r] : 0;
    const bool skip = a_t == 0.f || (ign && y == ignore_index), bad = !skip && (y < 0 || y >= C);
    const int yi = (skip || bad) ? 0 : (int)y;
    const ClsRow r1 = cls_row(in ? yt1[(int64_t)r * ld + lane] : -INFINITY, in, lane, yi);
    const ClsRow r2 = cls_row(in ? yt2[(int64_t)r * ld + lane] : -INFINITY, in, lane, yi);
    const float d = wave_sum_f(in ? fabsf(r1.e / r1.sum - r2.e / r2.sum) : 0.f);
    if (lane == 0) {
      save[2 * Ms + r] = r1.mx;
      save[2 * Ms + Mt + r] = r2.mx;
      save[R + 2 * Ms + r] = r1.sum;
      save[R + 2 * Ms + Mt + r] = r2.sum;
      s_dis[r] = d;
      float t = 0.f;
      if (!skip) t = bad ? NAN : (alpha ? alpha[yi] : 1.f) * (cls_term(r1, gamma) + cls_term(r2, gamma));
      s_lt[r] = t;
    }
  }
  __syncthreads();
  if (wave == 0) {
    double a = 0.0, b = 0.0, d = 0.0;
    int cs = 0, ct = 0;
    for (int i = lane; i < Ms; i += WAVE) {
      a += (double)s_ls[i];
      cs += !(ign && label[i] == ignore_index);
    }
    for (int i = lane; i < Mt && target; i += WAVE) {
      b += (double)s_lt[i];
      d += (double)s_dis[i];
      ct += !(ign && a_t != 0.f && label_t[i] == ignore_index);
    }
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    d = wave_sum_d(d);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cs += __shfl_xor(cs, o);
      ct += __shfl_xor(ct, o);
    }
    if (lane == 0) {
      const float ds = reduce_sum ? 1.f : (float)cs, dt = reduce_sum ? 1.f : (float)ct;   // no row counts -> 0 / 0 = NaN, as torch
      save[2 * R] = ds;
      save[2 * R + 1] = dt;
      const float Ls = (float)(a / (double)ds);
      const float lt = a_t != 0.f ? a_t * (float)(b / (double)dt) : 0.f;
      const float adv = a_d != 0.f ? -(a_d * (float)(d / ((double)Mt * (double)C))) : 0.f;
      float loss = a_s * Ls;
      if (a_t != 0.f) loss += lt;
      if (a_d != 0.f) loss += adv;
      const float ls = r_s * Ls;
      out[0] = loss; out[1] = ls; out[2] = adv; out[3] = lt;
      if (totals) {                                       // train_uda.py:180-184
        totals[0] += (double)ls * (double)Ms;
        totals[1] += (double)adv * (double)Ms;
        totals[2] += (double)Ms;
        totals[3] += (double)Mt;
      }
    }
  }
}

// A wave per row of the Ms + Mt rows (source rows first), a lane per class; the four gradient blocks are dense [rows, C].
__global__ __launch_bounds__(256) void cls_loss_bwd_kernel(const float* __restrict__ ys1, const float* __restrict__ ys2,
                                                           const float* __restrict__ yt1, const float* __restrict__ yt2, int64_t ld,
                                                           const int64_t* __restrict__ label, const int64_t* __restrict__ label_t,
                                                           int Ms, int Mt, int C, const float* __restrict__ alpha, float gamma,
                                                           int ign, int64_t ignore_index, float a_s, float a_t, float a_d,
                                                           const float* __restrict__ g, const float* __restrict__ save,
                                                           float* __restrict__ ds1, float* __restrict__ ds2, float* __restrict__ dt1,
                                                           float* __restrict__ dt2) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int row = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;    // wave-uniform
  if (row >= Ms + Mt) return;
  const bool in = lane < C;
  const int R = 2 * Ms + 2 * Mt;
  const float gv = g[0];
  if (row < Ms) {
    const int64_t y = label[row];
    const bool skip = ign && y == ignore_index, bad = !skip && (y < 0 || y >= C);
    const int yi = (skip || bad) ? 0 : (int)y;
    const int64_t o = (int64_t)row * ld + lane;
    const ClsRow r1 = cls_row_saved(in ? ys1[o] : -INFINITY, in, lane, yi, save[row], save[R + row]);
    const ClsRow r2 = cls_row_saved(in ? ys2[o] : -INFINITY, in, lane, yi, save[Ms + row], save[R + Ms + row]);
    const float f = gv * a_s / save[2 * R] * (alpha ? alpha[yi] : 1.f);
    float v1 = f * cls_grad(r1, gamma, lane, yi), v2 = f * cls_grad(r2, gamma, lane, yi);
    if (skip) v1 = v2 = 0.f;
    if (bad) v1 = v2 = NAN;
    if (in) {
      ds1[(int64_t)row * C + lane] = v1;
      ds2[(int64_t)row * C + lane] = v2;
    }
    return;
  }
  const int r = row - Ms;
  if (a_t == 0.f && a_d == 0.f) {                         // the target rows were not read: exact zeros
    if (in) dt1[(int64_t)r * C + lane] = dt2[(int64_t)r * C + lane] = 0.f;
    return;
  }
  const int64_t y = a_t != 0.f ? label_t[r] : 0;
  const bool skip = a_t == 0.f || (ign && y == ignore_index), bad = !skip && (y < 0 || y >= C);
  const int yi = (skip || bad) ? 0 : (int)y;
  const int64_t o = (int64_t)r * ld + lane;
  const ClsRow r1 = cls_row_saved(in ? yt1[o] : -INFINITY, in, lane, yi, save[2 * Ms + r], save[R + 2 * Ms + r]);
  const ClsRow r2 = cls_row_saved(in ? yt2[o] : -INFINITY, in, lane, yi, save[2 * Ms + Mt + r], save[R + 2 * Ms + Mt + r]);
  float v1 = 0.f, v2 = 0.f;
  if (a_d != 0.f) {                                       // mcd_loss_bwd_kernel's form, scaled by a_d
    const float p1 = r1.e / r1.sum, p2 = r2.e / r2.sum;
    const float df = p1 - p2;
    const float s = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);               // sign(0) = 0, as the backward of torch.abs
    // s_j - <s,p> written as sum_c p_c (s_j - s_c): with P+ / P0 / P- the probability mass of the classes with s = +1 / 0 / -1,
    // s_j = +1 -> P0 + 2 P-,  s_j = -1 -> -(P0 + 2 P+),  s_j = 0 -> P- - P+ (no cancellation for a class of probability ~ 1)
    const float up1 = wave_sum_f(s > 0.f ? p1 : 0.f), eq1 = wave_sum_f(s == 0.f ? p1 : 0.f), dn1 = wave_sum_f(s < 0.f ? p1 : 0.f);
    const float up2 = wave_sum_f(s > 0.f ? p2 : 0.f), eq2 = wave_sum_f(s == 0.f ? p2 : 0.f), dn2 = wave_sum_f(s < 0.f ? p2 : 0.f);
    const float t1 = s > 0.f ? eq1 + 2.f * dn1 : (s < 0.f ? -(eq1 + 2.f * up1) : dn1 - up1);
    const float t2 = s > 0.f ? eq2 + 2.f * dn2 : (s < 0.f ? -(eq2 + 2.f * up2) : dn2 - up2);
    const float k = gv * a_d / ((float)Mt * (float)C);
    v1 = -k * (p1 * t1);
    v2 = k * (p2 * t2);
  }
  if (!skip) {
    const float f = gv * a_t / save[2 * R + 1] * (alpha ? alpha[yi] : 1.f);
    v1 = bad ? NAN : v1 + f * cls_grad(r1, gamma, lane, yi);
    v2 = bad ? NAN : v2 + f * cls_grad(r2, gamma, lane, yi);
  }
  if (in) {
    dt1[(int64_t)r * C + lane] = v1;
    dt2[(int64_t)r * C + lane] = v2;
  }
}
}  // namespace

extern "C" int sug_ce_pair_fwd(const float* logits1, const float* logits2, int64_t ld, const int64_t* label, int M, int C,
                               float w, int64_t ignore_index, float* loss, float* lse, void* stream) {
  SUG_REQUIRE(logits1 && logits2 && label && loss && lse, "sug_ce_pair_fwd: null pointer");
  SUG_REQUIRE(M > 0 && 2 * M <= CE_MAXROWS && C > 0 && C <= CE_MAXC && ld >= C, "sug_ce_pair_fwd: M=%d rows, C=%d classes (2M <= %d, C <= %d)",
              M, C, CE_MAXROWS, CE_MAXC);
  hipLaunchKernelGGL(ce_pair_fwd_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, logits1, logits2, ld, label, M, C, w, ignore_index, loss, lse);
  SUG_LAUNCH_CHECK("sug_ce_pair_fwd");
  return SUG_OK;
}

extern "C" int sug_ce_pair_bwd(const float* logits1, const float* logits2, int64_t ld, const int64_t* label, int M, int Mtot,
                               int C, float w, int64_t ignore_index, const float* g, const float* lse, float* d1, float* d2,
                               void* stream) {
  SUG_REQUIRE(logits1 && logits2 && label && g && lse && d1 && d2, "sug_ce_pair_bwd: null pointer");
  SUG_REQUIRE(M > 0 && Mtot >= M && 2 * M <= CE_MAXROWS && C > 0 && C <= CE_MAXC && ld >= C, "sug_ce_pair_bwd: bad shape");
  const int64_t n = (int64_t)2 * Mtot * C;
  hipLaunchKernelGGL(ce_pair_bwd_kernel, dim3((unsigned)sug_divup(n, 256)), dim3(256), 0, (hipStream_t)stream, logits1, logits2, ld,
                     label, M, Mtot, C, w, ignore_index, g, lse, d1, d2);
  SUG_LAUNCH_CHECK("sug_ce_pair_bwd");
  return SUG_OK;
}

extern "C" int sug_ce_fwd(const float* logits, int64_t ld, const int64_t* label, int M, int C, int64_t ignore_index,
                          float label_smoothing, float* loss, float* lse, double* totals, void* stream) {
  SUG_REQUIRE(M >= 1 && M <= CE1_MAXROWS && C >= 2 && C <= CE1_MAXC && ld >= C,
              "sug_ce_fwd: unsupported shape M=%d rows, C=%d classes, ld=%lld (1 <= M <= %d, 2 <= C <= %d, ld >= C)", M, C,
              (long long)ld, CE1_MAXROWS, CE1_MAXC);
  SUG_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "sug_ce_fwd: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  SUG_REQUIRE(logits && label && loss && lse, "sug_ce_fwd: null pointer");
  const int waves = M < 16 ? M : 16;
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(1), dim3(WAVE * waves), 0, (hipStream_t)stream, logits, ld, label, M, C, ignore_index,
                     label_smoothing, loss, lse, totals);
  SUG_LAUNCH_CHECK("sug_ce_fwd");
  return SUG_OK;
}

extern "C" int sug_ce_bwd(const float* logits, int64_t ld, const int64_t* label, int M, int C, int64_t ignore_index,
                          float label_smoothing, const float* g, const float* lse, float* dlogits, void* stream) {
  SUG_REQUIRE(M >= 1 && M <= CE1_MAXROWS && C >= 2 && C <= CE1_MAXC && ld >= C,
              "sug_ce_bwd: unsupported shape M=%d rows, C=%d classes, ld=%lld (1 <= M <= %d, 2 <= C <= %d, ld >= C)", M, C,
              (long long)ld, CE1_MAXROWS, CE1_MAXC);
  SUG_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "sug_ce_bwd: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  SUG_REQUIRE(logits && label && g && lse && dlogits, "sug_ce_bwd: null pointer");
  hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)sug_divup((int64_t)M * C, 256)), dim3(256), 0, (hipStream_t)stream, logits, ld,
                     label, M, C, ignore_index, label_smoothing, g, lse, dlogits);
  SUG_LAUNCH_CHECK("sug_ce_bwd");
  return SUG_OK;
}

static int mcd_check(const char* who, int Ms, int Mt, int C, int64_t ld, float a_t) {
  SUG_REQUIRE(Ms >= 1 && Ms <= MCD_MAXROWS && Mt >= 1 && Mt <= MCD_MAXROWS && C >= 2 && C <= CE1_MAXC && ld >= C,
              "%s: unsupported shape Ms=%d, Mt=%d rows, C=%d classes, ld=%lld (1 <= Ms, Mt <= %d, 2 <= C <= %d, ld >= C)", who, Ms, Mt,
              C, (long long)ld, MCD_MAXROWS, CE1_MAXC);
  SUG_REQUIRE(a_t == a_t, "%s: a_t is NaN", who);
  return SUG_OK;
}

extern "C" int sug_mcd_loss_fwd(const float* ys1, const float* ys2, const float* yt1, const float* yt2, int64_t ld,
                                const int64_t* label, const int64_t* label_t, int Ms, int Mt, int C, float a_s, float a_t, float r_s,
                                float* out4, float* lse, double* totals, void* stream) {
  SUG_REQUIRE(ys1 && ys2 && yt1 && yt2 && label && out4 && lse && (label_t || a_t == 0.f), "sug_mcd_loss_fwd: null pointer");
  if (mcd_check("sug_mcd_loss_fwd", Ms, Mt, C, ld, a_t) != SUG_OK) return SUG_ERR_ARG;
  const int rows = Ms > Mt ? Ms : Mt, waves = rows < 16 ? rows : 16;
  hipLaunchKernelGGL(mcd_loss_fwd_kernel, dim3(1), dim3(WAVE * waves), 0, (hipStream_t)stream, ys1, ys2, yt1, yt2, ld, label, label_t,
                     Ms, Mt, C, a_s, a_t, r_s, out4, lse, totals);
  SUG_LAUNCH_CHECK("sug_mcd_loss_fwd");
  return SUG_OK;
}

extern "C" int sug_mcd_loss_bwd(const float* ys1, const float* ys2, const float* yt1, const float* yt2, int64_t ld,
                                const int64_t* label, const int64_t* label_t, int Ms, int Mt, int C, float a_s, float a_t,
                                const float* g, const float* lse, float* ds1, float* ds2, float* dt1, float* dt2, void* stream) {
  SUG_REQUIRE(ys1 && ys2 && yt1 && yt2 && label && g && lse && ds1 && ds2 && dt1 && dt2 && (label_t || a_t == 0.f),
              "sug_mcd_loss_bwd: null pointer");
  if (mcd_check("sug_mcd_loss_bwd", Ms, Mt, C, ld, a_t) != SUG_OK) return SUG_ERR_ARG;
  hipLaunchKernelGGL(mcd_loss_bwd_kernel, dim3((unsigned)sug_divup((int64_t)(Ms + Mt), 4)), dim3(256), 0, (hipStream_t)stream, ys1, ys2,
                     yt1, yt2, ld, label, label_t, Ms, Mt, C, a_s, a_t, g, lse, ds1, ds2, dt1, dt2);
  SUG_LAUNCH_CHECK("sug_mcd_loss_bwd");
  return SUG_OK;
}

static int cls_check(const char* who, int Ms, int Mt, int C, int64_t ld, float gamma, float a_s, float a_t, float a_d) {
  SUG_REQUIRE(Ms >= 1 && Ms <= MCD_MAXROWS && Mt >= 1 && Mt <= MCD_MAXROWS && C >= 2 && C <= CE1_MAXC && ld >= C,
              "%s: unsupported shape Ms=%d, Mt=%d rows, C=%d classes, ld=%lld (1 <= Ms, Mt <= %d, 2 <= C <= %d, ld >= C)", who, Ms, Mt,
              C, (long long)ld, MCD_MAXROWS, CE1_MAXC);
  SUG_REQUIRE(gamma == 0.f || (gamma >= 1.f && gamma < INFINITY),
              "%s: gamma=%g (0, or >= 1: for 0 < gamma < 1 the derivative is unbounded at p_y = 1)", who, (double)gamma);
  SUG_REQUIRE(a_s == a_s && a_t == a_t && a_d == a_d, "%s: a coefficient is NaN", who);
  return SUG_OK;
}

extern "C" int sug_cls_loss_fwd(const float* ys1, const float* ys2, const float* yt1, const float* yt2, int64_t ld,
                                const int64_t* label, const int64_t* label_t, int Ms, int Mt, int C, const float* alpha, float gamma,
                                int reduce_sum, int64_t ignore_index, float a_s, float a_t, float a_d, float r_s, float* out4,
                                float* save, double* totals, void* stream) {
  SUG_REQUIRE(ys1 && ys2 && label && out4 && save && ((yt1 && yt2) || (a_t == 0.f && a_d == 0.f)) && (label_t || a_t == 0.f),
              "sug_cls_loss_fwd: null pointer");
  if (cls_check("sug_cls_loss_fwd", Ms, Mt, C, ld, gamma, a_s, a_t, a_d) != SUG_OK) return SUG_ERR_ARG;
  const int rows = Ms > Mt ? Ms : Mt, waves = rows < 16 ? rows : 16;
  const int ign = !alpha && gamma == 0.f;                 // nn.CrossEntropyLoss: the one case with an ignore label
  hipLaunchKernelGGL(cls_loss_fwd_kernel, dim3(1), dim3(WAVE * waves), 0, (hipStream_t)stream, ys1, ys2, yt1, yt2, ld, label, label_t,
                     Ms, Mt, C, alpha, gamma, reduce_sum != 0, ign, ignore_index, a_s, a_t, a_d, r_s, out4, save, totals);
  SUG_LAUNCH_CHECK("sug_cls_loss_fwd");
  return SUG_OK;
}

extern "C" int sug_cls_loss_bwd(const float* ys1, const float* ys2, const float* yt1, const float* yt2, int64_t ld,
                                const int64_t* label, const int64_t* label_t, int Ms, int Mt, int C, const float* alpha, float gamma,
                                int reduce_sum, int64_t ignore_index, float a_s, float a_t, float a_d, float r_s, const float* g,
                                const float* save, float* ds1, float* ds2, float* dt1, float* dt2, void* stream) {
  (void)reduce_sum;                                       // (the divisors are in `save`)
  (void)r_s;
  SUG_REQUIRE(ys1 && ys2 && label && g && save && ds1 && ds2 && dt1 && dt2 && ((yt1 && yt2) || (a_t == 0.f && a_d == 0.f)) &&
              (label_t || a_t == 0.f), "sug_cls_loss_bwd: null pointer");
  if (cls_check("sug_cls_loss_bwd", Ms, Mt, C, ld, gamma, a_s, a_t, a_d) != SUG_OK) return SUG_ERR_ARG;
  const int ign = !alpha && gamma == 0.f;
  hipLaunchKernelGGL(cls_loss_bwd_kernel, dim3((unsigned)sug_divup((int64_t)(Ms + Mt), 4)), dim3(256), 0, (hipStream_t)stream, ys1, ys2,
                     yt1, yt2, ld, label, label_t, Ms, Mt, C, alpha, gamma, ign, ignore_index, a_s, a_t, a_d, g, save, ds1, ds2, dt1,
                     dt2);
  SUG_LAUNCH_CHECK("sug_cls_loss_bwd");
  return SUG_OK;
}

extern "C" int sug_loss_combine_fwd(const float* loss_cls, const float* v_geo, const float* v_sem1, const float* v_sem2, float wg,
                                    float ws, float* out3, void* stream) {
  SUG_REQUIRE(loss_cls && out3, "sug_loss_combine_fwd: null pointer");
  hipLaunchKernelGGL(loss_combine_fwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss_cls, v_geo, v_sem1, v_sem2, wg, ws, out3);
  SUG_LAUNCH_CHECK("sug_loss_combine_fwd");
  return SUG_OK;
}

extern "C" int sug_loss_combine_bwd(const float* g, float wg, float ws, float* out4, void* stream) {
  SUG_REQUIRE(g && out4, "sug_loss_combine_bwd: null pointer");
  hipLaunchKernelGGL(loss_combine_bwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, g, wg, ws, out4);
  SUG_LAUNCH_CHECK("sug_loss_combine_bwd");
  return SUG_OK;
}
