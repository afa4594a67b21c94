// Dense prediction: the per-point cross entropy of a segmentation batch and the ShapeNet-Part IoU books, on the device.
//
// sug_point_ce_fwd / _bwd: F.cross_entropy(logits [M, C], label [M], weight, ignore_index, reduction='mean') for M up to
// SUG_POINT_CE_MAX_ROWS rows.  ce_fwd_kernel's row layout (loss.hip: a WAVE per row, a LANE per class, cross-lane max and
// sum) over many workgroups: a workgroup takes SUG_POINT_CE_BLOCK_ROWS rows, its rows' terms meet in LDS and wave 0
// folds them in fp64 -- lane l takes rows l, l + 64 in order, then the butterfly -- into ONE partial (weighted loss sum,
// weight sum, counting rows) of the caller's workspace.  Workgroups do not talk to each other: a second launch of one
// workgroup adds the partials in block order, writes the loss and the denominator and keeps the epoch's books.
//
// sug_part_iou_accumulate: one workgroup per cloud, a thread per point; the prediction is the arg-max over the category's
// part range only, the per-part counts (label, prediction, both) are integer LDS atomics -- exact in any order -- and thread 0
// forms the shape's IoU in fp64 in part order and writes the cloud's record.  A second launch of one workgroup adds the
// records to the state block in cloud order: a thread per category (fp64 IoU sums), a thread per part, one for the totals.
//
// No float atomics, no memset node, every floating sum in one fixed order: capturable, bit-reproducible run to run.
#include "common.h"

namespace {
// ------------------------------------------------------------------------------------------------ per-point cross entropy
constexpr int PCE_THREADS = 512;
constexpr int PCE_WAVES = PCE_THREADS / WAVE;
constexpr int PCE_ROWS = SUG_POINT_CE_BLOCK_ROWS;
constexpr int PCE_WAVE_ROWS = PCE_ROWS / PCE_WAVES;        // consecutive rows of a workgroup that one wave takes
constexpr int PCE_MAXC = SUG_POINT_CE_MAX_CLASSES;
constexpr int PCE_WORDS = SUG_POINT_CE_PARTIAL_WORDS;      // weighted loss sum | weight sum | counting rows
constexpr int PCE_FOLD_THREADS = 256;
static_assert(PCE_MAXC <= WAVE, "a lane per class");
static_assert(PCE_ROWS == 2 * WAVE, "wave 0 folds rows l and l + 64");
static_assert(PCE_ROWS % PCE_WAVES == 0 && PCE_WAVE_ROWS <= WAVE, "a lane finishes each of its wave's rows");
static_assert((int64_t)SUG_POINT_CE_MAX_ROWS * PCE_MAXC < (int64_t)1 << 31, "the backward indexes the elements with an int");

// Wave-wide fp32 sum through the DPP cross-lane paths (the shape of wave_max_f), one fixed order; the total is returned to
// every lane.  The row_bcast steps take 0 where a row is masked out.
__device__ __forceinline__ float wave_sum_dpp_f(float v) {
  v += __int_as_float(sug_dpp<0xB1, 0xf>(__float_as_int(v)));     // quad_perm [1,0,3,2]
  v += __int_as_float(sug_dpp<0x4E, 0xf>(__float_as_int(v)));     // quad_perm [2,3,0,1]
  v += __int_as_float(sug_dpp<0x141, 0xf>(__float_as_int(v)));    // row_half_mirror
  v += __int_as_float(sug_dpp<0x140, 0xf>(__float_as_int(v)));    // row_mirror: every lane = its row's sum
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1, 3
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xc, 0xf, false));   // row_bcast:31 into rows 2, 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// A wave takes PCE_WAVE_ROWS consecutive rows: per row one coalesced load, the maximum (DPP), the lowest lane holding it, and
// the sum of exp(z - max) over the OTHER lanes (DPP sum; the maximum's own term is exactly 1), all wave-uniform; lane i keeps
// the scalars of the wave's row i.  Behind the loop the lanes finish their rows side by side: ls = log1p(sum) -- accurate
// relative to ls itself, where max + log(sum) would round at the logits' size, which is the whole loss of a confidently
// right row --, the row's term w * (ls + (max - z_y)) in fp64, and the coalesced stores.  Labels are loaded once per wave
// (lane i: row i) and reach the loop through readlane: no dependent load inside it.
__global__ __launch_bounds__(PCE_THREADS) void point_ce_rows_kernel(
    const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ label, int M, int C, int64_t ignore_index,
    const float* __restrict__ weight, float* __restrict__ lse, int32_t* __restrict__ pred, double* __restrict__ ws) {
  __shared__ double s_term[PCE_ROWS];
  __shared__ float s_w[PCE_ROWS];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int r0 = blockIdx.x * PCE_ROWS;
  const int nrow = min(PCE_ROWS, M - r0);
  const int w0 = wave * PCE_WAVE_ROWS;                      // first row (in the workgroup) of this wave
  const int wrows = min(PCE_WAVE_ROWS, nrow - w0);          // <= 0: nothing to do
  const bool in = lane < C, mine = lane < wrows;
  const int64_t ylab = mine ? label[r0 + w0 + lane] : ignore_index;
  const int ylo = (int)(ylab & 0xffffffff), yhi = (int)(ylab >> 32);
  float my_mx = 0.f, my_sum = 0.f, my_zy = 0.f;
  int my_pred = 0;
  for (int i0 = 0; i0 < wrows; i0 += 4) {                   // wave-uniform trip count; four rows in flight
    float z4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                           // a group's tail reloads the wave's last row: lane i >= wrows keeps nothing
      const float* row = logits + (int64_t)(r0 + w0 + min(i0 + j, wrows - 1)) * ld;
      z4[j] = in ? row[lane] : -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + j;
      const float z = z4[j];
      const float mx = wave_max_f(z);
      const unsigned long long hit = __ballot(in && z == mx);            // the lanes holding the maximum
      const int first = hit ? __ffsll(hit) - 1 : 0;                      // lowest index on ties (a row of NaN: 0)
      const float sum = wave_sum_dpp_f(in && lane != first ? expf(z - mx) : 0.f);
      const int64_t y = ((int64_t)__builtin_amdgcn_readlane(yhi, i) << 32) | (uint32_t)__builtin_amdgcn_readlane(ylo, i);
      const float zy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z), (y >= 0 && y < C) ? (int)y : 0));
      if (lane == i) {
        my_mx = mx;
        my_sum = sum;
        my_zy = zy;
        my_pred = first;
      }
    }
  }
  if (mine) {
    const int r = r0 + w0 + lane;
    const float ls = log1pf(my_sum);                        // log sum_c exp(z_c - max)
    // label contract of sug_ce_fwd: ignore_index rows count for nothing, any other label outside [0, C) poisons the loss
    double term = 0.0;
    float w = 0.f;
    if (ylab != ignore_index) {
      const bool ok = ylab >= 0 && ylab < C;
      w = ok ? (weight ? weight[ylab] : 1.f) : 0.f;         // the denominator stays finite: only this row's gradient is NaN
      term = ok ? (double)w * ((double)ls + ((double)my_mx - (double)my_zy)) : (double)NAN;    // -w[y] * log_softmax(row)[y]
    }
    lse[r] = my_mx;
    lse[M + r] = ls;
    if (pred) pred[r] = my_pred;
    s_term[w0 + lane] = term;
    s_w[w0 + lane] = w;
  }
  __syncthreads();
  if (wave == 0) {
    double a = 0.0, b = 0.0;
    int cnt = 0;
    for (int i = lane; i < nrow; i += WAVE) {
      a += s_term[i];
      b += (double)s_w[i];
      cnt += label[r0 + i] != ignore_index;
    }
    a = wave_sum_d(a);
    b = wave_sum_d(b);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) {
      double* p = ws + (int64_t)blockIdx.x * PCE_WORDS;
      p[0] = a;
      p[1] = b;
      p[2] = (double)cnt;
    }
  }
}

// One workgroup: the partials are staged through LDS a tile at a time (coalesced loads) and three threads, one per word, add
// them in block order.
__global__ __launch_bounds__(PCE_FOLD_THREADS) void point_ce_fold_kernel(const double* __restrict__ ws, int nblk, int M,
                                                                    float* __restrict__ loss, float* __restrict__ lse,
                                                                    double* __restrict__ totals) {
  __shared__ double s_p[PCE_WORDS][PCE_FOLD_THREADS];
  __shared__ double s_sum[PCE_WORDS];
  const int t = threadIdx.x;
  const int word = t / WAVE;                      // threads 0, 64, 128 each own one word
  const bool adder = (t & (WAVE - 1)) == 0 && word < PCE_WORDS;
  double acc = 0.0;
  for (int b0 = 0; b0 < nblk; b0 += PCE_FOLD_THREADS) {
    const int n = min(PCE_FOLD_THREADS, nblk - b0);
    for (int i = t; i < n * PCE_WORDS; i += PCE_FOLD_THREADS)
      s_p[i % PCE_WORDS][i / PCE_WORDS] = ws[(int64_t)b0 * PCE_WORDS + i];
    __syncthreads();
    if (adder) {
      int i = 0;
      for (; i + 8 <= n; i += 8) {                // eight independent LDS reads, then the adds in block order
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = s_p[word][i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += v[j];
      }
      for (; i < n; ++i) acc += s_p[word][i];
    }
    __syncthreads();
  }
  if (adder) s_sum[word] = acc;
  __syncthreads();
  if (t == 0) {
    const float v = (float)(s_sum[0] / s_sum[1]);       // no counting row -> 0 / 0 = NaN, as torch
    loss[0] = v;
    lse[2 * (int64_t)M] = (float)s_sum[1];              // the denominator: the backward divides by it
    if (totals) {
      totals[0] += (double)v * s_sum[2];
      totals[1] += s_sum[2];
    }
  }
}

__global__ __launch_bounds__(256) void point_ce_bwd_kernel(const float* __restrict__ logits, int64_t ld,
                                                           const int64_t* __restrict__ label, int M, int C, int64_t ignore_index,
                                                           const float* __restrict__ weight, const float* __restrict__ g,
                                                           const float* __restrict__ lse, float* __restrict__ d) {
  const int n = M * C;                                  // < 2^31 (static_assert above)
  const float f = g[0] / lse[2 * (int64_t)M];
  const int stride = gridDim.x * blockDim.x;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const int r = e / C, c = e - r * C;
    const int64_t y = label[r];
    float v = 0.f;
    if (y != ignore_index) {
      if (y < 0 || y >= C) {
        v = NAN;
      } else {
        const float fw = weight ? f * weight[y] : f;
        v = fw * (expf((logits[(int64_t)r * ld + c] - lse[r]) - lse[M + r]) - (c == y ? 1.f : 0.f));
      }
    }
    d[e] = v;
  }
}

// ------------------------------------------------------------------------------------------------ part IoU
constexpr int IOU_THREADS = 256;
constexpr int IOU_MAXP = SUG_SEG_MAX_CATEGORY_PARTS;
constexpr int IOU_MAXK = SUG_SEG_MAX_CATEGORIES;
constexpr int IOU_MAXC = SUG_SEG_MAX_PARTS;
constexpr int REC_WORDS = SUG_SEG_RECORD_WORDS;
// a cloud's record (64-bit words)
constexpr int REC_STATUS = 0;       // 0 scored, 1 not scored (category or a label outside its range)
constexpr int REC_CAT = 1;
constexpr int REC_IOU = 2;          // fp64
constexpr int REC_POINTS = 3;
constexpr int REC_CORRECT = 4;
constexpr int REC_PARTS = 8;        // [IOU_MAXP][2]: points labelled with the part, of them predicted as it
static_assert(REC_PARTS + 2 * IOU_MAXP <= REC_WORDS, "record layout");
static_assert(IOU_MAXK <= 64 && IOU_MAXC <= 64 && IOU_THREADS > 128, "the fold: threads 0..63 categories, 64..127 parts, 128 totals");

// The categories' part ranges travel by value with the launch (host arrays: checked there, no device copy to keep alive).
struct SegTable {
  int first[IOU_MAXK];
  int count[IOU_MAXK];
};

__global__ __launch_bounds__(IOU_THREADS) void part_iou_cloud_kernel(const float* __restrict__ logits,
                                                                     const int64_t* __restrict__ label,
                                                                     const int64_t* __restrict__ category, SegTable tab, int N,
                                                                     int C, int K, int64_t* __restrict__ records) {
  __shared__ int s_lab[IOU_MAXP], s_pred[IOU_MAXP], s_inter[IOU_MAXP];
  __shared__ int s_bad;
  const int t = threadIdx.x, b = blockIdx.x;
  int64_t* const rec = records + (int64_t)b * REC_WORDS;
  const int64_t cat = category[b];
  if (cat < 0 || cat >= K) {                           // the same for the whole workgroup
    if (t == 0) rec[REC_STATUS] = 1;
    return;
  }
  if (t < IOU_MAXP) s_lab[t] = s_pred[t] = s_inter[t] = 0;
  if (t == 0) s_bad = 0;
  __syncthreads();
  const int first = tab.first[cat], cnt = tab.count[cat];
  for (int n = t; n < N; n += IOU_THREADS) {
    const int64_t p = (int64_t)b * N + n;
    const float* row = logits + p * C + first;
    float best = row[0];
    int bi = 0;
    for (int j = 1; j < cnt; ++j) {                     // arg-max over the category's range, lowest index on ties
      const float v = row[j];
      if (v > best) {
        best = v;
        bi = j;
      }
    }
    const int64_t y = label[p] - first;
    if (y < 0 || y >= cnt) {
      atomicOr(&s_bad, 1);                              // integer flag and counts: the result does not depend on the order
    } else {
      atomicAdd(&s_lab[y], 1);
      atomicAdd(&s_pred[bi], 1);
      if (bi == (int)y) atomicAdd(&s_inter[y], 1);
    }
  }
  __syncthreads();
  if (t == 0) {
    if (s_bad) {
      rec[REC_STATUS] = 1;
      return;
    }
    double sum = 0.0;
    int correct = 0;
    for (int j = 0; j < cnt; ++j) {                     // part order
      const int inter = s_inter[j], uni = s_lab[j] + s_pred[j] - inter;
      sum += uni == 0 ? 1.0 : (double)inter / (double)uni;
      correct += inter;
      rec[REC_PARTS + 2 * j] = s_lab[j];
      rec[REC_PARTS + 2 * j + 1] = inter;
    }
    rec[REC_STATUS] = 0;
    rec[REC_CAT] = cat;
    rec[REC_IOU] = __double_as_longlong(sum / (double)cnt);
    rec[REC_POINTS] = N;
    rec[REC_CORRECT] = correct;
  }
}

__global__ __launch_bounds__(IOU_THREADS) void part_iou_fold_kernel(const int64_t* __restrict__ records, SegTable tab, int B, int C,
                                                                    int K, int64_t* __restrict__ state) {
  const int t = threadIdx.x;
  double* const dst = reinterpret_cast<double*>(state);
  if (t < K) {                                          // category t: its shapes' IoUs, in cloud order
    double s = dst[SUG_SEG_CAT_IOU + t];
    int64_t n = 0;
    for (int b = 0; b < B; ++b) {
      const int64_t* rec = records + (int64_t)b * REC_WORDS;
      if (rec[REC_STATUS] == 0 && rec[REC_CAT] == t) {
        s += __longlong_as_double(rec[REC_IOU]);
        ++n;
      }
    }
    dst[SUG_SEG_CAT_IOU + t] = s;
    state[SUG_SEG_CAT_SHAPES + t] += n;
  } else if (t >= 64 && t < 64 + C) {                   // part t - 64
    const int p = t - 64;
    int64_t seen = 0, corr = 0;
    for (int b = 0; b < B; ++b) {
      const int64_t* rec = records + (int64_t)b * REC_WORDS;
      if (rec[REC_STATUS] != 0) continue;
      const int cat = (int)rec[REC_CAT];
      const int j = p - tab.first[cat];
      if (j >= 0 && j < tab.count[cat]) {
        seen += rec[REC_PARTS + 2 * j];
        corr += rec[REC_PARTS + 2 * j + 1];
      }
    }
    state[SUG_SEG_PART_POINTS + p] += seen;
    state[SUG_SEG_PART_CORRECT + p] += corr;
  } else if (t == 128) {
    int64_t shapes = 0, points = 0, correct = 0, errors = 0;
    for (int b = 0; b < B; ++b) {
      const int64_t* rec = records + (int64_t)b * REC_WORDS;
      if (rec[REC_STATUS] != 0) {
        ++errors;
      } else {
        ++shapes;
        points += rec[REC_POINTS];
        correct += rec[REC_CORRECT];
      }
    }
    state[SUG_SEG_SHAPES] += shapes;
    state[SUG_SEG_POINTS] += points;
    state[SUG_SEG_CORRECT] += correct;
    state[SUG_SEG_ERROR] += errors;
  }
}

int point_ce_shape_ok(const char* name, int M, int C, int64_t ld) {
  SUG_REQUIRE(M >= 1 && M <= SUG_POINT_CE_MAX_ROWS && C >= 2 && C <= PCE_MAXC && ld >= C,
              "%s: unsupported shape M=%d rows, C=%d classes, ld=%lld (1 <= M <= %d, 2 <= C <= %d, ld >= C)", name, M, C,
              (long long)ld, SUG_POINT_CE_MAX_ROWS, PCE_MAXC);
  return SUG_OK;
}
}  // namespace

extern "C" int sug_point_ce_workspace(int M) {
  SUG_REQUIRE(M >= 1 && M <= SUG_POINT_CE_MAX_ROWS, "sug_point_ce_workspace: M=%d rows (1 <= M <= %d)", M, SUG_POINT_CE_MAX_ROWS);
  return sug_divup(M, PCE_ROWS) * PCE_WORDS;
}

extern "C" int sug_point_ce_fwd(const float* logits, int64_t ld, const int64_t* label, int M, int C, int64_t ignore_index,
                                const float* class_weight, float* loss, float* lse, int32_t* pred, double* workspace,
                                double* totals, void* stream) {
  if (int rc = point_ce_shape_ok("sug_point_ce_fwd", M, C, ld)) return rc;
  SUG_REQUIRE(logits && label && loss && lse && workspace, "sug_point_ce_fwd: null pointer");
  const int nblk = sug_divup(M, PCE_ROWS);
  hipLaunchKernelGGL(point_ce_rows_kernel, dim3(nblk), dim3(PCE_THREADS), 0, (hipStream_t)stream, logits, ld, label, M, C,
                     ignore_index, class_weight, lse, pred, workspace);
  SUG_LAUNCH_CHECK("sug_point_ce_fwd");
  hipLaunchKernelGGL(point_ce_fold_kernel, dim3(1), dim3(PCE_FOLD_THREADS), 0, (hipStream_t)stream, workspace, nblk, M, loss, lse,
                     totals);
  SUG_LAUNCH_CHECK("sug_point_ce_fwd (fold)");
  return SUG_OK;
}

extern "C" int sug_point_ce_bwd(const float* logits, int64_t ld, const int64_t* label, int M, int C, int64_t ignore_index,
                                const float* class_weight, const float* g, const float* lse, float* dlogits, void* stream) {
  if (int rc = point_ce_shape_ok("sug_point_ce_bwd", M, C, ld)) return rc;
  SUG_REQUIRE(logits && label && g && lse && dlogits, "sug_point_ce_bwd: null pointer");
  const int grid = min(sug_divup((int64_t)M * C, 256), 2048);
  hipLaunchKernelGGL(point_ce_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, ld, label, M, C, ignore_index,
                     class_weight, g, lse, dlogits);
  SUG_LAUNCH_CHECK("sug_point_ce_bwd");
  return SUG_OK;
}

extern "C" int sug_part_iou_accumulate(const float* logits, const int64_t* label, const int64_t* category,
                                       const int32_t* part_first, const int32_t* part_count, int B, int N, int C, int K,
                                       void* records, void* state, void* stream) {
  SUG_REQUIRE(B >= 1 && B <= SUG_SEG_MAX_CLOUDS && N >= 1 && C >= 1 && C <= IOU_MAXC && K >= 1 && K <= IOU_MAXK,
              "sug_part_iou_accumulate: B=%d clouds, N=%d points, C=%d parts, K=%d categories (1 <= B <= %d, N >= 1, 1 <= C <= %d, "
              "1 <= K <= %d)", B, N, C, K, SUG_SEG_MAX_CLOUDS, IOU_MAXC, IOU_MAXK);
  SUG_REQUIRE(logits && label && category && part_first && part_count && records && state,
              "sug_part_iou_accumulate: null pointer");
  SegTable tab = {};
  for (int k = 0; k < K; ++k) {                         // host arrays: a range outside the logits' columns never reaches a launch
    const int f = part_first[k], n = part_count[k];
    SUG_REQUIRE(n >= 1 && n <= IOU_MAXP && f >= 0 && f <= C - n,
                "sug_part_iou_accumulate: category %d owns parts [%d, %d + %d) (1 <= part_count <= %d, inside [0, C = %d))", k, f, f,
                n, IOU_MAXP, C);
    tab.first[k] = f;
    tab.count[k] = n;
  }
  hipLaunchKernelGGL(part_iou_cloud_kernel, dim3(B), dim3(IOU_THREADS), 0, (hipStream_t)stream, logits, label, category, tab, N, C,
                     K, (int64_t*)records);
  SUG_LAUNCH_CHECK("sug_part_iou_accumulate");
  hipLaunchKernelGGL(part_iou_fold_kernel, dim3(1), dim3(IOU_THREADS), 0, (hipStream_t)stream, (const int64_t*)records, tab, B, C, K,
                     (int64_t*)state);
  SUG_LAUNCH_CHECK("sug_part_iou_accumulate (fold)");
  return SUG_OK;
}
