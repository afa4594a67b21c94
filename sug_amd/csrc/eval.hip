// One evaluation batch's share of eval_worker (utils/eval_utils.py:37-61) in one launch, with no host synchronisation:
//   output = (logits1 + logits2) / 2 (fp32, the reference's rounding; logits1 alone when logits2 is null), optionally written;
//   pred   = the index torch.max(output, 1) returns (first maximum, first NaN);
//   loss   = nn.CrossEntropyLoss(output, label) computed here (ce_mode 1: mean, 2: sum; rows summed in fp64, rounded to fp32)
//            or a device scalar the caller's criterion produced (ce_mode 0);
//   integer counts of the batch (correct rows, rows and correct rows per class), then thread 0 folds them into the fp64 /
//   int64 accumulators of the state block in a fixed order: the per-class ratio (double)correct_c / (double)rows_c and the
//   batch ratio (double)correct / (double)B are plain IEEE double divisions, so class_acc equals numpy's `+=` sequence and
//   batch_acc the list of Python float divisions bit for bit.
// One workgroup of 256 threads (4 x wave64): rows strided over threads, reductions through LDS in a fixed order, no atomics
// on floating-point values.
#include "common.h"

namespace {
constexpr int EV_THREADS = 256;
constexpr int EV_MAXB = SUG_EVAL_MAX_ROWS;
constexpr int EV_MAXC = SUG_EVAL_MAX_CLASSES;
static_assert(EV_THREADS % EV_MAXC == 0, "class counting splits the workgroup into EV_THREADS / EV_MAXC parts");
constexpr int EV_PARTS = EV_THREADS / EV_MAXC;

__device__ __forceinline__ float ev_out(const float* __restrict__ l1, const float* __restrict__ l2, int64_t o) {
  return l2 ? (l1[o] + l2[o]) / 2.f : l1[o];
}

__global__ __launch_bounds__(EV_THREADS) void eval_accumulate_kernel(
    const float* __restrict__ l1, const float* __restrict__ l2, int64_t ld, const int64_t* __restrict__ label, int B, int C,
    const float* __restrict__ loss_in, int ce_mode, int64_t ignore_index, float smoothing, float* __restrict__ out,
    int64_t* __restrict__ pred_out, int cls_eval, int64_t* __restrict__ state, int cap) {
  __shared__ int s_lab[EV_MAXB];              // label of the row, -1 where it is outside [0, C)
  __shared__ unsigned char s_ok[EV_MAXB];     // prediction == label
  __shared__ double s_nll[EV_THREADS], s_smooth[EV_THREADS];
  __shared__ int s_cnt[EV_THREADS], s_kept[EV_THREADS], s_rows[EV_THREADS], s_corr[EV_THREADS];
  __shared__ int s_err;
  const int t = threadIdx.x;
  if (t == 0) s_err = 0;
  __syncthreads();

  int correct = 0, kept = 0, err = 0;
  double nll = 0.0, smooth = 0.0;               // this thread's rows, ascending
  for (int r = t; r < B; r += EV_THREADS) {
    const int64_t base = (int64_t)r * ld;
    float best = ev_out(l1, l2, base);
    int bi = 0;
    if (out) out[(int64_t)r * C] = best;
    for (int c = 1; c < C; ++c) {
      const float v = ev_out(l1, l2, base + c);
      if (out) out[(int64_t)r * C + c] = v;
      if (!isnan(best) && (isnan(v) || v > best)) {   // torch.max: first NaN, else first maximum
        best = v;
        bi = c;
      }
    }
    if (pred_out) pred_out[r] = bi;
    const int64_t y = label[r];
    const bool in = y >= 0 && y < C;
    if (!in) err = 1;                           // eval_utils.py:53 indexes class_acc[j]: IndexError there
    s_lab[r] = in ? (int)y : -1;
    const int ok = in && bi == (int)y;
    s_ok[r] = (unsigned char)ok;
    correct += ok;
    if (ce_mode != 0 && y != ignore_index) {
      float mx = -INFINITY;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, ev_out(l1, l2, base + c));
      float s = 0.f, sx = 0.f;
      for (int c = 0; c < C; ++c) {
        const float v = ev_out(l1, l2, base + c);
        s += expf(v - mx);
        sx += v;
      }
      const float lse = mx + logf(s);
      // -log_softmax(row)[y]; a label outside [0, C) that is not ignore_index poisons the loss (torch raises)
      nll += in ? (double)(lse - ev_out(l1, l2, base + y)) : (double)NAN;
      smooth += (double)C * (double)lse - (double)sx;       // sum_c -log_softmax(row)[c] (label smoothing)
      ++kept;
    }
  }
  if (err) atomicOr(&s_err, err);               // integer flag: the result does not depend on the order
  s_cnt[t] = correct;
  s_kept[t] = kept;
  s_nll[t] = nll;
  s_smooth[t] = smooth;
  __syncthreads();

  // per-class rows / correct rows: class t % 64, a quarter of the rows each, then the quarters summed (integers)
  {
    const int c = t % EV_MAXC, q = t / EV_MAXC;
    int rows = 0, corr = 0;
    if (c < C) {
      for (int r = q; r < B; r += EV_PARTS) {
        if (s_lab[r] == c) {
          ++rows;
          corr += s_ok[r];
        }
      }
    }
    s_rows[t] = rows;
    s_corr[t] = corr;
  }
  __syncthreads();

  if (t == 0) {
    int64_t* const st = state;
    double* const dst = reinterpret_cast<double*>(state);
    int ncorrect = 0, nkept = 0;
    double snll = 0.0, ssmooth = 0.0;
    for (int i = 0; i < EV_THREADS; ++i) {
      ncorrect += s_cnt[i];
      nkept += s_kept[i];
      snll += s_nll[i];
      ssmooth += s_smooth[i];
    }
    float loss;
    if (ce_mode == 0) {
      loss = loss_in[0];
    } else {
      const double eps = (double)smoothing;
      const double den = ce_mode == 1 ? (double)nkept : 1.0;   // mean over the rows that count (0 rows: NaN, as torch)
      double v = snll / den;
      if (smoothing != 0.f) v = (1.0 - eps) * v + eps / (double)C * (ssmooth / den);
      loss = (float)v;
    }
    int64_t e = st[SUG_EVAL_ERROR] | s_err;
    const int64_t n = st[SUG_EVAL_BATCH_COUNT];
    st[SUG_EVAL_DATA_TOTAL] += B;
    st[SUG_EVAL_CORRECT_TOTAL] += ncorrect;
    dst[SUG_EVAL_LOSS_TOTAL] += (double)loss * (double)B;        // loss.item() * data.size(0)
    for (int c = 0; c < C; ++c) {
      int rows = 0, corr = 0;
      for (int q = 0; q < EV_PARTS; ++q) {
        rows += s_rows[q * EV_MAXC + c];
        corr += s_corr[q * EV_MAXC + c];
      }
      st[SUG_EVAL_CLASS_ROWS + c] += rows;
      st[SUG_EVAL_CLASS_CORRECT + c] += corr;
      if (cls_eval && rows > 0) {
        dst[SUG_EVAL_CLASS_ACC + 2 * c] += (double)corr / (double)rows;
        dst[SUG_EVAL_CLASS_ACC + 2 * c + 1] += 1.0;
      }
    }
    if (n < cap) {
      dst[SUG_EVAL_BATCH_ACC + n] = (double)ncorrect / (double)B;
    } else {
      e |= 2;                                   // more batches than the state block has room for
    }
    st[SUG_EVAL_BATCH_COUNT] = n + 1;
    st[SUG_EVAL_ERROR] = e;
  }
}
}  // namespace

extern "C" int sug_eval_accumulate(const float* logits1, const float* logits2, int64_t ld, const int64_t* label, int B, int C,
                                   const float* loss_in, int ce_mode, int64_t ignore_index, float label_smoothing, float* out,
                                   int64_t* pred, int cls_eval, void* state, int cap, void* stream) {
  SUG_REQUIRE(state, "sug_eval_accumulate: null state");
  SUG_REQUIRE(logits1 && label, "sug_eval_accumulate: null pointer");
  SUG_REQUIRE(B > 0 && B <= EV_MAXB && C > 0 && C <= EV_MAXC && ld >= C,
              "sug_eval_accumulate: B=%d rows, C=%d classes, ld=%lld (B <= %d, C <= %d, ld >= C)", B, C, (long long)ld, EV_MAXB,
              EV_MAXC);
  SUG_REQUIRE(cap > 0, "sug_eval_accumulate: cap=%d batches", cap);
  SUG_REQUIRE(ce_mode >= 0 && ce_mode <= 2, "sug_eval_accumulate: ce_mode=%d (0 loss_in, 1 mean, 2 sum)", ce_mode);
  SUG_REQUIRE(ce_mode != 0 || loss_in, "sug_eval_accumulate: ce_mode 0 needs loss_in");
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(EV_THREADS), 0, (hipStream_t)stream, logits1, logits2, ld, label, B, C,
                     loss_in, ce_mode, ignore_index, label_smoothing, out, pred, cls_eval, (int64_t*)state, cap);
  SUG_LAUNCH_CHECK("sug_eval_accumulate");
  return SUG_OK;
}
