// Functions that cross translation units of libsug_amd.so without being part of the C ABI (include/sug_amd.h), each
// declared here once.  Host-only units (layers.cpp) include this header alone; the .hip units include it after common.h.
//
// common.h keeps five more such prototypes (sug_stats_finalize, sug_reduce_partials, sug_reverse_lists, sug_knn_pc,
// sug_knn_pc_supported) and the .hip units' SUG_REQUIRE: it is one of the four sources whose hash names the committed
// PMC traffic files, so they move here when those kernels are next measured.  edgeconv_fused.hip, pinned the
// same way, still carries its own copies of sug_affine_act_groups and sug_edgeconv_bn_act.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "../../include/sug_amd.h"

void sug_set_error(const char* fmt, ...);

#ifndef SUG_REQUIRE      // common.h's, for the units that cannot include it
#define SUG_REQUIRE(cond, ...) do { if (!(cond)) { sug_set_error(__VA_ARGS__); return SUG_ERR_ARG; } } while (0)
#endif

// Return protocol of every function below that takes `groups` (the grouped forms: one launch over all domain groups of
// a layer): 0 = done, 1 = the layout does not allow the grouped launch, so the caller goes group by group through
// the C ABI entry points, < 0 = error (SUG_ERR_*, message set).

// ---- bn_rows.hip: BatchNorm (+ activation) over the rows of a channel-last [rows, C] tensor, `rows` rows per group
//   statistics + BatchNorm coefficients of y -> coef [groups,5,C], running buffers updated in group order
int sug_col_stats_bn_groups(const float* y, int64_t ldy, int64_t rows, int C, int groups, const float* gamma,
                            const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                            float* coef, float* ws, hipStream_t st);
//   the same with the bits of `groups` sug_col_stats_bn calls, at any size: each group is cut into workgroups as a call
//   of its own would be and folded in that call's order.  ws: groups * SUG_STATS_BLOCKS * 2C floats (a block per group)
int sug_col_stats_bn_own_ws(const float* y, int64_t ldy, int64_t rows, int C, int groups, const float* gamma,
                            const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                            float* coef, float* ws, hipStream_t st);
//   out = act(coef_g . z) with the coefficient set of each row's group
int sug_affine_act_groups(const float* z, int64_t ldz, const float* coef, int64_t rows, int groups, int C, float slope,
                          float* out, int64_t ldo, hipStream_t st);
//   a = scale*G (a == nullptr: sums only) and the BatchNorm backward sums red [groups, 2C];  dgb (may be null):
//   dbeta | dgamma [2Co] summed over the groups, fp32 (sug_fold_groups of red)
int sug_bwd_reduce_groups(const float* gout, int64_t ldg, const float* z, const float* coef, int64_t rows, int Co,
                          int groups, float slope, float* a, double* red, float* ws, hipStream_t st, float* dgb);
//   dy of all groups (rows_g rows each).  from_g: `a` is the upstream gradient gout (row stride lda) instead of the
//   precomputed a = scale*G
int sug_bn_bwd_apply_groups(const float* a, int64_t lda, int from_g, float slope, const float* y, int64_t ldy,
                            const float* coef, const double* red, int64_t rows_g, int groups, int C, float* dy,
                            int64_t lddy, hipStream_t st);

// ---- bnpool.hip: sug_bn_act_pool_fwd / _bwd over B clouds in `groups` domain groups, coefficient set per group
int sug_bn_act_pool_fwd_groups(const float* y, int64_t ldy, const float* coef, int B, int groups, int N, int C, float slope,
                               float* out_max, float* out_mean, int64_t ld_pool, int32_t* arg, float* ws, hipStream_t st);
int sug_bn_act_pool_bwd_groups(const float* y, int64_t ldy, const float* coef, const float* gmax, const float* gmean,
                               int64_t ld_pool, const int32_t* arg, int B, int groups, int N, int C, float slope, double* red,
                               float* ws, float* dy, int64_t lddy, float* dgb, hipStream_t st);

// ---- edgeconv.hip (these two fall back to the per-group launches themselves: 0 or an error)
//   EdgeConv forward + BatchNorm coefficients + activation for `groups` domain groups of B/groups clouds
int sug_edgeconv_fwd_bn_act_groups(const float* pq, int64_t ldpq, const int32_t* idx, const float* gamma,
                                   const float* beta, int B, int N, int k, int Co, int groups, float eps, float momentum,
                                   float slope, float* running_mean, float* running_var, float* z, uint8_t* arg,
                                   float* s1, float* coef, float* out, int64_t ldo, float* ws, void* stream);
//   sug_edgeconv_bwd_scatter over `groups` BatchNorm groups: group g reads coef + g*coef_stride and red + g*red_stride
//   (strides in elements; a zero red_stride shares one row, e.g. the zero row of eval mode)
int sug_edgeconv_bwd_scatter_groups(const float* a, const uint8_t* arg, const float* s1, const float* pq, int64_t ldpq,
                                    const int32_t* rev_off, const int32_t* rev_ent, const float* coef, const double* red,
                                    int B, int N, int k, int Co, int groups, int64_t coef_stride, int64_t red_stride,
                                    float* dpq, int64_t lddpq, void* stream);

// ---- edgeconv_fused.hip: statistics fold + BatchNorm + LeakyReLU of an EdgeConv layer in one launch; ws = `groups` x
// nblk partial rows [2Co] (group-major) with the pivot rows behind them, z [groups*rows_g, Co] dense (0 or an error)
int sug_edgeconv_bn_act(const float* ws, int nblk, int Co, int groups, const float* gamma, const float* beta, double count,
                        float eps, float momentum, float* running_mean, float* running_var, float* coef, const float* z,
                        int64_t rows_g, float slope, float* out, int64_t ldo, hipStream_t st);

// ---- knn.hip: LDS bytes of sug_reverse_lists (common.h) for this shape; ranges (may be null): destination ranges per cloud
size_t sug_reverse_lists_lds_bytes(int B, int E, int N, int* ranges);

// Grid of an elementwise grid-stride launch of 256 threads (bn_rows.hip, bnpool.hip)
static inline int sug_ew_grid(int64_t total) {
  int64_t g = (total + 255) / 256;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}
