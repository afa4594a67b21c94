/*
 * sug_amd.h -- C ABI of libsug_amd.so: MI355X (gfx950) kernels for SUG's
 * point-cloud encoder + MMD alignment hot path.
 *
 * Conventions (mirroring the reference's only native interface, the pybind
 * module of model/pointnet2/src/pointnet2_api.cpp:10-24):
 *   - the caller owns every buffer (device pointers), pre-allocates all outputs
 *     and scratch; kernels write in place and retain nothing;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*),
 *     re-entrant, holds no global state, never synchronises, never allocates (the only process-wide note kept is, per device, that a
 *     kernel's dynamic-LDS limit has been raised);
 *   - return 0 on success or a negative SUG_ERR_* code (never exit());
 *     sug_last_error() returns a thread-local message for the last failure;
 *   - feature tensors are point-major rows ("channel-last"): element (b,n,c) of
 *     a [B,N,C] tensor lives at base[(b*N+n)*ld + c]; `ld` (row stride, in
 *     elements, >= C) lets a caller write/read a column slice of a wider
 *     buffer.  xyz tensors are dense [B,N,3].  Indices are int32.
 *   - all arithmetic is IEEE fp32 with a fixed operation order (stated per
 *     function) so that index results are bit-reproducible against the CPU
 *     reference path; nothing is compiled with fast-math or fp contraction.
 */
#ifndef SUG_AMD_H
#define SUG_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUG_OK 0
#define SUG_ERR_ARG (-1)          /* bad argument / unsupported size        */
#define SUG_ERR_LAUNCH (-2)       /* hipLaunch failed                       */
/* Per-channel sums (BN statistics, BN gradients) are reduced without atomics so that
 * results are bit-reproducible run to run: kernels write one fp32 partial row per
 * workgroup into a caller-provided workspace `ws` of SUG_STATS_BLOCKS * 2*C floats,
 * then an ordered fp64 pass fills the 2*C-double result (no zeroing needed).
 * The BatchNorm entry points (sug_col_stats_bn, sug_bn_act_rows_fwd, sug_pointmlp_max_layer_fwd,
 * sug_sa_first_fwd, sug_bn_act_pool_layer_fwd) take the batch statistics about a pivot row (one value of
 * the group's data per channel: sum(x - p), sum((x - p)^2) in fp32, mean = p + S1/n and
 * var = S2/n - (S1/n)^2 in fp64), so that data with |mean| >> std keeps its variance, like the two-pass /
 * Welford forms of nn.BatchNorm; the pivot rows live in the last 8 rows of the same workspace. */
#define SUG_STATS_BLOCKS 1024

const char* sug_last_error(void);
/* ABI version of the loaded library (bumped when a signature changes; 3: sug_adam_step_capturable gained lr_dev,
 * round-3 entry points; 4: sug_chamfer / sug_node_offset_bwd became reproducible -- sug_chamfer takes a workspace; 5: sug_ce_pair_* take ignore_index, lse has 2M + 1 entries; sug_pointmlp_max_layer_fwd_xf and sug_col_stats_bn_grouped added; 6: sug_ptran_fused_fwd / sug_ptran_fused_supported added, sug_group_max_bwd fails instead of changing its summation order when the LDS opt-in is refused; 7: sug_adam_chain_step, sug_edge_weight_split_multi, sug_soft_mmd_multi_fwd / _bwd, sug_sda_prob_weights_multi, sug_chamfer_weights and sug_bn_replay_multi added, sug_bn_act_pool_* take the row stride ld_pool of the pooled outputs / their gradients; still 7 after sug_eval_accumulate, the KPConv entry points (sug_grid_subsample .. sug_seg_mean_bwd), sug_ptcls_head_supported / _fwd / _bwd and the multi-scale grouping / feature propagation entry points (sug_ball_query_multi, sug_three_nn_direct, sug_fp_interp_fwd / _bwd) and sug_grad_scale16 were added: purely additive entry points, no signature changed; still 7 after the shape limits SUG_CE_PAIR_MAX_* / SUG_CE_MAX_* / SUG_MCD_MAX_ROWS / SUG_CLASS_MMD_MAX_* / SUG_PREP_MAX_POINTS / SUG_ICP_MAX_POINTS became defines of this header: the values the kernels already had; still 7 after sug_cl_loss_fwd / _bwd and their SUG_CL_LOSS_* limits were added; still 7 after sug_point_ce_workspace / _fwd / _bwd and sug_part_iou_accumulate were added; still 7 after sug_reverse_lists_build was added; still 7 after sug_edgemlp_supported, sug_edge_expand_fwd / _bwd and sug_edgemlp_max_layer_fwd_xf were added; still 7 after sug_reverse_lists_tiled / _supported and their SUG_REV_TILED_* limits were added; 8: the KPConv entry points keep one row layout -- the eight sug_*_cap twins are gone, sug_grid_subsample takes C, level and the nullable record, sug_kpconv_fwd takes nq_valid, sug_seg_instnorm_fwd / _bwd take N; still 8 after sug_edgeconv_path and sug_bn_rows_plan were added). A binding checks sug_abi_version() == SUG_ABI_VERSION of the header it was written against. */
#define SUG_ABI_VERSION 8
int sug_abi_version(void);

/* ---- kNN graph ----------------------------------------------------------
 * replaces knn(), model/model_utils.py:178-185 (the [B,N,N] matrix + topk).
 * score(i,j) = (-|x_j|^2 - (-2 * <x_i,x_j>)) - |x_i|^2, <.,.> an ascending-c
 * fma chain, |.|^2 a sequential sum of separately rounded squares; the k
 * largest scores per i, descending, ties -> lowest j first.  Requires
 * N >= k, 1 <= k <= 32. x: [B,N,C] rows (ld = ldx). idx: [B,N,k]. */
int sug_knn(const float* x, int64_t ldx, int B, int N, int C, int k,
            int32_t* idx, void* stream);

/* Reverse neighbour lists of a kNN graph (needed by the EdgeConv backward):
 * for every destination point m the entries e = n*k + j with idx[b,n,j] == m,
 * ascending in e.  rev_off: [B,N+1] (exclusive prefix, per cloud), rev_ent:
 * [B,N*k].  No reference counterpart (autograd's index_put_ does this
 * implicitly, model/model_utils.py:204).  The LDS-resident build of
 * sug_reverse_lists_build where that takes B clouds of N*k entries, else
 * sug_reverse_lists_tiled with its own choice of tile (same lists). */
int sug_knn_reverse(const int32_t* idx, int B, int N, int k,
                    int32_t* rev_off, int32_t* rev_ent, void* stream);

/* The same build for any index array: idx [B,E] with destinations in [0,N).  For each cloud rev_ent holds the
 * entries e whose destination is valid, in ascending (destination, e) order -- the stable argsort of the row --
 * rev_off [B,N+1] the exclusive prefix of the destinations' counts, rev_off[b,N] the number of valid entries.
 * Entries with a destination outside [0,N) are skipped and rev_ent [B,E] behind the valid count is not written.
 * sorted = 0 says that the caller does not need the order; the lists come out ascending all the same.  One launch,
 * everything in LDS: fails with SUG_ERR_ARG, launching nothing, when 4 * (2 * ceil(N / R) + 32 + E) exceeds 160 KB,
 * R the destination ranges per cloud (doubled from 1 while R < 8, B * R < 256 and N / (2 R) >= 64). */
int sug_reverse_lists_build(const int32_t* idx, int B, int E, int N, int sorted,
                            int32_t* rev_off, int32_t* rev_ent, void* stream);

/* The same lists, to the same contract (ascending (destination, e) order, rev_off the exclusive prefix, rev_off[b,N] the
 * valid count, destinations outside [0,N) skipped, rev_ent behind the valid count and everything outside the two arrays
 * not written), for clouds beyond the LDS-resident build: N <= SUG_REV_TILED_MAX_DEST destinations and
 * E <= SUG_REV_TILED_MAX_ENTRIES entries per cloud.  A workgroup owns a destination range of one cloud and streams the
 * cloud's entries through LDS in tiles, twice (counts, then a stable placement at one running cursor per destination):
 * one launch, no workspace, no atomics on global memory, no host wait (capturable), the same integers run to run.
 * tile: the entries of a cloud one streaming step holds; 0 = the library's choice (the cloud rounded up to 1024, at most
 * SUG_REV_TILED_MAX_TILE), else a multiple of 1024 in [1024, SUG_REV_TILED_MAX_TILE], taken as given.  SUG_ERR_ARG,
 * launching nothing, for a null pointer, a shape outside the limits or another tile.
 * sug_reverse_lists_tiled_supported: 1 for B > 0 clouds inside the two limits, else 0. */
#define SUG_REV_TILED_MAX_DEST 32768
#define SUG_REV_TILED_MAX_ENTRIES 2097152
#define SUG_REV_TILED_MAX_TILE 20480
int sug_reverse_lists_tiled_supported(int B, int E, int N);
int sug_reverse_lists_tiled(const int32_t* idx, int B, int E, int N, int tile,
                            int32_t* rev_off, int32_t* rev_ent, void* stream);

/* ---- farthest point sampling -------------------------------------------
 * replaces farthest_point_sample(), model/point_utils.py:5-26,
 * model/pointnet2_utils.py:60-81, model/PTran_utils.py:53-73, and
 * furthest_point_sampling_wrapper (model/pointnet2/src/sampling.cpp:38-39).
 * d = ((dx*dx + dy*dy) + dz*dz); running min; arg-max ties -> lowest index.
 * start[b] is the first centroid (the caller draws it the way the reference
 * does: torch.randint on the CPU generator).  xyz [B,N,3], out [B,npoint].
 * N <= 8192. */
int sug_fps(const float* xyz, const int32_t* start, int B, int N, int npoint,
            int32_t* out, void* stream);

/* ---- ball query -----------------------------------------------------------
 * replaces query_ball_point(radius != None), model/point_utils.py:99-106,
 * model/pointnet2_utils.py:97-103 and ball_query_wrapper_fast
 * (model/pointnet2/src/ball_query.cpp:14-15) with the *torch path's* rule:
 * d = ((-2*<q,p>) + |q|^2) + |p|^2; keep !(d > r2); first nsample hits in
 * ascending index order, short rows padded with the first hit, rows with no
 * hit filled with N.  xyz [B,N,3], query [B,S,3], out [B,S,nsample]. */
int sug_ball_query(const float* xyz, const float* query, int B, int N, int S,
                   float r2, int nsample, int32_t* out, void* stream);

/* ---- k nearest candidates of a few queries (full-sort semantics) ---------
 * replaces query_ball_point(radius=None), model/point_utils.py:107-108
 * (sort of the [B,S,N] distances, first k): ascending d (same formula as the
 * ball query), ties -> lowest index.  k <= 64, N <= 4096.
 * dist_out may be NULL; else [B,S,k]. */
int sug_knn_query(const float* xyz, const float* query, int B, int N, int S,
                  int k, int32_t* idx_out, float* dist_out, void* stream);
/* Same selection on the direct-form distance sum((q - p)^2) of the Point Transformer path:
 * `square_distance(...).argsort()[:, :, :k]`, Ptran_transformer.py:32-33, PTran_utils.py:117-119. */
int sug_knn_query_direct(const float* xyz, const float* query, int B, int N, int S, int k,
                         int32_t* idx_out, float* dist_out, void* stream);

/* ---- 3 nearest of few candidates for many queries --------------------------
 * replaces the sort + [:3] of upsample_inter(), model/point_utils.py:153-155
 * and three_nn_wrapper_fast (model/pointnet2/src/interpolate.cpp:14-15).
 * query [B,N,3] (the dense cloud), cand [B,S,3] (the nodes), S <= 2048.
 * idx3/dist3: [B,N,3], ascending d, ties -> lowest index; d is the raw
 * expanded-form value (the 1e-10 clamp is the caller's). */
int sug_three_nn(const float* query, const float* cand, int B, int N, int S,
                 int32_t* idx3, float* dist3, void* stream);

/* The same selection on the direct-form distance ((q-c)_x^2 + (q-c)_y^2) + (q-c)_z^2 of model/PTran_utils.py:36
 * (PTran_utils.PointNetFeaturePropagation, Ptran_model.TransitionUp).  Both forms take 3 <= S <= 2048. */
int sug_three_nn_direct(const float* query, const float* cand, int B, int N, int S,
                        int32_t* idx3, float* dist3, void* stream);

/* ---- ball query for several radii in one pass ------------------------------
 * query_ball_point of PointNetSetAbstractionMsg.forward (model/pointnet2_utils.py:246-248) for R radii, 1 <= R <= 4:
 * every query / point distance is computed once, in sug_ball_query's operation order, and feeds the R lists
 * out[r] [B,S,nsample[r]] by that entry point's rules; the lists equal R sug_ball_query calls bit for bit.
 * r2, nsample and out are HOST arrays of R entries (out: device pointers). */
int sug_ball_query_multi(const float* xyz, const float* query, int B, int N, int S, int R, const float* r2,
                         const int32_t* nsample, int32_t* const* out, void* stream);

/* ---- feature propagation: 3-NN inverse-distance interpolation ---------------
 * PointNetFeaturePropagation.forward, model/pointnet2_utils.py:305-308 and model/PTran_utils.py:296-299:
 *   r_t = 1 / (d3[b,n,t] + 1e-8), w_t = r_t / ((r_0 + r_1) + r_2), out[b,n,0:D) = (w_0 src[i_0] + w_1 src[i_1]) + w_2 src[i_2]
 * with i_t = idx3[b,n,t] a row of src [B,S,D] (row stride lds).  d3 is used as it is: no clamp, a negative value (the
 * expanded form's rounding residue of a point's distance to itself) divides as in the reference.  out has row stride ldo
 * and may be a column slice of a wider [B,N,ldo] buffer (the torch.cat of :312 then costs no pass of its own).  w3
 * [B,N,3] receives the weights for the backward.  Nothing of shape [B,N,3,D] is formed.
 * Backward: dsrc[b,s,0:D) (row stride ldd) = sum over the entries e = 3n + t with idx3[b,n,t] == s, ascending in e, of
 * w3[b,n,t] * g[b,n,0:D) (g: row stride ldg, may be a column slice): sorted reverse lists, no float atomics, every row
 * of dsrc written, bit-identical from run to run.  Scratch: rev_off [B,S+1], rev_ent [B,3N] ints.  No gradient is
 * formed for the coordinates.  3 <= S; 3N entries per cloud must fit the LDS-resident reverse-list build (N <= 8192). */
int sug_fp_interp_fwd(const float* src, int64_t lds, const int32_t* idx3, const float* d3, int B, int N, int S, int D,
                      float* out, int64_t ldo, float* w3, void* stream);
int sug_fp_interp_bwd(const float* g, int64_t ldg, const int32_t* idx3, const float* w3, int B, int N, int S, int D,
                      int32_t* rev_off, int32_t* rev_ent, float* dsrc, int64_t ldd, void* stream);

/* dst[r][0..C) = src[r][0..C), r < rows, row strides lds / ldd in floats (C, lds, ldd multiples of 4; 16-byte aligned):
 * a dense tensor into a column slice of a wider row buffer (the torch.cat of DGCNN.forward, model/Model.py:111) or back. */
int sug_copy_rows2d(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int C, void* stream);

/* ---- row gather / scatter (index_points) ------------------------------------
 * replaces index_points(), model/point_utils.py:60-83,
 * model/pointnet2_utils.py:41-57 and gather_points/group_points wrappers
 * (model/pointnet2/src/pointnet2_api.cpp:13-18).
 * out[b,s,:] = feat[b, idx[b,s], :]; idx [B,S] (S may be npoint*nsample).
 * Out-of-range indices (the reference's zero-hit value N) read as 0. */
int sug_gather_rows(const float* feat, int64_t ldf, const int32_t* idx,
                    int B, int N, int S, int C, float* out, int64_t ldo, void* stream);
/* dfeat[b, idx[b,s], :] += g[b,s,:]  (dfeat must be zero-initialised by the caller) */
int sug_scatter_add_rows(const float* g, int64_t ldg, const int32_t* idx,
                         int B, int N, int S, int C, float* dfeat, int64_t ldf, void* stream);
/* The same sum in ONE fixed order (reproducible bit for bit): sorted reverse lists of idx (which entries name point n,
 * ascending), then dfeat[b,n,:] = sum over n's entries of g -- every row of dfeat is WRITTEN (no zero fill by the caller).
 * ws: sug_scatter_rows_workspace(B, N, S) int32.  The reverse lists are built in LDS: sug_scatter_rows_ordered_supported()
 * is 0 when S entries per cloud do not fit (callers then use sug_scatter_add_rows: atomics, unordered, as the reference's
 * index_points backward). */
int64_t sug_scatter_rows_workspace(int B, int N, int S);
int sug_scatter_rows_ordered_supported(int B, int N, int S);
int sug_scatter_rows_ordered(const float* g, int64_t ldg, const int32_t* idx, int B, int N, int S, int C,
                             float* dfeat, int64_t ldf, int32_t* ws, void* stream);

/* out[b,s,c] = max_j feat[b, idx[b,s,j], c], arg[b,s,c] = the winning point index
 * (replaces index_points + torch.max(dim=-1), model/model_utils.py:122-123). */
int sug_group_max(const float* feat, int64_t ldf, const int32_t* idx, int B, int N, int S,
                  int ns, int C, float* out, int32_t* arg, void* stream);
/* The same over B = P * Bsrc "virtual clouds" (pass-major) that share the Bsrc clouds of feat: cloud b reads
 * feat[b % Bsrc] (the semantic and the node pass of a step in one launch; sug_group_max is the case Bsrc == B). */
int sug_group_max_shared(const float* feat, int64_t ldf, int Bsrc, const int32_t* idx, int B, int N, int S,
                         int ns, int C, float* out, int32_t* arg, void* stream);
/* Backward: dfeat[b, arg[b,s,c], c] += g[b,s,c].  CONTRACT: dfeat [B, N, ldf] must be ZERO-FILLED by the caller; it is not an
 * accumulate-into entry point.  (S <= 64: a fixed-order kernel that STORES the sums of the touched entries; otherwise float
 * atomics that ADD -- identical on a zeroed buffer, unspecified on any other.) */
int sug_group_max_bwd(const float* g, const int32_t* arg, int B, int N, int S, int C,
                      float* dfeat, int64_t ldf, void* stream);

/* ---- EdgeConv: neighbour gather + BN statistics + max over k -----------------
 * replaces get_graph_feature + conv_2d + max(dim=-1),
 * model/model_utils.py:188-210, :8-32 and model/Model.py:88-109, using
 * W.[x_j - x_i ; x_i] = W1.x_j + (W2-W1).x_i: the caller provides
 * PQ[b,n,:] = [P | Q] = x[b,n,:] . [W1 ; W2-W1]^T (one dense GEMM, [B*N, 2*Co],
 * row stride ldpq) and this kernel forms y[b,n,j,c] = P[b,idx[b,n,j],c] + Q[b,n,c]
 * on the fly, never materialising the k-expanded tensor.
 * Outputs: z[b,n,c]   = max_j y (gamma[c] >= 0) or min_j y (gamma[c] < 0) -- the
 *                       element BN+LeakyReLU (monotone per channel) maps to the max;
 *          arg[b,n,c] = the winning j (uint8);
 *          s1[b,n,c]  = sum_j y (may be NULL; needed for the backward);
 *          stats[0:Co] = sum y, stats[Co:2Co] = sum y^2 over all B*N*k values (fp64);
 *          ws: workspace, SUG_STATS_BLOCKS*2*Co floats.
 * Co % 4 == 0, Co <= 1024, k <= 255. */
int sug_edgeconv_fwd(const float* pq, int64_t ldpq, const int32_t* idx, const float* gamma,
                     int B, int N, int k, int Co, float* z, uint8_t* arg, float* s1,
                     double* stats, float* ws, void* stream);

/* Train-mode BatchNorm bookkeeping for a channel-last tensor: from fp64 sums of
 * `count` values per channel produce mean/rstd and the folded affine
 * scale = gamma*rstd, shift = beta - mean*scale; update running_mean/var the
 * way nn.BatchNorm2d does (momentum, unbiased running variance).
 * coef: [5,C] = scale, shift, mean, rstd, unbiased variance.  running_* may be NULL. */
int sug_bn_finalize(const double* stats, const float* gamma, const float* beta, int C,
                    double count, float eps, float momentum, float* running_mean,
                    float* running_var, float* coef, void* stream);

/* Fused forms used by the layer entry points: the producer's per-workgroup partial statistics are
 * folded (same fixed order) and turned into coef / running-buffer updates by one kernel.
 * sug_edgeconv_fwd_bn = sug_edgeconv_fwd + sug_bn_finalize (count = B*N*k);
 * sug_col_stats_bn    = sug_col_stats   + sug_bn_finalize (count = rows). */
int sug_edgeconv_fwd_bn(const float* pq, int64_t ldpq, const int32_t* idx, const float* gamma,
                        const float* beta, int B, int N, int k, int Co, float eps, float momentum,
                        float* running_mean, float* running_var, float* z, uint8_t* arg, float* s1,
                        float* coef, float* ws, void* stream);
int sug_col_stats_bn(const float* y, int64_t ldy, int64_t rows, int C, const float* gamma, const float* beta,
                     float eps, float momentum, float* running_mean, float* running_var, float* coef,
                     float* ws, void* stream);

/* sug_col_stats_bn for `groups` equal consecutive row blocks of y [rows, C] (the domain groups of a paired batch): coef
 * [groups][5][C], running buffers updated in group order; one launch pair for all groups where the layout allows. */
int sug_col_stats_bn_grouped(const float* y, int64_t ldy, int64_t rows, int C, int groups, const float* gamma,
                             const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                             float* coef, float* ws, void* stream);
/* The same with the bits of `groups` sug_col_stats_bn calls at every size: the grouped launch above shares one workspace
 * among the groups and, for tall inputs, cuts them into fewer workgroups than separate calls would (other fp32 partial
 * sums).  Here every group is cut and folded exactly as a call of its own, which needs a workspace block per group:
 * ws = groups * SUG_STATS_BLOCKS * 2*C floats (block g: the partial rows and the pivot row of group g).  One launch pair
 * for 2..16 groups in a float4 layout, else the calls one after the other (in block 0). */
int sug_col_stats_bn_groups_exact(const float* y, int64_t ldy, int64_t rows, int C, int groups, const float* gamma,
                                  const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                                  float* coef, float* ws, void* stream);

/* Replay of the running-statistics update for G more train-mode forwards over batches whose
 * statistics are already in coef [G,5,C] (rows 2 and 4 of each group), in group order, with
 * sug_bn_finalize's arithmetic: what nn.BatchNorm would do when the encoder prefix is evaluated
 * again on the same batch (model/Model.py:88-92 run once per forward call). */
int sug_bn_replay(const float* coef, int G, int C, float momentum, float* running_mean, float* running_var,
                  void* stream);
/* The same for n <= 16 layers in one launch (HOST arrays of n entries; a layer must not appear twice). */
int sug_bn_replay_multi(int n, const void* const* coef, const int32_t* G, const int32_t* C, const float* momentum,
                        void* const* running_mean, void* const* running_var, void* stream);

/* out[r,c] = act(scale[c]*z[r,c] + shift[c]), act = LeakyReLU(slope) (slope 0: ReLU,
 * slope 1: identity).  rows = B*N.  */
int sug_affine_act(const float* z, int64_t ldz, const float* coef, int64_t rows, int C,
                   float slope, float* out, int64_t ldo, void* stream);

/* Column sums for BN over rows of a channel-last tensor: stats[0:C] = sum,
 * stats[C:2C] = sum of squares (fp64).  Used for per-point conv_2d layers
 * (model/model_utils.py:8-32 on [B,C,N,1]).  ws: SUG_STATS_BLOCKS*2*C floats. */
int sug_col_stats(const float* y, int64_t ldy, int64_t rows, int C, double* stats, float* ws,
                  void* stream);
/* How the column reduction behind every BatchNorm entry point of this header (the statistics of sug_col_stats,
 * sug_col_stats_bn and its grouped forms: mode 0; the backward sums of sug_edgeconv_bwd_reduce / sug_bn_act_rows_bwd:
 * mode 1 with the [rows, C] intermediate a = scale*G, mode 2 without) would be launched over `groups` blocks of `rows`
 * rows each, row stride ld; own_ws: a workspace block per group (sug_col_stats_bn_groups_exact); aligned: every pointer
 * the mode reads or writes is 16-byte aligned.  plan (HOST, 4 ints) = float4 kernel (1) or scalar (0) | its lanes
 * along the channels (LX resp. CW) | rows per workgroup | workgroups per group, -1 where the launch is refused (more
 * than 16 groups, more partial rows than the workspace holds, a scalar layout with groups > 1 or in mode 2) and the
 * caller goes group by group.  The launch itself is computed by the same function.  Launches nothing, touches no
 * device memory. */
int sug_bn_rows_plan(int64_t rows, int C, int64_t ld, int groups, int own_ws, int mode, int aligned, int32_t* plan);

/* EdgeConv backward, step 1: G = gout * act'(scale*z+shift);
 * a[b,n,c] = scale[c]*G;  red[0:Co] = sum G, red[Co:2Co] = sum G*(z-mean)*rstd (fp64).
 * ws: SUG_STATS_BLOCKS*2*Co floats. */
int sug_edgeconv_bwd_reduce(const float* gout, int64_t ldg, const float* z, const float* coef,
                            int64_t rows, int Co, float slope, float* a, double* red, float* ws,
                            void* stream);
/* EdgeConv backward, step 2: dPQ [B*N, 2*Co] (row stride lddpq) from a, arg, s1, PQ,
 * the reverse lists and the reduced sums (exact train-mode BN gradient):
 *  dQ[n,c] = a[n,c] - (scale/M)*(k*dbeta + rstd*dgamma*(s1[n,c] - k*mean))
 *  dP[m,c] = sum_{(n,j) in rev(m)} (a[n,c]*[arg[n,c]==j] - (scale/M)*rstd*dgamma*Q[n,c])
 *            - (scale/M)*cnt[m]*(dbeta + rstd*dgamma*(P[m,c]-mean)),   M = B*N*k. */
int sug_edgeconv_bwd_scatter(const float* a, const uint8_t* arg, const float* s1,
                             const float* pq, int64_t ldpq, const int32_t* rev_off,
                             const int32_t* rev_ent, const float* coef, const double* red,
                             int B, int N, int k, int Co, float* dpq, int64_t lddpq, void* stream);

/* ---- weight gradient of a per-point linear layer ----------------------------------------------
 * dw[M,N] = g^T . x, g [R,M] (row stride ldg), x [R,N] (row stride ldx): the backward of every
 * 1x1 conv of the encoders (conv_2d / Conv1d, model/model_utils.py:13, model/Model.py:68-70)
 * w.r.t. its weight, R = B*N rows.  Split over row chunks, fp32 MFMA, ordered combine
 * (bit-reproducible).  ws: sug_linear_dw_workspace(R,M,N) floats. */
int64_t sug_linear_dw_workspace(int64_t R, int M, int N);
int sug_linear_dw(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t R, int M, int N,
                  float* dw, float* ws, void* stream);
/* Ordered fold of nchunk split-K partials part[nchunk][MN] -> dw[MN] (fp64 accumulation in a fixed order; no atomics,
 * no memset): the second half of sug_linear_dw, for partials a batched library GEMM over row chunks produced. */
int sug_linear_dw_fold(const float* part, int nchunk, int64_t MN, float* dw, void* stream);
/* The same launch also forms the bias gradient db[M] = column sums of g (the Conv bias, nn.Conv2d(bias=True) of
 * model/pointnet2_utils.py:172 and the nn.Linear biases of model/Ptran_transformer.py:17-33) from the g elements
 * it already holds, instead of a second pass over g.  db == NULL: sug_linear_dw. */
int sug_linear_dw_bias(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t R, int M, int N,
                       float* dw, float* db, float* ws, void* stream);

/* out[c] = sign * sum over rows of x[r, c] (fp32 sums of fp32 (dtype 0) or fp16 (1) rows, row stride ld): the bias
 * gradients autograd forms with sum(dim=0) / sum_to_size (nn.Linear / Conv biases, model/pointnet2_utils.py:172,
 * model/Ptran_transformer.py:17-33), without the memset torch's reduction issues for tall shapes.
 * ws: sug_colsum_workspace(rows, C) floats. */
int64_t sug_colsum_workspace(int64_t rows, int C);
int sug_colsum(const void* x, int64_t ld, int64_t rows, int C, int dtype, float sign, float* out, float* ws, void* stream);

/* Channel-attention gate of CALayer (model/Model.py:28-34): out = x * sigmoid(z) + x over n elements, z = the
 * output of the second 1x1 conv; backward dx = g * sigmoid(z) + g, dz = g * x * sigmoid'(z). */
int sug_gate_fwd(const float* x, const float* z, int64_t n, float* out, void* stream);
int sug_gate_bwd(const float* g, const float* x, const float* z, int64_t n, float* dx, float* dz, void* stream);
/* The gate followed by CALayer's BatchNorm1d (model/Model.py:442-449: attention_s / attention_t on [M, 4096] node
 * features, M = the clouds of one domain): out = BN(x * sigmoid(z) + x), train mode = batch statistics over the M rows
 * (two-pass) with the running buffers updated (null: not tracked), eval mode = running statistics; stat [2, C] = mean |
 * invstd for the backward, which returns dx, dz of the gate and dgamma, dbeta [C].  One launch each way. */
int sug_gate_bn_fwd(const float* x, const float* z, int M, int C, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int training, float eps, float momentum, float* out,
                    float* stat, void* stream);
int sug_gate_bn_bwd(const float* g, const float* x, const float* z, int M, int C, const float* gamma, const float* stat,
                    int training, float* dx, float* dz, float* dgamma, float* dbeta, void* stream);
/* The same for 1 <= layers <= 4 attention layers in one launch each way (attention_s / attention_t on the two row blocks
 * of a paired batch): layer l owns rows [l*M, (l+1)*M) of the dense x, z, out, g, dx, dz [layers*M, C], stat + l*2C and
 * dgb + l*2C (dgb [layers][2][C] = dgamma | dbeta); gamma, beta, running_mean, running_var are HOST arrays of `layers`
 * device pointers (the two buffer arrays, or their entries, null: not tracked).  Per layer bit for bit the calls above. */
int sug_gate_bn_fwd_multi(int layers, const float* x, const float* z, int M, int C, const void* const* gamma,
                          const void* const* beta, void* const* running_mean, void* const* running_var, int training,
                          float eps, float momentum, float* out, float* stat, void* stream);
int sug_gate_bn_bwd_multi(int layers, const float* g, const float* x, const float* z, int M, int C,
                          const void* const* gamma, const float* stat, int training, float* dx, float* dz, float* dgb,
                          void* stream);

/* ---- Channel attention (CALayer, model/Model.py:16-34) for up to two attention layers per launch ------------------
 * v [M, C] -> h = relu(v . W0^T + b0) [M, Hd] -> z = h . W2^T + b2 [M, C] (the two 1x1 Conv2d on a 1x1 map; the gate
 * v * sigmoid(z) + v and the BatchNorm1d behind it are sug_gate_bn_fwd / _bwd).  Net_MDA has two such layers
 * (attention_s on the source rows, attention_t on the target rows of a paired batch): x [layers * M, C] holds the rows of
 * layer 0 first; W0 / b0 / W2 / b2 (and the gradient outputs) are HOST arrays of `layers` device pointers.
 * M <= 64, Hd = 512, C % 512 == 0 (C = 4096).  Scratch: hp [layers][C/512][M][Hd], dhp [layers][C/32][M][Hd].
 * Forward writes h [layers][M][Hd] and z [layers*M, C]; backward takes dz (from sug_gate_bn_bwd) and dxg (the gate's
 * own input gradient, added to dx; may be null) and writes dW0 [Hd,C], db0 [Hd], dW2 [C,Hd], db2 [C] per layer, dh
 * [layers][M][Hd] (scratch) and dx [layers*M, C] (row stride lddx).  Fixed summation order, no atomics. */
int sug_calayer_supported(int layers, int M, int C, int Hd);
int sug_calayer_fwd(int layers, const float* x, int64_t ldx, int M, int C, int Hd, const float* const* W0,
                    const float* const* b0, const float* const* W2, const float* const* b2, float* hp, float* h, float* z,
                    void* stream);
int sug_calayer_bwd(int layers, const float* x, int64_t ldx, int M, int C, int Hd, const float* const* W0,
                    const float* const* W2, const float* h, const float* dz, const float* dxg, float* const* dW0,
                    float* const* db0, float* const* dW2, float* const* db2, float* dhp, float* dh, float* dx, int64_t lddx,
                    void* stream);

/* ---- Classifier heads: Linear layers with M <= 128 rows, one launch per layer for up to two heads ----------------
 * Pointnet_c (model/Model.py:412-449): fc_layer(1024, 512) -> Dropout -> fc_layer(512, 256) [= mid feature] -> Dropout ->
 * Linear(256, num_class), fc_layer = Linear -> LayerNorm -> LeakyReLU(0.2) / ReLU (model/model_utils.py:35-57); Net_MDA
 * runs two such heads (c1, c2) on the same pooled feature.  All per-head operands are HOST arrays of `heads` device
 * pointers (entries / whole arrays may be null where noted).  Every sum runs in a fixed order.  8 launches replace the
 * ~47 library / elementwise launches of the two heads per training step.
 *
 * sug_head_linear_fwd: z[h] [M, No] = pro(in[h]) . W[h]^T + bias[h].  pro != 0: in[h] is the PREVIOUS layer's
 *   pre-LayerNorm output and pro(v) = Dropout(act(LayerNorm(v; gamma[h], beta[h]))), dropout from uniform randoms u[h]
 *   [M, K] (keep when u >= p_drop, scale 1/(1-p_drop); u null: no dropout); side outputs stats[h] [M, 2] = mean | rstd of
 *   the rows of in[h] and act[h] [M, K] = the activation before the dropout (null: not written).
 *   K % 256 == 0 (pro: K <= 1024), No <= 32, or a multiple of 4 up to 64 (a last layer: no epilogue), or 256 or 512,
 *   M <= 128 (sug_head_linear_supported).
 * sug_head_ln_bwd: dz[h] [M, No] = gradient of a layer's Linear output z[h] from gup[h] [M, No] (row stride ldg) = the
 *   gradient of Dropout(act(LayerNorm(z))), plus gextra[h] = a gradient of the activation BEFORE the dropout (the mid
 *   feature's; may be null); also dgamma[h], dbeta[h] [No] and db[h] [No] = the column sums of dz (null: none).
 *   No = 256 or 512.
 * sug_head_linear_bwd: from dz[h] [M, No] (row stride ldg): dW[h] [No, K] = dz^T . a, db[h] [No] = column sums of dz
 *   (null: none) and the input gradient dz . W[h] [M, K] (row stride ldda): da[h] per head, or with sum_da != 0 the sum
 *   over the heads into da[0] (the heads share their input).  The layer input a is in[h] itself (pro == 0) or
 *   pro(in[h]) recomputed from stats_in / gamma_in / beta_in / u_in (dropout probability p_drop_in). */
int sug_head_linear_supported(int M, int K, int No, int pro, int epi);
int sug_head_linear_fwd(int heads, const float* const* in, int64_t ldin, const float* const* W, const float* const* bias,
                        float* const* z, const float* const* gamma, const float* const* beta, const float* const* u,
                        float* const* stats, float* const* act, int M, int K, int No, int pro, float slope, float eps,
                        float p_drop, void* stream);
int sug_head_ln_bwd(int heads, const float* const* gup, int64_t ldg, const float* const* z, const float* const* stats,
                    const float* const* gamma, const float* const* beta, const float* const* u,
                    const float* const* gextra, float* const* dz, float* const* dgamma, float* const* dbeta,
                    float* const* db, int M, int No, float slope, float p_drop, void* stream);
int sug_head_linear_bwd(int heads, int sum_da, const float* const* dz, int64_t ldg, const float* const* in, int64_t ldin,
                        const float* const* stats_in, const float* const* gamma_in, const float* const* beta_in,
                        const float* const* u_in, const float* const* W, float* const* dW, float* const* db,
                        float* const* da, int64_t ldda, int M, int K, int No, int pro, float slope, float p_drop_in,
                        void* stream);

/* ---- LayerNorm + (Leaky)ReLU of the FC heads ---------------------------------------------------
 * fc_layer (model/model_utils.py:35-57: nn.Linear -> nn.LayerNorm -> LeakyReLU(0.2) / ReLU) behind the Linear:
 * y = act(LN(x)) over rows of x [rows, C] (C <= 1024), stat [rows, 2] = mean | rstd for the backward.
 * Backward: dx [rows,C], dgamma, dbeta [C] (rows summed in order); ws: rows*C floats. */
int sug_ln_act_fwd(const float* x, const float* gamma, const float* beta, int rows, int C, float eps, float slope,
                   float* y, float* stat, void* stream);
int sug_ln_act_bwd(const float* g, const float* x, const float* gamma, const float* beta, const float* stat, int rows,
                   int C, float slope, float* dx, float* dgamma, float* dbeta, float* ws, void* stream);

/* ---- optimizer step ------------------------------------------------------------------------
 * torch.optim.Adam (no amsgrad; L2 weight decay added to the gradient; bias correction; eps
 * outside the square root) over T tensors in one launch per 384 tensors: the update of
 * optimizer_g / optimizer_c / optimizer_dis, train_dg_single_gpu.py:193-203 and :333-335.
 * table: device int64 [T,4] = {param ptr, exp_avg ptr, exp_avg_sq ptr, numel}; block_first:
 * device + host copies of the int32 [T+1] prefix sum of ceil(numel / sug_adam_chunk());
 * grads_host: HOST array of T device pointers (null = tensor without gradient, skipped);
 * bias_corr1 = 1 - beta1^step, bias_corr2 = 1 - beta2^step.  Hyper-parameters are doubles and the
 * derived constants (1 - beta, lr / bias_corr1) are rounded to fp32 once, as torch does. */
int sug_adam_chunk(void);
int sug_adam_step(const int64_t* table, const int32_t* block_first, const int32_t* block_first_host, int T,
                  const void* const* grads_host, double lr, double beta1, double beta2, double eps,
                  double weight_decay, double bias_corr1, double bias_corr2, void* stream);
/* Same update for replay from a hipGraph: the step count is a device int32 (advanced by the call),
 * the bias-correction scalars are derived on the device into scalars_dev[2]; gradient pointers must
 * be stable across replays (graph-private allocations are).  lr_dev (may be null): the learning rate as
 * one device-resident double that overrides `lr`, so that a learning-rate schedule
 * (train_dg_single_gpu.py:194-212) changes a value in memory and ONE captured graph serves every epoch. */
int sug_adam_step_capturable(const int64_t* table, const int32_t* block_first, const int32_t* block_first_host,
                             int T, const void* const* grads_host, double lr, double beta1, double beta2,
                             double eps, double weight_decay, int32_t* step_dev, float* scalars_dev,
                             const double* lr_dev, void* stream);

/* The three optimizer steps of train_dg_single_gpu.py:333-335 in ONE update launch.  optimizer_dis and optimizer_g both
 * own the encoder's parameters (:193-203), so a tensor carries an ordered list of up to SUG_ADAM_CHAIN_SLOTS
 * (exp_avg, exp_avg_sq, bucket) slots; the updates of a tensor are applied one after the other on the value held in
 * registers, each with exactly sug_adam_step's arithmetic: bit-identical to stepping the optimizers in that order, with
 * the parameter and its gradient read and written once.  A bucket = one set of hyper-parameters + one step count
 * (at most SUG_ADAM_CHAIN_BUCKETS).
 * table: device int64 [T,8] = {param, numel, exp_avg0, exp_avg_sq0, exp_avg1, exp_avg_sq1,
 *        nslots | bucket0 << 8 | bucket1 << 16, 0};  block_map: device int32 [blocks,2] = (tensor, chunk) per workgroup of
 *        sug_adam_chain_chunk() elements, tensors in table order;  block_first_host: HOST int32 [T+1] prefix sum of the
 *        tensors' workgroup counts;  grads_host: HOST array of T device pointers (null = skipped);
 * hyper_host: HOST double [nbuckets,6] = {lr, beta1, beta2, eps, weight_decay, t} with t the step count the update
 *        belongs to (1-based; read only when steps_dev is null);
 * steps_dev / scalars_dev (both or neither): device int32 [nbuckets] advanced by the call and float [nbuckets,2] scratch,
 *        for replay from a hipGraph (as sug_adam_step_capturable); lr_dev (may be null): device double [nbuckets]
 *        overriding hyper_host's lr. */
#define SUG_ADAM_CHAIN_SLOTS 2
#define SUG_ADAM_CHAIN_BUCKETS 8
int sug_adam_chain_chunk(void);
int sug_adam_chain_step(const int64_t* table, const int32_t* block_map, const int32_t* block_first_host, int T,
                        const void* const* grads_host, int nbuckets, const double* hyper_host, int32_t* steps_dev,
                        float* scalars_dev, const double* lr_dev, void* stream);

/* ---- SA-node module glue (adapt_layer_off, model/model_utils.py:103-128) --------------------
 * off[b,s,:] = mean_j tanh(proj[b,g_j,:] - proj[b,f,:]) * (loc[b,g_j,:] - loc[b,f,:]),
 * nloc = loc[b,f,:] + off, with f = fidx[b,s], g_j = gidx[b,s,j], proj = fea . W_pred_offset^T
 * ([B,N,3]; :110-119).  Backward: dproj [B,N,3], written entirely by the call (accumulated per cloud in LDS). */
int sug_node_offset_fwd(const float* proj, const float* loc, const int32_t* fidx,
                        const int32_t* gidx, int B, int N, int S, int ns, float* off, float* nloc,
                        void* stream);
int sug_node_offset_bwd(const float* proj, const float* loc, const int32_t* fidx,
                        const int32_t* gidx, const float* goff, int B, int N, int S, int ns,
                        float* dproj, void* stream);
/* Forward over B = P * Bsrc pass-major virtual clouds: loc / fidx / gidx / off / nloc are [B,...], proj is [Bsrc,N,3]
 * and cloud b reads proj[b % Bsrc].  Same lanes and order per cloud as sug_node_offset_fwd (the case Bsrc == B). */
int sug_node_offset_fwd_shared(const float* proj, int Bsrc, const float* loc, const int32_t* fidx,
                               const int32_t* gidx, int B, int N, int S, int ns, float* off, float* nloc,
                               void* stream);
/* out[b,n,:] = [ fea[b,n,0:C1] | sum_t w_t * node[b, idx3[b,n,t], 0:C2] ] with the inverse-distance
 * weights of upsample_inter (model/point_utils.py:156-162) from the 3-NN distances d3 (C1 == 0: fea may be null).
 * Backward (g = d out): dnode [B,S,C2] and dnloc [B,S,3] (both zero-initialised by the caller,
 * atomics); dnloc carries d3's gradient through d = |xyz - nloc|^2; d fea is g[:, :, 0:C1]. */
int sug_interp3_cat_fwd(const float* fea, int64_t ldf, int C1, const float* node,
                        const int32_t* idx3, const float* d3, int B, int N, int S, int C2,
                        float* out, int64_t ldo, void* stream);
/* Forward over B = P * Bsrc pass-major virtual clouds: node / idx3 / d3 / out are [B,...], fea is [Bsrc,N,ldf] and
 * cloud b copies fea[b % Bsrc] (sug_interp3_cat_fwd is the case Bsrc == B). */
int sug_interp3_cat_fwd_shared(const float* fea, int64_t ldf, int C1, int Bsrc, const float* node,
                               const int32_t* idx3, const float* d3, int B, int N, int S, int C2,
                               float* out, int64_t ldo, void* stream);
int sug_interp3_cat_bwd(const float* g, int64_t ldg, int C1, const float* node, const int32_t* idx3,
                        const float* d3, const float* xyz, const float* nloc, int B, int N, int S,
                        int C2, float* dnode, float* dnloc, void* stream);
/* The same gradient by destination node over the (sorted) reverse lists of idx3: no accumulation in LDS, fixed
 * summation order; dnode / dnloc are written entirely.  Scratch: rev_off [B,S+1], rev_ent [B,3N] ints, ddw [B,N,6] floats. */
int sug_interp3_cat_bwd_lists(const float* g, int64_t ldg, int C1, const float* node, const int32_t* idx3,
                              const float* d3, const float* xyz, const float* nloc, int B, int N, int S, int C2,
                              int32_t* rev_off, int32_t* rev_ent, float* ddw, float* dnode, float* dnloc,
                              void* stream);
/* 1 when the reverse lists of idx3 (3N entries per cloud) fit the LDS-resident build sug_interp3_cat_bwd_lists needs;
 * 0: zero-fill dnode / dnloc and call sug_interp3_cat_bwd (float atomics: not reproducible bit for bit). */
int sug_interp3_cat_bwd_lists_supported(int B, int N, int S);

/* ---- BatchNorm(+act) on rows: backward, and the fused DGCNN tail ----------------------------
 * Exact train-mode BN gradient for a per-point layer (conv_2d on [B,C,N,1],
 * model/model_utils.py:8-32): with a = scale*G and red = (sum G, sum G*xhat) from
 * sug_edgeconv_bwd_reduce (z := y, the BN input),
 *   dy = a - (scale/rows) * (dbeta + xhat*dgamma).   a: dense [rows,C]. */
int sug_bn_bwd_apply(const float* a, const float* y, int64_t ldy, const float* coef,
                     const double* red, int64_t rows, int C, float* dy, int64_t lddy, void* stream);

/* BatchNorm1d -> LeakyReLU(slope) -> max over N | mean over N  (model/Model.py:112-116),
 * one read of y [B,N,C]; coef from sug_bn_finalize.  out_max/out_mean [B,C] with row stride ld_pool (ld_pool = 2C and
 * out_mean = out_max + C: the two land in the torch.cat((max, mean), 1) of Model.py:116 directly), arg [B,C] dense =
 * row of the (first) maximum.  ws: workspace of 12*B*C floats (per-chunk partial max/sum/arg). */
int sug_bn_act_pool_fwd(const float* y, int64_t ldy, const float* coef, int B, int N, int C,
                        float slope, float* out_max, float* out_mean, int64_t ld_pool, int32_t* arg, float* ws,
                        void* stream);
/* Backward of the above including the BN statistics terms: dy [B,N,C] (row stride lddy),
 * red[0:C] = dbeta, red[C:2C] = dgamma (fp64).  train = 0: statistics are constants (eval mode).
 * gmax / gmean [B,C] with row stride ld_pool (the two column halves of the gradient of the concatenated feature).
 * ws: SUG_STATS_BLOCKS*2*C floats. B <= SUG_STATS_BLOCKS/4. */
int sug_bn_act_pool_bwd(const float* y, int64_t ldy, const float* coef, const float* gmax,
                        const float* gmean, int64_t ld_pool, const int32_t* arg, int B, int N, int C, float slope,
                        int train, double* red, float* ws, float* dy, int64_t lddy, void* stream);

/* ---- layer-level entry points ---------------------------------------------------------------
 * One call per BatchNorm-carrying layer, chaining the kernels above for `groups` equal contiguous
 * parts of the batch (the domains the reference sends through the network in separate forward
 * calls: statistics, normalisation and running-buffer updates are per part, in order).  coef is
 * [groups,5,C]: written in training mode, read in eval mode (caller fills it from the running
 * buffers).  stats: fp64 [2C] scratch; ws: SUG_STATS_BLOCKS*2*C floats.
 *
 * EdgeConv layer = get_graph_feature + conv_2d + max over k (model_utils.py:188-210, :8-32,
 * Model.py:88-109): z/arg/s1 as sug_edgeconv_fwd, out [B,N,Co] (row stride ldo). */
int sug_edgeconv_layer_fwd(const float* pq, int64_t ldpq, const int32_t* idx, const float* gamma,
                           const float* beta, int B, int N, int k, int Co, int groups, int training,
                           float eps, float momentum, float slope, float* running_mean,
                           float* running_var, float* z, uint8_t* arg, float* s1, float* coef,
                           float* out, int64_t ldo, double* stats, float* ws, void* stream);
/* Which kernel the layer above (backward = 0: the gather / reduce of sug_edgeconv_fwd, _fwd_bn and the layer forward,
 * B = the clouds of the call, i.e. of one group where the layer runs group by group) or sug_edgeconv_layer_bwd's
 * scatter (backward = 1) takes for a shape: 1 = the LDS-resident kernel (k == 20, Co % 16 == 0 and the cloud's slice
 * within the LDS budget: N <= 2272 forward, N <= 1094 backward; the backward not with SUG_EDGECONV_BWD_LEGACY in the
 * environment), 0 = the generic one.  The shape part of the dispatch's own condition -- the dispatch calls the same
 * function; with pointers that are not 16-byte aligned it takes the generic kernel whatever this says.  Launches
 * nothing; 0 for a shape with a non-positive extent. */
int sug_edgeconv_path(int backward, int B, int N, int k, int Co);
/* The same layer with the 1x1 convolution inside the gather kernel (edgeconv_fused.hip): x [B*N, Cin] rows (row
 * stride ldx; Cin in {3, 64, 128}), wcat [2Co, Cin] = [W1 ; W2-W1] of the layer's weight W = [W1 | W2] [Co, 2Cin]
 * (sug_edge_weight_split), qbias [Co] = the conv bias or NULL.  A workgroup = (cloud, 16-channel slice) forms its
 * slice of [P | Q] = x.wcat^T with v_mfma_f32_32x32x2_f32 straight into the LDS image its gathers read; [P|Q] is
 * never written to HBM unless pq_out (row stride ldpq >= 2Co) is given -- sug_edgeconv_layer_bwd wants it.  Two
 * launches: MFMA + gather + BatchNorm partial rows, then statistics fold + BatchNorm + LeakyReLU (the fold runs in
 * every workgroup of the second launch; coef [groups,5,Co] and the running buffers are written by one of them).
 * Requires k == 20, Co % 16 == 0, N*64 bytes of LDS (N <= 2400): sug_edgeconv_fused_supported.
 * ws: SUG_STATS_BLOCKS*2*Co floats.  training = 0: coef is an input (running-statistics coefficients).
 * arg, s1 and pq_out serve the backward only and may be NULL (a forward without autograd writes z and out alone). */
int sug_edgeconv_fused_supported(int N, int k, int Cin, int Co);
int sug_edgeconv_fused_layer_fwd(const float* x, int64_t ldx, int Cin, const float* wcat, const float* qbias,
                                 const int32_t* idx, const float* gamma, const float* beta, int B, int N, int k,
                                 int Co, int groups, int training, float eps, float momentum, float slope,
                                 float* running_mean, float* running_var, float* z, uint8_t* arg, float* s1,
                                 float* pq_out, int64_t ldpq, float* coef, float* out, int64_t ldo, float* ws,
                                 void* stream);
/* (All three layer backward entry points take `dgb`: NULL, or fp32 [2C] receiving the BatchNorm parameter
 * gradients dbeta | dgamma summed over the groups -- sug_fold_groups on `red`.)
 * Its backward: reverse neighbour lists (rev_off [B,N+1], rev_ent [B,N*k], scratch), per-group BN
 * sums red [groups+1, 2Co] (row g: dbeta | dgamma; the spare last row must be zero when
 * training = 0), a [B,N,Co] scratch, dpq [B,N,2Co] (row stride lddpq). */
int sug_edgeconv_layer_bwd(const float* gout, int64_t ldg, const float* z, const uint8_t* arg,
                           const float* s1, const float* pq, int64_t ldpq, const int32_t* idx,
                           const float* coef, int B, int N, int k, int Co, int groups, int training,
                           float slope, float* a, double* red, int32_t* rev_off, int32_t* rev_ent,
                           float* dpq, int64_t lddpq, float* ws, float* dgb, void* stream);
/* ---- first layer of a set-abstraction MLP on the neighbour lists (no grouped tensor) ----------------
 * Replaces index_points(xyz, idx) - new_xyz, index_points(points, idx), torch.cat, mlp_convs[0],
 * mlp_bns[0], F.relu of PointNetSetAbstraction.forward (model/pointnet2_utils.py:107-135, 193-198).
 * W.[x_j - c_s ; f_j] + b = P[j] - Q[s] with P [B,N,C] = W.[x ; f] per point (row stride ldp) and
 * Q [B,S,C] = Wx.c - b per centroid, both formed by the caller (two small GEMMs); idx [B,S,ns] are the
 * ball-query lists (values in [0,N)).  Forward: train-mode statistics of y = P[idx] - Q over the B/groups*S*ns
 * rows of each domain group (coef [groups,5,C] as the other BatchNorm entry points; training = 0: coef is
 * an input), Z [B,S,ns,C] = relu(BN(y)).  C in {64, 128}.  ws: SUG_STATS_BLOCKS*2*C floats.
 * Backward: gz [B,S,ns,C] -> dP [B,N,C] (by destination point over the reverse lists of idx: plain stores, no
 * atomics; the order of a point's sum is as unordered as index_points' backward in the reference), dQ [B,S,C];
 * red [groups+1, 2C] doubles (row g: dbeta | dgamma, the spare last row zero for training = 0); scratch:
 * rev_off [B,N+1], rev_ent [B,S*ns] ints, segsum [2,B,S,C] floats; dgb: NULL or fp32 [2C] = red folded over the groups. */
int sug_sa_first_fwd(const float* P, int64_t ldp, const float* Q, const int32_t* idx, int B, int N, int S,
                     int ns, int C, int groups, const float* gamma, const float* beta, int training,
                     float eps, float momentum, float* running_mean, float* running_var, float* coef,
                     float* Z, float* ws, void* stream);
int sug_sa_first_bwd(const float* gz, const float* P, int64_t ldp, const float* Q, const int32_t* idx, int B,
                     int N, int S, int ns, int C, int groups, int training, const float* coef, double* red,
                     int32_t* rev_off, int32_t* rev_ent, float* segsum, float* dP, float* dQ, float* ws, float* dgb,
                     void* stream);
/* The same layer with the coordinate part taken from the difference the reference forms (pointnet2_utils.py:120
 * grouped_xyz - new_xyz): y = Pf[j] + bias + Wx . (xyz[j] - cent[s]), Pf [B,N,C] = Wf . f per point (NULL when the layer has no
 * input features), xyz [B,N,3], cent [B,S,3] (= new_xyz), Wx [C,3] with row stride ldw (the coordinate columns of the conv
 * weight), bias [C] or NULL.  (An alternative to P[j] - Q[s] kept for diagnostics: measured equally accurate against fp64
 * and 1 % slower per step, so the host mirror uses it only with SUG_SA_FIRST_GEO=1.)  Backward: the same dP (= the gradient of Pf AND of Wx . xyz as autograd sees them) and
 * dQ (= -sum_j dy per centroid: the gradient of Wx . cent - bias). */
int sug_sa_first_geo_fwd(const float* Pf, int64_t ldp, const float* xyz, const float* cent, const float* Wx, int ldw,
                         const float* bias, const int32_t* idx, int B, int N, int S, int ns, int C, int groups,
                         const float* gamma, const float* beta, int training, float eps, float momentum,
                         float* running_mean, float* running_var, float* coef, float* Z, float* ws, void* stream);
int sug_sa_first_geo_bwd(const float* gz, const float* Pf, int64_t ldp, const float* xyz, const float* cent, const float* Wx,
                         int ldw, const float* bias, const int32_t* idx, int B, int N, int S, int ns, int C, int groups,
                         int training, const float* coef, double* red, int32_t* rev_off, int32_t* rev_ent, float* segsum,
                         float* dP, float* dQ, float* ws, float* dgb, void* stream);

/* conv_2d / Conv1d + BatchNorm + (Leaky)ReLU on rows (model_utils.py:8-32, pointnet2_utils.py:195-198):
 * out = act(BN(y)), y [rows,C]. */
int sug_bn_act_rows_fwd(const float* y, int64_t ldy, int64_t rows, int C, int groups, const float* gamma,
                        const float* beta, int training, float eps, float momentum, float slope,
                        float* running_mean, float* running_var, float* coef, float* out, int64_t ldo,
                        double* stats, float* ws, void* stream);
/* Backward: a [rows,C] scratch (= dy when training = 0), red [groups,2C], dy [rows,C]; y dense. */
int sug_bn_act_rows_bwd(const float* gout, int64_t ldg, const float* y, int64_t ldy, const float* coef,
                        int64_t rows, int C, int groups, int training, float slope, float* a, double* red,
                        float* dy, float* ws, float* dgb, void* stream);
/* bn5 -> LeakyReLU -> max | mean over the points (Model.py:112-116) per group; ws_pool: 12*(B/groups)*C floats. */
int sug_bn_act_pool_layer_fwd(const float* y, int64_t ldy, int B, int N, int C, int groups,
                              const float* gamma, const float* beta, int training, float eps, float momentum,
                              float slope, float* running_mean, float* running_var, float* coef,
                              float* out_max, float* out_mean, int64_t ld_pool, int32_t* arg, double* stats, float* ws_stats,
                              float* ws_pool, void* stream);
int sug_bn_act_pool_layer_bwd(const float* y, int64_t ldy, const float* coef, const float* gmax,
                              const float* gmean, int64_t ld_pool, const int32_t* arg, int B, int N, int C, int groups,
                              float slope, int training, double* red, float* ws, float* dy, int64_t lddy,
                              float* dgb, void* stream);
/* The same two entry points with every domain group in each launch (train mode, 2..16 groups, float4 layout; B*4 <=
 * SUG_STATS_BLOCKS and C/4 dividing 256 for the backward): 2 + 2 launches forward and 3 backward whatever `groups` is,
 * bit for bit the results of the per-group loops above, which run in every other case.  Other workspaces:
 * ws_stats = groups * SUG_STATS_BLOCKS * 2*C floats (sug_col_stats_bn_groups_exact), ws_pool = 12*B*C floats. */
int sug_bn_act_pool_groups_fwd(const float* y, int64_t ldy, int B, int N, int C, int groups,
                               const float* gamma, const float* beta, int training, float eps, float momentum,
                               float slope, float* running_mean, float* running_var, float* coef,
                               float* out_max, float* out_mean, int64_t ld_pool, int32_t* arg, double* stats, float* ws_stats,
                               float* ws_pool, void* stream);
int sug_bn_act_pool_groups_bwd(const float* y, int64_t ldy, const float* coef, const float* gmax,
                               const float* gmean, int64_t ld_pool, const int32_t* arg, int B, int N, int C, int groups,
                               float slope, int training, double* red, float* ws, float* dy, int64_t lddy,
                               float* dgb, void* stream);

/* ---- per-point MLP layer fused with the max over a group of rows ------------------------------
 * replaces `conv_2d(K, Co)` (1x1 Conv2d + bias -> BatchNorm2d -> ReLU) followed by the max over the
 * points of a cloud: Pointnet_g.conv5 + torch.max (model/Model.py:274-279), transform_net.conv2d3 +
 * maxpool (model/model_utils.py:72-79), Pointnet_cls (model/model_pointnet.py:36-48); and the last
 * layer of a set-abstraction MLP + max over nsample (model/pointnet2_utils.py:193-207).
 * y = x . w^T + bias ([rows,K] x [Co,K]^T, an ascending-k fp32 fma chain on the matrix pipe) is never
 * stored.  Rows form segments of `seg` consecutive rows (a cloud's N points, or a group's nsample
 * points); per (segment, channel) the kernel keeps zext = max_rows y (gamma >= 0) or min_rows y
 * (gamma < 0) -- the element BN + (Leaky)ReLU maps to the max -- and arg = its row inside the segment
 * (lowest row on ties), and it accumulates the BatchNorm sums of y as per-row-block partial rows in
 * ws ([*nblk][2*Co]: sum | sum of squares; *nblk <= SUG_STATS_BLOCKS; ws = SUG_STATS_BLOCKS*2*Co floats: when the
 * grid would leave CUs idle, a segment of >= 1024 rows is split over up to 8 workgroups -- more partial rows, and the
 * rows of ws behind them serve as scratch for the partial extremes, combined in part order by a second small launch:
 * same zext / arg bit for bit).
 * K in {64, 128}; Co % 128 == 0; seg % 32 == 0; rows % seg == 0; x, w 16-byte aligned, ldx % 4 == 0. */
int sug_pointmlp_max_fwd(const float* x, int64_t ldx, int64_t rows, int K, const float* w, const float* bias,
                         const float* gamma, int Co, int seg, float* zext, int32_t* arg, float* ws, int* nblk,
                         void* stream);
/* y[r,:] = x[r,:] . w^T (+ bias) on the same fp32 MFMA pipeline, y stored ([rows, Co], row stride ldy): the
 * per-point 1x1 convolution itself (conv_2d, model/model_utils.py:8-32) where no reduction follows, e.g. the
 * EdgeConv operand PQ = x . [W1 ; W2-W1]^T.  Same shape limits as sug_pointmlp_max_fwd (rows arbitrary). */
int sug_rows_gemm(const float* x, int64_t ldx, int64_t rows, int K, const float* w, const float* bias, int Co,
                  float* y, int64_t ldy, void* stream);
/* Layer entry point: the above per domain group, then the BatchNorm coefficients (training: batch
 * statistics + running-buffer update; eval: coef read, caller fills it) and
 * out[s,c] = LeakyReLU_slope(scale[c]*zext[s,c] + shift[c]), out [rows/seg, Co] (row stride ldo).
 * coef [groups,5,Co]; ws SUG_STATS_BLOCKS*2*Co floats. */
int sug_pointmlp_max_layer_fwd(const float* x, int64_t ldx, int64_t rows, int K, const float* w, const float* bias,
                               const float* gamma, const float* beta, int Co, int seg, int groups, int training,
                               float eps, float momentum, float slope, float* running_mean, float* running_var,
                               float* zext, int32_t* arg, float* coef, float* out, int64_t ldo, float* ws,
                               void* stream);
/* The same layer fed with the PRE-activation rows y [rows, K] of the layer in front (round 5; model/pointnet2_utils.py:
 * 193-207, layers i and i+1 of a set-abstraction MLP): that layer's BatchNorm + (Leaky)ReLU -- xcoef [groups][5][K] as
 * sug_col_stats_bn / sug_bn_finalize write it (rows 0 / 1 = scale / shift), slope xslope -- is applied to the x operand on
 * its way into LDS.  zout [rows, ldz] (may be null): the activated rows z = act(scale * y + shift), written once, for a
 * backward (sug_pointmlp_max_bwd_sparse takes z as its x) or for a caller that needs z itself.  Replaces
 * sug_affine_act on [rows, K] + this kernel's read of its output. */
int sug_pointmlp_max_layer_fwd_xf(const float* y, int64_t ldy, int64_t rows, int K, const float* xcoef, float xslope,
                                  float* zout, int64_t ldz, const float* w, const float* bias, const float* gamma,
                                  const float* beta, int Co, int seg, int groups, int training, float eps, float momentum,
                                  float slope, float* running_mean, float* running_var, float* zext, int32_t* arg,
                                  float* coef, float* out, int64_t ldo, float* ws, void* stream);
/* Backward, the terms that follow the winning rows n*(s,c) = s*seg + arg[s,c], with
 * a[s,c] = scale[c] * gout[s,c] * act' (sug_edgeconv_bwd_reduce on the [rows/seg, Co] tensors):
 *   dx[n*(s,c), :] += a[s,c] * w[c,:]   (dx holds the dense BatchNorm-statistics term -(x.A + v) or zeros)
 *   dw[c,:]         = sum_s a[s,c] * x[n*(s,c), :]
 * both in a fixed summation order (bit-reproducible).  ws: sug_pointmlp_max_bwd_workspace floats. */
/* The dense (rank-K) BatchNorm-statistics terms of the same backward, dy = a_full - k1 - k2*y over ALL rows:
 *   dx = ... - (x.A + v),  A = W^T diag(k2) W,  v = (k1 + k2*b).W;   dW = ... - kb (x) sum(x) - diag(k2) W.(X^T X)
 * _coef: from one group's coefficients coef [5,Co] and folded sums red [2Co] (dbeta | dgamma) over `rows` rows:
 *   k2 = scale/rows*rstd*dgamma, kb = scale/rows*(dbeta - mean*rstd*dgamma) + k2*bias (fp64), and the operands
 *   nkb = -kb [Co], nwk = -diag(k2).W [Co,K] of the two small library products -A = nwk^T.W, -v = nkb.W.
 * _dwfix: dw += dws - (kb (x) sx + diag(k2) W.XtX) with XtX [K,K], sx [K] from sug_linear_dw_bias(x, x)
 *   (with_stats = 0, eval mode: dw += dws). */
int sug_pointmlp_max_bwd_coef(const float* coef, const double* red, const float* bias, const float* w, int64_t rows,
                              int K, int Co, float* kb, float* k2, float* nkb, float* nwk, void* stream);
int sug_pointmlp_max_bwd_dwfix(float* dw, const float* dws, const float* kb, const float* k2, const float* w,
                               const float* xtx, const float* sx, int K, int Co, int with_stats, void* stream);
int64_t sug_pointmlp_max_bwd_workspace(int64_t rows, int K, int Co, int seg);
int sug_pointmlp_max_bwd_sparse(const float* a, const int32_t* arg, const float* x, int64_t ldx, const float* w,
                                int64_t rows, int K, int Co, int seg, float* dx, int64_t lddx, float* dw,
                                float* ws, void* stream);

/* ---- two-layer EdgeConv block --------------------------------------------------------------------
 * The EdgeConv block with TWO 1x1 convolutions in front of the max over the k neighbours: the blocks of the DGCNN
 * part-segmentation network, and transform_net's DGCNN form (model/model_utils.py:70-77).  With [P | Q] formed by the
 * caller as for sug_edgeconv_fwd (bias on the Q half):
 *   y1[b,i,j,c] = P[b, idx[b,i,j], c] + Q[b,i,c]                   one fp32 add
 *   a1          = LeakyReLU_s1(scale1 * y1 + shift1)               BatchNorm 1 over all B*N*k values
 *   y2[b,i,j,:] = a1[b,i,j,:] . w^T (+ bias)                       fp32 matrix pipe, ascending-k chain (sug_pointmlp_max_fwd)
 *   out[b,i,c]  = LeakyReLU_s2(scale2 * ext_j y2 + shift2)         BatchNorm 2 over all B*N*k values
 * ext = max_j where gamma2[c] >= 0, min_j where gamma2[c] < 0; arg = the lowest such j.  The edge feature [B,N,k,2C],
 * y2 and a2 are never formed.  Statistics as sug_pointmlp_max_layer_fwd: sums about a pivot row, one fp32 partial row
 * per workgroup in ws, folded in fp64 in a fixed order; no float atomics; training = 0 reads coef (caller fills it).
 * sug_edgemlp_supported: 2 <= k <= 32, C1 == 64, Co in {64, 128}.
 * sug_edge_expand_fwd: y1 [B,N,k,C1] (dense) and, training != 0, coef [5,C1] of BatchNorm 1 + its running-buffer
 *   update; idx [B,N,k] entries are clamped into [0,N); ws: SUG_STATS_BLOCKS*2*C1 floats.
 * sug_edgemlp_max_layer_fwd_xf: the short-segment sibling of sug_pointmlp_max_layer_fwd_xf, same arguments and
 *   outputs (zext / arg [rows/seg, Co], coef [5,Co], out [rows/seg, Co] with row stride ldo, zout = a1 or null) for
 *   segments of `seg` = k consecutive rows that do not line up with the 32-row tiles; any number of whole segments;
 *   groups must be 1; ws: SUG_STATS_BLOCKS*2*Co floats.
 * sug_edge_expand_bwd: dpq[b,m,0:C1) = sum of dy1 over the entries e = i*k + j with idx[b,i,j] == m in ascending e
 *   (rev_off / rev_ent = sug_knn_reverse(idx)); dpq[b,i,C1:2C1) = sum_j dy1[b,i,j,:] in ascending j; dpq has row
 *   stride lddpq; a point that no list names gets zeros; every row is written. */
int sug_edgemlp_supported(int k, int C1, int Co);
int sug_edge_expand_fwd(const float* pq, int64_t ldpq, const int32_t* idx, int B, int N, int k, int C1,
                        const float* gamma, const float* beta, int training, float eps, float momentum,
                        float* running_mean, float* running_var, float* y1, float* coef, float* ws, void* stream);
int sug_edgemlp_max_layer_fwd_xf(const float* y, int64_t ldy, int64_t rows, int K, const float* xcoef, float xslope,
                                 float* zout, int64_t ldz, const float* w, const float* bias, const float* gamma,
                                 const float* beta, int Co, int seg, int groups, int training, float eps, float momentum,
                                 float slope, float* running_mean, float* running_var, float* zext, int32_t* arg,
                                 float* coef, float* out, int64_t ldo, float* ws, void* stream);
int sug_edge_expand_bwd(const float* dy1, const int32_t* rev_off, const int32_t* rev_ent, int B, int N, int k, int C1,
                        float* dpq, int64_t lddpq, void* stream);

/* ---- Point Transformer vector attention (BASELINE config 5) --------------------------------------
 * The memory-bound parts of TransformerBlock.forward (model/Ptran_transformer.py:32-45) around the three
 * 512 x 512 linears of the k-expanded rows (library GEMMs: fp32, or fp16 MFMA with fp32 accumulation):
 * rows r = (b*n + i)*k + j, d = 512 channels contiguous, nbr [B,n,k] = neighbour index inside the cloud
 * (sug_knn_query_direct).  dtype: 0 = fp32, 1 = fp16 for the k-expanded tensors T0 / delta / U / L and their
 * gradients (void*); q, K, V [B,n,512], xyz [B,n,3], weights and all reductions are fp32.  k <= 16.
 *   pos1: T0[r,:] = relu(w1 . (xyz_i - xyz_nbr) + b1), w1 [512,3]                    (fc_delta[0] + ReLU, :39)
 *   qk:   U[r,:]  = q[i,:] - K[nbr,:] + delta[r,:]                                    (input of fc_gamma, :41)
 *   attn: mixed[i,:] = sum_j softmax_j(L[r,:]*scale) * (V[nbr,:] + delta[r,:]); mx / sm [B,n,512] = the
 *         per-channel max and sum of exponentials, kept for the backward               (:42-44)
 * Backward: rev_off / rev_ent = sug_knn_reverse(nbr) (dK and dV are gathered over reverse neighbour lists:
 * no atomics).  sug_ptran_attn_bwd: g = d mixed, mixed = the forward's output (its product with g is the softmax
 * backward's row term, so the rows are visited once) -> dlogits, da = the gradient of delta through (v + delta),
 * dv [B,n,512].  sug_ptran_qk_bwd: du = dU; da is read and overwritten with d delta = du + da; dq, dk
 * [B,n,512].  sug_ptran_pos1_bwd: g = dT0 -> dw1 [512,3], db1 [512]; ws: 1024*4*512 floats.
 * attn_bwd and qk_bwd also return the column sums (the bias gradients the caller needs next: model/Ptran_transformer.py's
 * nn.Linear biases of fc_gamma / fc_delta) of the [B*n*k,512] gradient they write - dlogits for attn, d delta for
 * qk - from the same pass instead of one more read of that tensor: db [512] (NULL = skip), ws =
 * sug_ptran_colsum_workspace(B*n) floats.  sug_ptran_relu_bwd_db: in place G <- G*[T1>0] over `rows` rows (the ReLU
 * inside fc_gamma), db [512] = its column sums, ws = sug_ptran_colsum_workspace(rows) floats. */
int sug_ptran_pos1_fwd(const float* xyz, const int32_t* nbr, const float* w1, const float* b1, int B, int n, int k,
                       int d, int dtype, void* out, void* stream);
int sug_ptran_pos1_bwd(const void* g, const float* xyz, const int32_t* nbr, const float* w1, const float* b1, int B,
                       int n, int k, int d, int dtype, float* dw1, float* db1, float* ws, void* stream);
int sug_ptran_qk_fwd(const float* q, const float* kf, const void* delta, const int32_t* nbr, int B, int n, int k, int d,
                     int dtype, void* out, void* stream);
int sug_ptran_qk_bwd(const void* du, void* da, const int32_t* rev_off, const int32_t* rev_ent, int B, int n, int k, int d,
                     int dtype, float* dq, float* dk, float* db, float* ws, void* stream);
int sug_ptran_attn_fwd(const void* logits, const void* delta, const float* vf, const int32_t* nbr, int B, int n, int k,
                       int d, int dtype, float scale, float* mixed, float* mx, float* sm, void* stream);
int sug_ptran_attn_bwd(const float* g, const float* mixed, const void* logits, const void* delta, const float* vf,
                       const int32_t* nbr, const float* mx, const float* sm, const int32_t* rev_off, const int32_t* rev_ent,
                       int B, int n, int k, int d, int dtype, float scale, void* dlogits, void* da, float* dv, float* db,
                       float* ws, void* stream);
/* The fp16 forward of the vector attention as ONE kernel on the matrix cores (csrc/ptran_fused.hip; round 6): pos1, the three
 * 512 x 512 linears of fc_delta[2] / fc_gamma[0] / fc_gamma[2] (v_mfma_f32_32x32x16_f16, activations resident in LDS, weights
 * streamed from L2), U = (q - K_nbr) + delta, the softmax over the 16 neighbours and the weighted sum of V_nbr + delta --
 * model/Ptran_transformer.py:39-44 in the 16-bit mode of BASELINE config 5.  w2 / b2 / wg1 / bg1 / wg2 / bg2: fp16 ([512,512]
 * row-major = nn.Linear.weight, [512]); q / kf / vf / xyz / w1 / b1 fp32.  delta [B n 16, 512] fp16 is always written
 * (the kernel reads it back for the weighted sum); save = 1 additionally writes T0, U, T1 and the logits (what
 * sug_ptran_*_bwd read), save = 0 leaves those pointers unused (NULL allowed).  mixed / mx / sm [B n, 512] fp32 as
 * sug_ptran_attn_fwd.  sug_ptran_fused_supported: 1 for d = 512, k = 16 and B*n a multiple of 8. */
int sug_ptran_fused_supported(int B, int n, int k, int d);
int sug_ptran_fused_fwd(const float* xyz, const int32_t* nbr, const float* q, const float* kf, const float* vf,
                        const float* w1, const float* b1, const void* w2, const void* b2, const void* wg1, const void* bg1,
                        const void* wg2, const void* bg2, int B, int n, int k, int d, float scale, int save, void* T0,
                        void* delta, void* U, void* T1, void* Lg, float* mixed, float* mx, float* sm, void* stream);
int64_t sug_ptran_colsum_workspace(int64_t rows);
int sug_ptran_relu_bwd_db(void* G, const void* T1, int64_t rows, int d, int dtype, float* db, float* ws, void* stream);
/* Range scaling of an fp16 backward: out[0] = s, out[1] = 1 / s, s the power of two that brings the largest |g| over up to
 * three fp32 tensors (g1, g2 nullable; n elements each) into [2^(log2_target-1), 2^log2_target), clamped to 2^+-100
 * (all-zero input: 2^100).  Computed on the device from the exponent field of the maximum; ws: 768 floats.  No memset,
 * no atomics, no host read. */
int sug_grad_scale16(const float* g0, int64_t n0, const float* g1, int64_t n1, const float* g2, int64_t n2, int log2_target,
                     float* out, float* ws, void* stream);

/* out[i] = (float) sum over g of red[g][i], i < n (fp64 partial rows of `groups` domain groups, in order). */
int sug_fold_groups(const double* red, int groups, int n, float* out, void* stream);

/* ---- Gaussian multi-kernel MMD --------------------------------------------------
 * replaces _mix_rbf_kernel + _mmd2(biased=True), model/mmd.py:239-254, :274-312.
 * Z = [X;Y] : [2m, D] rows (ld = ldz).  e_ij = n_i - 2<z_i,z_j> + n_j with n the
 * Gram diagonal; K = sum_s exp(-e/(2 sigma_s^2)); w (NULL or [m]) multiplies the
 * column sums of K_XY.  sums[0..2] += S_XX, S_YY, S_wXY (fp64, caller zeroes);
 * mmd2 = (S_XX + S_YY - 2 S_wXY)/m^2 is formed by the caller.
 * wt (NULL or [2m,2m]) receives c'_ij * dK_ij/de_ij for the backward
 * (dZ = 2*(diag(rowsum(wt)) - wt) . Z).  neg_gamma: device array [nsigma] holding
 * -1/(2 sigma_s^2) rounded to fp32 (the way torch rounds the python scalar,
 * model/mmd.py:251-252); nsigma <= 8. */
int sug_mmd_rbf(const float* z, int64_t ldz, int m, int D, const float* w,
                const float* neg_gamma, int nsigma, double* sums, float* wt, void* stream);

/* sug_mmd_rbf with the scalar formed on the device: zeroes sums (3 doubles of scratch), runs the kernel and
 * writes value[0] = (S_XX + S_YY - 2 S_wXY) / m^2 as fp32 (model/mmd.py:300-312, biased estimator). */
int sug_mmd_rbf_value(const float* z, int64_t ldz, int m, int D, const float* w, const float* neg_gamma,
                      int nsigma, double* sums, float* wt, float* value, void* stream);

/* Backward of sug_mmd_rbf: dz[i,:] = gscale[0] * 2 * (rowsum(wt)[i]*z[i,:] - (wt.z)[i,:])
 * (the autograd of model/mmd.py:239-312 w.r.t. the features); gscale: device scalar = dL/dmmd2. */
int sug_mmd_rbf_bwd(const float* z, int64_t ldz, const float* wt, int m, int D, const float* gscale,
                    float* dz, int64_t lddz, void* stream);

/* Row-block forms for the batch-sharded global MMD (no reference counterpart: the WIP DDP
 * trainer uses per-rank MMD, train_dg.py:357-368).  z is the gathered [2m, D] matrix (all ranks' X rows,
 * then all ranks' Y rows); this rank owns X rows [row0, row0+mloc) and Y rows m + [row0, row0+mloc).
 * sug_mmd_rbf_rows adds the contributions of the pairs (i in own rows, j in all columns) to sums[0..2]
 * (the ranks' partial sums are then added: an all-reduce of 3 doubles) and writes wt for the own rows
 * only, [2*mloc, 2m]; sug_mmd_rbf_rows_bwd turns that into the gradient of the OWN rows,
 * dz [2*mloc, D] = gmul * gscale[0] * 2 * (rowsum(wt) z_i - wt.z): no collective in the backward.
 * row0 = 0, mloc = m are sug_mmd_rbf / sug_mmd_rbf_bwd. */
int sug_mmd_rbf_rows(const float* z, int64_t ldz, int m, int D, const float* w, const float* neg_gamma,
                     int nsigma, int row0, int mloc, double* sums, float* wt, void* stream);
int sug_mmd_rbf_rows_bwd(const float* z, int64_t ldz, const float* wt, int m, int D, int row0, int mloc,
                         const float* gscale, float gmul, float* dz, int64_t lddz, void* stream);

/* SDA sample weights from class probabilities: prob_weights_soft + distance2weights,
 * model/mmd.py:134-148 and :178-202 (the reference computes them on the CPU with scipy's kl_div).
 * pred_* [m,num_class] logits (row strides lds/ldt >= num_class), label_* int64 [m]; method 0 "none", 1 "naive_inverse",
 * 2 "exp_inverse", 3 "mean2one"; weights [m].  2 <= num_class <= SUG_SDA_MAX_CLASSES: 10 runs the compile-time body, every
 * other count a body that streams the row (same passes, same order of arithmetic).  A label outside [0, num_class) gets no
 * one-hot entry and raises nothing. */
#define SUG_SDA_MAX_CLASSES 64
int sug_sda_prob_weights(const float* pred_s, int64_t lds, const float* pred_t, int64_t ldt,
                         const int64_t* label_s, const int64_t* label_t, int m, int num_class,
                         float label_weight, int method, float* weights, void* stream);
/* The same for the logits of n <= 4 heads on one batch (same labels), one launch: HOST arrays of n device pointers / strides. */
int sug_sda_prob_weights_multi(int n, const void* const* pred_s, const int64_t* lds, const void* const* pred_t,
                               const int64_t* ldt, const int64_t* label_s, const int64_t* label_t, int m, int num_class,
                               float label_weight, int method, void* const* weights, void* stream);

/* Z [2m, D+num_class] = [feat_s ; feat_t | one-hot(label) * label_scale]: the label-augmented operand of soft_mmd
 * (model/mmd.py:56-66, create_one_hot_labels utils/common_utils.py:161-164) in one launch; feat_* [m,D] with row
 * strides lds / ldt, label_* int64 [m]. */
int sug_mmd_assemble(const float* feat_s, int64_t lds, const float* feat_t, int64_t ldt, const int64_t* label_s,
                     const int64_t* label_t, int m, int D, int num_class, float label_scale, float* z, void* stream);

/* Up to 4 soft-MMD terms of ONE batch (same m samples per domain, same labels; a SUG step has three:
 * train_dg_single_gpu.py:300-322 -> mmd_cal -> soft_mmd, model/mmd.py:25-41, :56-66) with one launch per stage instead of
 * one per stage and term: assemble (sug_mmd_assemble; it also clears sums), kernel sums + derivative weights
 * (sug_mmd_rbf: each term through the kernel that call would choose), the n values; backward: sug_mmd_rbf_bwd of every
 * term in one launch.  Per-term results are bit-identical to the single-term calls.  HOST arrays of n entries:
 * feat_s / feat_t [m, D[i]] (row strides lds / ldt), label_scale, w (device [m] or null), z (device [2m, D[i] + num_class],
 * written), wt (device [2m, 2m] written, or null: no backward).  sums: device double [3n] scratch; values: device float [n].
 * Backward: gscale[i] = device scalar (upstream gradient of value i) or null (term skipped), dz[i] device [2m, D[i]]
 * dense = the gradient of [feat_s ; feat_t] (the label columns of z are constants), written entirely. */
int sug_soft_mmd_multi_fwd(int n, const void* const* feat_s, const int64_t* lds, const void* const* feat_t,
                           const int64_t* ldt, const int32_t* D, const float* label_scale, const int64_t* label_s,
                           const int64_t* label_t, int m, int num_class, const void* const* w, const float* neg_gamma,
                           int nsigma, void* const* z, void* const* wt, double* sums, float* values, void* stream);
int sug_soft_mmd_multi_bwd(int n, const void* const* z, const int32_t* D, const void* const* wt,
                           const void* const* gscale, int m, int num_class, void* const* dz, void* stream);

/* Class-aligned MMD (hard_mmd / max_hard_mmd, model/mmd.py:69-104) with the row selection and its size n on the device:
 * no host wait, no data-dependent shape, one launch sequence for every batch.
 * sug_mmd_select (one workgroup): label_* int64 [m], 1 <= m <= SUG_CLASS_MMD_MAX_ROWS, 1 <= num_class <=
 *   SUG_CLASS_MMD_MAX_CLASSES.
 *   mode 0 (hard): the rows with label_s[i] == label_t[i], ascending i; idx_s == idx_t.
 *   mode 1 (stable max-overlap): for c = 0 .. num_class-1 the first min(a_c, b_c) rows of class c of each domain, lowest
 *   index first, the classes in ascending order (a_c, b_c: rows of class c in label_s, label_t).  A label outside
 *   [0, num_class) is never paired, on either side, and is no error.
 *   idx_s / idx_t int32 [m]: the selected rows (first n entries; -1 after them); pos_s / pos_t int32 [m]: a row's position
 *   in the selection or -1; count int32 [1]: n.  Fixed order, no atomics.
 * sug_class_mmd_fwd: z [2m, D] (first 2n rows written) = [feat_s[idx_s[0..n)] ; feat_t[idx_t[0..n)]]; sug_mmd_rbf_value of
 *   those rows with m := n (the kernel form by that function's rule applied to n; wt [2m, 2m] or null, used with row
 *   stride 2n; sums: 3 doubles of scratch, cleared here); value[0] = (S_XX + S_YY - 2 S_XY) / n^2, NaN when n == 0.
 *   feat_* fp32 [m, D] with row strides lds / ldt; 1 <= D <= SUG_CLASS_MMD_MAX_D; nsigma <= 8.
 * sug_class_mmd_bwd: sug_mmd_rbf_bwd with m := n into dz [2m, D] scratch, then EVERY row of dfeat_s / dfeat_t [m, D] (row
 *   strides ldds / lddt) is written: a selected row's gradient, exact zeros elsewhere (all rows when n == 0). */
#define SUG_CLASS_MMD_MAX_ROWS 1024
#define SUG_CLASS_MMD_MAX_CLASSES 64
#define SUG_CLASS_MMD_MAX_D 1048576
int sug_mmd_select(const int64_t* label_s, const int64_t* label_t, int m, int num_class, int mode, int32_t* idx_s,
                   int32_t* idx_t, int32_t* pos_s, int32_t* pos_t, int32_t* count, void* stream);
int sug_class_mmd_fwd(const float* feat_s, int64_t lds, const float* feat_t, int64_t ldt, int m, int D,
                      const int32_t* idx_s, const int32_t* idx_t, const int32_t* count, const float* neg_gamma,
                      int nsigma, float* z, float* wt, double* sums, float* value, void* stream);
int sug_class_mmd_bwd(const float* z, const float* wt, int m, int D, const int32_t* count, const int32_t* pos_s,
                      const int32_t* pos_t, const float* gscale, float* dz, float* dfeat_s, int64_t ldds,
                      float* dfeat_t, int64_t lddt, void* stream);

/* The MMD^2 / variance / ratio estimator (mix_rbf_mmd2_and_ratio, model/mmd.py:263-266, :315-373) and the linear-time
 * estimators over adjacent rows (linear_mmd2 / poly_mmd2, :211-236).  No host read, no atomics, no memset: capturable,
 * bit-reproducible.  Limits (checked before any launch): 2 <= m <= SUG_MMD_EST_MAX_ROWS rows per domain,
 * 1 <= D <= SUG_MMD_EST_MAX_D, 1 <= nsigma <= SUG_MMD_EST_MAX_SIGMAS, poly degree 1 .. SUG_MMD_POLY_MAX_DEGREE.
 * sug_mmd_ratio_fwd: z = [X ; Y] fp32 [2m, D], row stride ldz.  K, G: fp32 [2m, 2m] scratch (kernel matrix and its
 *   derivative sums, the pair arithmetic of sug_mmd_rbf); rows: fp64 [SUG_MMD_RATIO_ROW_FIELDS * m] scratch (row sums);
 *   stats: fp64 [SUG_MMD_RATIO_STATS] scratch; out3 = {loss, mmd2, var_est} fp32 with loss = mmd2 / sqrt(max(var_est, 1e-8)),
 *   mmd2 biased (biased != 0) or unbiased.  wt_m, wt_v: fp32 [2m, 2m] (d mmd2 / dK . G and d var_est / dK . G, symmetrised,
 *   zero diagonal) for the backward, or both null.
 * sug_mmd_ratio_bwd: g3 = the upstream gradients of {loss, mmd2, var_est} (device); dz [2m, D] (row stride lddz) =
 *   2 sum_j (f_m wt_m + f_v wt_v)[i,j] (z_i - z_j), f_m = g3[1] + g3[0] / sqrt(v_c), f_v = g3[2] - g3[0] mmd2 v_c^(-3/2) / 2
 *   (that term only while var_est >= 1e-8), v_c = max(var_est, 1e-8), read from out3 on the device.
 * sug_mmd_adjacent_fwd: x, y fp32 [m, D] (row strides ldx, ldy); mode 0 (linear): value = mean_i <x_i - y_i, x_{i+1} -
 *   y_{i+1}>; mode 1 (poly): mean_i of kxx^d + kyy^d - kxy^d - kyx^d, k = alpha <., .> + c over rows i, i+1.  part: fp64
 *   [m - 1] scratch; coef: fp32 [4, m - 1] for the backward (mode 1; may be null); value: fp32 device scalar.
 * sug_mmd_adjacent_bwd: dx, dy [m, D] written entirely; gscale = upstream gradient (device scalar). */
#define SUG_MMD_EST_MAX_ROWS 1024
#define SUG_MMD_EST_MAX_D 1048576
#define SUG_MMD_EST_MAX_SIGMAS 8
#define SUG_MMD_POLY_MAX_DEGREE 8
#define SUG_MMD_RATIO_ROW_FIELDS 9
#define SUG_MMD_RATIO_STATS 16
int sug_mmd_ratio_fwd(const float* z, int64_t ldz, int m, int D, const float* neg_gamma, int nsigma, int biased, float* K,
                      float* G, double* rows, double* stats, float* out3, float* wt_m, float* wt_v, void* stream);
int sug_mmd_ratio_bwd(const float* z, int64_t ldz, int m, int D, const float* wt_m, const float* wt_v, const float* out3,
                      const float* g3, float* dz, int64_t lddz, void* stream);
int sug_mmd_adjacent_fwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int m, int D, int mode, int degree,
                         double alpha, double c, double* part, float* coef, float* value, void* stream);
int sug_mmd_adjacent_bwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int m, int D, int mode, const float* coef,
                         const float* gscale, float* dx, int64_t lddx, float* dy, int64_t lddy, void* stream);

/* The contrastive alignment mode (NAME: CL; contrastive_loss_weighted, model/mmd.py:80-94, with the trainer's
 * nn.CosineEmbeddingLoss(margin, reduction='none'), train_dg_single_gpu.py:236-242) of n <= SUG_CL_LOSS_MAX_TERMS terms of ONE
 * batch (same m rows per domain, same labels) in one launch sequence.  Per term and row i, x_i / y_i fp32 rows of length D:
 *   dot = sum x y, a = sum x x + 1e-12, b = sum y y + 1e-12, cos = dot / sqrt(a b);
 *   l_i = 1 - cos where label_s[i] == label_t[i], max(0, cos - margin) elsewhere; value = (1/m) sum_i w_i l_i (w_i = 1 without w).
 * No host read, no atomics, no memset: capturable.  Every sum is carried in fp64 in one fixed order (per lane ascending, lane
 * tree, waves in index order) and rounded to fp32 once, at the outputs; a row's numbers depend on that row alone, and a
 * strided view gives the bits of its contiguous copy (16-byte loads where base pointer and row stride allow, else 4-byte
 * loads of the same elements by the same lanes).  Limits (checked before any launch): 1 <= m <= SUG_CL_LOSS_MAX_ROWS,
 * 1 <= D <= SUG_CL_LOSS_MAX_D, row strides >= D, finite margins, no null pointer except the entries of w (and of coef / dx / dy
 * as stated).  HOST arrays of n entries: x / y (device [m, D[i]], row strides ldx / ldy), D, margin, w (device fp32 [m] or
 * null), coef (device fp64 [SUG_CL_LOSS_ROW_FIELDS * m], written: the three backward coefficients of the rows and their cos;
 * or null: no backward).  sums: device fp64 [n * SUG_CL_LOSS_SUM_FIELDS * m] scratch; values: device fp32 [n].
 * sug_cl_loss_fwd: two launches (row sums over (row, term); fold, one workgroup per term).
 * sug_cl_loss_bwd: one launch; gscale[i] = device scalar (upstream gradient of value i) or null (term skipped); dx[i] / dy[i]
 *   device [m, D[i]] (row strides lddx / lddy; either may be null: one-sided, both null: term skipped), STORED:
 *   dx_i = g (c1 y_i - c2 x_i), dy_i = g (c1 x_i - c3 y_i), c1 = w s / (m sqrt(a b)), c2 = w s cos / (m a), c3 = w s cos / (m b),
 *   s = -1 for a positive pair, +1 for a negative pair with cos > margin, 0 otherwise.  The weights are constants. */
#define SUG_CL_LOSS_MAX_ROWS 1024
#define SUG_CL_LOSS_MAX_D 1048576
#define SUG_CL_LOSS_MAX_TERMS 4
#define SUG_CL_LOSS_SUM_FIELDS 3
#define SUG_CL_LOSS_ROW_FIELDS 4
int sug_cl_loss_fwd(int n, const void* const* x, const int64_t* ldx, const void* const* y, const int64_t* ldy, const int32_t* D,
                    const double* margin, const int64_t* label_s, const int64_t* label_t, int m, const void* const* w,
                    double* sums, void* const* coef, float* values, void* stream);
int sug_cl_loss_bwd(int n, const void* const* x, const int64_t* ldx, const void* const* y, const int64_t* ldy, const int32_t* D,
                    int m, const void* const* coef, const void* const* gscale, void* const* dx, const int64_t* lddx,
                    void* const* dy, const int64_t* lddy, void* stream);

/* The EdgeConv GEMM operand of a conv_2d weight W [Co, 2C] (get_graph_feature's cat(x_j - x_i, x_i) folded into
 * the weights, model/model_utils.py:188-210): backward = 0: in = W, out [2Co, C] = [W[:, :C] ; W[:, C:] - W[:, :C]];
 * backward = 1: in = d out [2Co, C], out = dW [Co, 2C]. */
int sug_edge_weight_split(const float* in, int Co, int C, int backward, float* out, void* stream);
/* The same for n <= 8 weights in ONE launch (the four EdgeConv layers of Model.py:54-121): HOST arrays of n device
 * pointers and shapes; an entry whose in or out pointer is null is skipped (a layer without a gradient). */
int sug_edge_weight_split_multi(const void* const* in_host, const int32_t* Co_host, const int32_t* C_host, int n,
                                int backward, void* const* out_host, void* stream);

/* Chamfer distance per cloud pair (SDA geometric weights; geometric_weights(),
 * model/mmd.py:107-131 -- third-party op in the reference, parity unpinned):
 * out[b] = mean_i min_j |a_i-b_j|^2 + mean_j min_i |a_i-b_j|^2, direct-form distance.
 * a [B,N,3], b [B,M,3], out [B] (written, not accumulated); ws: sug_chamfer_workspace(B, N, M) floats -- the partial sums
 * of the workgroups, folded per cloud in block order (no float atomics: the value is reproducible run to run). */
int64_t sug_chamfer_workspace(int B, int N, int M);
int sug_chamfer(const float* a, const float* b, int B, int N, int M, float* out, float* ws, void* stream);
/* sug_chamfer followed by distance2weights (model/mmd.py:178-202) in the fold's own launch: out[b] = the SDA geometric weight
 * of pair b; method 1 naive_inverse, 2 exp_inverse, 3 mean2one (1 / mean truncated to an integer, :200).  Sums over the
 * batch in fp64, fixed order. */
int sug_chamfer_weights(const float* a, const float* b, int B, int N, int M, int method, float* out, float* ws, void* stream);
/* The two entry points above with both directions (a -> b, b -> a) in ONE launch instead of two: same workspace, same
 * partial sums in the same places, same fold; the results are bit-identical. */
int sug_chamfer_merged(const float* a, const float* b, int B, int N, int M, float* out, float* ws, void* stream);
int sug_chamfer_weights_merged(const float* a, const float* b, int B, int N, int M, int method, float* out, float* ws,
                               void* stream);
/* ChamferDistance as an op (the third-party op model/mmd.py imports; cd_distance, model/mmd.py:169-175 -- parity unpinned as
 * above): dist1[b,i] = min_j d(a_i, b_j), idx1[b,i] = the LOWEST j attaining it, dist2 / idx2 [B,M] the same for b against a;
 * d = ((dx*dx + dy*dy) + dz*dz) of the fp32 differences, every operation rounded once (bit-reproducible on a CPU).
 * a [B,N,3], b [B,M,3] contiguous, 1 <= N, M <= SUG_CHAMFER_MAX_POINTS, N != M allowed, B <= 65535.  One launch, no workspace. */
#define SUG_CHAMFER_MAX_POINTS 5000
int sug_chamfer_nn(const float* a, const float* b, int B, int N, int M, float* dist1, float* dist2, int32_t* idx1, int32_t* idx2,
                   void* stream);
/* Its gradient for upstream g1 [B,N], g2 [B,M]: ga_i = 2 g1_i (a_i - b_idx1[i]) + sum_{j: idx2[j] = i} 2 g2_j (a_i - b_j) over j
 * ascending, gb the symmetric form; written, not accumulated.  ga or gb may be null: that side is skipped.  No atomics: a
 * point's terms are added in an order fixed by the indices inside its cloud pair (chamfer.hip), whatever B and the pair's
 * place in the batch.  An index outside the other cloud is not followed (that point's gradient is NaN).  One launch. */
int sug_chamfer_nn_bwd(const float* g1, const float* g2, const float* a, const float* b, const int32_t* idx1, const int32_t* idx2,
                       int B, int N, int M, float* ga, float* gb, void* stream);

/* ---- the scalar tail of a step ---------------------------------------------------------------------------
 * Cross entropy of both classifier heads on the source rows of the paired logits (train_dg_single_gpu.py:269-292 with
 * nn.CrossEntropyLoss(), :167): loss[0] = w * (CE(logits1[:M], label) + CE(logits2[:M], label)), CE = mean over the M
 * rows of -log_softmax(row)[label]; w = 0.5 * SRC_LOSS_WEIGHT * CLS_WEIGHT folded by the caller.  logits* [>= M, C] with
 * row stride ld, label int64 [M], lse [2M + 1] (saved log-sum-exp of the rows; lse[2M] = number of rows that count).
 * 2M <= SUG_CE_PAIR_MAX_ROWS, C <= SUG_CE_PAIR_MAX_CLASSES.  Labels as nn.CrossEntropyLoss takes them: a row whose label ==
 * ignore_index (-100 by default in torch) contributes nothing and is left out of the mean; any other label outside [0, C) --
 * where torch raises -- makes the loss (and the gradient) NaN: never scored as some class. */
#define SUG_CE_PAIR_MAX_ROWS 512      /* source rows x 2 heads */
#define SUG_CE_PAIR_MAX_CLASSES 32
int sug_ce_pair_fwd(const float* logits1, const float* logits2, int64_t ld, const int64_t* label, int M, int C, float w,
                    int64_t ignore_index, float* loss, float* lse, void* stream);
/* Its gradient for the WHOLE paired logits: d1, d2 [Mtot, C] = g[0] * w * (softmax - onehot) / lse[2M] in the counting rows
 * < M, zero in ignored rows and in rows M .. Mtot-1 (the target half of a paired batch: no torch.stack / zero fill rebuilds
 * the pair's gradient). */
int sug_ce_pair_bwd(const float* logits1, const float* logits2, int64_t ld, const int64_t* label, int M, int Mtot, int C,
                    float w, int64_t ignore_index, const float* g, const float* lse, float* d1, float* d2, void* stream);
/* Cross entropy of ONE classifier head, the source-only loop's loss (train_source.py:86, :120):
 * nn.CrossEntropyLoss(reduction='mean', ignore_index, label_smoothing) of logits [M, C] (fp32, row stride ld >= C) against
 * label int64 [M]: loss[0] = mean over the counting rows of (1-eps)*(lse - z[label]) + eps * mean_c(lse - z_c); lse [M + 1] =
 * the rows' log-sum-exp, lse[M] = the number of counting rows.  Labels as sug_ce_pair_fwd takes them (ignore_index rows are
 * skipped and left out of the mean; any other label outside [0, C) makes loss and gradient NaN; no counting row: NaN, as
 * torch).  totals (device double[2], may be null) keeps the epoch's books in the same launch, train_source.py:130-131 without
 * the .item(): totals[0] += (double)loss * M, totals[1] += M (M, not the counting rows, as the reference).
 * 1 <= M <= SUG_CE_MAX_ROWS, 2 <= C <= SUG_CE_MAX_CLASSES, checked on the host before any launch (-1, sug_last_error()).  One
 * workgroup, a wave per row; the rows' terms are summed in fp64 in one fixed order; no float atomics, no memset node: capturable. */
#define SUG_CE_MAX_ROWS 1024
#define SUG_CE_MAX_CLASSES 64
int sug_ce_fwd(const float* logits, int64_t ld, const int64_t* label, int M, int C, int64_t ignore_index, float label_smoothing,
               float* loss, float* lse, double* totals, void* stream);
/* Its gradient: dlogits [M, C] (dense) = g[0] * (softmax - target) / lse[M] in the counting rows, target =
 * (1-eps)*onehot + eps/C; zero in ignored rows. */
int sug_ce_bwd(const float* logits, int64_t ld, const int64_t* label, int M, int C, int64_t ignore_index, float label_smoothing,
               const float* g, const float* lse, float* dlogits, void* stream);
/* The scalar tail of phase 1 of the two-phase UDA step (train_uda.py:149-160, train_dg_naive_mmd.py:225-241) in one launch:
 * logits ys1, ys2 [Ms, C] (source, heads 1 and 2) and yt1, yt2 [Mt, C] (target), fp32, ALL FOUR with row stride ld >= C (the row
 * halves of two paired [Ms + Mt, C] tensors are pointer offsets); label int64 [Ms], label_t int64 [Mt] (may be null when a_t == 0).
 *   CEs = CE(ys1, label) + CE(ys2, label), CEt = CE(yt1, label_t) + CE(yt2, label_t)  (CE = mean over rows, nn.CrossEntropyLoss()),
 *   D = mean over Mt*C of |softmax(yt1) - softmax(yt2)|  (utils/train_utils.py:51-54),
 * out4 = { a_s*CEs - D + a_t*CEt, r_s*CEs, -D, a_t*CEt };  lse [2*Ms + 2*Mt] = the rows' log-sum-exp (ys1, ys2, yt1, yt2), kept for
 * the backward.  totals (device double[4], may be null) keeps the epoch's books in the same launch, train_uda.py:180-184 without the
 * .item(): += { out4[1]*Ms, out4[2]*Ms, Ms, Mt }.  A label outside [0, C) makes the loss (and that row's gradient) NaN; there is no
 * ignore_index.  1 <= Ms, Mt <= SUG_MCD_MAX_ROWS, 2 <= C <= SUG_CE_MAX_CLASSES, checked on the host before any launch (-1,
 * sug_last_error()).  One workgroup, a wave per row; the rows' terms are summed in fp64 in one fixed order; no atomics, no memset
 * node: capturable, bit-reproducible. */
#define SUG_MCD_MAX_ROWS 1024
int sug_mcd_loss_fwd(const float* ys1, const float* ys2, const float* yt1, const float* yt2, int64_t ld, const int64_t* label,
                     const int64_t* label_t, int Ms, int Mt, int C, float a_s, float a_t, float r_s, float* out4, float* lse,
                     double* totals, void* stream);
/* Its gradient for the upstream scalar g[0], four dense blocks ds1, ds2 [Ms, C] and dt1, dt2 [Mt, C] (ds1 | dt1 adjacent = the dense
 * gradient of a paired tensor): source rows g*a_s*(softmax - onehot)/Ms; target rows, with s = sign(p1 - p2) and sign(0) = 0,
 * dt1 = -g/(Mt*C) * p1*(s - <s,p1>), dt2 = +g/(Mt*C) * p2*(s - <s,p2>), plus g*a_t*(softmax - onehot)/Mt when a_t != 0
 * (s_j - <s,p> is evaluated as sum_c p_c (s_j - s_c), which does not cancel for a class of probability close to 1). */
int sug_mcd_loss_bwd(const float* ys1, const float* ys2, const float* yt1, const float* yt2, int64_t ld, const int64_t* label,
                     const int64_t* label_t, int Ms, int Mt, int C, float a_s, float a_t, const float* g, const float* lse,
                     float* ds1, float* ds2, float* dt1, float* dt2, void* stream);
/* The classification loss of the shipped configurations (CLS_LOSS: ClassWeighting / FocalLoss, TARGET_LOSS, ADV_WEIGHT:
 * train_dg_single_gpu.py:163-180, :269-292; train_dg_naive_mmd.py:156-165, :225-241) in one launch: sug_mcd_loss_fwd generalised.
 * Logits and labels as sug_mcd_loss_fwd takes them (four blocks with ONE row stride ld >= C).  Per row
 *   L(z, y) = alpha[y] * m(q) * (-log p_y),  p = softmax(z),  q = 1 - p_y,  m(q) = 1 if gamma == 0, else q^gamma
 * (model_utils.focal_loss.forward); alpha: device fp32 [>= C], null = all ones.  With R = the mean over the rows, or their sum
 * when reduce_sum != 0:
 *   Ls = R(L(ys1, label)) + R(L(ys2, label)),  Lt = R(L(yt1, label_t)) + R(L(yt2, label_t)),
 *   D  = mean over Mt*C of |softmax(yt1) - softmax(yt2)|,
 *   out4 = { a_s*Ls + a_t*Lt - a_d*D, r_s*Ls, -a_d*D, a_t*Lt }.
 * alpha == null and gamma == 0 is nn.CrossEntropyLoss: only then rows labelled ignore_index are skipped and left out of the mean,
 * exactly as sug_ce_pair_fwd does; with alpha given, or gamma != 0, there is no ignore label.  Any other label outside [0, C)
 * makes the loss and that row's gradient NaN.  a_t == 0 and a_d == 0: the target rows are not read (yt1, yt2 may be null) and their
 * gradient is exact zeros; label_t may be null when a_t == 0.  save [2*(2*Ms + 2*Mt) + 2] floats, kept for the backward: the rows'
 * max, then their sums of exp(z - max) (rows in the order ys1, ys2, yt1, yt2), then the divisors of R for source and target.
 * totals (device double[4], may be null) += { (double)out4[1]*Ms, (double)out4[2]*Ms, Ms, Mt } in the same launch.
 * Numerics: p = exp(z - max)/sum; q is the sum of the OTHER classes' probabilities (not 1 - p_y); log p_y = (z_y - max) - log(sum).
 * 1 <= Ms, Mt <= SUG_MCD_MAX_ROWS, 2 <= C <= SUG_CE_MAX_CLASSES, gamma == 0 or gamma >= 1 (for 0 < gamma < 1 the derivative is
 * unbounded at p_y = 1): checked on the host before any launch (-1, sug_last_error()).  One workgroup, a wave per row; the
 * rows' terms are summed in fp64 in one fixed order; no atomics, no memset node: capturable, bit-reproducible. */
int sug_cls_loss_fwd(const float* ys1, const float* ys2, const float* yt1, const float* yt2, int64_t ld, const int64_t* label,
                     const int64_t* label_t, int Ms, int Mt, int C, const float* alpha, float gamma, int reduce_sum,
                     int64_t ignore_index, float a_s, float a_t, float a_d, float r_s, float* out4, float* save, double* totals,
                     void* stream);
/* Its gradient for the upstream scalar g[0], four dense blocks ds1, ds2 [Ms, C] and dt1, dt2 [Mt, C].  A source row, with
 * f = g*a_s/Ms (g*a_s for the sum):  dz_j = f * alpha_y * [m(q) - gamma*q^(gamma-1)*p_y*log p_y] * (p_j - delta_jy), p_y - 1 taken as
 * -q; the second term is absent for gamma == 0.  A target row: the same with a_t and Mt, plus the discrepancy gradient of
 * sug_mcd_loss_bwd scaled by a_d. */
int sug_cls_loss_bwd(const float* ys1, const float* ys2, const float* yt1, const float* yt2, int64_t ld, const int64_t* label,
                     const int64_t* label_t, int Ms, int Mt, int C, const float* alpha, float gamma, int reduce_sum,
                     int64_t ignore_index, float a_s, float a_t, float a_d, float r_s, const float* g, const float* save,
                     float* ds1, float* ds2, float* dt1, float* dt2, void* stream);
/* out3 = { loss_cls + wg*v_geo + ws*(v_sem1 + v_sem2), wg*v_geo, ws*(v_sem1 + v_sem2) } (train_dg_single_gpu.py:314-324; the
 * weights MMD_WEIGHT * GEO_SCALE and 0.5 * MMD_WEIGHT * SEM_SCALE folded by the caller); null v_* = term absent.
 * Backward: out4 = g[0] * {1, wg, ws, ws}. */
int sug_loss_combine_fwd(const float* loss_cls, const float* v_geo, const float* v_sem1, const float* v_sem2, float wg, float ws,
                         float* out3, void* stream);
int sug_loss_combine_bwd(const float* g, float wg, float ws, float* out4, void* stream);

/* ---- evaluation metrics -----------------------------------------------------------------------------------
 * One batch of eval_worker (utils/eval_utils.py:37-61) on the device, one launch, no host synchronisation (capturable).
 * output = (logits1 + logits2) / 2 in fp32 (logits1 alone when logits2 is null), written to out [B, C] (dense) when out is
 * given; pred[r] (int64, optional) = the index torch.max(output, 1) returns (first maximum; a row holding NaN: its first
 * NaN).  The batch loss is the device scalar loss_in[0] (ce_mode 0: the caller's criterion) or nn.CrossEntropyLoss of
 * output computed here (ce_mode 1: mean over the rows whose label != ignore_index, 2: sum; label_smoothing as torch;
 * per-row terms in fp32, summed in fp64 in a fixed order, rounded to fp32).  The state block (int64 / fp64 words, zeroed
 * by the caller before the first batch, SUG_EVAL_STATE_WORDS(cap) words) accumulates, in a fixed order by one thread:
 * data_total += B, correct_total += correct rows, loss_total += (double)loss * B, the per-class totals of rows and correct
 * rows, with cls_eval for every class c present in the batch class_acc[c] += {(double)correct_c / (double)rows_c, 1.0},
 * batch_acc[batch_count++] = (double)correct / (double)B.  A label outside [0, C) sets bit 0 of the error word (the
 * reference raises IndexError), a batch beyond `cap` bit 1.  logits* [B, C] fp32 with row stride ld, label int64 [B].
 * B <= SUG_EVAL_MAX_ROWS, C <= SUG_EVAL_MAX_CLASSES. */
#define SUG_EVAL_MAX_ROWS 4096
#define SUG_EVAL_MAX_CLASSES 64
#define SUG_EVAL_BATCH_COUNT 0        /* int64 */
#define SUG_EVAL_DATA_TOTAL 1         /* int64 */
#define SUG_EVAL_CORRECT_TOTAL 2      /* int64 */
#define SUG_EVAL_ERROR 3              /* int64 */
#define SUG_EVAL_LOSS_TOTAL 4         /* fp64 */
#define SUG_EVAL_CLASS_ACC 8          /* fp64 [64][2]: sum of ratios, batches present */
#define SUG_EVAL_CLASS_ROWS 136       /* int64 [64] */
#define SUG_EVAL_CLASS_CORRECT 200    /* int64 [64] */
#define SUG_EVAL_BATCH_ACC 264        /* fp64 [cap] */
#define SUG_EVAL_STATE_WORDS(cap) (SUG_EVAL_BATCH_ACC + (cap))
int sug_eval_accumulate(const float* logits1, const float* logits2, int64_t ld, const int64_t* label, int B, int C,
                        const float* loss_in, int ce_mode, int64_t ignore_index, float label_smoothing, float* out,
                        int64_t* pred, int cls_eval, void* state, int cap, void* stream);

/* ---- dense prediction: per-point cross entropy and the part-IoU books (csrc/seg.hip) ------------------------------
 * F.cross_entropy(logits [M, C], label [M], weight=class_weight, ignore_index, reduction='mean') of a segmentation batch's
 * rows: loss[0] = sum_r w[y_r] * (lse_r - z_r[y_r]) / sum_r w[y_r] over the counting rows (class_weight: device fp32 [C],
 * null = all ones).  logits fp32 with any row stride ld >= C, label int64.  Labels as sug_ce_fwd takes them: a row labelled
 * ignore_index contributes nothing; any other label outside [0, C) makes the loss NaN and that row's gradient NaN: no row is
 * ever scored as some class; no counting row: NaN, as torch.  lse [2M + 1], kept for the backward: the rows' maxima, then the
 * rows' log sum_c exp(z_c - max) (the log-sum-exp as two floats: their fp32 sum would round away, at the logits' size, the
 * digits that are the whole loss and gradient of a confidently right row), then lse[2M] = the denominator.  pred [M] (int32, may be null): the arg-max of every row, ignored ones included, the lowest
 * index on ties.  Two launches: workgroups of SUG_POINT_CE_BLOCK_ROWS rows each write ONE partial of
 * SUG_POINT_CE_PARTIAL_WORDS doubles (weighted loss sum, weight sum, counting rows; the rows' fp32 terms summed in fp64 in a
 * fixed order) into workspace -- sug_point_ce_workspace(M) doubles, or -1 --, then one workgroup adds the partials in block
 * order and writes loss (fp32) and lse[2M].  totals (device double[2], may be null) is advanced by the fold:
 * totals[0] += (double)loss * counting rows, totals[1] += counting rows.  1 <= M <= SUG_POINT_CE_MAX_ROWS,
 * 2 <= C <= SUG_POINT_CE_MAX_CLASSES, checked on the host before any launch (-1, sug_last_error()).  No float atomics, no
 * memset node: capturable, bit-reproducible. */
#define SUG_POINT_CE_MAX_ROWS 4194304
#define SUG_POINT_CE_MAX_CLASSES 64
#define SUG_POINT_CE_BLOCK_ROWS 128
#define SUG_POINT_CE_PARTIAL_WORDS 3
int sug_point_ce_workspace(int M);
int sug_point_ce_fwd(const float* logits, int64_t ld, const int64_t* label, int M, int C, int64_t ignore_index,
                     const float* class_weight, float* loss, float* lse, int32_t* pred, double* workspace, double* totals,
                     void* stream);
/* Its gradient, one launch: dlogits [M, C] (dense) = g[0] * w[y] * (softmax - onehot) / lse[2M] in the counting rows, zero in
 * ignored rows. */
int sug_point_ce_bwd(const float* logits, int64_t ld, const int64_t* label, int M, int C, int64_t ignore_index,
                     const float* class_weight, const float* g, const float* lse, float* dlogits, void* stream);
/* The ShapeNet-Part protocol for one batch, on the device, no host synchronisation (capturable).  logits [B, N, C] fp32
 * (dense), label [B, N] int64, category [B] int64 on the device; part_first, part_count [K] int32 are HOST arrays (they
 * travel by value with the launch and are checked before it): category k owns the parts
 * [part_first[k], part_first[k] + part_count[k]).  Per cloud: the prediction of a point is the arg-max over its category's
 * range ONLY (lowest index on ties); for every part p of the range I = #(pred == p and label == p), U = #(pred == p or
 * label == p), the part's IoU is 1 where U == 0, else (double)I / (double)U; the shape's IoU is their fp64 sum in part order
 * divided by part_count.  A cloud whose category is outside [0, K), or with a label outside its category's range, is NOT
 * scored: it raises the error word by one and changes nothing else.  Two launches: a workgroup per cloud writes the cloud's
 * record (records: B * SUG_SEG_RECORD_WORDS 64-bit words of scratch), one workgroup adds the records to state in cloud
 * order.  state: SUG_SEG_STATE_WORDS int64 / fp64 words, zeroed by the caller before the first batch.
 * 1 <= B <= SUG_SEG_MAX_CLOUDS, N >= 1, C <= SUG_SEG_MAX_PARTS, K <= SUG_SEG_MAX_CATEGORIES,
 * 1 <= part_count[k] <= SUG_SEG_MAX_CATEGORY_PARTS and every range inside [0, C): checked on the host before any launch. */
#define SUG_SEG_MAX_PARTS 64
#define SUG_SEG_MAX_CATEGORIES 64
#define SUG_SEG_MAX_CATEGORY_PARTS 16
#define SUG_SEG_MAX_CLOUDS 1024
#define SUG_SEG_RECORD_WORDS 40
#define SUG_SEG_SHAPES 0              /* int64: clouds scored */
#define SUG_SEG_POINTS 1              /* int64: their points */
#define SUG_SEG_CORRECT 2             /* int64: of them predicted as labelled */
#define SUG_SEG_ERROR 3               /* int64: clouds not scored */
#define SUG_SEG_CAT_IOU 8             /* fp64 [64]: sum of the shape IoUs of a category */
#define SUG_SEG_CAT_SHAPES 72         /* int64 [64] */
#define SUG_SEG_PART_POINTS 136       /* int64 [64]: points labelled with a part */
#define SUG_SEG_PART_CORRECT 200      /* int64 [64]: of them predicted as it */
#define SUG_SEG_STATE_WORDS 264
int sug_part_iou_accumulate(const float* logits, const int64_t* label, const int64_t* category, const int32_t* part_first,
                            const int32_t* part_count, int B, int N, int C, int K, void* records, void* state, void* stream);


/* ---- KPConv backbone (model/KPConv_model.py, model/KPConv_blocks.py; rigid kernel points, linear influence, sum) ----
 * Row layout: clouds are packed.  Level l owns a buffer of C_l rows; rows [0, off[B]) are valid -- the clouds back to back
 * at the device offsets off[B+1] (int32) -- and rows [off[B], C_l) are dead.  A neighbour table [Cq, H] holds global
 * support indices, a missing slot the shadow index Cs (the rows of the support buffer).  No float atomics: every sum has
 * one fixed order.  Invariants:
 *   1. every dead row of every level tensor is exactly zero (coordinates, activations, and the gradients of both);
 *   2. a dead query's table row is all shadow;
 *   3. a dead support's reverse list is empty;
 *   4. every function reads the valid counts from device memory, never reads a dead input row, and writes zeros to the
 *      dead rows of its outputs;
 *   5. no buffer, grid or host branch depends on a value in device memory: a launch sequence is static (a graph-capturable
 *      pyramid).
 * Exact sizes are the case with no dead rows, C_l == off[B]: 1. to 4. hold trivially.  sug_kpconv_bwd,
 * sug_seg_max_pool_fwd and sug_seg_max_pool_bwd need nothing beyond 2. and 3. (Nq / Ns = the row counts).
 *
 * sug_grid_subsample: per cloud, the voxels floor(p / dl) (fp32 true division) in order of their first point, each the
 * fp32 point-order sum of its points divided once by the count.  out_pad [B, cap, 3] and cnt [B] are scratch / counts,
 * out [C, 3] the packed result with offsets out_off [B+1], C <= B*cap.  cap >= every input cloud's length,
 * cap <= SUG_KPCONV_MAX_CLOUD.  out_off is clamped to C (the rows past C are dropped) and the dead rows of out are zeroed.
 * record (may be null; then level is not looked at): int32 [SUG_KPCONV_RECORD_INTS], zeroed by the caller once, into
 * which the unclamped total is folded: record[level] = max(record[level], total), level in [0, 4); record[4] = forwards in
 * which any level overflowed (counted once per forward; the level-0 call opens a forward), record[5] = scratch. */
#define SUG_KPCONV_MAX_CLOUD 4096
#define SUG_KPCONV_RECORD_INTS 8
int sug_grid_subsample(const float* pts, const int32_t* off, int B, int cap, float dl, int C, int level, float* out_pad,
                       int32_t* cnt, float* out, int32_t* out_off, int32_t* record, void* stream);
/* out [Nq, limit]: per query the first `limit` supports of its cloud, in support order, with d^2 < radius^2
 * (d^2 = (s-q)_x^2 + (s-q)_y^2 + (s-q)_z^2 in fp32, left to right); the rest, and a dead query's whole row, Ns.
 * Nq / Ns: the rows of q / s.  limit <= 64. */
int sug_radius_neighbors(const float* q, const int32_t* qoff, int Nq, const float* s, const int32_t* soff, int Ns, int B,
                         float radius, int limit, int32_t* out, void* stream);
/* Reverse lists of a neighbour table: the entries e = q*H + h naming support s, ascending, are
 * rev_ent[rev_be[2s] .. rev_be[2s+1]); rev_ent [Nq*H] (cloud b's lists lie in [qoff[b]*H, qoff[b+1]*H)), rev_be [Ns, 2]:
 * (0, 0) for the dead supports [soff[B], Ns).  Shadow slots appear in no list.  cap >= every cloud's support count,
 * <= SUG_KPCONV_MAX_CLOUD. */
int sug_radius_reverse(const int32_t* nbr, const int32_t* qoff, const int32_t* soff, int B, int H, int Ns, int cap,
                       int32_t* rev_be, int32_t* rev_ent, void* stream);
/* wf [Nq, K*Cin] = (sum_h w[q,k,h] x[s_h, :]) / cnt[q] with w = max(0, 1 - |(s_h - q) - kp_k| / extent) (shadow: 0) and
 * cnt = max(1, #{h : sum_c x[s_h, c] > 0}); the layer output is wf . W viewed as [K*Cin, Cout].  Also written for the
 * backward: w [Nq, H, K], cnt [Nq] (fp32).  nq_valid: device pointer to the number of valid queries (qoff + B), never
 * null; dead rows: wf = 0, w = 0, cnt = 1.  H <= 64, K <= 16. */
int sug_kpconv_fwd(const float* q, const float* s, const int32_t* nbr, const int32_t* nq_valid, int Nq, int H, int Ns,
                   const float* kp, int K, float extent, const float* x, int Cin, float* wf, float* w, float* cnt,
                   void* stream);
/* dx [Ns, Cin] = sum over the reverse entries (q, h) of s, ascending, of (sum_k w[q,h,k] dwf[q,k,:]) / cnt[q] */
int sug_kpconv_bwd(const int32_t* rev_be, const int32_t* rev_ent, int H, int K, const float* w, const float* cnt,
                   const float* dwf, int Ns, int Cin, float* dx, void* stream);
/* Per-cloud InstanceNorm1d (biased variance, no affine) over the rows of each cloud, x / y / dx / dsc [N, C]; mode 0:
 * plain, 1: LeakyReLU(0.1) after it, 2: LeakyReLU(0.1)(norm + sc).  mean / rstd [B, C] are kept for the backward, which
 * writes dx and, in mode 2, dsc (the gradient of sc).  An empty cloud: mean = rstd = 0, nothing normalised. */
int sug_seg_instnorm_fwd(const float* x, const int32_t* off, int B, int N, int C, float eps, int mode, const float* sc,
                         float* y, float* mean, float* rstd, void* stream);
int sug_seg_instnorm_bwd(const float* g, const float* y, const float* x, const float* mean, const float* rstd,
                         const int32_t* off, int B, int N, int C, int mode, float* dx, float* dsc, void* stream);
/* y [Nq, C] = max over the H slots of x[slot] (a shadow slot reads 0), arg = the first slot h holding it; the backward
 * routes g[q, c] to the support of slot arg[q, c] through the reverse lists (a shadow winner: nowhere). */
int sug_seg_max_pool_fwd(const float* x, const int32_t* nbr, int Nq, int H, int Ns, int C, float* y, int32_t* arg,
                         void* stream);
int sug_seg_max_pool_bwd(const float* g, const int32_t* arg, const int32_t* rev_be, const int32_t* rev_ent, int H, int Ns,
                         int C, float* dx, void* stream);
/* y [B, C] = per-cloud mean of x [N, C], an empty cloud's row 0; dx [N, C] = g[b] / N_b, rows >= off[B] = 0 */
int sug_seg_mean_fwd(const float* x, const int32_t* off, int B, int C, float* y, void* stream);
int sug_seg_mean_bwd(const float* g, const int32_t* off, int B, int N, int C, float* dx, void* stream);
/* sample_tensor_slices (model/KPConv_blocks.py:159-176) from device offsets: out [B, S, D], out[b, j] = x[off[b] + i],
 * i = j * (n / S) for n = off[b+1] - off[b] >= S, j mod n below that, zeros for n = 0.  Forward only. */
int sug_kp_sample_rows(const float* x, const int32_t* off, int B, int S, int D, float* out, void* stream);

/* ---- Point Transformer classifier head (PointTransformerCls.fc2 on points.mean(1), model/Ptran_model.py:104-117) ----
 * logits [B, NC] = L3(relu(L2(relu(L1(mean_P(points)))))), points [B, P, K] dense, Li(x) = x . Wi^T + bi with W1 [N1, K],
 * W2 [N2, N1], W3 [NC, N2] (nn.Linear layout).  fp32, every sum in one fixed order, no atomics: bit-reproducible.
 * Supported (sug_ptcls_head_supported): 1 <= B <= 128, 1 <= P <= 64, K % 64 == 0 and K <= 1024, N1 % 64 == 0 and
 * N1 <= 1024, N2 == 64, 2 <= NC <= 64.  points, W1, W2, W3, mean and h1 16-byte aligned.
 * sug_ptcls_head_fwd (2 launches): mean [B, K] = sum over P in point order / P, h1 [B, N1], h2 [B, N2] (post-ReLU),
 * logits.  sug_ptcls_head_bwd (2 launches): from dlogits [B, NC] and the forward's mean / h1 / h2: dz1 [B, N1] and
 * dz2 [B, N2] (caller's scratch: pre-activation gradients), dpoints [B, P, K] = dmean / P for every point, and the
 * weight / bias gradients (overwritten, not accumulated). */
int sug_ptcls_head_supported(int B, int P, int K, int N1, int N2, int NC);
int sug_ptcls_head_fwd(const float* points, int B, int P, int K, const float* W1, const float* b1, int N1, const float* W2,
                       const float* b2, int N2, const float* W3, const float* b3, int NC, float* mean, float* h1, float* h2,
                       float* logits, void* stream);
int sug_ptcls_head_bwd(const float* dlogits, const float* mean, const float* h1, const float* h2, int B, int P, int K,
                       const float* W1, int N1, const float* W2, int N2, const float* W3, int NC, float* dz1, float* dz2,
                       float* dpoints, float* dW1, float* db1, float* dW2, float* db2, float* dW3, float* db3,
                       void* stream);

/* ---- Device-resident data pipeline (UnifiedPointDG.__getitem__, data/dataloader.py:302-327, for a whole batch) ----
 * From the resident dataset pts [M, P, 3] and the device index list idx [B] write out [B, 3, N], one workgroup per cloud,
 * in the reference's order:
 *   1. SUG_PREP_NORMALIZE: normal_pc over all P points (mean in fp64 in one fixed order, centred in fp64 and rounded once,
 *      divided by the largest norm);
 *   2. pre_rot (HOST pointer to 9 floats, row-major, or null): p . R, rotate_shape's product;
 *   3. SUG_PREP_ROTATE_Z: p . [[c, -s, 0], [s, c, 0], [0, 0, 1]] with one angle per cloud (rotation_point_cloud);
 *      SUG_PREP_JITTER: + clip(sigma * n, -clip, clip) per coordinate, n standard normal (jitter_point_cloud);
 *   4. P < N: rows P .. N-1 are exact zeros; P > N: a uniformly random ordered subset of N points; P == N: identity
 *      (a random permutation with SUG_PREP_SHUFFLE: random_sample_pc of all the points);
 *   5. the transposed store.
 * Each random input comes from the caller when its pointer is given -- angles [B], noise [B, P, 3] (indexed by the source
 * point), sel [B, N] (source point per output row, needs N <= P) -- and is drawn in the kernel when it is null:
 * Philox4x32-10 with key = (seed low word, seed high word) and counter
 *      (c low word, c high word, cloud slot b in the batch, purpose | index),      c = *counter, read on the device,
 *   purpose SUG_PREP_DRAW_ANGLE,  index 0:      angle = (word0 >> 8) * 2^-24 * 2 pi;
 *   purpose SUG_PREP_DRAW_SUBSET, index q:      words 0..3 are the sort keys of points 4q .. 4q+3; the kept points are the
 *                                               first N in ascending (word, point index) order;
 *   purpose SUG_PREP_DRAW_NOISE,  index n:      the three normals of OUTPUT row n, Box-Muller with u = ((w >> 8) + 1) * 2^-24,
 *                                               v = (w >> 8) * 2^-24: r(word0) cos(2 pi v(word1)), r(word0) sin(2 pi v(word1)),
 *                                               r(word2) cos(2 pi v(word3)),  r(w) = sqrt(-2 ln u(w)).
 * A caller that bumps *counter by one per launch never repeats a counter; a captured launch replays with fresh draws.
 * counter may be null only when nothing is drawn.  Debug outputs (each may be null): angles_out [B], noise_out [B, N, 3]
 * (the unit normals used for each output row, zeros for padding), sel_out [B, N] (source point, -1 for padding).
 * An idx entry outside [0, M) or a sel entry outside [0, P) is never dereferenced: the cloud / row is written as NaN.
 * Limits, checked on the host before the launch: B >= 1, 1 <= P <= SUG_PREP_MAX_POINTS, N <= 1.5 * P (the reference raises
 * "Too few points" there).  Vector stores only, no atomics; bit-reproducible from (inputs, seed, *counter). */
#define SUG_PREP_MAX_POINTS 4096
#define SUG_PREP_NORMALIZE 1
#define SUG_PREP_ROTATE_Z 2
#define SUG_PREP_JITTER 4
#define SUG_PREP_SHUFFLE 8
#define SUG_PREP_DRAW_ANGLE 0x00000000u
#define SUG_PREP_DRAW_SUBSET 0x10000000u
#define SUG_PREP_DRAW_NOISE 0x20000000u
int sug_prepare_batch(const float* pts, int M, int P, const int32_t* idx, int B, int N, int stages,
                      const float* pre_rot, const float* angles, const float* noise, const int32_t* sel,
                      uint64_t seed, const uint64_t* counter, float sigma, float clip, float* out,
                      float* angles_out, float* noise_out, int32_t* sel_out, void* stream);

/* sug_prepare_batch plus the three augmentations that pc_augment (data/data_utils.py:169-175) lists behind the jitter, one
 * draw of each per cloud.  The same kernel; the stage order becomes
 *   1. normalise  2. pre_rot  3. z-rotation, jitter
 *   3a. SUG_PREP_SCALE:   p * s, s uniform in [scale_low, scale_high)                       (random_scale_point_cloud);
 *   3b. SUG_PREP_PERTURB: p . R, R = Rz (Ry Rx) of the three angles clip(angle_sigma * n, -angle_clip, angle_clip), n standard
 *       normal (rotate_perturbation_point_cloud).  R is formed once per cloud in fp64 (angles from the fp32 normals, sines and
 *       cosines in double) and rounded to fp32 once; the product is (x R0j + y R1j) + z R2j, as the pre-rotation's.  It is
 *       not merged with the z-rotation, nor is the scale folded into it;
 *   3c. SUG_PREP_SHIFT:   p + t, each component of t uniform in [-shift_range, shift_range)  (shift_point_cloud);
 *   4. pad / subset  5. the transposed store.
 * The three stages act on kept points only: padding rows stay exact zeros.  With none of the three bits set the output is
 * sug_prepare_batch's bit for bit, and the old purposes and words of the generator do not move.
 * aug_params: HOST pointer to SUG_PREP_AUG_PARAMS floats at the SUG_PREP_AUG_* positions (may be null when none of the three
 * stages is on); checked on the host: scale_low and scale_high finite, 0 < scale_low <= scale_high; shift_range, angle_sigma
 * and angle_clip finite and >= 0.
 * Draws: scales [B] (the factor), perturb [B, 3] (standard normals, as noise), shifts [B, 3] (the vector) when given, else
 * from the same Philox stream at index 0 of the purposes
 *   SUG_PREP_DRAW_SCALE:    s = scale_low + ((word0 >> 8) * 2^-24) * (scale_high - scale_low), in fp32 (like numpy's uniform
 *                           the sum may round up to scale_high itself);
 *   SUG_PREP_DRAW_PERTURB:  the three normals by the Box-Muller of SUG_PREP_DRAW_NOISE (words 0, 1 -> two, words 2, 3 -> the third);
 *   SUG_PREP_DRAW_SHIFT:    t_j = (2 * ((word_j >> 8) * 2^-24) - 1) * shift_range, j = 0..2.
 * A null counter is refused whenever any draw is needed.  Debug outputs (each may be null): scales_out [B] (1 when the stage
 * is off), perturb_out [B, 3] (the normals; 0 when off), shifts_out [B, 3] (0 when off). */
#define SUG_PREP_SCALE 16
#define SUG_PREP_PERTURB 32
#define SUG_PREP_SHIFT 64
#define SUG_PREP_DRAW_SCALE 0x30000000u
#define SUG_PREP_DRAW_PERTURB 0x40000000u
#define SUG_PREP_DRAW_SHIFT 0x50000000u
#define SUG_PREP_AUG_PARAMS 5
#define SUG_PREP_AUG_SCALE_LOW 0
#define SUG_PREP_AUG_SCALE_HIGH 1
#define SUG_PREP_AUG_SHIFT_RANGE 2
#define SUG_PREP_AUG_ANGLE_SIGMA 3
#define SUG_PREP_AUG_ANGLE_CLIP 4
int sug_prepare_batch_aug(const float* pts, int M, int P, const int32_t* idx, int B, int N, int stages,
                          const float* pre_rot, const float* angles, const float* noise, const int32_t* sel,
                          const float* scales, const float* perturb, const float* shifts, uint64_t seed,
                          const uint64_t* counter, float sigma, float clip, const float* aug_params, float* out,
                          float* angles_out, float* noise_out, int32_t* sel_out, float* scales_out, float* perturb_out,
                          float* shifts_out, void* stream);

/* The part-segmentation batch: sug_prepare_batch_aug for clouds of different lengths that carry extra channels and one part
 * label per point, in one launch, one workgroup per cloud (a second kernel; the one above is untouched).
 * Resident data: pts [M, P, 3] fp32; extra [M, P, E] fp32 (null when E == 0, 0 <= E <= SUG_PREP_SEG_MAX_EXTRA);
 * point_label [M, P] uint8 (part ids, below SUG_SEG_MAX_PARTS); category [M] int64 (may be null when category_out is);
 * lengths [M] int32: the valid points of cloud m are its rows 0 .. lengths[m]-1 (null: every cloud has P points).
 * Outputs: out [B, 3 + E, N] fp32 (xyz, then the extra channels: Pointnet2PartSeg.forward's input), label_out [B, N] int64,
 * category_out [B] int64 (may be null).  With ci = idx[b] and L = lengths[ci], in stage order:
 *   1. SUG_PREP_NORMALIZE: normal_pc over the first L points only, sug_prepare_batch's arithmetic and summation order with L
 *      in place of P.  A cloud whose L points coincide has a largest norm of 0 and comes out NaN, as the reference's
 *      normal_pc gives; it is not special-cased.
 *   2. The source point src of output row n -- every row has one, there are no padding rows:
 *        sel [B, N] given: src = sel[b, n]; values may repeat, N <= P is not required;
 *        L > N:  the subset rule above: keys from SUG_PREP_DRAW_SUBSET (points >= L keyed ~0), the first N in ascending
 *                (word, point) order;
 *        L <= N: rows 0 .. L-1 are the points in index order (in sorted-key order with SUG_PREP_SHUFFLE); rows L .. N-1 are
 *                drawn with replacement: row n takes word (n - L) % 4 of the Philox block at purpose SUG_PREP_DRAW_FILL,
 *                index (n - L) / 4, and src = (uint64(word) * L) >> 32.
 *      Whether a cloud sorts is decided in its workgroup from L; the host never reads a length.
 *   3. Coordinates: pre_rot, z-rotation, jitter, scale, perturbation, shift, in sug_prepare_batch_aug's order and arithmetic.
 *      In-kernel jitter normals are per OUTPUT row (a point taken twice jitters independently); supplied noise [B, P, 3] is
 *      indexed by the source point.
 *   4. Extra channels: out[b, 3 + e, n] = extra[ci, src, e], copied through.  With SUG_PREP_NORMALS (needs E >= 3) channels
 *      0..2 are a direction: they go through pre_rot, the z-rotation and the perturbation matrix in the coordinates'
 *      forms ((x R0j + y R1j) + z R2j; x c + y s, y c - x s), and through nothing else (no normalise, jitter, scale, shift).
 *   5. label_out[b, n] = point_label[ci, src]; category_out[b] = category[ci].
 * Bad inputs are never dereferenced and never silently scored.  idx[b] outside [0, M) or L outside [1, P]: the whole cloud
 * is NaN, its labels are -1 and its category is -1 (debug outputs: sel -1, the draws those of a launch with every stage
 * off).  A sel entry outside [0, L): that row is NaN and its label -1.  A label of -1 makes sug_point_ce_fwd's loss NaN and
 * sug_part_iou_accumulate raise its error word.
 * The draws, seed, counter and aug_params are sug_prepare_batch_aug's; the old purposes and words of the generator do not
 * move.  counter may be null only when sel is given and no other draw is needed.  Debug outputs (each may be null): those
 * of sug_prepare_batch_aug, with sel_out [B, N] the source of every row, fill rows included.
 * With lengths null, E == 0 and P >= N, out equals sug_prepare_batch_aug's bit for bit (P < N: rows 0 .. P-1).
 * Limits, checked on the host before the launch: B, M, P, N >= 1; P, N <= SUG_PREP_MAX_POINTS.  Vector stores only, no
 * atomics; bit-reproducible from (inputs, seed, *counter); a cloud's output depends on the batch only through its slot b. */
#define SUG_PREP_NORMALS 128
#define SUG_PREP_DRAW_FILL 0x60000000u
#define SUG_PREP_SEG_MAX_EXTRA 8
int sug_prepare_seg_batch(const float* pts, const float* extra, const uint8_t* point_label, const int64_t* category,
                          const int32_t* lengths, int M, int P, int E, const int32_t* idx, int B, int N, int stages,
                          const float* pre_rot, const float* angles, const float* noise, const int32_t* sel,
                          const float* scales, const float* perturb, const float* shifts, uint64_t seed,
                          const uint64_t* counter, float sigma, float clip, const float* aug_params, float* out,
                          int64_t* label_out, int64_t* category_out, float* angles_out, float* noise_out, int32_t* sel_out,
                          float* scales_out, float* perturb_out, float* shifts_out, void* stream);

/* ---- Batched point-to-point ICP fitness (the geometric sub-domain splitter, dataset_splitter.py:217-231) ----------------
 * icp_distance() calls open3d's registration_icp(source, target, max_correspondence_distance=0.15) once per cloud; this
 * entry point registers B (source, target) pairs in one launch, one workgroup per pair.  src [B or 1, Ns, 3] fp32 with
 * src_batch_stride in floats: 0 = one source for all pairs (the splitter's anchor), else 3*Ns; tgt [B, Nt, 3] fp32.
 * Per pair: count [B] (correspondences of the last evaluation; fitness = count / Ns), rmse [B] (inlier RMSE), iters [B]
 * (updates applied), transform [B, 4, 4] row-major (the accumulated source -> target transform).
 *
 * open3d cannot be run where this library is built or tested, so what follows is a RESTATEMENT of its registration_icp with
 * the defaults (identity init, TransformationEstimationPointToPoint without scaling, ICPConvergenceCriteria(1e-6, 1e-6,
 * 30)) under these assumptions: (a) open3d converts the points to double and works in double; (b) its KD-tree radius
 * search returns the exact nearest neighbour and accepts it when d2 < r*r, strictly; which of two equidistant targets it
 * returns is not specified there, here the lowest index wins; (c) the update is Eigen::umeyama without scaling, i.e.
 * the formula below; (d) the source cloud is transformed cumulatively by each update, not from the composed transform.
 *   evaluate: for each moving source point p the target q of least d2 = (dx*dx + dy*dy) + dz*dz on direct differences
 *     (fp64 on the fp32 input values, no fma), ties -> lowest index; a correspondence when d2 < r*r;
 *     count = their number, rmse = sqrt(sum d2 / count), 0 when count == 0.
 *   loop: result = evaluate; at most max_iteration times: { stop if count == 0;  with the means pbar, qbar and
 *     Sigma = (1/n) sum (q - qbar)(p - pbar)^T = U S V^T:  R = U diag(1, 1, sign(det U det V)) V^T, t = qbar - R pbar;
 *     p <- R p + t for every source point; transform <- [R t; 0 1] . transform; keep the previous result, evaluate;
 *     stop when |d fitness| < rel_fitness and |d rmse| < rel_rmse }.
 * Sigma is formed from the raw sums (sum q p^T / n - qbar pbar^T; the splitter's clouds lie in the unit ball about their
 * mean, where that loses nothing that matters) and decomposed by a cyclic one-sided Jacobi iteration (at most 12 sweeps).
 * R is assembled as u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T from the two leading singular pairs, which equals the
 * formula above whenever Sigma has rank >= 2 and is a proper rotation for EVERY Sigma: with rank 1 the rotation about the
 * determined axis is arbitrary (an orthogonal completion: deterministic, but set by rounding residue when Sigma's second
 * column does not vanish exactly), with rank 0 (all correspondences on one point) R = I; never NaN.
 * All sums run in one fixed order without atomics: results are bit-identical from run to run, and a pair's result does
 * not depend on the batch it is launched in.
 * Checked on the host before the launch: no null pointer, B >= 1, 1 <= Ns, Nt <= SUG_ICP_MAX_POINTS, 0 <= max_iteration <= 64,
 * max_corr_dist > 0, src_batch_stride 0 or 3*Ns. */
#define SUG_ICP_MAX_POINTS 1024
int sug_icp_fitness(const float* src, int64_t src_batch_stride, const float* tgt, int B, int Ns, int Nt,
                    double max_corr_dist, int max_iteration, double rel_fitness, double rel_rmse, int32_t* count,
                    double* rmse, int32_t* iters, double* transform, void* stream);

/* ---- Point Feature Histograms and the histogram cloud distance (utils/pfh.py: PFH.calc_normals :270-301, PFH.calcHistArray
 * :303-348, pfh_hist_distance :146-159) --------------------------------------------------------------------------------------
 * sug_pfh_descriptors: M clouds pts [M, N, 3] fp32 in one launch, one workgroup per cloud -> hist [M, N, div^3] fp64,
 * normals [M, N, 3] fp64, nbr_idx [M, N, k] int32 (padded with -1), nbr_cnt [M, N] int32, used_cnt [M] int32, with
 * k = nneighbors.  All arithmetic is fp64 on the fp32 coordinates converted once (the reference works in double and the bin
 * decisions are thresholds), without fma; every sum in one fixed order, no atomics: bit-identical from run to run, and a
 * cloud's result does not depend on the batch it is launched in.
 *   neighbours (getNeighbors :253-268): the candidates of point i are all j, j = i included, with
 *     sqrt((dx*dx + dy*dy) + dz*dz) <= rad on direct differences; ordered by (distance, index); the FIRST of that order is
 *     dropped -- normally i itself; with an exact duplicate of lower index it is the duplicate, and i stays its own
 *     neighbour, as in the reference -- and the next k are the neighbours, in that order.  A point left without a neighbour
 *     is UNUSED.
 *   normal (:289-299): the covariance of the neighbours only (not the point), centred on their mean, divided by their
 *     count; the eigenvector of its smallest eigenvalue by a cyclic Jacobi iteration (at most 12 sweeps; equal eigenvalues
 *     -> the lowest column); negated when normal . (-p_i) < 0.  With fewer than three non-collinear neighbours the null space
 *     is more than a line: the reference returns whatever LAPACK leaves there, here the result is deterministic, finite and
 *     of unit length, but not pinned to anything.
 *   histogram (:303-348): p_list = [i] + neighbours; for every unordered pair (z before p in the list), with
 *     a = n_p . (p_z - p_p) and b = n_z . (p_p - p_z), p is the source iff arccos(a) <= arccos(b), i.e. iff |a| <= 1 and
 *     |b| <= 1 and a >= b (a NaN from |.| > 1 makes the comparison false); u = n_s, d = (p_t - p_s) / |p_t - p_s|,
 *     v = d x u, w = u x v, alpha = v . n_t, phi = u . d, theta = atan((w . n_t) / (u . n_t)); dot products as
 *     (x*x' + y*y') + z*z'.  IEEE semantics throughout: a zero distance gives NaN features, a division by zero +-pi/2.
 *     bin = step(alpha) + div * step(phi) + div^2 * step(theta), step(f) = the number of thresholds <= f with the
 *     thresholds -1 + i * (2 / div) for alpha and phi and -pi/2 + i * (pi / div) for theta, i = 1 .. div - 1 (:441-495);
 *     a NaN compares false everywhere and lands in the last bin.  row = counts / comb(k + 1, 2) with the CONFIGURED k, not
 *     the found count (:311), one correctly rounded fp64 division: bit-identical to numpy's.
 *   unused points: the reference means to drop them (pc_[used_idx]) while its neighbour indices still refer to the full
 *     cloud, so a cloud with an isolated point raises there or is "skipped".  Here an unused point has a zero histogram row,
 *     nbr_cnt 0 and a zero normal and takes no part in distances; no other point can have it as a neighbour, so the rest of
 *     the cloud is unaffected.  used_cnt[m] == N marks the clouds the reference itself can process.
 * sug_pfh_hist_distance: B (source, target) pairs in one launch, one workgroup per pair.  histS [B or 1, Ns, D] fp64 and
 * cntS [B or 1, Ns] int32 (the nbr_cnt above: a row is used iff its count is > 0) with src_batch_stride in doubles: 0 = one
 * source for all pairs (the splitter's anchor), else Ns*D; histT [B, Nt, D], cntT [B, Nt] -> out [B] fp64: over the used rows
 * i of S the minimum over the used rows j of T of sqrt(sum_d (hS_i[d] - hT_j[d])^2) (d ascending), then np.median of those
 * minima (an even count: the mean of the two middle values); NaN when either side has no used row.  Finite histograms
 * are assumed.
 * Checked on the host before the launch: no null pointer, M, B >= 1, 1 <= N, Ns, Nt <= SUG_PFH_MAX_POINTS,
 * 1 <= nneighbors <= SUG_PFH_MAX_NEIGHBORS, 2 <= div <= 5 (D one of 8, 27, 64, 125), rad positive and finite,
 * src_batch_stride 0 or Ns*D. */
#define SUG_PFH_MAX_POINTS 1024
#define SUG_PFH_MAX_NEIGHBORS 16
int sug_pfh_descriptors(const float* pts, int M, int N, double rad, int nneighbors, int div, double* hist, double* normals,
                        int32_t* nbr_idx, int32_t* nbr_cnt, int32_t* used_cnt, void* stream);
int sug_pfh_hist_distance(const double* histS, const int32_t* cntS, int64_t src_batch_stride, const double* histT,
                          const int32_t* cntT, int B, int Ns, int Nt, int D, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUG_AMD_H */
