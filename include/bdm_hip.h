/*
 * bdm_hip.h -- C ABI of libbdm_hip.so, the MI355X (gfx950) implementation of BDM's
 * coupled-diffusion sampling hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named host_*; tensors are contiguous,
 *     channel-first (B, C, N), fp32 / int32 -- the layout of the reference plugin;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call only
 *     enqueues work on that stream (no allocation, no synchronisation: safe to capture
 *     into a hipGraph);
 *   - outputs and workspaces are caller-allocated; the callee never allocates;
 *   - the return value is 0 on success, non-zero otherwise (1 bad argument, 2 launch
 *     failure, 3 unsupported configuration); bdm_last_error() returns a thread-local
 *     message.  Nothing in the library calls exit() (the reference's CUDA_CHECK_ERRORS
 *     does: experiments/model/pvcnn/modules/functional/src/cuda_utils.cuh:28-37).
 *
 * Section 1 replaces, one entry point per function, the forward half of the reference's
 * pybind11 plugin `_pvcnn_backend`
 *   (experiments/model/pvcnn/modules/functional/src/bindings.cpp:10-37; identical copy
 *    in experiments/pvd/modules/functional/src/).
 * Sections 2-4 replace the stock-PyTorch operators and the Python loops the reference
 * runs around that plugin inside the per-step denoiser forward and the DDPM loop
 * (reference file:line given per function).
 */
#ifndef BDM_HIP_H
#define BDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *bdm_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int bdm_abi_version(void);

/* ------------------------------------------------------------------------------------
 * 1. `_pvcnn_backend` forward operators
 * ---------------------------------------------------------------------------------- */

/* furthest_point_sampling (sampling.cpp:43-58, sampling.cu:86-167).
 * coords (b,3,n) -> indices (b,m) int32.  indices[.,0] = 0; ties between equal maxima
 * resolve to the smallest (k mod 512), then the smallest k, as the reference's 512-thread
 * reduction does.  centers_out (b,3,m) may be NULL; when given it receives
 * gather(coords, indices), i.e. functional/sampling.py:37-48 in one launch. */
int bdm_furthest_point_sampling(int b, int n, int m, const float *coords, int *indices,
                                float *centers_out, void *stream);

/* gather_features_forward (sampling.cpp:6-23, sampling.cu:17-31).
 * features (b,c,n), indices (b,m) -> out (b,c,m). */
int bdm_gather_features_forward(int b, int c, int n, int m, const float *features,
                                const int *indices, float *out, void *stream);

/* ball_query (ball_query.cpp:6-30, ball_query.cu:19-50).
 * centers (b,3,m), points (b,3,n) -> neighbors (b,m,u) int32: first u points (ascending
 * index) with d2 < radius*radius (strict), padded with the first hit, all zero when no hit. */
int bdm_ball_query(int b, int n, int m, float radius, int u, const float *centers,
                   const float *points, int *neighbors, void *stream);

/* grouping_forward (grouping.cpp:6-24, grouping.cu:18-36).
 * features (b,c,n), indices (b,m,u) -> out (b,c,m,u). */
int bdm_grouping_forward(int b, int c, int n, int m, int u, const float *features,
                         const int *indices, float *out, void *stream);

/* three_nearest_neighbors_interpolate_forward (neighbor_interpolate.cpp:6-40,
 * neighbor_interpolate.cu:20-129).  points (b,3,n), centers (b,3,m), features (b,c,m)
 * -> out (b,c,n), indices (b,3,n) int32, weights (b,3,n). */
/* PointNetFPModule input assembly in one launch (pointnet.py:104-112): out0 = cat[interpolate(fa), fs] (c_a + c_s rows),
 * out1 = interpolate(ft) (c_t rows), with the (indices, weights) of bdm_three_nn_search.  Same arithmetic as
 * bdm_three_nn_apply (three products, two adds, no contraction). */
int bdm_fp_assemble(int b, int m, int n, const int *indices, const float *weights, int c_a, const float *fa, long long bs_a,
                    int ld_a, int c_s, const float *fs, long long bs_s, int ld_s, int c_t, const float *ft, long long bs_t,
                    int ld_t, float *out0, long long bs_0, int ld_0, float *out1, long long bs_1, int ld_1, void *stream);
/* The same with the kernel form chosen by the caller (equality tests): 0 = by sizes as bdm_fp_assemble (source rows staged in LDS per
 * (shape, channel chunk) wherever a row of m floats fits 64 KB), 1 = the per-point kernel (three scattered loads per element), 2 = the
 * staged kernel or BDM_ERR_ARG.  All forms evaluate the same expression per element: identical bits. */
int bdm_fp_assemble_form(int form, int b, int m, int n, const int *indices, const float *weights, int c_a, const float *fa,
                         long long bs_a, int ld_a, int c_s, const float *fs, long long bs_s, int ld_s, int c_t, const float *ft,
                         long long bs_t, int ld_t, float *out0, long long bs_0, int ld_0, float *out1, long long bs_1, int ld_1,
                         void *stream);
int bdm_three_nn_interpolate_forward(int b, int c, int m, int n, const float *points,
                                     const float *centers, const float *features, float *out,
                                     int *indices, float *weights, void *stream);
/* The two halves of the above, so that one search can serve several feature tensors
 * (the reference repeats the search for t_emb: modules/pointnet.py:107-108). */
int bdm_three_nn_search(int b, int m, int n, const float *points, const float *centers,
                        int *indices, float *weights, void *stream);
/* features (b,c,m) with row stride ld_f and batch stride bs_f (elements);
 * out likewise (ld_o, bs_o): lets the caller write straight into a concat buffer. */
int bdm_three_nn_apply(int b, int c, int m, int n, const float *features, long long bs_f, int ld_f,
                       const int *indices, const float *weights, float *out, long long bs_o, int ld_o,
                       void *stream);

/* avg_voxelize_forward (vox.cpp:17-43, vox.cu:18-72).
 * features (b,c,n), coords (b,3,n) int32 in [0,r) -> out (b,c,r^3), ind (b,n), cnt (b,r^3).
 * Deterministic: every voxel sums its points in ascending point index (the reference's
 * float atomicAdd leaves the order to thread timing).  workspace: bdm_voxelize_workspace_bytes. */
size_t bdm_voxelize_workspace_bytes(int b, int n, int r);
int bdm_avg_voxelize_forward(int b, int c, int n, int r, const float *features, const int *coords,
                             float *out, int *ind, int *cnt, void *workspace, void *stream);

/* trilinear_devoxelize_forward, inference form (trilinear_devox.cpp:18-55,
 * trilinear_devox.cu:21-105).  coords (b,3,n) float in [0,r-1], grid (b,c,r^3) -> out (b,c,n). */
int bdm_trilinear_devoxelize_forward(int b, int c, int n, int r, const float *coords,
                                     const float *grid, float *out, void *stream);

/* --- the training half of the plugin (bindings.cpp:10-37): gradient operators and the training-mode devoxelisation.
 * Outside the sampling hot path (they serve training_bdm_merging, main_merging.py:242-366); present so that the plugin
 * surface is complete.  grad_x is fully written by the callee (zero-filled, then accumulated).  Scatter-adds are float
 * atomics as in the reference (grouping.cu:58-77, neighbor_interpolate.cu:145-170, trilinear_devox.cu:119-162,
 * sampling.cu:52-66); avg_voxelize_backward (vox.cu:86-110) is a gather. */
int bdm_gather_features_backward(int b, int c, int n, int m, const float *grad_y, const int *indices,
                                 float *grad_x, void *stream);
int bdm_grouping_backward(int b, int c, int n, int m, int u, const float *grad_y, const int *indices,
                          float *grad_x, void *stream);
int bdm_three_nn_interpolate_backward(int b, int c, int n, int m, const float *grad_y, const int *indices,
                                      const float *weights, float *grad_x, void *stream);
int bdm_trilinear_devoxelize_backward(int b, int c, int n, int r, const int *inds, const float *wgts,
                                      const float *grad_y, float *grad_x, void *stream);
int bdm_avg_voxelize_backward(int b, int c, int n, int r, const int *ind, const int *cnt, const float *grad_y,
                              float *grad_x, void *stream);
/* trilinear_devoxelize_forward with is_training = true: also returns inds (b,8,n) int32 and wgts (b,8,n), corner order
 * 000, 001, 010, 011, 100, 101, 110, 111 (trilinear_devox.cu:21-105). */
int bdm_trilinear_devoxelize_forward_training(int b, int c, int n, int r, const float *coords, const float *grid,
                                              float *out, int *inds, float *wgts, void *stream);

/* ------------------------------------------------------------------------------------
 * 2. Dense per-point / per-voxel operators of one denoiser forward
 *    (stock nn.Modules in the reference; hand-written gfx950 kernels here)
 *    Strided operands: a (B, C, L) tensor is addressed as base + b*bs + c*ld + l (elements),
 *    so callers can read from / write into channel slices of concat buffers
 *    (torch.cat in pvcnn.py:104,120 and pointnet.py:110) without copies.
 * ---------------------------------------------------------------------------------- */

/* Conv1d / Conv2d with kernel 1 (+ bias [+ per-shape bias] [+ LeakyReLU]):
 *   y[b] (m x n) = act(w (m x k, row stride ldw) * x[b] (k x n) + bias[m] + batch_bias[b][m]) + residual[b]
 * Replaces nn.Conv1d/nn.Conv2d(k=1) in modules/shared_mlp.py:25-30, the q/k/v/out projections of
 * modules/pvconv.py:21-31, pvcnn_fuse.py:111-123 and the classifier (pvcnn.py:62-69).
 * act: 0 none, 2 LeakyReLU(slope), 3 exact GELU; bias, batch_bias and residual may be NULL (residual: the
 * `proj(x) + skip` additions of pvcnn_fuse.py:203-212).  f32-input MFMA, fp32 accumulate. */
int bdm_pointwise_conv(int b, int m, int k, int n, const float *w, int ldw, const float *x,
                       long long bs_x, int ld_x, const float *bias, const float *batch_bias,
                       int ld_bb, const float *residual, long long bs_r, int ld_r, float *y,
                       long long bs_y, int ld_y, int act, float slope, void *stream);
/* Host only: the kernel the 1x1 convolutions (bdm_pointwise_conv, bdm_pointwise_conv_gn*) launch for this shape -- what the launch
 * path itself decides, not a restatement.  Returns 0: the general kernel, *mi / *ni / *bk receive its tile (32 mi rows x 128 ni
 * columns per workgroup, K chunk bk); 1 or 2: the skinny K-split kernel with that many 32-column blocks (*mi = *ni = *bk = 0).
 * The out pointers are HOST pointers and may be NULL.  The choice depends on (b, m, k, n) only. */
int bdm_pointwise_conv_variant(int b, int m, int k, int n, int *mi, int *ni, int *bk);

/* nn.GroupNorm(groups, c) over (b, c, l) with optional residual added first and optional Swish
 * (shared_mlp.py:27-29; pvconv.py:78-86; Attention: norm(h + x) then Swish, pvconv.py:59-61).
 * act: 0 none, 1 Swish.  In-place (y == x) is allowed.  Deterministic two-pass reduction. */
size_t bdm_group_norm_workspace_bytes(int b, int groups);
int bdm_group_norm(int b, int c, int l, int groups, const float *x, long long bs_x, int ld_x,
                   const float *residual, long long bs_r, int ld_r, const float *gamma,
                   const float *beta, float eps, int act, float *y, long long bs_y, int ld_y,
                   void *workspace, void *stream);
/* Host only: the kernels bdm_group_norm launches for these sizes, strides and pointers -- what the launch path itself decides, not a
 * restatement.  0: one pass (a (shape, group) chunk of at most 65536 floats kept in registers), 1: the float4 two-pass pair, 2: the
 * scalar two-pass pair (rows not dense, l % 4 != 0, or a base / batch stride off 16 bytes).  Only the ADDRESSES of x, residual
 * (may be NULL) and y are looked at; no GPU call.  bdm_group_norm_stats takes 1 or 2 by the same rule with residual = NULL, y = x. */
int bdm_group_norm_route(int c, int l, int groups, const float *x, long long bs_x, int ld_x, const float *residual,
                         long long bs_r, int ld_r, const float *y, long long bs_y, int ld_y);

/* features.max(dim=-1) over the neighbour axis (pointnet.py:86): x (b,c,m,u) -> y (b,c,m) strided. */
/* SharedMLP = [Conv k=1 -> GroupNorm(8) -> Swish]* (modules/shared_mlp.py:25-30) without a pass per GroupNorm.
 *   bdm_pointwise_conv_gn: y = W x' + bias with
 *     x' = x, or (in_partial != NULL) x' = Swish(GroupNorm(x)) applied while the operand is staged, the statistics of x taken
 *          from the slice partials in_partial (b, in_groups, in_slices, 2 doubles) its producer left (in_groups <= 8, k <= 1024);
 *     amax != NULL: amax[s * ceil(m / amax_rows) + i] (b * ceil(m / amax_rows) slots, ZERO on entry) receives max |y| over rows
 *          [i * amax_rows, (i + 1) * amax_rows) of shape s (amax_rows % 32 == 0): the per-shape scales of the fp16x3
 *          attention, bdm_attention_core_h2;
 *     x2 != NULL: the operand is torch.cat([x (k1 rows), x2 (k - k1 rows)], dim=1) read in place (pointnet.py:108-110, the skip
 *          features of an FP module are never copied next to the interpolated ones);
 *     and (out_partial != NULL) the (sum, sum of squares) of y per (shape, group of m / out_groups channels) written as
 *          bdm_pointwise_conv_gn_slices(b, m, k, n, out_groups) slices per (shape, group) into out_partial
 *          (b, out_groups, slices, 2 doubles); channels per group must be a power of two >= 4.
 *   bdm_max_over_neighbors_gn: max over the neighbour axis of Swish(GroupNorm(x)), statistics from such partials
 *     (pointnet.py:86 after the last MLP layer).
 * Deterministic (fixed summation orders, no float atomics). */
int bdm_pointwise_conv_gn_slices(int b, int m, int k, int n, int groups);
int bdm_pointwise_conv_gn(int b, int m, int k, int n, const float *w, int ldw, const float *x, long long bs_x, int ld_x,
                          const float *x2, long long bs_x2, int ld_x2, int k1, const float *bias, float *y, long long bs_y,
                          int ld_y, const void *in_partial, int in_slices, int in_groups, const float *in_gamma,
                          const float *in_beta, float in_eps, int out_groups, void *out_partial, float *amax, int amax_rows,
                          void *stream);
/* bdm_pointwise_conv_gn with a per-element addend: y = W x' + bias + add (add (b, m, n) strided as y), statistics and amax taken
 * over y including the addend -- the hoisted share of a layer whose other input columns were applied to the conditioning image once
 * per trajectory (bdm_sparse_conv_rows_from_map, ops.Conditioning).  Not for the skinny shapes. */
int bdm_pointwise_conv_gn_add(int b, int m, int k, int n, const float *w, int ldw, const float *x, long long bs_x, int ld_x,
                              const float *x2, long long bs_x2, int ld_x2, int k1, const float *bias, float *y, long long bs_y,
                              int ld_y, const void *in_partial, int in_slices, int in_groups, const float *in_gamma,
                              const float *in_beta, float in_eps, int out_groups, void *out_partial, float *amax, int amax_rows,
                              const float *add, long long bs_add, int ld_add, void *stream);
/* The same with a per-SHAPE bias batch_bias (b, ld_bb >= m): y = (W x' + bias) + batch_bias[shape] (+ add; may be NULL), statistics and
 * amax over that y.  The share of a layer whose remaining input columns are constant along a shape's points -- the time embedding
 * concatenated to the features (pvcnn.py:88, pointnet.py:104-112): W . [x ; t 1^T] = W_x . x + (W_t . t) 1^T. */
int bdm_pointwise_conv_gn_bb(int b, int m, int k, int n, const float *w, int ldw, const float *x, long long bs_x, int ld_x,
                             const float *x2, long long bs_x2, int ld_x2, int k1, const float *bias, float *y, long long bs_y,
                             int ld_y, const void *in_partial, int in_slices, int in_groups, const float *in_gamma,
                             const float *in_beta, float in_eps, int out_groups, void *out_partial, float *amax, int amax_rows,
                             const float *batch_bias, int ld_bb, const float *add, long long bs_add, int ld_add, void *stream);

#ifdef BDM_EXPERIMENTAL
/* bf16x6 form of the two entry points above (csrc/experimental/pointwise_s3.hip; measured: no faster, the GEMMs are staging-bound): the weights are split ONCE into exact bf16 triples
 * (bdm_pointwise_s3_pack_weights: packed = bdm_pointwise_s3_weight_elems(m, k) 16-bit elements), the activations while they are
 * staged; six partial products per fp32 product on v_mfma_f32_32x32x16_bf16, fp32 accumulate: fp32-grade (no scale, no range limit)
 * at 2.7x the matrix rate of the fp32-MFMA kernel.  Same arguments and semantics otherwise; statistics slices are always
 * ceil(n / 128) * max(1, (m / groups) / 32) (the canonical layout).  Not for the skinny shapes (n <= 64, k >= 128: K-split kernel). */
size_t bdm_pointwise_s3_weight_elems(int m, int k);
int bdm_pointwise_s3_pack_weights(int m, int k, const float *w, int ldw, void *packed, void *stream);
int bdm_pointwise_conv_s3(int b, int m, int k, int n, const void *packed_w, const float *x, long long bs_x, int ld_x,
                          const float *bias, const float *batch_bias, int ld_bb, const float *residual, long long bs_r,
                          int ld_r, float *y, long long bs_y, int ld_y, int act, float slope, void *stream);
int bdm_pointwise_conv_gn_s3(int b, int m, int k, int n, const void *packed_w, const float *x, long long bs_x, int ld_x,
                             const float *x2, long long bs_x2, int ld_x2, int k1, const float *bias, float *y, long long bs_y,
                             int ld_y, const void *in_partial, int in_slices, int in_groups, const float *in_gamma,
                             const float *in_beta, float in_eps, int out_groups, void *out_partial, float *amax,
                             int amax_rows, void *stream);
#endif /* BDM_EXPERIMENTAL */
int bdm_max_over_neighbors_gn(int b, int c, int m, int u, const float *x, const void *in_partial, int in_slices, int groups,
                              const float *gamma, const float *beta, float eps, float *y, long long bs_y, int ld_y,
                              void *stream);
/* Host only: lanes that share a row of u floats in bdm_max_over_neighbors_gn (the launch path's own choice): u / 4 when u % 4 == 0,
 * u <= 256, u / 4 is a power of two and x is 16-byte aligned, else 1.  Only the ADDRESS of x is looked at; no GPU call. */
int bdm_max_over_neighbors_gn_lanes(int u, const float *x);
int bdm_max_over_neighbors(int b, int c, int m, int u, const float *x, float *y, long long bs_y,
                           int ld_y, void *stream);

/* BallQuery.forward's grouped tensor (modules/ball_query.py:16-30) in one launch:
 * out (b, 3+c, m, u) = cat[ grouping(coords, idx) - centers[..., None], grouping(features, idx) ].
 * workspace: NULL -> channel-first gather: for 256 <= n <= 8192 points a workgroup stages three channel rows of ALL the shape's points in
 * LDS (LDS-DMA, global_load_lds_dwordx4, when n % 256 == 0 and the rows are 16-byte aligned) and gathers from there (round 6), otherwise
 * one scattered load per element; else >= bdm_sa_group_workspace_bytes(b, c, n) bytes (16-byte aligned): [coords ; features] are first
 * repacked point-major so the gather reads 16-byte runs.  Same values in every form (a gather). */
size_t bdm_sa_group_workspace_bytes(int b, int c, int n);
int bdm_sa_group(int b, int c, int n, int m, int u, const float *coords, const float *centers,
                 const float *features, long long bs_f, int ld_f, const int *indices, float *out,
                 void *workspace, void *stream);

/* PointNetSAModule.forward (modules/pointnet.py:80-90) at the first level, WITHOUT the grouped tensor or either layer's output in
 * memory: grouping ([xyz - centre ; features], 1 <= c <= 32 feature rows), two SharedMLP layers (shared_mlp.py:11-37: Conv2d k=1 ->
 * GroupNorm(8) -> Swish; widths m1 = 32, m2 = 64), max over the u = 32 neighbours -> out (b, m2, m).  Four launches: the features
 * repacked point-major into `rows` (bdm_sa_mlp2_fused_rows_bytes(b, c, n) bytes, 16-byte aligned), then three passes that each
 * re-gather the neighbours' rows and recompute what they need (pass 1: GroupNorm-1 statistics; pass 2: GroupNorm-2 statistics;
 * pass 3: the output).  w1 (m1, 3 + c), w2 (m2, m1) as the convolutions hold them.  partial1 / partial2: fp64 scratch,
 * b * 8 * bdm_sa_mlp2_fused_slices(b, m) * 2 elements each.  Deterministic. */
size_t bdm_sa_mlp2_fused_rows_bytes(int b, int c, int n);
int bdm_sa_mlp2_fused_slices(int b, int m);
int bdm_sa_mlp2_fused(int b, int c, int n, int m, int u, int m1, int m2, const float *coords, const float *features,
                      long long bs_f, int ld_f, const float *centers, const int *indices, const float *w1, const float *b1,
                      const float *g1w, const float *g1b, float eps1, const float *w2, const float *b2, const float *g2w,
                      const float *g2b, float eps2, int groups, void *rows, void *partial1, void *partial2, float *out,
                      long long bs_o, int ld_o, void *stream);

/* y[b][ci][:] = v[b][ci]  -- t_emb[:, :, None].expand(-1, -1, N) (pvcnn.py:88) written into a concat slice. */
int bdm_broadcast_rows(int b, int c, int l, const float *v, int ld_v, float *y, long long bs_y,
                       int ld_y, void *stream);
/* strided row copy (building torch.cat operands in place) */
/* torch.cat([x0, x1], dim=1) in one launch.  A part with ld == 0 is a point-invariant column: element (shape, channel) at
 * x[shape * bs + channel], broadcast along l (the time embedding before the first SA level). */
int bdm_concat2_rows(int b, int l, int c0, const float *x0, long long bs_0, int ld_0, int c1, const float *x1, long long bs_1,
                     int ld_1, float *y, long long bs_y, int ld_y, void *stream);
int bdm_copy_rows(int b, int c, int l, const float *x, long long bs_x, int ld_x, float *y,
                  long long bs_y, int ld_y, void *stream);
/* (b, rows, cols) -> (b, cols, rows): PointCloudModel.forward's transposes (point_cloud_model.py:65). */
int bdm_transpose(int b, int rows, int cols, const float *x, float *y, void *stream);

/* get_timestep_embedding + embedf (pvcnn_utils.py:171-185, pvcnn.py:72-76,87-88):
 * t (b,) float -> out (b, dim) = Linear(LeakyReLU_0.1(Linear([sin, cos](t * freq)))). */
int bdm_time_embedding(int b, int dim, const float *t, const float *w0, const float *b0,
                       const float *w2, const float *b2, float *out, void *stream);
/* the same from int64 timesteps (what the schedulers hand over): t.float() inside the kernel */
int bdm_time_embedding_i64(int b, int dim, const long long *t, const float *w0, const float *b0,
                           const float *w2, const float *b2, float *out, void *stream);

/* Voxelization.forward's coordinate maths (modules/voxelization.py:16-25, normalize=True):
 * coords (b,3,n) -> norm_coords (b,3,n) float in [0, r-1], vox_coords (b,3,n) int32 (round half even). */
int bdm_voxel_coords(int b, int n, int r, float eps, const float *coords, float *norm_coords,
                     int *vox_coords, void *stream);

/* SE3d gate (modules/se.py:8-19, ReLU variant): gate (b,c) = sigmoid(w2 relu(w1 mean_l x)).
 * x (b,c,l) contiguous; mean_ws (b,c) scratch.  counters: NULL -> two launches (row means, then the FC layers); else b
 * ints that are ZERO on entry (and are left zero) -> one launch, the last workgroup of each shape runs the FC layers. */
int bdm_se_gate(int b, int c, int hidden, int l, const float *x, const float *w1, const float *w2,
                float *mean_ws, float *gate, int *counters, void *stream);

/* PVConv tail (pvconv.py:95-96): out = trilinear_devoxelize(grid * gate[:, :, None]) + add.
 * gate and add may be NULL. */
int bdm_devoxelize_gate_add(int b, int c, int n, int r, const float *coords, const float *grid,
                            const float *gate, const float *add, long long bs_a, int ld_a,
                            float *out, long long bs_o, int ld_o, void *stream);

/* Attention core (pvconv.py:46-55): out[c][i] = sum_j v[c][j] softmax_j(sum_c' q[c'][i] k[c'][j]),
 * no 1/sqrt(c) scale.  q, k, v share strides.  l <= 64: one workgroup per shape (global attention);
 * otherwise a flash-style MFMA kernel (c <= 64; the 16^3-token voxel attention).
 * workspace: NULL -> fp32-input MFMA kernel (only in `make EXPERIMENTAL=1` builds; BDM_ERR_UNSUPPORTED otherwise); else >= bdm_attention_workspace_bytes(b, c, l) bytes -> the bf16x6
 * kernel (q, k, v pre-split into exact bf16 triples, six partial products per fp32 product; fp32-grade accuracy). */
size_t bdm_attention_workspace_bytes(int b, int c, int l);
int bdm_attention_core(int b, int c, int l, const float *q, const float *k, const float *v,
                       long long bs_qkv, int ld_qkv, float *out, long long bs_o, int ld_o,
                       void *workspace, void *stream);
/* fp16x3 form (half the matrix work of the bf16x6 kernel behind bdm_attention_core): needs amax[3 s + 0..2] = max |q|, |k|, |v| of
 * shape s (the projection GEMM leaves them: bdm_pointwise_conv_gn amax with amax_rows = c) and a workspace of bdm_attention_h2_workspace_bytes;
 * 64 < l, c <= 64 */
size_t bdm_attention_h2_workspace_bytes(int b, int c, int l, int key_slices);
/* key_slices = key ranges per (shape, query tile), 1 .. 8: each range leaves an unnormalised partial result, merged in ascending key order
 * (deterministic).  The CALLER chooses the count and passes it to both functions (no environment look-up in the library: the workspace and
 * the launch cannot disagree, and the launch checks workspace_bytes).  bdm_attention_h2_key_slices(b, l) is the library's recommendation
 * for b shapes of l positions -- 1 when the (shape, query tile) items fill the chip, 2 or 4 for few shapes; a shape's bits depend on the
 * count, so a caller that wants them independent of the launch's batch passes a fixed one (host side: BDM_ATTN_KSPLIT, read once). */
int bdm_attention_h2_key_slices(int b, int l);
int bdm_attention_core_h2(int b, int c, int l, const float *q, const float *k, const float *v, long long bs_qkv, int ld_qkv,
                          const float *amax, float *out, long long bs_o, int ld_o, void *workspace, size_t workspace_bytes,
                          int key_slices, void *stream);

#ifdef BDM_EXPERIMENTAL  /* fp32-input MFMA convolution family (csrc/experimental/conv3d.hip): `make EXPERIMENTAL=1` */
/* nn.Conv3d(cin, cout, 3, padding=1) on (b, cin, r, r, r), r in {8, 16, 32} (pvconv.py:75-85).
 * packed_w = bdm_conv3d_pack_weights(w) : [27][cin][cout] from the module's (cout, cin, 3, 3, 3). */
int bdm_conv3d_pack_weights(int cout, int cin, const float *w, float *packed, void *stream);
int bdm_conv3d_3x3x3(int b, int cin, int cout, int r, const float *x, const float *packed_w,
                     const float *bias, float *y, void *stream);
/* Same convolution for an input that is a freshly voxelised point cloud (first Conv3d of a PVConv): rowocc
 * (b, r*r) uint8 flags the (x, y) grid rows holding at least one point (bdm_voxel_row_occupancy from the
 * voxeliser's cnt); work on all-zero operand rows is skipped.  Results are bit-identical to the dense call. */
int bdm_conv3d_3x3x3_sparse(int b, int cin, int cout, int r, const float *x, const float *packed_w,
                            const float *bias, const unsigned char *rowocc, float *y, void *stream);
#endif /* BDM_EXPERIMENTAL */
/* rowocc (b, r*r) uint8: grid row (x, y) holds an occupied cell (from the voxeliser's cnt) */
int bdm_voxel_row_occupancy(int b, int r, const int *cnt, unsigned char *rowocc, void *stream);

/* --- the same convolution at fp32 accuracy on the BF16 matrix cores ("bf16x6", conv3d_s3.hip) ---
 * Every fp32 operand is split exactly into three bf16 terms and the six leading partial products are accumulated in
 * fp32 (dropped terms <= 2^-23 of the product).  Activations travel in the S3 layout (b, ceil(c/8), 3, r^3, 8) bf16,
 * produced directly by the voxeliser and by the GroupNorm(+Swish) between the two convolutions of a PVConv. */
size_t bdm_conv3d_s3_weight_elems(int cout, int cin);   /* number of bf16 elements of the packed weights */
int bdm_conv3d_s3_pack_weights(int cout, int cin, const float *w, void *packed, void *stream);
int bdm_conv3d_3x3x3_s3(int b, int cin, int cout, int r, const void *x_s3, const void *packed_w,
                        const float *bias, float *y, void *stream);
/* x (b, c, v) fp32 contiguous -> S3 of GroupNorm(groups)(x) [Swish when act == 1]; groups == 0: plain conversion.
 * workspace: bdm_group_norm_workspace_bytes. */
int bdm_group_norm_to_s3(int b, int c, int v, int groups, const float *x, const float *gamma,
                         const float *beta, float eps, int act, void *out_s3, void *workspace, void *stream);
int bdm_group_norm_stats(int b, int c, int l, int groups, const float *x, long long bs_x, void *workspace,
                         int *slices_out, void *stream);
/* avg_voxelize_forward writing S3 (features strided: bs_f, ld_f); same deterministic summation order. */
int bdm_voxelize_plan(int b, int n, int r, const int *coords, int *ind, int *cnt, void *workspace, void *stream);
/* the plan plus bdm_voxel_compact and bdm_voxel_row_occupancy of the same shape in ONE launch (same values).  It also leaves one
 * 32-byte cell record {count, start, first six list entries} per occupied row in the workspace (layout: csrc/common.h, VoxWs), which
 * bdm_sparse_voxel_features_s3 / _f32 read instead of walking occ_list -> cnt / start -> list; a workspace filled by
 * bdm_voxelize_plan carries a cleared flag instead, and they walk the lists. */
int bdm_voxelize_plan_full(int b, int n, int r, int n_max, const int *coords, int *ind, int *cnt, void *workspace,
                           int *occ_index, int *occ_list, int *n_occ, unsigned char *rowocc, void *stream);
int bdm_avg_voxelize_s3(int b, int c, int n, int r, const float *features, long long bs_f, int ld_f,
                        const int *coords, void *out_s3, int *ind, int *cnt, void *workspace, void *stream);

/* fp16x3 form of the dense convolution (default for the second convolution of every PVConv): operands stored as two
 * fp16 terms (hi, lo) after exact power-of-two scaling, three partial products per fp32 product on
 * v_mfma_f32_16x16x32_f16 -- half the matrix work of bf16x6 at the same accuracy (csrc/conv3d_h2.hip).
 *   packed_w : bdm_conv3d_h2_weight_elems(cout, cin) fp16; inv_scale (cout floats) = 2^-e[co] for the epilogue;
 *              scale_ws (cout floats) is scratch of the pack.
 *   x_h2     : (b, ceil(c/8), 2, v, 8) fp16 = act_scale * swish(group_norm(x)) split in two, from
 *              bdm_group_norm_to_h2 (groups = 0: plain split of act_scale * x).  act_scale is a power of two chosen by
 *              the caller so that the scaled values sit high in fp16's range (|act_scale * x| saturates at 65504);
 *              the convolution receives x_inv_scale = 1 / act_scale. */
size_t bdm_conv3d_h2_weight_elems(int cout, int cin);
int bdm_conv3d_h2_pack_weights(int cout, int cin, const float *w, void *packed, float *scale_ws, float *inv_scale,
                               void *stream);
/* saturated (may be NULL): one device word that is OR-ed with 1 when any scaled value left fp16's range (|act_scale * y| >
 * 65504, or NaN) and was clamped by the split -- the accuracy guard of the fp16x3 path: the host polls the word once per
 * trajectory and re-routes that layer to the bf16x6 kernels (bdm_amd/ops.py: poll_h2_saturation). */
int bdm_group_norm_to_h2(int b, int c, int v, int groups, const float *x, const float *gamma, const float *beta,
                         float eps, int act, float act_scale, void *out_h2, void *workspace,
                         unsigned int *saturated, void *stream);
/* bdm_group_norm_to_h2 with the statistics given as `slices` slice partials per (shape, group) (b, groups, slices, 2 doubles)
 * instead of a statistics pass over x; channels per group >= 4 */
int bdm_group_norm_to_h2_stats(int b, int c, int v, int groups, const float *x, const float *gamma, const float *beta,
                               float eps, int act, float act_scale, void *out_h2, const void *partial, int slices,
                               unsigned int *saturated, void *stream);
/* bdm_group_norm_to_h2_stats for the COMPACT output of the first convolution (bdm_sparse_conv_dil, compact = 1): xc (b, n_dil_max, c)
 * one row per entry of the dilated voxel list, dil_index (b, v) row of voxel v or -1; every voxel outside the list has the value
 * bias[channel] (NULL: 0).  Same result as densifying xc first; the dense fp32 grid is never written or read. */
int bdm_group_norm_to_h2_stats_compact(int b, int c, int v, int groups, const float *xc, int n_dil_max, const int *dil_index,
                                       const float *bias, const float *gamma, const float *beta, float eps, int act,
                                       float act_scale, void *out_h2, const void *partial, int slices,
                                       unsigned int *saturated, void *stream);
int bdm_conv3d_3x3x3_h2(int b, int cin, int cout, int r, const void *x_h2, float x_inv_scale, const void *packed_w,
                        const float *inv_scale, const float *bias, float *y, void *stream);
/* Host only: the kernel instance conv3d_h2q_kernel<mt, nt, r, tx, ty, nw> that bdm_conv3d_3x3x3_h2 / _h2_gn launch for this shape
 * -- what the launch path itself decides, not a restatement: a workgroup of nw waves owns 16 mt output channels x a tx x ty x r
 * brick of voxels (nt 16-voxel blocks per wave).  Returns 0, or BDM_ERR_UNSUPPORTED (3) for a resolution other than 8, 16, 32
 * (the outputs are then 0).  The out pointers are HOST pointers and may be NULL; no GPU call.  Depends on (b, cout, r) only. */
int bdm_conv3d_h2_variant(int b, int cin, int cout, int r, int *mt, int *nt, int *tx, int *ty, int *nw);

/* GroupNorm-folded tail of a PVConv without attention (pvconv.py:84-96): the second convolution leaves its output raw and
 * the GroupNorm(groups) statistics of that output as slice partials (layout / size: bdm_group_norm_workspace_bytes;
 * *slices_out slices per (shape, group)); the consumers then normalise + Swish on the fly instead of rewriting the grid:
 *   bdm_se_gate_gn            per (shape, channel): coef (b, c, 2) = (gamma rstd, beta - mean gamma rstd), and the SE gate
 *                             sigmoid(w2 relu(w1 mean_l swish(coef.x x + coef.y))) (w1 == NULL: only coef is produced)
 *   bdm_devoxelize_gn_gate_add out = trilinear_devoxelize(swish(coef.x grid + coef.y) * gate) + add */
int bdm_conv3d_3x3x3_h2_gn(int b, int cin, int cout, int r, const void *x_h2, float x_inv_scale, const void *packed_w,
                           const float *inv_scale, const float *bias, float *y, int groups, void *gn_workspace,
                           int *slices_out, void *stream);
int bdm_se_gate_gn(int b, int c, int hidden, int l, int groups, const float *x, const void *gn_workspace, int slices,
                   const float *gamma, const float *beta, float eps, const float *w1, const float *w2, float *mean_ws,
                   float *coef, float *gate, void *stream);
int bdm_devoxelize_gn_gate_add(int b, int c, int n, int r, const float *coords, const float *grid, const float *coef,
                               const float *gate, const float *add, long long bs_a, int ld_a, float *out,
                               long long bs_o, int ld_o, void *stream);
/* Point branch of the PVConv folded in as well: bdm_se_gate_gn_pf also turns the slice partials that the branch's 1x1
 * convolution left (bdm_pointwise_conv_gn; pf_groups groups over the same c channels, pf_n points per row) into affine forms
 * pf_coef (b, c, 2), and bdm_devoxelize_gn_gate_add_pf adds Swish(pf_coef.x add + pf_coef.y) with add the RAW convolution
 * output -- the branch's GroupNorm needs no launch of its own. */
int bdm_se_gate_gn_pf(int b, int c, int hidden, int l, int groups, const float *x, const void *gn_workspace, int slices,
                      const float *gamma, const float *beta, float eps, const float *w1, const float *w2, float *mean_ws,
                      float *coef, float *gate, const void *pf_partial, int pf_slices, int pf_groups, int pf_n,
                      const float *pf_gamma, const float *pf_beta, float pf_eps, float *pf_coef, void *stream);
int bdm_devoxelize_gn_gate_add_pf(int b, int c, int n, int r, const float *coords, const float *grid, const float *coef,
                                  const float *gate, const float *add, long long bs_a, int ld_a, const float *add_coef,
                                  float *out, long long bs_o, int ld_o, void *stream);
/* the same with the SE gate computed inside the kernel from se_mean (b, c) = the channel means bdm_se_gate_gn(w1 = NULL) left:
 * one launch less per PVConv, bit-identical gate (same summation order as the separate FC kernel). hidden <= 64. */
int bdm_devoxelize_gn_se_add(int b, int c, int n, int r, const float *coords, const float *grid, const float *coef,
                             const float *se_mean, int hidden, const float *w1, const float *w2, const float *add,
                             long long bs_a, int ld_a, float *out, long long bs_o, int ld_o, void *stream);
/* Host only: the kernel the three bdm_devoxelize_gn_* entry points launch (the launch path's own choice): 0 the global-memory gather,
 * 1 the LDS-cached form.  with_se_mean != 0: bdm_devoxelize_gn_se_add (always 0).  Honours BDM_STAGING (0: never LDS, 1: LDS wherever
 * it fits), read at every call.  Only the ADDRESS of grid is looked at; no GPU call. */
int bdm_devoxelize_gn_route(int b, int c, int r, const float *grid, int with_se_mean);

/* ---- PVConv tail on the SMALL voxel grids (8^3 levels; csrc/pvconv_small.hip) -- per-shape workgroups, no hand-off between them ----
 * bdm_pvconv_tail_small: SE gate (both FC layers of se.py:8-19, from se_mean (b, c) = bdm_se_gate_gn(w1 = NULL)'s channel means)
 * + Swish(GroupNorm-2(grid)) * gate + trilinear devoxelisation at the n points + Swish(GroupNorm(point branch)) (add_coef; NULL: `add`
 * is added as it is) -> out (pvconv.py:91-97), one workgroup per (shape, 8 channels); bit-identical to bdm_se_gate_gn_pf +
 * bdm_devoxelize_gn_gate_add_pf.  With xh != NULL the same workgroups also form the NEXT PVConv's first-convolution operand on the same
 * voxel plan (cnt / plan_workspace / occ_list / n_occ / n_max of bdm_voxelize_plan_full): per occupied cell the mean of `out` over its
 * points (vox.cu:18-72 on the plan's ordered lists: the values of bdm_sparse_voxel_features_f32), times the power of two x_scale,
 * split into (hi, lo) fp16 records xh (b, c/8, 2, n_max) -- what bdm_sparse_split_h2 writes -- and amax_out (b) such that
 * bdm_sparse_conv_gemm_h2 derives x_scale from it; *saturated |= 1 when a scaled value leaves fp16's range. */
int bdm_pvconv_tail_small(int b, int c, int n, int r, int hidden, const float *coords, const float *grid, const float *coef,
                          const float *se_mean, const float *w1, const float *w2, const float *add, long long bs_a, int ld_a,
                          const float *add_coef, float *out, long long bs_o, int ld_o, const int *cnt, const void *plan_workspace,
                          const int *occ_list, const int *n_occ, int n_max, float x_scale, void *xh, float *amax_out, int *saturated,
                          void *stream);
#ifdef BDM_EXPERIMENTAL  /* csrc/experimental/sparse_gather_h2_small.hip: measured not faster */
/* bdm_sparse_conv_gather_h2_small: bdm_sparse_conv_gather_gn + bdm_group_norm_to_h2_stats in one launch, one workgroup per (shape,
 * GroupNorm group): y (b, n_max, 27, cout) = the GEMM's output, out_h2 (b, cout/8, 2, r^3) records = act_scale *
 * Swish(GroupNorm(groups)(conv1 output)) as two fp16 terms (the second convolution's operand); the dense fp32 output of the first
 * convolution is not written.  Needs 8 | cout / groups <= 64. */
int bdm_sparse_conv_gather_h2_small(int b, int cout, int r, int n_max, const float *y, const int *occ_index, const float *bias,
                                    int groups, const float *gamma, const float *beta, float eps, float act_scale, void *out_h2,
                                    unsigned int *saturated, void *stream);
#endif /* BDM_EXPERIMENTAL */

/* bf16x6 form of the two steps above (default): operands pre-split into exact bf16 triples ("S3" records of 8
 * channels x 16 bytes), GEMM on v_mfma_f32_32x32x16_bf16 with six partial products per fp32 product.
 *   xs (b, ceil(c/8), 3, n_max) records; ws (ceil(cin/8), 3, 27*cout) records = bdm_sparse_conv_s3_weight_elems bf16. */
int bdm_sparse_voxel_features_s3(int b, int c, int n, int r, int n_max, const float *features, long long bs_f,
                                 int ld_f, const int *cnt, const void *plan_workspace, const int *occ_list,
                                 const int *n_occ, void *xs, void *stream);
size_t bdm_sparse_conv_s3_weight_elems(int cout, int cin);
int bdm_sparse_conv_pack_weights_s3(int cout, int cin, const float *w, void *ws, void *stream);
int bdm_sparse_conv_gemm_s3(int b, int n_max, int cin, int n27, const void *xs, const void *ws, const int *n_occ,
                            float *y, void *stream);
/* + col_bias (b, n27; batch stride bs_cb floats): y[b][k][tap * cout + co] += col_bias[b][tap * cout + co] on every row -- the share of input channels that are
 * CONSTANT over a shape's occupied cells: the time embedding the reference concatenates to the features before the first PVConv of
 * set-abstraction levels 1.. (pvcnn.py:103; avg_voxelize of a per-shape constant is that constant on every occupied cell, vox.cu:18-72),
 * col_bias[b][tap][co] = sum_c W[co][cin + c][tap] t[b][c].  The gather adds a row once per OCCUPIED neighbour: exactly the
 * zero-padded convolution of the concatenated grid, with the GEMM's K and the feature pass reduced to the real feature channels. */
int bdm_sparse_conv_gemm_s3_cb(int b, int n_max, int cin, int n27, const void *xs, const void *ws, const int *n_occ,
                               const float *col_bias, long long bs_cb, float *y, void *stream);

/* Hoisted form of bdm_sparse_voxel_features* + bdm_sparse_conv_gemm* for an input whose feature channels are a gather of a per-image
 * map (the projection conditioning x_in[i] = [xyz_i, F[pix_i]], projection_model.py:179-231): with hmap (b, hw, n27) = F . Wf^T
 * computed once per trajectory (n27 = 27 * cout columns ordered tap * cout + co) and wx (n27, 3) the coordinate columns of the
 * weights,  y (b, n_max, n27)[k] = mean over the points i of occupied cell k (ascending i) of (hmap[pix_i] (0 where pix_i < 0) +
 * wx . xyz_i): the rows bdm_sparse_conv_gather consumes.  xyz (b, 3, n), pix (b, n) from bdm_rasterize_points. */
int bdm_sparse_conv_rows_from_map(int b, int n, int r, int n_max, int n27, int hw, const float *hmap, const int *pix,
                                  const float *xyz, const float *wx, const int *cnt, const void *plan_workspace,
                                  const int *occ_list, const int *n_occ, float *y, void *stream);

/* --- first convolution of a PVConv on the occupied voxels only (sparse_conv.hip) ---
 * out = Conv3d(avg_voxelize(features)) without materialising the dense grid:
 *   bdm_voxel_compact          cnt (b, r^3) -> occ_index (b, r^3) [-1 = empty], occ_list (b, n_max), n_occ (b)
 *   bdm_sparse_voxel_features  per-voxel mean features of the occupied cells, xc (b, c, n_max) (zeros beyond n_occ);
 *                              plan_workspace = the workspace bdm_voxelize_plan filled
 *   bdm_sparse_conv_gemm       y (b, n_max, 27*cout) = xc^T . wt,   wt = bdm_sparse_conv_pack_weights(w) (cin, 27*cout)
 *   bdm_sparse_conv_gather     out (b, cout, r^3) = bias + sum over taps (fixed order) of the occupied neighbours' y rows
 * Deterministic; equals bdm_conv3d_3x3x3(avg_voxelize) up to fp32 summation order. */
int bdm_voxel_compact(int b, int r, int n_max, const int *cnt, int *occ_index, int *occ_list, int *n_occ,
                      void *stream);
int bdm_sparse_voxel_features(int b, int c, int n, int r, int n_max, const float *features, long long bs_f,
                              int ld_f, const int *cnt, const void *plan_workspace, const int *occ_list,
                              const int *n_occ, float *xc, void *stream);
int bdm_sparse_conv_pack_weights(int cout, int cin, const float *w, float *wt, void *stream);
int bdm_sparse_conv_gemm(int b, int n_max, int cin, int n27, const float *xc, const float *wt,
                         const int *n_occ, float *y, void *stream);
int bdm_sparse_conv_gather(int b, int cout, int r, int n_max, const float *y, const int *occ_index,
                           const unsigned char *rowocc, const float *bias, float *out, void *stream);
/* the same gather + the GroupNorm(groups) statistics of its output as r*r slice partials per (shape, group):
 * gn_partial (b, groups, r*r, 2 doubles); consumed by bdm_group_norm_to_h2_stats */
int bdm_sparse_conv_gather_gn(int b, int cout, int r, int n_max, const float *y, const int *occ_index,
                              const unsigned char *rowocc, const float *bias, float *out, int groups, void *gn_partial,
                              void *stream);

/* --- fp32 feature records of the occupied cells (sparse_conv_h2.hip), and the same first convolution in ONE kernel, no
 *     (n_occ x 27*cout) intermediate (experimental: correct and deterministic but slower than GEMM + gather) ---
 *   bdm_sparse_voxel_features_f32  occupied cells' mean features as fp32 records xr (b, ceil(c/8), n_max) x 8 channels,
 *                                  rows >= n_occ zero; amax[i] (b slots, ZERO on entry) receives max |value| of shape i
 *   bdm_sparse_conv_fused_pack_weights  (cout, cin, 3,3,3) fp32 -> [ceil(cin/8)][27][2][cout] records of 8 fp16
 *                                  (hi / lo of w * 2^e[co]); inv_scale[co] = 2^-e[co]; scale_ws (cout floats) scratch
 *   bdm_sparse_conv_fused          out (b, cout, r^3) = bias + conv: workgroup = (shape, slab of output x-planes, 32 output
 *                                  channels) with the slab's accumulators in LDS; occupied cells (sorted by voxel index:
 *                                  occ_list of bdm_voxelize_plan_full) are multiplied on the matrix cores (fp16x3, activation
 *                                  scale derived on the device from amax) and scattered tap by tap, phases separated by
 *                                  barriers: deterministic.  r in {8, 16, 32}. */
int bdm_sparse_voxel_features_f32(int b, int c, int n, int r, int n_max, const float *features, long long bs_f,
                                  int ld_f, const int *cnt, const void *plan_workspace, const int *occ_list,
                                  const int *n_occ, void *xr, float *amax, void *stream);
#ifdef BDM_EXPERIMENTAL  /* one-kernel form (csrc/experimental/sparse_conv_fused.hip): `make EXPERIMENTAL=1` */
size_t bdm_sparse_conv_fused_weight_elems(int cout, int cin);
int bdm_sparse_conv_fused_pack_weights(int cout, int cin, const float *w, void *packed, float *scale_ws,
                                       float *inv_scale, void *stream);
int bdm_sparse_conv_fused(int b, int cin, int cout, int r, int n_max, const void *xr, const float *amax,
                          const void *packed_w, const float *inv_scale, const int *occ_list, const int *n_occ,
                          const float *bias, float *out, void *stream);
#endif /* BDM_EXPERIMENTAL */

/* fp16x3 form of bdm_sparse_conv_gemm_s3 (the default GEMM of the first convolution): half the matrix work.  xr / amax from
 * bdm_sparse_voxel_features_f32, split once into (hi, lo) fp16 records xh (b, ceil(cin/8), 2, n_max) by bdm_sparse_split_h2;
 * weights [ceil(cin/8)][2][27*cout] fp16 records with per-output-channel scale
 * (bdm_sparse_conv_pack_weights_h2; inv_scale (cout floats)); y (b, n_max, 27*cout) fp32 as the other GEMM forms. */
size_t bdm_sparse_conv_h2_weight_elems(int cout, int cin);
int bdm_sparse_conv_pack_weights_h2(int cout, int cin, const float *w, void *packed, float *scale_ws,
                                    float *inv_scale, void *stream);
int bdm_sparse_split_h2(int b, int cin, int n_max, const void *xr, const float *amax, void *xh, void *stream);
int bdm_sparse_conv_gemm_h2(int b, int n_max, int cin, int cout, const void *xh, const float *amax, const void *packed_w,
                            const float *inv_scale, const int *n_occ, float *y, void *stream);
/* + the per-shape column addend of bdm_sparse_conv_gemm_s3_cb (col_bias (b, 27 * cout)) */
int bdm_sparse_conv_gemm_h2_cb(int b, int n_max, int cin, int cout, const void *xh, const float *amax, const void *packed_w,
                               const float *inv_scale, const int *n_occ, const float *col_bias, long long bs_cb, float *y, void *stream);

/* The same first convolution as ONE output-stationary implicit GEMM with tap skipping (sparse_conv_os.hip, round 4; the default
 * wherever the input is not the hoisted conditioning map): no (n_occ x 27*cout) intermediate, no gather, no operand-split pass.  Only
 * the voxels that can differ from the bias -- the once-dilated occupied set, listed in voxel order -- are computed, in tiles of
 * consecutive list entries whose occupied neighbours are ONE contiguous range of compact rows (staged in LDS per 8-channel chunk).
 *   bdm_voxel_dilate        cnt (b, r^3) -> dil_list (b, n_dil_max) voxel ids of the dilated set in ascending order (n_dil_max = r^3
 *                           always suffices), dil_index (b, r^3) rank in that list or -1, plane_start (b, r + 2): occupied cells in
 *                           x-planes < x, tile_start (b, bdm_voxel_dilate_slices(r, tile), 16): per tile [first entry, end entry, first voxel of
 *                           the linear range it owns, its end, first compact row of its input range, rows, 0, live tiles of the
 *                           shape].  Depends on (coords, r) only: part of the voxel plan of a level.  r in {8, 16, 32}.
 *   bdm_sparse_conv_dil     xr / amax: bdm_sparse_voxel_features_f32 (fp32 records (b, ceil(cin/8), n_max) x 8 channels + per-shape
 *                           max |value|); occ_index (b, r^3) compact row of every cell or -1; packed_w / inv_scale:
 *                           bdm_conv3d_h2_pack_weights (the dense fp16x3 convolution's weight image).  fp16x3 arithmetic, activation
 *                           scale per shape.  compact = 1: y (b, n_dil_max, cout), one row per list entry (every other voxel of the
 *                           grid equals bias: bdm_group_norm_to_h2_stats_compact consumes this form); compact = 0: y (b, cout, r^3),
 *                           every cell written.
 *                           work_counter: one int, ZERO on entry (left non-zero): the persistent workgroups (one per CU) pull their
 *                           (tile, channel block, shape) items from it.
 *   bdm_sparse_conv_dil_gn  also leaves GroupNorm(groups) partials of the DENSE output (bias voxels included) in gn_partial
 *                           (b, groups, tiles, 2 doubles), *slices_out = tiles = bdm_voxel_dilate_slices(r, tile).
 * `tile` (round 6) selects the tile form of a plan and of the convolutions that run on it (the two must agree):
 *   0            FULL tiles (<= 512 / 256 / 128 entries at r = 32 / 16 / 8, one row range of <= 3 r^2 rows, one workgroup per CU);
 *   64/128/256   HALF tiles (EXPERIMENTAL=1 builds only: measured not faster, profiles/r06_sparse_dil_half_tiles.txt; the default library
 *                refuses them): that many entries, four waves and 80 KB of LDS per workgroup, TWO workgroups per CU; a tile
 *                inside one x-plane lists three row ranges ((x-1, x, x+1) x y-rows y0-1 .. y1+1), a tile across planes one range of
 *                whole planes; never more than 1376 rows (<= 3 tile + 12 r inside a plane; across planes only when they fit).
 * A tile record is 16 ints: [first entry, end entry, first voxel of the owned linear range, its end, range 0 first row, range 0 rows,
 * (first x-plane << 8) | last, live tiles of the shape, range 1 first row, rows, range 2 first row, rows, tile, 0, 0, 0]. */
int bdm_voxel_dilate_slices(int r, int tile);
int bdm_voxel_dilate(int b, int r, int n_dil_max, const int *cnt, int *dil_list, int *dil_index, int *plane_start, int *tile_start,
                     int tile, void *stream);
int bdm_sparse_conv_dil(int b, int cin, int cout, int r, int n_max, int n_dil_max, const void *xr, const float *amax,
                        const int *occ_index, const int *dil_list, const int *dil_index, const int *tile_start,
                        const void *packed_w, const float *inv_scale, const float *bias, float *y, int compact, int tile,
                        int *work_counter, void *stream);
/* Host only: the kernel instance sconv_dil_kernel<mt, nt, nw, r, h2in> and the launch geometry that bdm_sparse_conv_dil / _dil_gn
 * (h2in = 0) and bdm_sparse_conv_dil_h2_gn (h2in = 1, always compact) use for this shape on full tiles (tile = 0) -- what the launch
 * path itself decides, not a restatement: a workgroup of nw waves owns bm = 16 mt output channels (ncb channel blocks) x a tile of
 * <= tile = 16 nt nw list entries whose input range holds <= xcap compact rows; tiles_max records per shape
 * (= bdm_voxel_dilate_slices(r, 0)); lds_bytes of dynamic LDS.  Returns 0, or BDM_ERR_UNSUPPORTED (3) for a resolution other than
 * 8, 16, 32 or cout < 1 (the outputs are then 0).  The out pointers are HOST pointers and may be NULL; no GPU call.  Depends on
 * (cout, r, compact) only. */
int bdm_sparse_conv_dil_variant(int b, int cin, int cout, int r, int h2in, int compact, int *mt, int *nt, int *nw, int *bm, int *ncb,
                                int *tile, int *xcap, int *tiles_max, int *lds_bytes);
int bdm_sparse_conv_dil_gn(int b, int cin, int cout, int r, int n_max, int n_dil_max, const void *xr, const float *amax,
                           const int *occ_index, const int *dil_list, const int *dil_index, const int *tile_start,
                           const void *packed_w, const float *inv_scale, const float *bias, float *y, int compact, int groups,
                           void *gn_partial, int *slices_out, int tile, int *work_counter, void *stream);

/* --- the whole voxel branch of a PVConv without dense grids (pvconv_compact.hip, sparse_conv_os.hip; pvconv.py:74-97) ---
 * After GroupNorm + Swish the first convolution's output is a per-channel CONSTANT outside the once-dilated set D1, so the second
 * convolution differs from one of 27 per-class constants (class = 9 cx + 3 cy + cz, c = 0 / 1 / 2: first plane / interior / last
 * plane of the axis -- the zero padding removes taps there) only on the twice-dilated set D2, and the devoxelisation only reads D1.
 *   bdm_voxel_dilate_again        D2 from D1's ranks (dil_index of bdm_voxel_dilate): list, ranks, tiles (input ranges = rows of D1),
 *                                 class_count (b, 27): voxels outside D2 per class
 *   bdm_group_norm_to_h2_rows     GroupNorm + Swish + fp16 split of the FIRST convolution's output on the rows of D1: x = compact rows
 *                                 (b, n_rows_max, c) [dense_in = 0] or the grid (b, c, v) read at dil_list [dense_in = 1]; statistics
 *                                 from `partial` (b, groups, slices, 2).  -> rows_h2 (b, ceil(c/8), 2, n_rows_max) records of 8 fp16,
 *                                 const_h2 (b, ceil(c/8), 2) records and const_f32 (b, c): the value outside D1 (from bias)
 *   bdm_sparse_conv_dil_h2_gn     the SECOND convolution on D2's tiles from those rows: y (b, n_dil_max, cout) compact rows; GroupNorm
 *                                 partials (b, groups, slices, 2), *slices_out = bdm_voxel_dilate_slices(r, tile) + 27 (the tiles'; the last 27
 *                                 are left for bdm_conv3d_class_constants); work_counter as bdm_sparse_conv_dil
 *   bdm_conv3d_class_weight_sums  (cout, cin, 3,3,3) -> wsum (27, cin, cout) doubles: per class, the sum of the taps inside the grid
 *   bdm_conv3d_class_constants    class_vals (b, 27, cout) = bias + wsum[k] . const_f32[b] (fp64, rounded once) and slices
 *                                 slice0 .. slice0 + 26 of gn_partial: class_count x (sum, sum of squares) per group
 *   bdm_se_gate_gn_rows(_pf)      bdm_se_gate_gn(_pf) from the rows of D2 + counts x class constants: coef (b, c, 2), mean_ws (b, c),
 *                                 gate (b, c) (w1 = NULL: no FC layers); part_ws: bdm_se_gate_gn_rows_workspace_elems(b, c) floats
 *   bdm_devoxelize_gn_gate_add_rows(_pf)  bdm_devoxelize_gn_gate_add(_pf) reading the 8 corner rows through D2's ranks */
int bdm_voxel_dilate_again(int b, int r, int n_dil_max, const int *dil_index_in, int *dil_list, int *dil_index, int *plane_start,
                           int *tile_start, int *class_count, int tile, void *stream);
int bdm_group_norm_to_h2_rows(int b, int c, int v, int groups, const float *x, int dense_in, int n_rows_max, const int *dil_list,
                              const int *tile_start, int tiles_max, const float *bias, const float *gamma, const float *beta,
                              float eps, int act, float act_scale, void *rows_h2, void *const_h2, float *const_f32,
                              const void *partial, int slices, unsigned int *saturated, void *stream);
int bdm_sparse_conv_dil_h2_gn(int b, int cin, int cout, int r, int n_rows_max, int n_dil_max, const void *rows_h2, const void *xconst,
                              float x_inv_scale, const int *in_index, const int *dil_list, const int *dil_index,
                              const int *tile_start, const void *packed_w, const float *inv_scale, const float *bias, float *y,
                              int groups, void *gn_partial, int *slices_out, int tile, int *work_counter, void *stream);
size_t bdm_conv3d_class_weight_elems(int cout, int cin);
int bdm_conv3d_class_weight_sums(int cout, int cin, const float *w, void *wsum, void *stream);
int bdm_conv3d_class_constants(int b, int cin, int cout, const void *wsum, const float *bias, const float *const_f32,
                               const int *class_count, float *class_vals, int groups, void *gn_partial, int slices, int slice0,
                               void *stream);
size_t bdm_se_gate_gn_rows_workspace_elems(int b, int c);
int bdm_se_gate_gn_rows(int b, int c, int hidden, int v, int groups, const float *rows, int n_rows_max, const int *tile_start,
                        int tiles_max, const float *class_vals, const int *class_count, const void *gn_partial, int slices,
                        const float *gamma, const float *beta, float eps, const float *w1, const float *w2, float *part_ws,
                        float *mean_ws, float *coef, float *gate, void *stream);
int bdm_se_gate_gn_rows_pf(int b, int c, int hidden, int v, int groups, const float *rows, int n_rows_max, const int *tile_start,
                           int tiles_max, const float *class_vals, const int *class_count, const void *gn_partial, int slices,
                           const float *gamma, const float *beta, float eps, const float *w1, const float *w2, float *part_ws,
                           float *mean_ws, float *coef, float *gate, const void *pf_partial, int pf_slices, int pf_groups, int pf_n,
                           const float *pf_gamma, const float *pf_beta, float pf_eps, float *pf_coef, void *stream);
int bdm_devoxelize_gn_gate_add_rows(int b, int c, int n, int r, const float *coords, const float *rows, int n_rows_max,
                                    const int *dil_index, const float *class_vals, const float *coef, const float *gate,
                                    const float *add, long long bs_a, int ld_a, float *out, long long bs_o, int ld_o, void *stream);
int bdm_devoxelize_gn_gate_add_rows_pf(int b, int c, int n, int r, const float *coords, const float *rows, int n_rows_max,
                                       const int *dil_index, const float *class_vals, const float *coef, const float *gate,
                                       const float *add, long long bs_a, int ld_a, const float *add_coef, float *out, long long bs_o,
                                       int ld_o, void *stream);

/* ------------------------------------------------------------------------------------
 * 3. Per-step glue of the coupled DDPM loop
 * ---------------------------------------------------------------------------------- */

/* PC^2 scheduler step: diffusers 0.21.0 DDPMScheduler.step (epsilon prediction, fixed_small
 * variance, clip_sample=False), call sites experiments/model/model.py:193,286,563.
 *   x0   = (x - sqrt_beta_prod * eps) / sqrt_alpha_prod
 *   out  = coef_x0 * x0 + coef_x * x  [+ sigma * noise   when noise != NULL, i.e. t > 0]
 * The five scalars are the scheduler's per-timestep float32 coefficients (host side).  `out` may be `x` (elementwise: the reverse
 * loops step in place); the same holds for bdm_ddpm_step_philox / bdm_pvd_step_philox. */
int bdm_ddpm_step(long long n, const float *x, const float *eps, const float *noise,
                  float sqrt_beta_prod, float sqrt_alpha_prod, float coef_x0, float coef_x,
                  float sigma, float *out, void *stream);
/* The same step with {sqrt_beta_prod, sqrt_alpha_prod, coef_x0, coef_x, sigma} read from device memory (coef[5]), so
 * that ONE captured hipGraph of a reverse step can be replayed for every timestep; sigma == 0 (t == 0) adds no noise.
 * out may alias x. */
int bdm_ddpm_step_dev(long long n, const float *x, const float *eps, const float *noise, const float *coef,
                      float *out, void *stream);

/* DDIM step (diffusers 0.21.0 DDIMScheduler.step; the reference's schedulers_map['ddim'], model/model.py:60):
 *   x0 = (x - sqrt_beta_prod * eps) / sqrt_alpha_prod;  out = coef_x0 * x0 + coef_eps * eps [+ sigma * noise when eta > 0] */
int bdm_ddim_step(long long n, const float *x, const float *eps, const float *noise, float sqrt_beta_prod,
                  float sqrt_alpha_prod, float coef_x0, float coef_eps, float sigma, float *out, void *stream);

/* out = (c0*x0 [+ c1*x1 [+ c2*x2 [+ c3*x3]]]) / div over n floats, k <= 4 terms, evaluated left to right: the linear
 * multistep combinations and the transfer step of the PNDM scheduler (diffusers 0.21.0 PNDMScheduler, the reference's
 * schedulers_map['pndm'], model/model.py:61).  out may alias any input. */
int bdm_lincomb(long long n, int k, float c0, const float *x0, float c1, const float *x1, float c2,
                const float *x2, float c3, const float *x3, float div, float *out, void *stream);

/* PVD scheduler step: GaussianDiffusion.p_sample (experiments/pvd/__init__.py:136-224):
 *   x0 = sqrt_recip_abar * x - sqrt_recipm1_abar * eps;  mean = coef1 * x0 + coef2 * x;
 *   out = mean + sigma * noise      (sigma = 0 at t == 0; noise is always drawn, as the reference does).  `out` may be `x` (elementwise). */
int bdm_pvd_step(long long n, const float *x, const float *eps, const float *noise,
                 float sqrt_recip_abar, float sqrt_recipm1_abar, float coef1, float coef2,
                 float sigma, float *out, void *stream);

/* Per-shape counter-based random streams (rng_ops.hip).  The reference draws the initial cloud, the DDPM / PVD noise and
 * the blend masks from ONE per-process generator seeded seed + rank (training_utils.py:373-378; draw sites
 * main_blending.py:228,330-338, model/model.py:286, pvd/__init__.py:213,232), so a shape's sample depends on its rank and
 * batch slot.  Here element e of draw `draw` of purpose `purpose` of the shape with key keys[s] is
 *   Philox4x32-10(key = keys[s], counter = (e / 4, 0, draw, purpose))[e % 4]
 * (keys[s] is derived on the host from (run seed, GLOBAL shape index)): rank-count- and batch-invariant, one launch per
 * batch.  Normals: Box-Muller on 24-bit uniforms.  out (b, per_shape) float / int64 (bit 0 of each word: Bernoulli 1/2,
 * the `torch.randint(0, 2, ...)` of main_blending.py:330-338). */
int bdm_philox_normal(int b, long long per_shape, const unsigned long long *keys, unsigned int draw,
                      unsigned int purpose, float *out, void *stream);
int bdm_philox_bits(int b, long long per_shape, const unsigned long long *keys, unsigned int draw,
                    unsigned int purpose, long long *out, void *stream);
/* bdm_ddpm_step / bdm_pvd_step with the noise of bdm_philox_normal(b, per_shape, keys, draw, purpose) generated inside the
 * kernel (never written to memory); same bits as the two-launch form.  DDPM: sigma == 0 (t == 0) uses no draw. */
int bdm_ddpm_step_philox(int b, long long per_shape, const float *x, const float *eps,
                         const unsigned long long *keys, unsigned int draw, unsigned int purpose,
                         float sqrt_beta_prod, float sqrt_alpha_prod, float coef_x0, float coef_x, float sigma,
                         float *out, void *stream);
int bdm_pvd_step_philox(int b, long long per_shape, const float *x, const float *eps,
                        const unsigned long long *keys, unsigned int draw, unsigned int purpose,
                        float sqrt_recip_abar, float sqrt_recipm1_abar, float coef1, float coef2, float sigma,
                        float *out, void *stream);

/* x (b, n, 3) point-major: subtract the per-shape mean over points, in place
 * (main_blending.py:229; model/model.py:530-531). */
int bdm_center_points(int b, int n, float *x, void *stream);

/* BDM-Blending per-point select (main_blending.py:326-344):
 * out[p] = mask[p] ? prior[p] : recon[p] for num_points = B*N points of 3 floats; mask int64. */
int bdm_blend_select(long long num_points, const float *recon, const float *prior,
                     const long long *mask, float *out, void *stream);

/* Projection conditioning, per-step part (model/projection_model.py:127-157; pytorch3d
 * PerspectiveCameras + naive PointsRasterizer, radius in NDC, one point per pixel).
 * points (b,n,3) point-major world coordinates; cameras (b,16) = R row-major (9), T (3),
 * focal (2), principal point (2).  pix_of_point (b,n): flat index h*W+w of the LAST pixel
 * (row-major) owned by the point, or -1. */
size_t bdm_rasterize_workspace_bytes(int b, int h, int w);
int bdm_rasterize_points(int b, int n, int h, int w, float radius, const float *points,
                         const float *cameras, int *pix_of_point, void *workspace, void *stream);
/* Point-cloud rendering (render.hip; experiments/diffusion_utils.py:185-295 renders with pytorch3d's PointsRasterizer and its
 * NormWeighted / Alpha compositors, restated here: pytorch3d is absent, parity unpinned).  Projection and pixel centres as
 * bdm_rasterize_points (ortho = 1 drops the division by the view depth: ndc = focal * X_view.xy + pp); for h != w each axis spans
 * [-1, 1] (this project's convention, not pytorch3d's aspect-scaled one).  A point is a candidate of a pixel when
 * dx*dx + dy*dy < radius*radius and z >= 0; the pixel keeps the k candidates with the smallest (z, point index), ascending.
 *   frag_idx / frag_z / frag_d2 (b,h,w,k): point index WITHIN its cloud (0 .. n-1; pytorch3d stores the index into the packed
 *     batch), view depth, squared NDC distance; -1 in unused slots.  Any of the three may be NULL (not stored).
 *   image (b,h,w,c), may be NULL: with w_j = 1 - d2_j / radius^2 over the used slots in slot order,
 *     compositor 0 (norm_weighted) sum_j w_j f_j / max(sum_j w_j, 1e-4);  compositor 1 (alpha) sum_j f_j w_j prod_{i<j} (1 - w_i);
 *     a pixel whose slot 0 is empty takes background (c) unchanged.  features (b,n,c) or NULL = zeros.
 * Limits: 1 <= k <= 16, 1 <= c <= 4, radius * max(h,w) / 2 <= 8 (pixel pitches).  Deterministic: no atomics, the result does not
 * depend on execution order.  workspace: bdm_render_workspace_bytes(b, n, h, w, radius) bytes. */
size_t bdm_render_workspace_bytes(int b, int n, int h, int w, float radius);
int bdm_render_points(int b, int n, int h, int w, int k, int c, float radius, int ortho, int compositor,
                      const float *points, const float *cameras, const float *features, const float *background,
                      int *frag_idx, float *frag_z, float *frag_d2, float *image, void *workspace, void *stream);
/* get_input_with_conditioning's output (projection_model.py:179-231):
 * out (b, n, 3+c) = cat[x_t, feature_image[pix_of_point]] with zeros for points owning no pixel;
 * feature_image is stored pixel-major (b, h*w, c). */
int bdm_condition_gather(int b, int n, int c, int hw, const float *x_t, const float *feature_image,
                         const int *pix_of_point, float *out, void *stream);
/* the same, written channel-first: out (b, 3 + c, n) -- the layout the denoiser consumes (no transpose pass) */
int bdm_condition_gather_cf(int b, int n, int c, int hw, const float *x_t, const float *feature_image,
                            const int *pix_of_point, float *out, void *stream);
/* rows 0..2 (the coordinates) of that tensor only; rows 3.. stay UNWRITTEN until bdm_condition_gather_cf completes the same tensor.  For
 * the reverse loop when every consumer of the feature rows reads a hoisted per-pixel map instead (100 MB per step at b = 16). */
int bdm_condition_xyz_cf(int b, int n, int c, const float *x_t, float *out, void *stream);

/* Quality metrics of the evaluation scripts (evaluation/evaluation_cd.py:111-131, evaluation_f1.py:90-110):
 * out (b, n) = min over the m target points of the squared distance; src (b,n,3), tgt (b,m,3) point-major. */
int bdm_nn_sqdist(int b, int n, int m, const float *src, const float *tgt, float *out, void *stream);

/* ------------------------------------------------------------------------------------
 * 4. Image encoder of the projection conditioning (ViT-S/16), once per image batch
 *    (experiments/model/feature_model.py:85-132; timm VisionTransformer; hoisted out of the per-step loop)
 *    Tokens are channel-first (b, d, t): Linear layers = bdm_pointwise_conv (bias / GELU / residual fused),
 *    attention = bdm_attention_core per head.
 * ---------------------------------------------------------------------------------- */
/* (b,3,h,w) in [0,1] -> ImageNet-normalised patches (b, 3*p*p, t), row k = c*p*p + py*p + px; mean3/std3 are HOST arrays */
int bdm_vit_patchify(int b, int h, int w, int patch, const float *host_mean3, const float *host_std3, const float *img,
                     float *out, void *stream);
/* out (b, d, t+1): column 0 = cls + pos[0], column 1+i = patches[:, :, i] + pos[1+i]; pos token-major (t+1, d) */
int bdm_vit_assemble_tokens(int b, int d, int t, const float *patches, const float *cls, const float *pos,
                            float *out, void *stream);
/* nn.LayerNorm(d) over the channel axis of (b, d, t) */
int bdm_layer_norm_channels(int b, int d, int t, const float *x, const float *gamma, const float *beta, float eps,
                            float *y, void *stream);
/* conditioning image (b, h*w, 3+d) pixel-major = cat[(img - colors_mean)/colors_std, bilinear(tokens[:, :, 1:] as grid x grid)]
 * with align_corners=False (projection_model.py:110-125 + feature_model.py:107-119) */
int bdm_vit_conditioning_image(int b, int d, int grid, int h, int w, float colors_mean, float colors_std,
                               const float *tokens, const float *img, float *out, void *stream);


/* ------------------------------------------------------------------------------------
 * 5. Step executor: one recorded reverse step replayed by ONE call
 *    Replaces the per-step Python of the reference's reverse loop (experiments/model/model.py:275-287: conditioning ->
 *    denoiser -> scheduler.step, ~230 dependent launches) once its arguments are static: the host framework records the
 *    step's C-ABI calls (function name + arguments, 8 bytes per argument: integers and pointers as they are, float / double
 *    arguments as the bit pattern of a double), its memsets / device copies and its stream / event edges, and replays the
 *    list from C.  No allocation, no synchronisation, nothing Python per launch.  The tape does NOT own the buffers whose
 *    addresses it holds: the recorder keeps them alive (bdm_amd/tape.py).
 * ---------------------------------------------------------------------------------- */
void *bdm_tape_create(void);
void bdm_tape_destroy(void *tape);
int bdm_tape_length(const void *tape);
/* append `function` (an `int bdm_*(...)` entry point of this header, by name) with n_args 8-byte argument slots */
int bdm_tape_append_call(void *tape, const char *function, const unsigned long long *args, int n_args);
int bdm_tape_append_memset(void *tape, void *dst, int byte_value, size_t bytes, void *stream);
int bdm_tape_append_memcpy(void *tape, void *dst, const void *src, size_t bytes, void *stream);
/* `waiter` waits for everything enqueued on `other` up to this point of the replay (torch's Stream.wait_stream) */
int bdm_tape_append_wait_stream(void *tape, void *waiter, void *other);
int bdm_tape_append_event_record(void *tape, void *event, void *stream);
int bdm_tape_append_event_wait(void *tape, void *stream, void *event);
/* replay entries [first, first + count) (count < 0: to the end); returns 0 or the status of the first failing entry, whose
 * index bdm_tape_failed_entry reports (-1: none) */
int bdm_tape_replay(void *tape, int first, int count);
int bdm_tape_failed_entry(const void *tape);
/* test hook of the argument marshalling (no GPU work): writes its arguments, converted to double, to out16 (host memory) */
int bdm_tape_echo(int a, long long b, float c, const void *d, unsigned int e, float f, int g, void *out16);

/* ------------------------------------------------------------------------------------
 * 6. Simple point denoiser (experiments/model/simple/simple_model.py:9-34, simple_model_utils.py:158-279;
 *    also the first half of pvcnn/pvcnn_plus_plus.py:9-42), csrc/simple_point.hip
 *    The state x is channel-first (b, 128, n).  Every kernel that writes x leaves the per-shape pooling partials of
 *    what it wrote (max, sum, sum of squares per 128-point slice and channel) in `partials`
 *    (bdm_simple_partials_bytes(b, n) bytes); bdm_simple_layer_prep turns them into the layer's per-shape state
 *    (bdm_simple_state_elems(b) floats: max[128], std[128] (unbiased), their sum, their squared deviation from their
 *    mean, and the 1024-wide pooled share of [W1; V]).  Fixed reduction orders: a shape's results do not depend on b.
 * ---------------------------------------------------------------------------------- */
size_t bdm_simple_partials_bytes(int b, int n);
size_t bdm_simple_state_elems(int b);
/* prepare_inputs + input_projection (simple_model_utils.py:250-273): y = W [x ; posenc(x[:, 0:3])] + batch_bias[b],
 * x (b, c_in, n), freq (10) the PositionalEncoding buffer, w_packed (ceil(K/2), 4, 64) with K = c_in + 63: element
 * [s][o][l] = W[32 o + (l & 31)][2 s + (l >> 5)] (zero beyond K); batch_bias (b, 128) = bias + W_t t_emb. */
int bdm_simple_input_proj(int b, int n, int c_in, const float *x, const float *freq, const float *w_packed,
                          const float *batch_bias, float *y, void *partials, void *stream);
/* per-shape prologue of one layer from the partials of its input; w_ms (1024, 256) = [W1; V][:, 128:384] * gamma[128:384] */
int bdm_simple_layer_prep(int b, int n, const void *partials, const float *w_ms, float *state, void *stream);
/* y = x + W2 (silu(W1 LN(x_in)) * V LN(x_in)), x_in = [x, max, std] (simple_model.py:27-30); y must not alias x.
 * w1_packed / wv_packed (16, 64, 64): [k][s][l] = W[32 k + (l & 31)][s + 64 (l >> 5)] * gamma[s + 64 (l >> 5)];
 * w2_packed (16, 4, 16, 64): [k][o][r][l] = W2[32 o + (l & 31)][32 k + (r & 3) + 8 (r >> 2) + 4 (l >> 5)];
 * vec (4, 512) = [d1, e1, dv, ev]: d = W[:, 128:384] gamma[128:384], e = W beta. */
int bdm_simple_layer(int b, int n, const float *x, const float *state, const float *w1_packed, const float *wv_packed,
                     const float *w2_packed, const float *vec, float *y, void *partials, void *stream);
/* out = a + b elementwise over n floats (PVCNN++'s residual x + PVCNN(x), pvcnn_plus_plus.py:40); out may alias a or b */
int bdm_simple_add(long long n, const float *a, const float *b, float *out, void *stream);

/* ------------------------------------------------------------------------------------
 * 7. Generation metrics: all-pairs cloud-to-cloud distance matrices (csrc/metrics.hip; bdm_amd/metrics.py reduces them to
 *    MMD, COV and 1-NNA).  Clouds are point-major: a (s, n, 3), b (r, m, 3).  No workspace (but for bdm_pairwise_emd_large,
 *    csrc/metrics_emd_large.hip); no atomics: entry (i, j) is reduced in a fixed order that depends on the point counts alone,
 *    so it carries the bits of the 1 x 1 call on clouds i and j.  s = 0 or r = 0 is a no-op.
 * ---------------------------------------------------------------------------------- */
/* out_ab[i, j] = mean over the points p of a_i of min over the points q of b_j of |p - q|^2, out_ba[i, j] the same with the
 * roles swapped; both (s, r), either may be NULL.  Distances in the difference form dx^2 + dy^2 + dz^2. */
int bdm_pairwise_chamfer(int s, int r, int n, int m, const float *a, const float *b, float *out_ab, float *out_ba,
                         void *stream);
/* Host only: the instance pairwise_chamfer_kernel<p> with tj target clouds per workgroup that ONE direction of bdm_pairwise_chamfer
 * launches for s source clouds of n points against r target clouds -- what the launch path itself decides (the b -> a direction is
 * the query (r, s, m)).  p, tj are HOST pointers and may be NULL; no GPU call.  Returns 0, or 1 for sizes below 1 (outputs 0). */
int bdm_pairwise_chamfer_variant(int s, int r, int n, int *p, int *tj);
/* Approximate-match earth mover's distance (Fan et al., approxmatch + matchcost: ten levels exp(-4^j d^2), j = 7 .. -1, then 0;
 * DESIGN.md section 10) between equal-sized clouds: out[i, j] = cost(a_i, b_j) / n, (s, r).  Not symmetric in (a, b).
 * n above 2048 returns 3 (unsupported): bdm_pairwise_emd_large below takes any size. */
int bdm_pairwise_emd_approx(int s, int r, int n, const float *a, const float *b, float *out, void *stream);
/* The same measure for clouds of any size up to 65536 points (csrc/metrics_emd_large.hip), all pairs or paired; beside
 * bdm_pairwise_emd_approx, whose bits it need not reproduce (the final sum over the points is ordered differently).  One
 * workgroup per pair in a persistent grid of at most 256 workgroups, each with a slab of the caller's workspace for the per-point
 * state (20 bytes per point padded to a multiple of 4): the workspace does not grow with the number of pairs beyond 256.
 * Two forms of one algorithm with the same bits: RESIDENT (both clouds in LDS; n <= 4096) and STREAMED (the other cloud passes
 * through LDS in stages of 1024 points; any n).  Entry (i, j) carries the bits of the 1 x 1 call in either form, paired or not.
 * The upper limit of n is a budget, not a capacity: a pair is never split over workgroups, so its time grows with n^2 on one CU. */
/* bytes of workspace a call on `pairs` pairs (s * r, or s when paired) of n-point clouds needs; 0 for pairs < 1, n < 1 or n > 65536 */
size_t bdm_pairwise_emd_large_workspace_bytes(int pairs, int n);
/* Host only: what a call with (n, mode) launches -- resident (1) or streamed (0), threads per workgroup, owned points per thread
 * and row tile, points per LDS stage (0 for the resident form).  Outputs are HOST pointers and may be NULL; no GPU call.
 * Returns 0; 1 for n < 1 or an unknown mode; 3 for mode 1 above 4096 points and for n above 65536 (outputs 0). */
int bdm_pairwise_emd_large_variant(int n, int mode, int *resident, int *threads, int *kpt, int *stage);
/* paired = 0: out[i, j] = cost(a_i, b_j) / n, (s, r).  paired = 1: s == r, out[i] = cost(a_i, b_i) / n, (s).
 * mode 0: resident while it fits, else streamed; 1: resident (3 if n > 4096); 2: streamed.  workspace: device memory of at least
 * bdm_pairwise_emd_large_workspace_bytes(pairs, n) bytes, 4-byte aligned, contents irrelevant before and after.
 * Returns 1 and launches nothing for bad sizes, a NULL pointer with work to do, s != r when paired, or a workspace too small;
 * 3 for n > 65536.  s = 0 or r = 0 is a no-op. */
int bdm_pairwise_emd_large(int s, int r, int n, int paired, int mode, const float *a, const float *b, void *workspace,
                           size_t workspace_bytes, float *out, void *stream);

/* ------------------------------------------------------------------------------------
 * 8. PC^2 colouring model (experiments/model/model_coloring.py, point_cloud_transformer_model.py:13-80 with
 *    use_attn = False), csrc/color_block.hip.  Tokens are channel-first (b, e, n); e = 64 is the only width the
 *    configuration reaches, any other returns 3 (unsupported) and writes nothing.  A point's results depend on that
 *    point alone: not on b, n or the tile it falls in.
 * ---------------------------------------------------------------------------------- */
/* floats of the packed fc1 / fc2 record of one block (0 for an unsupported e) */
size_t bdm_color_block_packed_elems(int e);
/* fc1_w (4e, e), fc2_w (e, 4e) row-major (timm Mlp) -> packed: first [k][s][l] = fc1_w[32 k + (l & 31)][s + 32 (l >> 5)]
 * (k < 8, s < 32, l < 64), then [k][o][r][l] = fc2_w[32 o + (l & 31)][32 k + (r & 3) + 8 (r >> 2) + 4 (l >> 5)] (o < 2, r < 16). */
int bdm_color_block_pack_weights(int e, const float *fc1_w, const float *fc2_w, float *packed, void *stream);
/* Second half of one PointCloudModelBlock, per point: r = h + p (p: the block's PVCNN output), y = r + fc2(gelu(fc1(LN(r))))
 * with LN = LayerNorm(e) (norm2: biased variance, eps inside the root) and the exact (erf) GELU; y (b, e, n) is always written
 * and must not alias h or p.  At most one of:
 *   ln_next (b, e, n) = LayerNorm(y) with next_w / next_b / next_eps (the next block's norm0);
 *   colors (b, n, 3) point-major = clamp((out_w y + out_b) * colors_std + colors_mean, 0, 1), out_w (3, e) row-major
 * selected by a non-NULL pointer.  fp32 arithmetic, fp32-input MFMA contractions; the 4e-wide hidden vector is never stored. */
int bdm_color_block_tail(int b, int e, int n, const float *h, const float *p, const float *norm2_w,
                         const float *norm2_b, float norm2_eps, const float *w_packed, const float *fc1_b,
                         const float *fc2_b, float *y, const float *next_w, const float *next_b, float next_eps,
                         float *ln_next, const float *out_w, const float *out_b, float colors_mean,
                         float colors_std, float *colors, void *stream);

/* ------------------------------------------------------------------------------------
 * 9. Occupancy-grid histograms of a set of clouds (csrc/occupancy.hip; bdm_amd/metrics.py reduces them to the JSD between two
 *    sets and to the mean occupancy entropy; experiments/pvd/utils/metrics.py:13-31, 142-232).  DESIGN.md section 13.
 * ---------------------------------------------------------------------------------- */
/* clouds (s, n, 3) point-major; axis: the r ascending, evenly spaced coordinates every grid axis shares; cell_mask (r^3 bytes,
 * cell (i, j, k) at (i r + j) r + k with centre (axis[i], axis[j], axis[k])): non-zero = the cell is kept.
 * A point belongs to the kept cell that minimises (x - gx)^2 + (y - gy)^2 + (z - gz)^2 in fp32 (unfused, in that order); a point
 * with a NaN or infinite coordinate belongs to none.  Equal fp32 distances: when the cell the point rounds to is kept, each axis
 * index is the lowest among that axis's equal squared differences (two cells whose sums round to the same value although one axis
 * differs are not told apart by flat index); otherwise the lowest flat index among the kept cells.
 * hits[c] = points of all clouds that belong to cell c; active[c] = clouds with at least one such point; both r^3 ints, zeroed
 * by the call (cells with cell_mask 0 stay 0), either may be NULL.  Integer sums: the same bits for any order, and the sum over any
 * split of the clouds into several calls equals the one call.  s = 0 only zeroes.  Returns 1 without launching for s < 0, n < 1,
 * r < 2, r > 32 (the r^3 histogram and a 32-bit mask word per column live in one workgroup's LDS) or s n >= 2^31. */
int bdm_occupancy_grid(int s, int n, int r, const float *clouds, const float *axis, const unsigned char *cell_mask,
                       int *hits, int *active, void *stream);

/* ------------------------------------------------------------------------------------
 * 10. Point-cloud normals (csrc/normals.hip): K nearest neighbours of every point within its own cloud, the covariance of the
 *     neighbourhood and its eigen-decomposition, restating pytorch3d's estimate_pointcloud_normals (ops/points_normals.py) from
 *     its published behaviour (pytorch3d is not installed: parity unpinned, as for the renderer).  DESIGN.md section 14.
 * ---------------------------------------------------------------------------------- */
/* points (b, n, 3) point-major.
 * Neighbours: for query point i the candidates are all points j of the same cloud, i itself included.  dx = fl(x_j - x_i),
 *   likewise dy and dz; d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), no FMA contraction.  The neighbourhood is the k candidates
 *   with the smallest (d2, j), in ascending order; knn_idx (b, n, k) holds those j as the index within the cloud.  These indices
 *   are bit-exact quantities, like the library's other neighbour indices.
 * Covariance: e_j = p_j - p_i over the neighbourhood, C = (1/k) sum_j (e_j - ebar)(e_j - ebar)^T with ebar the mean of the e_j;
 *   formed from these differences, never from sum p p^T - k mean^2; the summation order is the kernel's (fixed); all float32.
 * Eigen-decomposition: curvatures (b, n, 3) = the three eigenvalues of C, ascending; normals (b, n, 3) = the unit eigenvector of
 *   the smallest (cyclic Jacobi, a fixed sweep count, on the trace-scaled matrix).
 * Sign: orient = 0: the component of largest magnitude is positive (ties: lowest axis).  orient = 1 (pytorch3d's
 *   _disambiguate_vector_directions): n_pos = the number of neighbours with e_j . normal > 0; the normal is negated when
 *   n_pos < 0.5 k.  orient = 2: negated when normal . (viewpoint_b - p_i) < 0, viewpoints (b, 3).
 * Non-finite input: a point with a non-finite coordinate is nobody's neighbour; its own normal and curvatures are NaN and its
 *   knn_idx row is -1.  A cloud with fewer than k finite points gets these values everywhere.
 * Limits: 3 <= k <= 64, n > k, b >= 0 (b == 0 launches nothing and returns 0), b n k < 2^31, orient in {0, 1, 2}; viewpoints
 *   non-NULL if and only if orient == 2.  Outside these the call returns 1 and launches nothing.  knn_idx and curvatures may be
 *   NULL (the other outputs keep their bits).
 * Determinism: no floating-point atomics; cloud j of a batch has the same bits as the same cloud run alone, and so does a
 *   repeated call.  workspace: bdm_estimate_normals_workspace_bytes(b, n, k) bytes (0 in this implementation: NULL is accepted). */
size_t bdm_estimate_normals_workspace_bytes(int b, int n, int k);
int bdm_estimate_normals(int b, int n, int k, int orient, const float *points, const float *viewpoints, int *knn_idx,
                         float *normals, float *curvatures, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 11. Consistent orientation of point-cloud normals by visibility voting (csrc/orient.hip).  The cloud is looked at from v
 *     directions; a point that survives a splatted z-buffer test in a view votes for the side of its normal that faces that
 *     viewer; points no view decided take the sign their decided neighbours give them.  DESIGN.md section 15.
 * ---------------------------------------------------------------------------------- */
/* points, normals_in, normals_out (b, n, 3) point-major; knn_idx (b, n, k) as bdm_estimate_normals writes it; views (v, 3, 3).
 * All arithmetic is float32, every operation rounded on its own (no FMA contraction), division and sqrt correctly rounded;
 * everything after the projection is integer.  dot(p, p') = fl(fl(fl(x x') + fl(y y')) + fl(z z')).
 * Per cloud: only the points whose three coordinates are finite take part ("finite points").  c = the centre of their bounding
 *   box, fl(0.5 * fl(min + max)) per axis (min and max are exact: no summation order enters).  q_i = fl(p_i - c) per axis.
 *   rho = the largest d2(q_i) = fl(fl(fl(qx*qx) + fl(qy*qy)) + fl(qz*qz)) (section 10's form).  h = fl(1.02f * sqrt(rho)).
 *   A cloud with no finite point, or with rho == 0, has no visible point in any view: votes and seen are zero.
 * Per view: three rows u, w, d; d points from the cloud to the viewer (orthographic).  No trigonometry, no normalisation: the
 *   rows are taken as passed.  a = dot(q, u), b = dot(q, w), t = dot(q, d).
 *   Pixel X = clamp(floor(fl(fl(fl(a / h) + 1) * (r / 2))), 0, r - 1) with r / 2 = fl(0.5 * r) (exact), Y the same from b.
 *   Depth key Z = clamp(floor(fl(fl(1 - fl(t / h)) * 32768)), 0, 65535): smaller is nearer the viewer.  A NaN clamps to 0.
 * Z-buffer: zb[x, y] = the minimum Z_i over the finite points with |x - X_i| <= splat and |y - Y_i| <= splat, inside the image.
 *   Point i is visible in view v if and only if it is finite and Z_i <= zb[X_i, Y_i] + eps.
 * Votes: sigma(i, v) = +1 if dot(n_i, d_v) > 0, -1 if it is < 0, 0 if it is zero or NaN.  votes_i = sum_v visible(i, v) sigma(i, v),
 *   seen_i = sum_v visible(i, v), both int32 (b, n): integer sums, the same bits in any order.  s_i = sgn(votes_i).
 * Fallback: at most `rounds` Jacobi rounds; every round reads the state s as it stood when the round began.  For every i with
 *   s_i == 0: the window of i is the first kg entries j of knn_idx[i] (in row order, all k entries are looked at) that have 0 <= j < n
 *   and j != i; t_i = sum over the window of s_j * sgn(dot(n_i, n_j)) (an undecided j, s_j == 0, adds nothing; sgn of NaN is 0);
 *   s_i <- sgn(t_i).  Points with s_i != 0 keep it.  The rounds stop early when one changes nothing.
 * Output: normals_out_i = the bits of n_i, with the sign bit of all three components flipped when s_i < 0 (so NaN stays NaN).
 *   A point still undecided (s_i == 0: it keeps its input sign) is counted in undecided (b); non-finite points are among them.
 *   Wherever s_i != 0 the output does not depend on the signs of the input normals.
 * votes, seen, undecided may be NULL.  normals_out must not alias normals_in.
 * Limits: b >= 0 (b == 0 launches nothing and returns 0), 1 <= n <= 32768 (the state s of a cloud lives twice in one workgroup's
 *   LDS), 1 <= k, b n k < 2^31, 1 <= v <= 256, b v < 2^31, 1 <= r <= 128 (the r x r z-buffer lives in one workgroup's LDS: 64 KiB at 128),
 *   0 <= splat <= 4, 0 <= eps <= 65535, 1 <= kg <= k, 0 <= rounds <= 32, no NULL among the inputs, normals_out and the
 *   workspace.  Outside these the call returns 1 and launches nothing.
 * Determinism: integer atomics in LDS only (minimum, sum), no floating-point atomics, no workgroup waits on another; cloud j of
 *   a batch has the same bits as the same cloud run alone, and so does a repeated call.
 * workspace: bdm_orient_normals_workspace_bytes(b, n, v) bytes (one byte per cloud, view and point: the vote of that pair),
 *   contents irrelevant before and after; 0 for sizes outside the limits. */
size_t bdm_orient_normals_workspace_bytes(int b, int n, int v);
int bdm_orient_normals(int b, int n, int k, int v, int r, int splat, int eps, int kg, int rounds, const float *points,
                       const float *normals_in, const int *knn_idx, const float *views, float *normals_out, int *votes,
                       int *seen, int *undecided, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 12. Triangle meshes from oriented clouds (csrc/surface.hip): the cloud is accumulated into a signed-distance grid (implicit
 *     moving least squares with a compact polynomial weight, in fixed point) and the grid is meshed by surface nets: one vertex
 *     per sign-change cell, one quad per sign-change edge.  DESIGN.md section 16.
 * ---------------------------------------------------------------------------------- */
/* points, normals (b, n, 3) point-major, the normals taken to point outwards; r grid nodes per axis, node (i, j, k) of a cloud at
 * (i r + j) r + k; s the support in voxels; min_weight.  All float32 arithmetic is rounded operation by operation (no FMA
 * contraction), in the order written, division correctly rounded; fl() is left out below.  Everything after step 3 is integer
 * except the vertex positions.
 * 1. Valid points: a point is valid when its three coordinates and the three components of its normal are all finite; the others
 *    contribute nothing.  counts[3] = the number of valid points.  A cloud with no valid point, or whose valid points have
 *    min == max on every axis, is empty: SW = SU = 0 everywhere, V = F = skipped = 0.
 * 2. Grid coordinates: lo, hi = the per-axis minima and maxima of the valid points (exact).  c = 0.5 * (lo + hi) per axis,
 *    half = the largest 0.5 * (hi - lo) over the axes, inv = float(r - 1 - 2 (s + 1)) / (2 * half),
 *    q = (p - c) * inv + float(r - 1) / 2 per axis (float(r - 1) / 2 is exact).
 *    A valid point with a component of q outside [0, r - 1] (NaN included: an overflow on the way) contributes nothing.
 * 3. Contributions: base = floor(q) per axis.  For every node g = base + o, o in {-s + 1, ..., s}^3, inside the grid (a node with
 *    a coordinate outside 0 .. r - 1 is left out): d = float(g) - q per axis; d2 = (dx*dx + dy*dy) + dz*dz;
 *    t = float(s*s) - d2; no contribution if t <= 0; w = t / float(s*s); w3 = (w*w)*w; a = (nx*dx + ny*dy) + nz*dz; u = w3 * a;
 *    W = rint(w3 * 4096); U = rint(u * 4096) clamped to [-4096 s, 4096 s], rint rounding half to even; U = 0 if u * 4096 is NaN.
 * 4. Grid: SW(g) = sum W and SU(g) = sum U over the contributions, exact int32 sums (n <= 65536 and s <= 4 keep |SU| <= 2^30):
 *    integer sums have the same bits in any order.  thr = max(1, rint(min_weight * 4096)) (the product in float32).
 *    A node is defined iff SW >= thr, negative (inside) iff SU < 0; f(g) = float(SU) / float(SW), the conversions rounding to nearest even.
 * 5. Vertices: cell (i, j, k), 0 <= i, j, k < r - 1, with corners (i + dx, j + dy, k + dz), is active iff its 8 corners are all
 *    defined and 1 to 7 of them are negative.  Its 12 edges are taken in the order: corner a = (dx, dy, dz) in lexicographic
 *    order, then axis 0, 1, 2 with a[axis] == 0; the edge runs from a to b = a + e_axis.  An edge whose ends differ in sign gives
 *    tt = f(a) / (f(a) - f(b)) (the denominator is never 0: one end is < 0, the other >= 0) and the point float(a) with tt as its
 *    component along the axis.  The points are summed per component in that order, starting from the first, and divided by
 *    float(their count); grid = float(cell index) + that mean per axis; world = (grid - float(r - 1) / 2) / inv + c per axis.
 *    Vertex ids: the rank of the cell among the cloud's active cells in ascending (i (r - 1) + j)(r - 1) + k.
 * 6. Faces: for axis = 0, 1, 2 (outer), then for every node g with g[axis] <= r - 2 in ascending (i r + j) r + k, the edge from g
 *    to g + e_axis.  With u = (axis + 1) mod 3, v = (axis + 2) mod 3: the edge is a candidate when g[u] and g[v] lie in 1 .. r - 2,
 *    both ends are defined and the ends differ in sign.  The four cells around it, all with g's coordinate along the axis:
 *    c00 at (g[u] - 1, g[v] - 1), c10 at (g[u], g[v] - 1), c11 at (g[u], g[v]), c01 at (g[u] - 1, g[v]) in (u, v).
 *    A candidate with all four cells active emits the quad (c00, c10, c11, c01) when g is the negative end and
 *    (c01, c11, c10, c00) when g is the non-negative end (triangle normals point to the non-negative side: outward normals give a
 *    positive signed volume); the quad (q0, q1, q2, q3) gives the triangles (q0, q1, q2) then (q0, q2, q3) of vertex ids.
 *    A candidate with a non-active cell around it emits nothing and adds 1 to skipped.
 *    Faces are ordered by axis, then edge, then triangle.
 * bdm_surface_grid runs steps 1 - 4 and marks and counts the cells and edges of steps 5 and 6.  counts (b, 4) int32 =
 *   {V, F, skipped, valid points} per cloud.  The workspace then holds, from its start, SW (b, r, r, r) int32, SU (b, r, r, r) int32
 *   and the cell-to-vertex map (b, r, r, r) int32 (vertex id of the cell whose lowest corner is the node, -1 elsewhere), followed
 *   by what bdm_surface_extract needs; it has to stay untouched between the two calls.
 * bdm_surface_extract, with the same b, n, r, s and workspace: writes cloud c's vertices to verts + 3 vert_offsets[c] (V rows of 3
 *   floats) and its faces to faces + 3 face_offsets[c] (F rows of 3 int32 vertex ids local to the cloud); the offsets are b
 *   non-negative 64-bit integers on the device, counted in rows; nothing else is written.
 * Limits: b >= 0 (b == 0 launches nothing and returns 0), 1 <= n <= 65536, 16 <= r <= 256, 2 <= s <= 4, 0 <= min_weight <= 1 (a NaN is refused), b r^3 < 2^31, no NULL
 *   pointer, no output or the workspace equal to an input.  Outside these a call returns 1 and launches nothing.
 * Determinism: integer atomic sums in global memory only, no floating-point atomics, no workgroup waits on another, every loop
 *   is bounded by a launch argument; cloud j of a batch has the same bits as the same cloud run alone, and so does a repeated call.
 * workspace: bdm_surface_workspace_bytes(b, n, r, s) bytes (0 for sizes outside the limits), contents irrelevant before. */
size_t bdm_surface_workspace_bytes(int b, int n, int r, int s);
int bdm_surface_grid(int b, int n, int r, int s, float min_weight, const float *points, const float *normals, int *counts,
                     void *workspace, void *stream);
int bdm_surface_extract(int b, int n, int r, int s, const long long *vert_offsets, const long long *face_offsets, float *verts,
                        int *faces, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 13. Rendering of triangle meshes (csrc/mesh_render.hip): one face per pixel, all-integer coverage with a half-plane fill rule,
 *     float32 depth and barycentrics rounded operation by operation; restates pytorch3d's MeshRasterizer (faces_per_pixel = 1,
 *     blur_radius = 0) plus a Gouraud / flat shader from its published behaviour (pytorch3d is not installed: parity unpinned).
 *     DESIGN.md section 17.
 * ---------------------------------------------------------------------------------- */
/* Inputs: verts (sum V, 3) float32 world coordinates and faces (sum F, 3) int32 vertex indices WITHIN their own mesh, both packed
 *   mesh after mesh; vert_first, face_first (b + 1) int64 row offsets of the meshes into the two arrays (entry b = sum V, sum F),
 *   arrays in HOST memory: they are read during the call (they size the launches) and copied to the device as launch arguments,
 *   so they may be freed when the call returns.  A mesh with V == 0 or F == 0 is legal and renders as background.
 *   cameras (b, 16) as bdm_render_points takes them; ortho = 1: OrthographicCameras.
 * All float32 arithmetic is rounded operation by operation (no FMA contraction), in the order written, division correctly
 *   rounded; fl() is left out below.
 * Vertices: xv = ((x c0 + y c3) + z c6) + c9, yv and zv alike with c1, c4, c7, c10 and c2, c5, c8, c11 (bdm_render_points' view
 *   transform); ndc_x = (c12 xv) / zv + c14, ndc_y = (c13 yv) / zv + c15; ortho = 1 drops the two divisions.
 *   sx = (1 - ndc_x) * (0.5 w), sy = (1 - ndc_y) * (0.5 h) (0.5 w is exact): pixel (yi, xi) has its centre at (xi + 0.5, yi + 0.5),
 *   +X left and +Y up as in the point renderer; for h != w each axis spans [-1, 1].
 *   Snapped to 1/256 pixel: SX = rint(sx * 256), SY = rint(sy * 256), rint rounding half to even, as integers.
 *   A vertex is usable iff zv is finite and zv > 0 and both products sx * 256, sy * 256 are finite with magnitude <= 2^22.
 *   A face with an unusable vertex, or a vertex index outside [0, V), is dropped whole.  There is NO near-plane clipping: a
 *   triangle that crosses the camera plane disappears.
 * Coverage (all int64): edge(a, b, p) = (bx - ax)(py - ay) - (by - ay)(px - ax).  A = edge(v0, v1, v2); A == 0: dropped.
 *   A < 0 is a FRONT face, its geometric normal (v1 - v0) x (v2 - v0) points to the camera (view axes x left, y up, z into the
 *   screen are right-handed, and the screen reverses both x and y, which keeps the sign of the z component of the normal).
 *   cull = 1 drops the faces with A > 0.  If A < 0, v1 and v2 are swapped (and A negated), so that A > 0 from here on;
 *   everything below, the depth included, uses the swapped order and the barycentrics are swapped back at the end.
 *   P = (256 xi + 128, 256 yi + 128); E0 = edge(v1, v2, P), E1 = edge(v2, v0, P), E2 = edge(v0, v1, P).  The pixel is covered
 *   iff for every i: E_i > 0, or E_i == 0 and edge i owns its boundary; the edge from a to b with (dx, dy) = b - a owns its
 *   boundary iff dy > 0 || (dy == 0 && dx > 0).  Two faces on opposite sides of a shared edge see opposite directions, so a
 *   centre on the edge belongs to exactly one of them, and a centre on the shared vertex of a closed fan to exactly one face.
 * Depth and barycentrics: w_i = float(E_i) / float(A), the int64 -> float32 conversions rounding to nearest even.
 *   Orthographic: bary = w; z = ((w0 z0) + (w1 z1)) + (w2 z2).
 *   Perspective (perspective-correct): t_i = w_i / z_i; s = (t0 + t1) + t2; z = 1 / s; bary_i = t_i / s.
 *   A fragment whose z is not finite or not > 0 is dropped.  The pixel keeps the fragment with the smallest key
 *   (bits of z) << 32 | face index within the mesh: equal depths go to the lower index.  One face per pixel, no blur radius.
 * Outputs, any of which may be NULL: pix_to_face (b, h, w) int32, the face index WITHIN the mesh, -1 = empty; zbuf (b, h, w), -1 =
 *   empty; bary (b, h, w, 3) in the face's own vertex order, -1 = empty; image (b, h, w, c): from vert_features (sum V, c)
 *   ((b0 f0) + (b1 f1)) + (b2 f2) per channel, from face_features (sum F, c) the winning face's row (flat shading), with neither
 *   zeros; an empty pixel takes background (c).  Passing both feature arrays is an error.
 * Limits: b >= 0 (b == 0 launches nothing and returns 0), 1 <= c <= 4, 1 <= h, w <= 4096, ortho and cull in {0, 1}, sum V and
 *   sum F < 2^31, b h w < 2^31, offsets non-decreasing from 0, no NULL among verts, faces, vert_first, face_first, cameras and the
 *   workspace (nor background when image is given), no output and no part of the workspace overlapping an input or each other.
 *   Outside these the call returns 1 and launches nothing.
 * Determinism: one integer atomic minimum per surviving fragment in global memory, no floating-point atomics, no workgroup waits
 *   on another, every loop is bounded by a launch argument; mesh j of a batch has the bits of that mesh rendered alone, and so
 *   has a repeated call.
 * workspace: bdm_render_meshes_workspace_bytes(b, sum_v, sum_f, h, w) bytes (0 for sizes outside the limits), contents irrelevant
 *   before: the (b, h, w) 64-bit key image, 16 bytes per vertex (SX, SY, zv, usable) and the two offset arrays. */
size_t bdm_render_meshes_workspace_bytes(int b, long long sum_v, long long sum_f, int h, int w);
int bdm_render_meshes(int b, int h, int w, int c, int ortho, int cull, const float *verts, const int *faces,
                      const long long *vert_first, const long long *face_first, const float *cameras,
                      const float *vert_features, const float *face_features, const float *background, int *pix_to_face,
                      float *zbuf, float *bary, float *image, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 14. Mesh metrics (csrc/mesh_metrics.hip): area-weighted surface samples of triangle meshes and the squared distance from points
 *     to the nearest face of a mesh; restates pytorch3d's sample_points_from_meshes and the point-to-face half of
 *     point_mesh_face_distance from their published behaviour (pytorch3d is not installed: parity unpinned).  DESIGN.md section 18.
 * ---------------------------------------------------------------------------------- */
/* Meshes: verts, faces, vert_first, face_first exactly as bdm_render_meshes takes them (packed, indices within the mesh, the two
 *   offset arrays of b + 1 int64 in HOST memory, read during the call and free afterwards).
 * All float32 arithmetic is rounded operation by operation (no FMA contraction), in the order written, division and square root
 *   correctly rounded; fl() is left out below.  dot(a, b) = (ax bx + ay by) + az bz.
 *   cross(a, b) = (ay bz - az by, az bx - ax bz, ax by - ay bx), each component one subtraction of two products.
 * Face quantities (functions of the face alone): v0, v1, v2 its vertices in the face's order; e_i = v_{i+1} - v_i per component
 *   (indices mod 3), l2_i = dot(e_i, e_i); g = v2 - v0; n = cross(e_0, g); nn = dot(n, n).
 * Valid face: its three indices lie in [0, V), its nine coordinates are finite, and nn > 0 and nn < +inf.  Every other face is
 *   invalid: it weighs 0 in the sampler and is ignored by the distance (indices that are out of range are treated as an invalid
 *   face by the rule, not refused: the call cannot see them without reading device memory).
 *
 * bdm_mesh_sample_points: s samples per mesh.
 *   Weights: a_i = sqrt(nn_i) (twice the area), 0 for an invalid face.  amax = the maximum of a over the mesh (exact: an integer
 *     atomic maximum on the bit pattern of the non-negative floats).  q_i = (int64) rint((a_i / amax) * 1073741824.f), rint rounding
 *     half to even, and q_i = 0 for an invalid face: 0 <= q_i <= 2^30.  C_i = q_0 + ... + q_i within the mesh, int64, exact (count /
 *     scan / write in separate launches; no workgroup waits on another).  C_last = C_{F-1}.
 *   Sample j of mesh m: (w0, w1, w2, w3) = Philox4x32-10(key = keys[m], counter = (j, 0, draw, purpose)), the convention of
 *     bdm_philox_normal (counter words in that order, key = (low, high) half of the 64-bit key).
 *     t = floor(((w0 << 32 | w1) * C_last) / 2^64) (the high half of the 128-bit product): 0 <= t < C_last.
 *     The face is the first i with C_i > t (a face with q_i == 0 is never chosen).
 *     u1 = float(w2 >> 8) * 2^-24, u2 = float(w3 >> 8) * 2^-24 (both exact, in [0, 1)); su = sqrt(u1);
 *     b0 = 1 - su, b1 = su * (1 - u2), b2 = su * u2; point = ((b0 v0 + b1 v1) + b2 v2) per component.
 *     normal = n / a per component, of the chosen face.
 *   Outputs: points (b, s, 3); face_idx (b, s) int32, the index within the mesh (may be NULL); normals (b, s, 3) (may be NULL).
 *   Empty mesh (C_last == 0: no face, or no valid one): points 0, normals 0, face_idx -1 (pytorch3d's behaviour for empty meshes).
 *   keys: b 64-bit keys on the device.  max_faces: the largest face count of the batch (it sizes the scan; a value that is not
 *     exactly that maximum is refused).
 *   Limits: 0 <= b <= 65535 (b == 0 or s == 0 launches nothing and returns 0), 1 <= s, b s < 2^31, every mesh has at most 2^24
 *     faces (so C_last <= 2^54), sum V and sum F < 2^31, offsets non-decreasing from 0, no NULL among verts, faces, vert_first,
 *     face_first, keys, points and the workspace, no output and no part of the workspace overlapping an input or each other.
 *     Outside these the call returns 1 and launches nothing.
 *   workspace: bdm_mesh_sample_workspace_bytes(b, sum_f, max_faces) bytes (0 for sizes outside the limits), 16-byte aligned, contents
 *     irrelevant before.
 *
 * bdm_point_mesh_distance: for every point of points (b, p, 3), against the faces of its own mesh.
 *   Per (point x, valid face):
 *     Segment i (a = v_i, e = e_i, l2 = l2_i): r = x - a; h = dot(e, r); t = 0 if l2 == 0, otherwise h / l2, then t = 0 unless
 *       t > 0, then t = 1 unless t < 1 (a clamp to [0, 1] under which a NaN becomes 0);
 *       c = a + t e per component; w = x - c; d_i = dot(w, w).
 *     d_e = d_0; d_e = d_1 if d_1 < d_e; d_e = d_2 if d_2 < d_e.
 *     Inside test: s_i = dot(n, cross(e_i, x - v_i)); the point is inside iff s_0 >= 0 and s_1 >= 0 and s_2 >= 0.
 *     Plane: k = dot(n, x - v0); d_p = (k k) / nn.  d = d_p if the point is inside and d_p < d_e, otherwise d = d_e.
 *   sqdist (b, p) = the smallest d over the valid faces of the mesh, face_idx (b, p) int32 = the face that has it, the lowest index
 *     among equal d: the pair is the minimum of (d, index) in lexicographic order, so it does not depend on how the faces are tiled
 *     or visited.  Overflow: a face whose d is NaN or +inf is never chosen.
 *   A point with a non-finite coordinate gets sqdist = +inf and face_idx = -1; so does every point of a mesh without a valid face
 *     (or whose every d overflowed).
 *   order (b, p) int32, may be NULL: thread k of mesh m handles point order[m p + k] and writes that point's two results; NULL is
 *     the natural order.  It exists so that neighbouring lanes can be given neighbouring points; the bits of the result do not
 *     depend on it.  An entry outside [0, p) is skipped (nothing is read or written for it); if order is not a permutation, the
 *     points it leaves out keep whatever the outputs held.
 *   form: 0 = the chooser, 1 = exhaustive (every point visits every face of its mesh).  2 = culled by tile boxes is NOT BUILT and
 *     is refused: the rule's plane term has no lower bound in terms of the true distance (for a sliver face the computed n is
 *     rounding noise and the inside test passes far along the sliver's axis, where d_p can be 0), so no margin can be argued under
 *     which skipping a tile keeps every bit.  bdm_point_mesh_distance_variant returns the form the chooser
 *     takes for these sizes (always 1 in this implementation), 0 for sizes outside the limits.
 *   Limits: 0 <= b <= 65535 (b == 0 or p == 0 launches nothing and returns 0), b p < 2^31, every mesh has at most 2^24 faces, sum V
 *     and sum F < 2^31, offsets non-decreasing from 0, form in {0, 1}, no NULL among verts, faces, vert_first, face_first, points,
 *     sqdist, face_idx and the workspace, no output and no part of the workspace overlapping an input or each other.  Outside these
 *     the call returns 1 and launches nothing.
 *   workspace: bdm_point_mesh_distance_workspace_bytes(b, sum_f) bytes (0 outside the limits), 16-byte aligned, contents irrelevant before: one
 *     64-byte record per face (v0, v1, v2, n, nn, l2_0 .. l2_2; nn = 0 marks an invalid face) and the two offset arrays.
 * Determinism (both): one integer atomic maximum per face (the sampler's amax), no floating-point atomics, no workgroup waits on
 *   another, every loop is bounded by a launch argument or a face count; mesh j of a batch has the bits of that mesh alone, and
 *   so has a repeated call. */
size_t bdm_mesh_sample_workspace_bytes(int b, long long sum_f, long long max_faces);
int bdm_mesh_sample_points(int b, int s, long long max_faces, const float *verts, const int *faces, const long long *vert_first,
                           const long long *face_first, const unsigned long long *keys, unsigned int draw, unsigned int purpose,
                           float *points, int *face_idx, float *normals, void *workspace, void *stream);
size_t bdm_point_mesh_distance_workspace_bytes(int b, long long sum_f);
int bdm_point_mesh_distance_variant(int b, int p, long long sum_f, int has_order);
int bdm_point_mesh_distance(int b, int p, int form, const float *verts, const int *faces, const long long *vert_first,
                            const long long *face_first, const float *points, const int *order, float *sqdist, int *face_idx,
                            void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 15. K nearest neighbours between two point sets and the transfer of attributes through them (csrc/knn.hip); restates
 *     pytorch3d's knn_points / knn_gather from their published behaviour (pytorch3d is not installed: parity unpinned).
 *     DESIGN.md section 19.
 * ---------------------------------------------------------------------------------- */
/* Layout: queries (sum P, 3) and refs (sum R, 3), packed and point-major.  q_first and r_first are offset arrays of b + 1 int64 in
 *   HOST memory, taken exactly as bdm_mesh_sample_points takes vert_first (read during the call, free afterwards): entry i owns the
 *   query rows q_first[i] .. q_first[i + 1] - 1 and the reference rows r_first[i] .. r_first[i + 1] - 1.  Offsets are non-decreasing
 *   from 0.  A padded (N, P, 3) batch is the case q_first[i] = i P.
 *
 * bdm_knn_points: for every query row the K nearest reference rows of the same entry.
 *   Distance: dx = fl(r_x - q_x), likewise dy and dz; d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), no FMA contraction: the order of
 *     section 10.  The candidates are the reference rows j of the entry, j the index WITHIN the entry.  The neighbourhood is the k
 *     candidates with the smallest (d2, j), ascending.
 *   Outputs: idx (sum P, k) int32 and d2 (sum P, k) float32, addressed like the query rows.  Either may be NULL (the other keeps its
 *     bits; with both NULL nothing is launched).
 *   Non-finite input: a reference row with a non-finite coordinate is nobody's neighbour; a query with a non-finite coordinate has no
 *     neighbours.  Two finite points whose d2 overflows to +inf ARE neighbours (d2 = +inf with idx >= 0).
 *   Short neighbourhoods: a query with m < k neighbours gets its m neighbours in order, then idx = -1 and d2 = +inf.  This holds for
 *     every entry size, an empty reference set included; there is no n > k requirement (the deliberate difference from section 10,
 *     whose rows are all-or-nothing).
 *   Limits: 1 <= k <= 64, 0 <= b <= 65535, sum P, sum R and sum P * k all < 2^31.  No NULL among queries, refs, q_first, r_first and
 *     the workspace (an empty set still passes a valid pointer, which is not read).  No output and no part of the workspace overlaps
 *     an input or another output, judged on byte ranges.  b == 0 or sum P == 0 returns 0 without a launch; anything else outside the
 *     limits returns 1, launches nothing and leaves the outputs untouched.
 *   workspace: bdm_knn_points_workspace_bytes(b, sum_p, k) bytes (0 outside the limits), 16-byte aligned, contents irrelevant before:
 *     the two offset arrays.
 *
 * bdm_knn_interpolate: attributes attr (sum R, c) float32 of the reference rows carried to out (sum P, c) through an (idx, d2) pair
 *   that bdm_knn_points wrote for the same two offset arrays; 1 <= c <= 16.
 *   Entry l of a row takes part iff 0 <= idx_l < R of the entry (an index no search of this entry can have written is skipped, not
 *     refused: the call cannot see it without reading device memory); m = the number of entries that take part, a_l = attr[idx_l].
 *   mode = 0, nearest: out = a of the first entry that takes part, copied bit for bit.
 *   mode = 1, inverse squared distance: w_l = 1 / fl(d2_l + eps), the division correctly rounded; eps is a float argument, eps > 0 and
 *     finite required.  W = (..((w_0 + w_1) + w_2)..) over the entries that take part, ascending;
 *     out_c = (..((w_0 a_0c + w_1 a_1c) + w_2 a_2c)..) / W, each product, each sum and the quotient rounded on its own.  An entry with
 *     d2_l = +inf takes part with w_l = 0 (a row whose every d2 is +inf therefore gets 0 / 0 = NaN).
 *   m == 0: the row gets fill, a float argument, in every channel.
 *   Limits and conventions as above (no NULL among attr, idx, d2, out, the offsets and the workspace; mode in {0, 1}).
 *   workspace: bdm_knn_interpolate_workspace_bytes(b) bytes: the two offset arrays and nothing else.
 * Determinism (both): no atomics, no workgroup waits on another, every loop is bounded by a launch argument or an entry length;
 *   entry i of a batch has the bits of that entry alone, and so has a repeated call. */
size_t bdm_knn_points_workspace_bytes(int b, long long sum_p, int k);
int bdm_knn_points(int b, int k, const float *queries, const float *refs, const long long *q_first, const long long *r_first,
                   int *idx, float *d2, void *workspace, void *stream);
size_t bdm_knn_interpolate_workspace_bytes(int b);
int bdm_knn_interpolate(int b, int k, int c, int mode, float eps, float fill, const float *attr, const int *idx, const float *d2,
                        const long long *q_first, const long long *r_first, float *out, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 16. Mesh cleaning (csrc/mesh_clean.hip): the vertex adjacency of a packed batch of triangle meshes, its connected components, and
 *     Taubin smoothing over it; the smoothing restates pytorch3d's taubin_smoothing (norm_laplacian weights) from its published
 *     behaviour (pytorch3d is not installed: parity unpinned).  DESIGN.md section 20.
 * ---------------------------------------------------------------------------------- */
/* Meshes: verts, faces, vert_first, face_first exactly as bdm_point_mesh_distance takes them (packed, indices within the mesh, the
 *   two offset arrays of b + 1 int64 in HOST memory, read during the call and free afterwards).
 * Connected face: its three indices lie in [0, V) of its mesh and are pairwise different.  Coordinates are not looked at (this is
 *   NOT section 14's valid face).  Every other face is ignored, not refused: the call cannot see it without reading device memory.
 *
 * bdm_mesh_adjacency: E(m) = the unordered pairs {a, c} that are a side of a connected face of mesh m.  N(i) = the ascending list of
 *   the different j with {i, j} in E.  Output, a CSR over the packed vertices: nbr_first (sum V + 1) int32, nbr_first[0] = 0, and
 *   nbr (6 sum F, the upper bound, allocated by the caller) int32; the list of packed vertex g is nbr[nbr_first[g] .. nbr_first[g + 1])
 *   and holds indices WITHIN the mesh, as faces does.  Entries of nbr from nbr_first[sum V] on are left untouched.
 *   The lists are sorted sets, so they do not depend on the order in which faces are visited or slots are claimed (integer atomics
 *   claim the slots; count, scan and write are separate launches).  A vertex of very high valence is slow (one thread sorts its
 *   list), never wrong.
 *   workspace: bdm_mesh_adjacency_workspace_bytes(b, sum_v, sum_f) bytes: the offsets, two counters per vertex, the scan's partial sums
 *     and the 6 sum F unsorted incidences.
 *
 * Components: label(i) = the smallest vertex index within the mesh among the vertices joined to i through E (a vertex without
 *   neighbours is its own component).  The labels are the unique fixed point of the round
 *     m_i = min(l_i, l_j for j in N(i));  l'_i = l_{m_i}   (one pointer jump; every read is of the labels before the round)
 *   started from l_i = i, so the schedule of the rounds does not enter the result.
 *   bdm_mesh_components_init writes the starting labels into the workspace.  bdm_mesh_components_rounds performs `rounds` >= 1
 *   rounds and then writes *changed (one int32 on the device) = 1 if its LAST round changed a label, 0 otherwise; the caller
 *   repeats the call until it reads 0 (at most V of the largest mesh rounds are ever needed: a round of plain propagation fixes
 *   at least one more vertex).  bdm_mesh_components_finish, valid after a call that left *changed == 0, writes
 *     vert_comp (sum V) int32: the rank of i's component among the components of its mesh, ordered by their smallest index;
 *     face_comp (sum F) int32: the component of a connected face's vertices, -1 for every other face;
 *     comp_count (b) int32; comp_verts, comp_faces (sum V each) int32: row vert_first[m] + c holds the number of vertices and of
 *       connected faces of component c of mesh m (exact integer sums); the rows c >= comp_count[m] of a mesh are 0.
 *   All three calls take the same b, offsets and workspace, which has to stay untouched between them.  An entry of nbr outside
 *   [0, V) is skipped (nbr_first and nbr are meant to be bdm_mesh_adjacency's for the same offsets; they are not checked).
 *   workspace: bdm_mesh_components_workspace_bytes(b, sum_v) bytes: the offsets, two label arrays, the rank scan and its partial sums.
 *
 * bdm_mesh_taubin: num_iter iterations; one iteration is a half-step with factor lambd, then a half-step with factor mu.  Every
 *   half-step reads the positions of the previous one only (Jacobi).  Half-step with factor f at vertex i with neighbours
 *   j_1 < ... < j_d, all float32, every operation rounded on its own (no FMA contraction), division and square root correctly rounded:
 *     dx = x_i - x_j, dy, dz alike;  w_j = 1 / (sqrt((dx dx + dy dy) + dz dz) + 1e-12f) in mode 0 ("inverse_length", pytorch3d's
 *     norm_laplacian), w_j = 1 in mode 1 ("uniform");
 *     S = w_{j_1} v_{j_1}, then S = S + w_j v_j in ascending j, per component;  W = w_{j_1}, then W = W + w_j;
 *     new_i = ((1 - f) v_i) + (f (S / W)) per component, 1 - f rounded once in float32.
 *   d == 0: new_i = the bits of v_i (pytorch3d would form 0 / 0 here: a deliberate departure).  Nothing is special-cased for
 *   non-finite coordinates: they spread to the neighbours by the formula (which NaN, sign and payload, is not part of the rule).
 *   Two coincident neighbours give w = 1 / 1e-12f, finite.  num_iter == 0 copies verts to verts_out.  An entry of nbr outside [0, V)
 *   is skipped, as above.  verts_out must not alias verts.
 *   workspace: bdm_mesh_taubin_workspace_bytes(b, sum_v) bytes: the offsets and two arrays of 16-byte rows between which the
 *     half-steps alternate (one load per neighbour); the last half-step writes verts_out.
 *
 * Limits (all): 0 <= b <= 65535, sum V < 2^31, 6 sum F < 2^31 (nbr_first is int32), offsets non-decreasing from 0, rounds >= 1,
 *   0 <= num_iter <= 10000, mode in {0, 1}, lambd and mu finite, no NULL pointer, the workspace 16-byte aligned, no output and no part
 *   of the workspace overlapping an input or another output (judged on byte ranges).  b == 0 or sum V == 0 returns 0 and launches
 *   nothing; anything else outside the limits returns 1, launches nothing and leaves the outputs untouched.  The *_workspace_bytes
 *   functions return 0 outside the limits.
 * Determinism (all): integer atomics only (slot claims and counts), no floating-point atomics, no workgroup waits on another, every
 *   loop is bounded by a launch argument or a segment length; mesh j of a batch has the bits of that mesh alone, and so has a
 *   repeated call. */
size_t bdm_mesh_adjacency_workspace_bytes(int b, long long sum_v, long long sum_f);
int bdm_mesh_adjacency(int b, const int *faces, const long long *vert_first, const long long *face_first, int *nbr_first, int *nbr,
                       void *workspace, void *stream);
size_t bdm_mesh_components_workspace_bytes(int b, long long sum_v);
int bdm_mesh_components_init(int b, const long long *vert_first, const long long *face_first, void *workspace, void *stream);
int bdm_mesh_components_rounds(int b, int rounds, const long long *vert_first, const long long *face_first, const int *nbr_first,
                               const int *nbr, int *changed, void *workspace, void *stream);
int bdm_mesh_components_finish(int b, const int *faces, const long long *vert_first, const long long *face_first, int *vert_comp,
                               int *face_comp, int *comp_count, int *comp_verts, int *comp_faces, void *workspace, void *stream);
size_t bdm_mesh_taubin_workspace_bytes(int b, long long sum_v);
int bdm_mesh_taubin(int b, int num_iter, int mode, float lambd, float mu, const float *verts, const long long *vert_first,
                    const int *nbr_first, const int *nbr, float *verts_out, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 17. Face-to-point distance (csrc/face_point.hip, csrc/point_face.h): the squared distance from every face of a mesh to the nearest
 *     point of its cloud -- section 14's pair rule with the roles of the loops exchanged; with section 14's distance it gives
 *     pytorch3d's symmetric point_mesh_face_distance, restated from its published behaviour (pytorch3d is not installed: parity
 *     unpinned).  DESIGN.md section 21.
 * ---------------------------------------------------------------------------------- */
/* Meshes: verts, faces, vert_first, face_first exactly as bdm_point_mesh_distance takes them.  Clouds are ragged: points (sum P, 3)
 *   float32, packed and point-major; point_first holds b + 1 int64 in HOST memory under section 15's conventions (read during the
 *   call, free afterwards; non-decreasing from 0): cloud m owns the rows point_first[m] .. point_first[m + 1] - 1.
 * d(x, f) is section 14's d of the pair (point x, valid face f), its face quantities, valid faces and arithmetic included: one
 *   definition (csrc/point_face.h) serves both directions, so the two see the same bits for the same pair.
 *
 * bdm_face_point_distance: for a valid face f of mesh m,
 *   sqdist[f] = the smallest d(x, f) over the points x of cloud m, and point_idx[f] (int32) = the index WITHIN the cloud of the point
 *     that has it, the lowest index among equal d: the pair is the minimum of (d, index) in lexicographic order, so it does not
 *     depend on how the cloud is tiled, chunked or visited.
 *   A pair whose d is NaN or +inf is never chosen.  That covers every point with a non-finite coordinate without a rule of its
 *     own: t is clamped to [0, 1] (a NaN becomes 0), so c is finite and w = x - c is non-finite in that coordinate, w w is +inf or
 *     NaN, and so is every d_i and d_e; k has the term n (x - v0) of that coordinate, +-inf or NaN, so d_p is +inf or NaN as well,
 *     and d_p < d_e is false.
 *   An invalid face gets (+inf, -1); so does every face of a mesh whose cloud is empty, and a face all of whose d overflowed.
 *   Outputs are addressed like the packed face rows: sqdist (sum F) float32, point_idx (sum F) int32.
 * Sign: d never has its sign bit set.  Every branch of the rule ends in dot(w, w), a sum of products of a float with itself, or in
 *   (k k) / nn with nn > 0; a product of a float with itself is +0 or positive (or NaN), sums of such are not -0, and the quotient of
 *   a non-negative by a positive is non-negative.  So for the values that can be chosen (finite, non-negative) the bit patterns,
 *   read as unsigned integers, order like the numbers, and (bits of d) << 32 | index orders like (d, index).
 * form: 0 = the chooser, 1 = resident (one workgroup per 256 faces of a mesh visits the whole cloud), 2 = split (the tiles of 1024
 *   points of a cloud are divided over `chunks` workgroups per 256 faces; each thread sends its chunk's minimum, if it found a finite
 *   d, through one 64-bit integer atomic minimum of the key above into the workspace, preset to bits(+inf) << 32 | 0xFFFFFFFF; a
 *   last kernel decodes the keys, the untouched preset being (+inf, -1)).  The minimum of integers is order-free: the two forms give
 *   the same bits.  chunks: 0 = the chooser's count (with form 2: at least 2); 1 .. 65535 with form 2 only (form 1 also takes 1).
 *   A cloud with fewer tiles than chunks leaves the surplus workgroups idle.
 * Chooser: bdm_face_point_distance_variant(b, sum_f, sum_p, max_p, workgroups) is a function of sizes alone and queries no device;
 *   max_p is the largest cloud and workgroups = the sum over the meshes of ceil(F_m / 256), what the resident form keeps busy.  It
 *   returns 2 iff 0 < workgroups < 2048 (8 per compute unit of an MI355X, whose 256 are a constant here) and max_p > 1024, otherwise
 *   1; 0 outside the limits.  bdm_face_point_distance_chunks, same arguments: 1 for the resident form, otherwise
 *   min(ceil(4096 / workgroups), ceil(max_p / 1024), 65535) -- the fewest chunks that reach 16 workgroups per compute unit, at most
 *   one per tile.  The two constants are measured.
 * Limits: 0 <= b <= 65535, every mesh has at most 2^24 faces, sum V, sum F and sum P < 2^31, offsets non-decreasing from 0, form in
 *   {0, 1, 2}, no NULL among verts, faces, points, the three offset arrays, sqdist, point_idx and the workspace (an empty side still
 *   passes a valid pointer, which is not read), the workspace 16-byte aligned, no output and no part of the workspace overlapping an
 *   input or each other (judged on byte ranges).  b == 0 or sum F == 0 returns 0 without a launch; anything else outside the limits
 *   returns 1, launches nothing and leaves the outputs untouched.
 * workspace: bdm_face_point_distance_workspace_bytes(b, sum_f) bytes (0 outside the limits), contents irrelevant before: section 14's
 *   64-byte record and one 8-byte key per face, and the offset arrays.
 * Determinism: one integer atomic minimum per (face, chunk) in the split form, no floating-point atomics, vector atomics on global
 *   memory only, no workgroup waits on another, every loop is bounded by a launch argument or a count; mesh j of a batch has the
 *   bits of that mesh alone, and so has a repeated call, under either form and any chunk count. */
size_t bdm_face_point_distance_workspace_bytes(int b, long long sum_f);
int bdm_face_point_distance_variant(int b, long long sum_f, long long sum_p, long long max_p, long long workgroups);
int bdm_face_point_distance_chunks(int b, long long sum_f, long long sum_p, long long max_p, long long workgroups);
int bdm_face_point_distance(int b, int form, int chunks, const float *verts, const int *faces, const long long *vert_first,
                            const long long *face_first, const float *points, const long long *point_first, float *sqdist,
                            int *point_idx, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 18. Rigid and similarity alignment of point clouds (csrc/align.hip, csrc/align_solve.h): the similarity transform of a cloud, the
 *     closed-form alignment of paired points and iterative closest point; restates pytorch3d's corresponding_points_alignment and
 *     iterative_closest_point from their published behaviour (pytorch3d is not installed: parity unpinned).  DESIGN.md section 22.
 * ---------------------------------------------------------------------------------- */
/* Layout: x (sum P, 3) the source and y (sum R, 3) the target, float32, packed and point-major; x_first and y_first are offset arrays
 *   of b + 1 int64 in HOST memory under section 15's conventions (read during the call, free afterwards; non-decreasing from 0).
 *   A transform is 13 float32 per entry: R (9, row-major), T (3), s (1), in pytorch3d's row-vector convention xt = s (x @ R) + T.
 *
 * Apply rule (bdm_similarity_apply; transform (b, 13) and xt (sum P, 3) on the device): per point and output axis c, every operation
 *   rounded on its own (no FMA contraction),
 *     d = fl(fl(fl(x0 R0c) + fl(x1 R1c)) + fl(x2 R2c));   xt_c = fl(fl(s d) + T_c).
 *
 * Match.  mode 0, "nearest": the source point is transformed by the entry's current transform with the apply rule; its partner is
 *   the target row with the smallest (d2, j) of section 15 for K = 1 (d2 between the target row and the TRANSFORMED point, the lowest
 *   index among equal d2, a pair whose d2 overflowed to +inf included).  A source point whose transformed image has a non-finite
 *   coordinate (every non-finite source point has one) has no partner; a target row with a non-finite coordinate is nobody's partner.
 *   mode 1, "paired": the partner of source row i is target row i; the two lengths of every entry must be equal; a pair with a
 *   non-finite member is left out.
 * Moments.  Over the matched pairs (x, y) of an entry -- x the UNTRANSFORMED source point -- the count W and 17 integer sums in fixed
 *   point, 18 int64 in this order: W, Sx_a (3), Sy_b (3), S x_a y_b (9, a-major), S |x|^2, S |y|^2.
 *     amax = the largest |coordinate| over the finite rows of the entry's x and y (an integer atomic maximum of float bits), E its
 *     binary exponent (-126 for zero and denormals);  bits = min(24, (62 - ceil_log2(max(P, 1))) / 2), integer division;
 *     e = bits - 1 - E;  q(c) = (long long) rint((double) c * 2^e), so |q| <= 2^bits.
 *   Every product is an int64 product of two such values and every sum an int64 sum of at most P of them: below 2^62, exact.  Up to
 *   16384 source points per entry all 24 mantissa bits of the largest coordinate are kept.
 *   bdm_align_moments runs one match under `transform` ((b, 13) on the device, NULL = the identity; not read in mode 1) and writes
 *   moments (b, 18) int64, and where not NULL exponent (b) int32 = e and partner (sum P) int32 = the partner's index WITHIN the
 *   entry's target set, -1 for none.  It is there for tests and diagnostics.
 * Solve (csrc/align_solve.h, float64, one operation at a time, division and square root correctly rounded).  With the sums scaled
 *   back by the exact powers of two 2^-e and 2^-2e (the int64 -> float64 conversion rounds to nearest even) and W as a float64:
 *     mx_a = Sx_a / W, my_b = Sy_b / W;  M_ab = S x_a y_b / W - mx_a my_b;
 *     Xvar = S|x|^2 / W - ((mx_0^2 + mx_1^2) + mx_2^2), Yvar alike.
 *   Rotation: Horn's symmetric, trace-free 4 x 4 matrix
 *     N = [[Mxx+Myy+Mzz, Myz-Mzy, Mzx-Mxz, Mxy-Myx], [., Mxx-Myy-Mzz, Mxy+Myx, Mzx+Mxz], [., ., -Mxx+Myy-Mzz, Myz+Mzy],
 *          [., ., ., -Mxx-Myy+Mzz]]
 *   is diagonalised by 10 cyclic Jacobi sweeps over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) with normals_eig.h's rotation formulas
 *   (a pair whose entry is already 0 is skipped).  q = (w, x, y, z) is the eigenvector column of the largest diagonal entry, the
 *   lowest column among equals (M = 0 gives the identity), divided by its length; Rc is the rotation matrix of q and R = Rc^T.  This
 *   is the Kabsch / SVD solution with the determinant correction (allow_reflection = False): always a proper rotation, rank-deficient
 *   M included.  Reflections are not offered.
 *     tr = S_ab R_ab M_ab (a-major, sequential);  s = tr / max(Xvar, eps) with estimate_scale, else 1;
 *     T = my - s (mx @ R);  mse = max(0, (s s) Xvar - (2 s) tr + Yvar).
 *   mse is pytorch3d's "rmse": the mean squared residual of the pairs under the new transform, no square root taken.  It is ANALYTIC,
 *   formed from the moments and not by a second pass over the points; on clouds that fit exactly it is rounding noise around 1e-16 of
 *   the variance before the clamp.  R, T, s are rounded to float32; mse is kept in float64 for the stopping rule and rounded to float32
 *   for the caller.
 * bdm_corresponding_points_alignment: one paired match, one solve -> transform (b, 13) and, where not NULL, mse (b).  An entry
 *   without a matched pair gets the identity and mse = NaN.
 *
 * Iteration.  bdm_icp_init writes the per-entry state into the workspace: transform = start ((b, 13) on the device, NULL = the
 *   identity), iteration 0, not done, and amax.  bdm_icp_rounds performs `rounds` >= 1 times { match in mode 0 under the current
 *   transform, solve, stopping rule } on the entries that are not done, then writes *active (one int32 on the device) = the number of
 *   entries not done; the caller repeats the call until it reads 0, which happens after at most max_iterations rounds in all.
 *   Every iteration aligns the START cloud x to the current partners, as pytorch3d does: the transform is total, not composed.
 *   Stopping rule for an entry after its iteration t (counted from 1), prev = the mse of iteration t - 1, all in float64:
 *     W == 0: done, not converged, mse = NaN, the transform and the iteration count of before (so: the start transform and 0
 *       iterations when nothing ever matched);
 *     mse == 0: done, converged;
 *     t >= 2 and (prev - mse) / prev <= relative_rmse_thr: done, converged;
 *     t == max_iterations: done, not converged.
 *   An entry that is done is not touched again (its workgroups leave before their first barrier), so the number of rounds per call
 *   does not enter the result.  history, where not NULL, is (b, max_iterations, 13) float32: iteration t of entry i writes row
 *   (i, t - 1); the rows past an entry's last iteration are left untouched.  bdm_icp_finish writes xt (sum P, 3) by the apply rule
 *   under the entry's transform, transform (b, 13), mse (b) float32, converged (b) int32 and iterations (b) int32.  The three calls
 *   take the same b, offsets and workspace, which has to stay untouched between them; max_iterations, estimate_scale,
 *   relative_rmse_thr and eps have to be the same in every bdm_icp_rounds call of a run.
 *   Two deliberate differences from pytorch3d: (1) pytorch3d stops the whole batch when ALL entries pass the test, so an entry's result
 *   depends on its batch-mates; here every entry stops on its own, and entry i of a batch has the bits of that entry alone.
 *   (2) pytorch3d's relative test forms 0 / 0 on identical clouds and never converges; here mse == 0 is converged.
 *
 * Limits (all): 0 <= b <= 65535, sum P and sum R < 2^31, every entry at most 2^20 source and 2^20 target points, offsets
 *   non-decreasing from 0, mode in {0, 1}, rounds >= 1, 1 <= max_iterations <= 10000 (with a history, 13 b max_iterations < 2^31),
 *   eps finite and >= 0, relative_rmse_thr not NaN, no NULL among x, y, the offsets, the workspace and the outputs not marked
 *   optional (an empty side still passes a valid pointer, which is not read), the workspace 16-byte aligned, no output and no part of
 *   the workspace overlapping an input or another output (judged on byte ranges).  b == 0 or sum P == 0 returns 0 without a launch;
 *   anything else outside the limits returns 1, launches nothing and leaves the outputs untouched.
 * workspace: bdm_similarity_apply_workspace_bytes(b) bytes for the apply (the offsets); bdm_align_workspace_bytes(b) bytes for every
 *   other call (0 outside the limits), contents irrelevant before bdm_icp_init, bdm_align_moments and
 *   bdm_corresponding_points_alignment: the two offset arrays and a 240-byte state per entry (moments, transform, mse, amax, counters).
 * Determinism: 64-bit integer atomic adds (the moments) and one 32-bit integer atomic maximum (amax) on global memory, ordinary vector
 *   atomics; no floating-point atomics, no workgroup waits on another, every loop is bounded by a launch argument or an entry length.
 *   The sums are exact, so they do not depend on the launch geometry, on how an entry is split over workgroups or on its batch slot:
 *   entry i of a batch has the bits of that entry alone, and so has a repeated call. */
size_t bdm_similarity_apply_workspace_bytes(int b);
int bdm_similarity_apply(int b, const float *x, const long long *x_first, const float *transform, float *xt, void *workspace,
                         void *stream);
size_t bdm_align_workspace_bytes(int b);
int bdm_align_moments(int b, int mode, const float *x, const float *y, const long long *x_first, const long long *y_first,
                      const float *transform, long long *moments, int *exponent, int *partner, void *workspace, void *stream);
int bdm_corresponding_points_alignment(int b, int estimate_scale, double eps, const float *x, const float *y, const long long *x_first,
                                       const long long *y_first, float *transform, float *mse, void *workspace, void *stream);
int bdm_icp_init(int b, const float *x, const float *y, const long long *x_first, const long long *y_first, const float *start,
                 void *workspace, void *stream);
int bdm_icp_rounds(int b, int rounds, int max_iterations, int estimate_scale, double relative_rmse_thr, double eps, const float *x,
                   const float *y, const long long *x_first, const long long *y_first, float *history, int *active, void *workspace,
                   void *stream);
int bdm_icp_finish(int b, const float *x, const long long *x_first, const long long *y_first, float *xt, float *transform, float *mse,
                   int *converged, int *iterations, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 19. Hole filling (csrc/mesh_fill.hip): the boundary loops of a packed batch of triangle meshes and a centroid fan over every small
 *     simple one.  The rule is this project's own text.  DESIGN.md section 23.
 * ---------------------------------------------------------------------------------- */
/* Meshes: verts, faces, vert_first, face_first exactly as bdm_mesh_adjacency takes them; "connected face" as in section 16.  Every
 *   other face takes no part and is passed through untouched.  Everything below is per mesh, indices within the mesh.
 * 1. Half-edges: connected face f = (v0, v1, v2) has the half-edges 3 f + k, k = 0, 1, 2, running v_k -> v_{k+1}.  For an ordered pair
 *    (a, x): out = the number of half-edges a -> x, in = the number x -> a.  (out, in) = (1, 1): the edge is INTERIOR;
 *    (1, 0): a -> x is a BOUNDARY half-edge; every other combination is IRREGULAR (a fin, or two faces wound the same way).
 * 2. Successor by rotation: for the boundary half-edge h = p -> a in face (p, a, x) look at a -> x.  Boundary: it is succ(h).
 *    Interior: cross to the one face (x, a, y) that holds x -> a and go on with a -> y.  Irregular: h is BLOCKED.  This pairs the
 *    boundary edges correctly where two holes touch at a vertex; succ is injective on what is not blocked, so the boundary half-edges
 *    are disjoint cycles plus paths that end blocked, and every half-edge of such a path is blocked: blocked(h) = blocked(succ(h)).
 * 3. Loops: a loop is a cycle of succ; its label is its smallest half-edge index, its size its number of half-edges (>= 3).  Labels
 *    and blocked flags come from ceil(log2(3 max F)) + 1 rounds of pointer doubling (max F the largest face count of the batch; the
 *    count is fixed by the host, nothing is read back); a round reads one array and writes the other.  A loop is PINCHED when one
 *    vertex is the source of two of its half-edges and NON-FINITE when a source vertex has a non-finite coordinate.
 * 4. Filling: a loop is filled iff size <= max_hole_edges and it is neither pinched nor non-finite.  A filled loop gets one new vertex;
 *    the new vertices follow the mesh's old ones in ascending loop label.  Every half-edge a -> b of a filled loop gets one new face
 *    (b, a, c), c the loop's vertex; the new faces follow the mesh's old ones in ascending half-edge index.  Old vertices and faces,
 *    the faces that are not connected included, keep their place, order and bits.
 * 5. The new vertex is the mean of the loop's source vertices in integer fixed point: E = the exponent of the largest finite
 *    |coordinate| of the mesh (exponent field - 127, a field of 0 counting as 1), e = 39 - E, q(c) = rint(c 2^e) as a 64-bit integer
 *    (rint to nearest even; |q| < 2^40), S = the integer sum of the q, mean = float32((float64(S) 2^-e) / float64(size)): the int64 ->
 *    float64 conversion rounds to nearest even, the product with the power of two is exact, one correctly rounded float64 division,
 *    one rounding to float32.  DESIGN.md section 23 derives |mean - exact mean| <= 2^(E-40) (1 + 2^-23) + (2^-24 + 2^-51) |exact mean|.
 * 6. Attributes: attrs (sum V, c) float32 rows ride along (colours).  A new row is the same fixed-point mean per channel, its scale
 *    from the largest finite |attribute| of the mesh (all channels together); a channel with a non-finite source value gives NaN.
 *
 * bdm_mesh_boundary_loops writes, for the H = 3 sum F half-edges of the batch (half-edge 3 f + k of mesh m at 3 face_first[m] + 3 f + k):
 *     halfedge_loop (H) int32: the label of the half-edge's loop, -1 for a half-edge that is not on the boundary (or whose face is
 *       not connected), -2 for a blocked one;
 *     loop_size, loop_flags (H each) int32: at the slot of a loop's label its size and its flags, 1 filled | 2 too large (size >
 *       max_hole_edges) | 4 pinched | 8 non-finite (a loop that is not filled may carry several); 0 at every other slot;
 *     mesh_counts (b, 9) int32: boundary_edges (blocked ones included), loops, filled_loops, too_large_loops, pinched_loops,
 *       nonfinite_loops, blocked_edges, new_vertices, new_faces; exact integer sums; a loop with several flags is counted under each.
 *   It leaves the loops in the workspace for bdm_mesh_fill_holes.
 * bdm_mesh_fill_holes, after a bdm_mesh_boundary_loops call with the same b, verts, faces, offsets and workspace (untouched in between),
 *   writes the filled batch: verts_out (sum V', 3), attrs_out (sum V', c), faces_out (sum F', 3), packed by out_vert_first and
 *   out_face_first (b + 1 int64 in HOST memory), which the caller forms from mesh_counts: V' = V + new_vertices, F' = F + new_faces per
 *   mesh.  That read of mesh_counts is the only synchronisation of a fill.  Offsets that cannot be a filled mesh (V' < V, V' - V > F,
 *   F' < F, F' - F > 3 F, F' - F < 3 (V' - V)) are refused; a row that the given sizes do not hold is never written.
 * bdm_mesh_fill_variant(b, face_first): 0 when a call with these offsets launches nothing on the boundary list (b == 0, no faces, or
 *   outside the limits), else 256 + the number of doubling rounds.
 *
 * Limits: 0 <= b <= 65535, 6 sum F < 2^31, sum V + sum F < 2^31 (a new vertex index stays an int32), offsets non-decreasing from 0,
 *   3 <= max_hole_edges <= 65535, 0 <= c <= 16, no NULL pointer (with c == 0 attrs and attrs_out still point somewhere; they are not
 *   read or written), the workspace 16-byte aligned, no output and no part of the workspace overlapping an input or another output
 *   (judged on byte ranges).  b == 0 returns 0 and launches nothing; anything else outside the limits returns 1, launches nothing and
 *   leaves the outputs untouched.  bdm_mesh_fill_workspace_bytes returns 0 outside the limits.
 * workspace: bdm_mesh_fill_workspace_bytes(b, sum_v, sum_f) bytes, contents irrelevant before bdm_mesh_boundary_loops: the offsets, two
 *   counters per vertex, six 8-byte corner records per face (neighbour, direction, half-edge; sorted per vertex), and per half-edge the
 *   compaction scan and the arrays of the compacted boundary list, which is all the walk, the doubling rounds, the loop statistics and
 *   the fill touch.
 * Determinism: integer atomics only (slot claims, counts, flag bits, one maximum per mesh), no floating-point atomics, no workgroup
 *   waits on another, every loop is bounded by a launch argument, a segment length or a loop size.  The coordinate sums are integers,
 *   formed by one thread per loop.  Mesh j of a batch has the bits of that mesh alone, and so has a repeated call.  A vertex of very
 *   high valence or a very long filled loop is slow (one thread handles it), never wrong. */
size_t bdm_mesh_fill_workspace_bytes(int b, long long sum_v, long long sum_f);
int bdm_mesh_fill_variant(int b, const long long *face_first);
int bdm_mesh_boundary_loops(int b, int max_hole_edges, const float *verts, const int *faces, const long long *vert_first,
                            const long long *face_first, int *halfedge_loop, int *loop_size, int *loop_flags, int *mesh_counts,
                            void *workspace, void *stream);
int bdm_mesh_fill_holes(int b, int c, const float *verts, const float *attrs, const int *faces, const long long *vert_first,
                        const long long *face_first, const long long *out_vert_first, const long long *out_face_first, float *verts_out,
                        float *attrs_out, int *faces_out, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 20. Decimation by vertex clustering (csrc/mesh_decimate.hip): Open3D's simplify_vertex_clustering by name and meaning.  The rule
 *     is this project's own text.  DESIGN.md section 24.
 * ---------------------------------------------------------------------------------- */
/* Meshes: verts, faces, vert_first, face_first exactly as bdm_mesh_adjacency takes them; "connected face" as in sections 16 and 19:
 *   three indices in range and pairwise different.  Everything below is per mesh, indices within the mesh.
 * 1. Bounds: a vertex is finite when its three coordinates are finite.  lo[a], hi[a] = the minimum and maximum of coordinate a over
 *    the finite vertices, compared as floats (the sign of a zero does not matter below).
 * 2. Cell size h (float32): the caller gives one positive finite voxel_size per mesh, or one resolution R, 1 <= R <= 1024.  With R,
 *    h = max_a(hi[a] - lo[a]) / float32(R): float32 subtractions, a maximum, one correctly rounded float32 division, computed on the
 *    device (nothing is read back for it); if that h is zero or not finite (a mesh without finite vertices included), h = 1.
 * 3. Cell of a finite vertex: k_a = min(int(floorf((c_a - lo[a]) / h)), 2^21 - 1), float32 subtraction and correctly rounded float32
 *    division, no contraction; a quotient that is not below 2^21 (an infinite one included) gives 2^21 - 1.  The key is
 *    kx | ky << 21 | kz << 42.  The grid is anchored at lo: not at the origin, and not half a cell below lo as Open3D's is.
 * 4. Clusters: finite vertices with equal keys form one cluster; a non-finite vertex is a cluster of its own.  A cluster's leader is
 *    its smallest member index.  The new vertices are the clusters in ascending leader; vert_map[v] = the new index of v's cluster.
 * 5. Position: a cluster of one member copies that member's row bit for bit (a non-finite row too).  A larger cluster: contraction 1
 *    ("first") copies the leader's row bit for bit; contraction 0 ("average") takes section 19 rule 5's fixed-point mean over the
 *    members: E from the mesh's largest finite |coordinate|, e = 39 - E, q(c) = rint(c 2^e), S = the 64-bit integer sum,
 *    float32((float64(S) 2^-e) / float64(size)).  A mesh has fewer than 2^21 vertices and |q| < 2^40, so |S| < 2^61; section 19's
 *    bound on the mean holds unchanged.
 * 6. Attributes: attrs (sum V, c) float32 rows, c <= 16, ride along as in section 19 rule 6: copied for a cluster of one and for the
 *    leader under "first"; under "average" the same mean per channel, its scale from the mesh's largest finite |attribute|, and NaN for
 *    a channel with a non-finite member.  (The float32 mean of up to 65 535 uint8 values, rounded to nearest even and clamped, equals
 *    the correctly rounded integer mean: DESIGN.md section 23.  Larger clusters are averaged all the same, without that guarantee.)
 * 7. Faces, in this order: a face that is not connected is dropped, face_map = -3.  A connected face (a, b, c) becomes (vert_map[a],
 *    vert_map[b], vert_map[c]); if two of those are equal it has collapsed and is dropped, face_map = -1.  Among the remaining faces with
 *    the same vertex SET (orientation ignored) the one of the lowest old index is kept, the others are duplicates, face_map = -2.  Kept
 *    faces follow each other in ascending old index and keep their corner order; face_map[i] = the new index of a kept face.
 * 8. mesh_counts (b, 8) int32, exact: new_vertices, new_faces, collapsed_faces, duplicate_faces, bad_faces, nonfinite_vertices,
 *    largest_cluster, merged_vertices (the members of clusters of more than one).
 * Not promised: clustering can leave non-manifold edges and change the genus; nothing repairs that.
 *
 * bdm_mesh_cluster writes vert_map (sum V), face_map (sum F) and mesh_counts and leaves its plan (leaders, ranks, the members of every
 *   cluster, the kept faces) in the workspace.  voxel_size: b float32 in HOST memory, or NULL; with NULL `resolution` counts, with
 *   voxel sizes resolution must be 0.  contraction: 0 average, 1 first (the plan does not depend on it).
 * bdm_mesh_decimate, after a bdm_mesh_cluster call with the same b, verts, faces, offsets and workspace (untouched in between), writes
 *   verts_out (sum V', 3), attrs_out (sum V', c), faces_out (sum F', 3), packed by out_vert_first and out_face_first (b + 1 int64 in
 *   HOST memory), which the caller forms from mesh_counts: V' = new_vertices, F' = new_faces.  That read of mesh_counts is the only
 *   synchronisation.  Offsets that cannot be a decimated mesh (V' > V, V' = 0 with V > 0, F' > F, F' > 0 with V' < 3) are refused; a
 *   row that the given sizes do not hold is never written.
 *
 * Limits: 0 <= b <= 65535, every mesh fewer than 2^21 vertices, sum V < 2^31, 3 sum F < 2^31, offsets non-decreasing from 0,
 *   0 <= c <= 16, no NULL pointer other than voxel_size (with c == 0 attrs and attrs_out still point somewhere; they are not read or
 *   written), the workspace 16-byte aligned, no output and no part of the workspace overlapping an input or another output (judged
 *   on byte ranges).  b == 0 returns 0 and launches nothing; anything else outside the limits returns 1, launches nothing and leaves
 *   the outputs untouched.  bdm_mesh_decimate_workspace_bytes returns 0 outside the limits.
 * workspace: bdm_mesh_decimate_workspace_bytes(b, sum_v, sum_f) bytes, contents irrelevant before bdm_mesh_cluster: the offsets, per
 *   mesh bounds, maxima and h, one open-addressing table of 2 max(sum V, sum F) + b slots (12 bytes each; mesh m owns 2 V_m + 1 of
 *   them for its cells and afterwards 2 F_m + 1 for its face sets), six ints per vertex and two per face.
 * Determinism: integer atomics only (slot claims by 64-bit compare-and-swap, minima for leaders and kept faces, counts, cursors,
 *   per-workgroup minima / maxima of order-preserving float bits), no floating-point atomics, no workgroup waits on another, every
 *   probe loop is bounded by its region's size, every grid by host counts.  Where a key lands in the table depends on arrival order
 *   and nothing but key -> minimum leaves it; the order of a cluster's member segment depends on it too and only integer sums read it.
 *   Mesh j of a batch has the bits of that mesh alone, and so has a repeated call.  One thread averages one cluster: a very large
 *   cluster is slow, never wrong. */
size_t bdm_mesh_decimate_workspace_bytes(int b, long long sum_v, long long sum_f);
int bdm_mesh_cluster(int b, int resolution, const float *voxel_size, int contraction, const float *verts, const int *faces,
                     const long long *vert_first, const long long *face_first, int *vert_map, int *face_map, int *mesh_counts,
                     void *workspace, void *stream);
int bdm_mesh_decimate(int b, int resolution, const float *voxel_size, int contraction, int c, const float *verts, const float *attrs,
                      const int *faces, const long long *vert_first, const long long *face_first, const long long *out_vert_first,
                      const long long *out_face_first, float *verts_out, float *attrs_out, int *faces_out, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 21. Solid voxelisation (csrc/mesh_voxel.hip): the occupancy grid of a packed batch of triangle meshes by parity counting along
 *     grid-aligned rays.  The rule is this project's own text, restated by tests/mesh_voxel_ref.py.  DESIGN.md section 25.
 * ---------------------------------------------------------------------------------- */
/* Meshes: verts, faces, vert_first, face_first exactly as bdm_mesh_adjacency takes them.  Everything below is per mesh.
 * 1. Grid: R = resolution cells per axis, origin o = origin[3 m .. 3 m + 2], cell size h = cell[m] (float32; HOST arrays).  In snapped
 *    coordinates (256 per cell, as section 13's 256 per pixel) the centre of cell i along an axis sits at 256 i + 128.
 * 2. Snapping: q_a = rintf(((v_a - o_a) / h) * 256) in float32, operation by operation: no contraction, the division correctly
 *    rounded, ties to even.  A vertex is usable when its three coordinates are finite and every |q_a| <= 2^19 (compared as floats).
 * 3. Faces: a face with an index out of range, a repeated index or an unusable vertex is DROPPED and counted; every other is USED.
 * 4. The perturbed point: every predicate is evaluated at the cell centre moved by (eps, eps^2, eps^3) in (x, y, z), eps positive
 *    and infinitesimal; the ties of the three rays then describe one and the same point, which is never on the surface.  In integers:
 *    Ray along axis w, (u, v) = the two other axes in increasing order: (y, z), (x, z), (x, y).  A = the doubled area of the face
 *    projected to (u, v); A == 0: the face contributes nothing along w; A < 0: two corners are swapped.  The column centre is covered
 *    when each of the three int64 edge functions is > 0, or == 0 on an edge whose vector (du, dv) has dv < 0 || (dv == 0 && du > 0).
 *    (Not section 13's rule, whose image y points down.)  With n = (b - a) x (c - a) and g(k) = n . (p_k - a), p_k the centre of cell k
 *    of the column, cell k lies BELOW the face when sign~(g(k)) sign(n_w) < 0; sign~(g) = sign(g), or for g == 0 the sign of the first
 *    non-zero of (n_x, n_y, n_z).  Below is monotone in k; with c cells below, the face flips the parity of cells 0 .. c - 1.
 * 5. A cell is inside along an axis when its flips are odd.  mode 0 ("vote"): occupied when at least two axes say inside; mode 1, 2,
 *    3: the x, y, z axis alone.  A closed mesh gives the same grid along all three axes; an open one does not, and the vote repairs
 *    the cells that one ray alone gets wrong, not a hole that two rays see.
 * 6. Integers: |q| <= 2^19 and R <= 512 keep every difference within 2^20, edge functions and normal components within 2^41 and g
 *    within 3 * 2^61: int64 holds them exactly.
 *
 * bdm_mesh_voxelize writes occupancy (b, R, R, R) uint8, 0 / 1, indexed [m][ix][iy][iz]; axes (the same shape, or NULL): bit 0, 1, 2 =
 *   inside along x, y, z; counts (b, 8) int32, exact: faces used, faces dropped, cells inside along x, y, z, cells occupied (by mode),
 *   cells on which the three axes are not all equal ("disagree"), 0.
 *
 * Limits: 0 <= b <= 65535, 1 <= R <= 512, b R^3 < 2^31, sum V < 2^31, 3 sum F < 2^31, offsets non-decreasing from 0, mode 0 .. 3, every
 *   cell size positive and finite, every origin finite, no NULL pointer other than axes, the workspace 16-byte aligned, no output and
 *   no part of the workspace overlapping an input or another output (judged on byte ranges).  b == 0 returns 0 and launches nothing;
 *   anything else outside the limits returns 1, launches nothing and leaves the outputs untouched.
 *   bdm_mesh_voxelize_workspace_bytes returns 0 outside the limits.
 * workspace: bdm_mesh_voxelize_workspace_bytes(b, sum_v, sum_f, R) bytes, contents irrelevant before the call: the offsets, the frames,
 *   16 bytes per vertex and ceil(R / 32) 32-bit words per column, axis and mesh (3 b R^2 columns).
 * Determinism: integer atomics only (XOR of one bit per face and covered column, adds for the counts), no floating-point atomics, no
 *   workgroup waits on another, every loop is bounded by R, by a box or by a launch argument.  The offsets and the frames travel as
 *   launch arguments: nothing is copied or synchronised, and the call is safe under stream capture.  Mesh j of a batch has the bits of
 *   that mesh alone, and so has a repeated call. */
size_t bdm_mesh_voxelize_workspace_bytes(int b, long long sum_v, long long sum_f, int resolution);
int bdm_mesh_voxelize(int b, int resolution, int mode, const float *origin, const float *cell, const float *verts, const int *faces,
                      const long long *vert_first, const long long *face_first, unsigned char *occupancy, unsigned char *axes, int *counts,
                      void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 22. Closed triangle meshes from oriented clouds (csrc/surface_poisson.hip): Poisson surface reconstruction (Kazhdan et al. 2006) on
 *     the uniform grid of section 12.  The normals are splatted into a vector field V, Laplace(phi) = div V is solved by a fixed
 *     schedule of multigrid V-cycles, and the level set of phi through its mean at the samples is handed to the surface nets of
 *     section 12.  phi is defined on every node, so no quad is skipped and every edge of the mesh has an even number of faces.
 *     The rule is this project's own text, restated by tests/surface_poisson_ref.py.  DESIGN.md section 26.
 * ---------------------------------------------------------------------------------- */
/* points, normals, r, s, the node order and the float32 convention (every operation rounded on its own, in the order written, no
 * contraction, division correctly rounded, rint to even) are section 12's.
 * 1. Frame: steps 1 and 2 of section 12 with a margin of s + 3 voxels: inv = float(r - 1 - 2 (s + 3)) / (2 * half).  The same validity
 *    test, the same empty-cloud rule, counts[3] = the number of valid points.  The SAMPLES are the valid points whose q lies in [0, r - 1]^3.
 * 2. Splat: for every sample and every node g = floor(q) + o, o in {-s + 1, ..., s}^3, inside the grid: d, d2, t, w, w3 as in step 3 of
 *    section 12 (no contribution if t <= 0); W = rint(w3 * 4096); V_a = rint((w3 * n_a) * 4096) clamped to [-4096, 4096] (a normal
 *    longer than 1 counts as 1 per component), 0 if the product is NaN, a = x, y, z.  W, Vx, Vy, Vz are exact int32 sums per node: a
 *    sample reaches a node at most once, so n <= 65536 keeps every |sum| <= 65536 * 4096 = 2^28.
 * 3. Right-hand side: D(g) = Vx(g + ex) - Vx(g - ex) + Vy(g + ey) - Vy(g - ey) + Vz(g + ez) - Vz(g - ez), zero outside the grid, an exact
 *    int32 (|D| <= 6 * 2^28 < 2^31), converted to float32 once (to nearest even).
 * 4. Solve: levels l = 0, 1, ... of side m_0 = r, m_{l+1} = m_l / 2, halved while m_l is even and above 4 (16 -> 8 -> 4, 24 -> 12 -> 6 -> 3,
 *    40 -> 20 -> 10 -> 5, 56 -> 28 -> 14 -> 7).  Accepted r: the multiples of 8 in 16 .. 256 whose coarsest side is at most 8, that is
 *    16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256.  h2_l = 4^l.  On every level the unknowns sit at the cell
 *    centres and phi = 0 holds on the outer cell faces: a neighbour outside the level is minus the node's own value.
 *    lap(phi)(g) = (((xm + xp) + (ym + yp)) + (zm + zp)) - 6 * phi(g), xm, xp the neighbours at g -+ ex and so on.
 *    sweep:    phi'(g) = phi(g) + ((lap(phi)(g) - h2_l * f(g)) * c7), c7 = the float32 nearest 1 / 7 (damped Jacobi, omega = 6 / 7),
 *              every node from the old phi.
 *    residual: res(g) = f(g) - lap(phi)(g) * (1 / h2_l).
 *    restrict: f_{l+1}(G) = (the sum of res over the children 2 G + (a, b, c), started from (0, 0, 0) and added in lexicographic
 *              order of (a, b, c)) * 0.125.
 *    prolong:  along z, then y, then x: child 2 K + a takes 0.75 * e(K) + 0.25 * e(K - 1 + 2 a); a coarse index outside the level
 *              is clamped and the value negated, once per axis that is outside.  phi_l(g) += that value.
 *    V-cycle on level l: if l is the coarsest: phi_l = 0, then 32 sweeps.  Otherwise (phi_l = 0 first when l > 0; level 0 continues from
 *    the cycle before, and from 0 in the first) 2 sweeps, restrict the residual, the V-cycle on level l + 1, prolong, 2 sweeps.
 *    phi = level 0 after `cycles` V-cycles.  The schedule depends on (r, cycles) alone: no stopping test, nothing read back.
 * 5. Level: M = max |phi| over the nodes (exact: the bits of |phi| order as integers).  If M == 0 or there is no sample: iso = scale = 0.
 *    Otherwise scale = 2^22 / M, qs = scale * 256.  Per sample: base = min(floor(q), r - 2) per axis, t = q - float(base),
 *    lerp(a, b, t) = a + t * (b - a); the 8 nodes around it are reduced along z, then y, then x to v; I = rint(v * qs) (|I| <= 2^30 + 1).
 *    iso = (float(sum of I, an exact int64) / float(number of samples)) / qs.
 * 6. Hand-over: if scale == 0: SW = SU = 0 everywhere (no vertex, no face).  Otherwise SW = 4096 and
 *    SU = rint((phi - iso) * scale) clamped to [-2^23, 2^23] on every node; then a node of the outermost layer (a coordinate 0 or
 *    r - 1) with SU < 1 gets SU = 1 and is counted in border_raised.  Then two separation passes: in a pass, judged on the grid before it,
 *    a negative node becomes 1 when it lies on a grid face (four nodes g, g + eu, g + ev, g + eu + ev in one coordinate plane, all inside
 *    the grid) on which it and the node across the face are negative and the two others are not.  Surface nets would put four faces on
 *    the mesh edge between the two cells on either side of such a face; a pass can in principle leave new such faces next to the raised
 *    nodes, which is what the second pass is for (none was seen after the first).  Steps 5 and 6 of section 12 follow with thr = 1, unchanged:
 *    negative is inside, triangle normals point to the non-negative side.  Every sign-change edge has its negative end off the border,
 *    so it is a candidate and its four cells hold both signs: skipped == 0 and every mesh edge has an even number of faces.
 * 7. Density: per vertex, (the int32 sum of W over the 8 corners of its cell, as float32) * (1 / 32768).
 *
 * bdm_surface_poisson_grid runs steps 1 - 6 up to and including the mark stage of bdm_surface_grid; counts as in section 12;
 *   info (b, 3) int32 = {border_raised, the bits of iso, the bits of scale}.  bdm_surface_extract then runs on the same workspace as it
 *   is.  The workspace holds the section-12 layout at its start (bdm_surface_workspace_bytes(b, n, r, s) bytes) and behind it, each
 *   (b, r, r, r): W, Vx, Vy, Vz int32, D float32, phi float32; then the accumulators and the coarser levels.
 * bdm_surface_poisson_density, after the grid call with the same b, r and workspace: density[vert_offsets[c] + v] for every vertex v
 *   of cloud c (the offsets as bdm_surface_extract takes them); nothing else is written.
 * Limits: those of section 12 for b, n, r, s; r accepted (step 4); 1 <= cycles <= 32; no NULL pointer; no output or the workspace equal
 *   to an input or to another output.  b == 0 launches nothing and returns 0; outside the limits a call returns 1, launches nothing
 *   and leaves the outputs untouched.  bdm_surface_poisson_workspace_bytes returns 0 outside the limits.
 * Determinism: integer atomics only (sums of the splat, the 64-bit sum of the samples, the maximum of the bits, border_raised), no
 *   floating-point atomic or reduction, no workgroup waits on another, every loop is bounded by a launch argument, safe under stream
 *   capture.  Every cycle overwrites what it reads of the workspace: its contents before the call are irrelevant.  Cloud j of a batch
 *   has the same bits as the same cloud run alone, and so does a repeated call. */
size_t bdm_surface_poisson_workspace_bytes(int b, int n, int r, int s);
int bdm_surface_poisson_grid(int b, int n, int r, int s, int cycles, const float *points, const float *normals, int *counts, int *info,
                             void *workspace, void *stream);
int bdm_surface_poisson_density(int b, int r, const long long *vert_offsets, float *density, void *workspace, void *stream);
/* For tools/surface_poisson_bench.py: the launches of bdm_surface_poisson_grid in parts.  stages: bit 0 = frame, memset, splat and
 * divergence; bit 1 = the solve, which continues from the phi in the workspace (the memset of bit 0 zeroes it); bit 2 = level, hand-over
 * and mark.  per_level = 1 runs every level of the solve in global memory, one launch per level and operator and one per sweep of the
 * coarsest level, in place of the LDS tail: the same arithmetic, so the same bits.  stages = 7, per_level = 0 is
 * bdm_surface_poisson_grid.  The limits are the same; stages outside 1 .. 7 or per_level outside 0 .. 1 return 1. */
int bdm_surface_poisson_grid_staged(int b, int n, int r, int s, int cycles, int stages, int per_level, const float *points,
                                    const float *normals, int *counts, int *info, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------
 * 23. Decimation by quadric edge collapse in rounds (csrc/mesh_qem.hip): Open3D's simplify_quadric_decimation by name and meaning
 *     (Garland and Heckbert 1997); a closed, consistently wound manifold stays one.  Not Open3D's heap order and not an exact face
 *     count (Open3D is not installed: parity unpinned).  The rule is this project's own text, restated by tests/mesh_qem_ref.py,
 *     which is the definition wherever this text is silent.  DESIGN.md section 27.
 * ---------------------------------------------------------------------------------- */
/* Meshes: verts, faces, vert_first, face_first exactly as bdm_mesh_adjacency takes them; "connected face" as in section 16.  Everything
 *   below is per mesh, indices within the mesh.  Arithmetic: positions are float32 in and out; everything that decides is float64,
 *   every operation rounded on its own in the order written (no contraction), division and square root correctly rounded.
 *   dot(a, b) = (a0 b0 + a1 b1) + a2 b2;  cross(p0, p1, p2) = (p1 - p0) x (p2 - p0), each component u_i v_j - u_j v_i.
 * State: a position, a live flag, a locked flag and a quadric (10 float64: a2 ab ac ad b2 bc bd c2 cd d2 of a plane (a, b, c, d)) per
 *   vertex; three indices per face, a dead face holding -1 three times.  Indices are stable through the rounds.
 * Init.  A face that is not connected is dead from the start (face_map -3, "bad") and locks those of its indices that are in range; a
 *   vertex with a non-finite coordinate is locked.  Half-edge 3 f + c of live face f runs from its corner c to corner c + 1.  An
 *   undirected edge {a, b} with `out` half-edges a -> b and `in` half-edges b -> a is INTERIOR for (1, 1), BOUNDARY for (1, 0) or
 *   (0, 1) and IRREGULAR otherwise; its id is the lowest half-edge index over it, in either direction.
 *   Plane term of face (p0, p1, p2): n = cross, l2 = dot(n, n); skipped unless 0 < l2 < inf; area = 0.5 sqrt(l2); d = -dot(n, p0);
 *   the ten products (n_i n_j) s, (n_i d) s, (d d) s with s = area / l2.  Boundary term of a boundary half-edge p -> q of such a face:
 *   e = q - p, m = e x n, ml2 = dot(m, m), skipped unless 0 < ml2 < inf; d = -dot(m, p); s = (boundary_weight area) / ml2.
 *   The quadric of a vertex is 0 plus, for its faces in ascending index: the plane term, then the boundary term of the half-edge that
 *   leaves the vertex in that face, then that of the one that arrives, each term added coefficient by coefficient.
 * A round, for every edge of live faces (each is evaluated once, at its id h; lo < hi its ends), in this order:
 *   1. refused "nonmanifold" when the edge is irregular or an irregular edge ends at lo or hi; "locked" when lo or hi is locked.
 *   2. Q = Q_lo + Q_hi.  With A the 3 x 3 block and r = -(ad, bd, cd): c00 = b2 c2 - bc bc, c01 = ab c2 - bc ac, c02 = ab bc - b2 ac,
 *      det = (a2 c00 - ab c01) + ac c02, tr = (a2 + b2) + c2.  If |det| > 2^-40 ((tr tr) tr) the optimum is Cramer's
 *      m0 = r1 c2 - bc r2, m1 = r1 bc - b2 r2, m2 = ab r2 - r1 ac, x = ((r0 c00 - ab m0) + ac m1) / det, y = ((a2 m0 - r0 c01) + ac m2) / det,
 *      z = ((r0 c02 - a2 m1) - ab m2) / det, accepted when its squared distance to the midpoint (p_lo + p_hi) 0.5 is at most |p_hi - p_lo|^2.
 *      Otherwise the target is the cheapest of p_lo, p_hi and the midpoint, a later one only when strictly cheaper.
 *      error(v) = ((A + 2 B) + 2 C) + d2, A = ((a2 x) x + (b2 y) y) + (c2 z) z, B = ((ab x) y + (ac x) z) + (bc y) z, C = (ad x + bd y) + cd z;
 *      cost = error clamped: e > 0 ? e : 0 (a NaN stays), clamped before any comparison.  Refused "cost" unless cost <= maximum_error and
 *      float32(cost) is finite.  The position stored by a collapse is the target rounded to float32; step 3 uses that rounded value.
 *   3. Validity.  "link": lo and hi must have exactly 2 common neighbours (interior edge) or 1 (boundary edge).  "boundary": an
 *      interior edge between two vertices that each have a boundary edge.  "valence": the third vertex of a face at the edge needs at
 *      least 4 neighbours, or 3 if it has a boundary edge (it loses one and must keep a fan).  "flip": for every live face around lo
 *      that does not contain hi, and around hi that does not contain lo, dot(cross with that corner at the target, cross as it is)
 *      must be > 0 (a zero normal, before or after, refuses).  The first reason that applies is counted.
 *   4. key = bits(float32(cost)) << 32 | h for a valid edge, 2^64 - 1 otherwise.  m1[v] = the minimum key over the edges at v;
 *      m2[v] = the minimum of m1 over v and its neighbours; the edge is SELECTED iff key < 2^64 - 1 and key == m2[lo] == m2[hi].
 *      Selected edges neither share nor neighbour an endpoint, so rule 5 touches disjoint vertices and faces.
 *   5. Apply: lo takes the rounded target and Q (lo's quadric first in every sum); hi dies, vert_map chains hi -> lo; the faces
 *      around hi that contain lo die (face_map -1), the others get lo in hi's corner.
 * Stopping, per mesh, at a round boundary, first match: live faces <= target ("target", 1; tested before the first round too); the
 *   round selected nothing ("no_edge", 2); the number of rounds reached max_rounds ("max_rounds", 3).  Rounds are applied whole: the
 *   final face count lies in (target - the last round's removals, target].  A stopped mesh is not touched again, so neither its
 *   batch-mates nor the number of rounds per call enter its result.
 * mesh_counts (b, 20) int32: stop, rounds, collapses, faces_in, faces_out (live), vertices_in, vertices_out (live), locked_vertices,
 *   bad_faces, the bits of the largest applied float32 cost, then of the mesh's last round: selected, edges evaluated, and the edges
 *   refused as nonmanifold, locked, cost, link, boundary, valence, flip; last the target.
 *
 * bdm_mesh_qem_init checks the batch, copies it into the workspace, forms the quadrics and writes mesh_counts.  target_faces: b int64
 *   in HOST memory.  bdm_mesh_qem_rounds runs up to `rounds` rounds on the meshes that have not stopped, then writes mesh_counts and
 *   *active (one int32 on the device) = the number of meshes still running; the caller repeats the call until it reads 0, which is the
 *   only synchronisation.  maximum_error and max_rounds have to be the same in every call of a run.  bdm_mesh_qem_finish writes
 *   vert_map (sum V; the new index of the survivor a vertex's chain ends in), face_map (sum F; the new index, -1 collapsed, -3 bad),
 *   and verts_out (sum V', 3), attrs_out (sum V', c), faces_out (sum F', 3) packed by out_vert_first and out_face_first (b + 1 int64
 *   in HOST memory) that the caller forms from mesh_counts: survivors in ascending old index, live faces in old order and winding.
 *   Offsets that cannot be a decimated mesh are refused as in section 20; a row the given sizes do not hold is never written.
 *   attrs (sum V, c) float32: a survivor nothing was merged into copies its row bit for bit; another takes section 19 rule 6's
 *   fixed-point mean over the old vertices mapped to it (NaN for a channel with a non-finite member).  The three calls take the same
 *   b, offsets and workspace, which stays untouched in between.
 * Limits: 0 <= b <= 65535, sum V < 2^31, 6 sum F < 2^31, offsets non-decreasing from 0, boundary_weight finite and >= 0, every target
 *   in 0 .. 2^31 - 2, 1 <= rounds, max_rounds <= 2^20, maximum_error >= 0 (+inf allowed), 0 <= c <= 16, no NULL pointer (with c == 0
 *   attrs and attrs_out still point somewhere), the workspace 16-byte aligned, no output and no part of the workspace overlapping an
 *   input or another output.  b == 0 returns 0 and launches nothing; anything else outside the limits returns 1, launches nothing and
 *   leaves the outputs untouched.  bdm_mesh_qem_workspace_bytes returns 0 outside the limits.
 * workspace: bdm_mesh_qem_workspace_bytes(b, sum_v, sum_f) bytes, contents irrelevant before bdm_mesh_qem_init: 148 bytes per vertex
 *   and 104 per face (positions, quadrics, the two minima; the working faces, six 8-byte incidence records, a key and a flag per
 *   half-edge) plus the offsets and counters.
 * Determinism: the minima are gathered over the sorted incidence segments, without atomics; integer atomic adds and maxima only for
 *   slot claims and counts; no floating-point atomics, no workgroup waits on another, every loop is bounded by a segment length or a
 *   launch argument.  Mesh j of a batch has the bits of that mesh alone, and so has a repeated call.  One thread handles one vertex
 *   or edge: a vertex of very high valence is slow, never wrong. */
size_t bdm_mesh_qem_workspace_bytes(int b, long long sum_v, long long sum_f);
int bdm_mesh_qem_init(int b, double boundary_weight, const long long *target_faces, const float *verts, const int *faces,
                      const long long *vert_first, const long long *face_first, int *mesh_counts, void *workspace, void *stream);
int bdm_mesh_qem_rounds(int b, int rounds, int max_rounds, double maximum_error, const long long *vert_first, const long long *face_first,
                        int *mesh_counts, int *active, void *workspace, void *stream);
int bdm_mesh_qem_finish(int b, int c, const float *attrs, const long long *vert_first, const long long *face_first,
                        const long long *out_vert_first, const long long *out_face_first, float *verts_out, float *attrs_out, int *faces_out,
                        int *vert_map, int *face_map, void *workspace, void *stream);
/* For tests and diagnostics: where the state lies in the workspace.  offsets (6 int64 in HOST memory) = the byte offsets of the
 * positions (sum V, 3) float32, the quadrics (sum V, 10) float64, the vertex live flags (sum V) int32, the working faces (sum F, 3)
 * int32, the keys (3 sum F) uint64 and the selected flags (3 sum F) int32 of the last round.  Returns 1 outside the limits. */
int bdm_mesh_qem_layout(int b, long long sum_v, long long sum_f, long long *offsets);

/* ------------------------------------------------------------------------------------
 * 24. Rays against the meshes (csrc/mesh_bvh.hip, csrc/mesh_raycast.hip, csrc/bvh.h): a linear bounding-volume hierarchy over the
 *     faces of a packed batch, and the closest hit, the occlusion flag and the crossing count of arbitrary rays, with the tree and
 *     without it.  The rule is this project's own text, restated by tests/mesh_raycast_ref.py.  DESIGN.md section 28.
 * ---------------------------------------------------------------------------------- */
/* Meshes: verts, faces, vert_first, face_first exactly as bdm_mesh_adjacency takes them.  Float32 throughout, every operation rounded
 * on its own in the order written, no contraction, division correctly rounded; fmin / fmax ignore a NaN operand.
 * 1. Rays: rays (sum R, 8) float32 = origin o (3), direction d (3), tmin, tmax; mesh m owns the rows ray_first[m] .. ray_first[m + 1]
 *    (b + 1 int64 in HOST memory).  d need not be unit; t is in units of d.  A ray is INVALID when a component of o or d or tmin is
 *    not finite, d == (0, 0, 0), tmax is NaN or tmin > tmax (tmax = +inf is allowed).  An invalid ray misses everything and is counted.
 * 2. Faces: a face with an index outside its mesh, a repeated index or a non-finite vertex is DROPPED and counted; every other is USED.
 * 3. The triangle test (Woop, Benthin, Wald 2013).  kz = the axis of the largest |d| (the lowest on a tie), kx = (kz + 1) % 3,
 *    ky = (kz + 2) % 3, swapped when d[kz] < 0.  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  For each corner P of
 *    (a, b, c): p = P - o, Px = p[kx] - Sx * p[kz], Py = p[ky] - Sy * p[kz], Pz = Sz * p[kz].  U = Cx * By - Cy * Bx,
 *    V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax.  When one of them == 0 all three are taken again in float64 (the products of
 *    the float32 factors are exact there, the difference is rounded once).  The signs are judged on these values: the face is
 *    rejected when one is < 0 and another > 0.  Then U, V, W are rounded to float32, det = (U + V) + W, rejected when det == 0;
 *    t = ((U * Az + V * Bz) + W * Cz) / det, b1 = V / det, b2 = W / det (the weights of corners 1 and 2), back = det < 0 (the ray
 *    runs along the normal (b - a) x (c - a)).
 * 4. The face interval.  lo, hi = the float32 min / max of the three corners per axis.  Per axis with inv = 1 / d (the infinity of
 *    its sign for a zero): d >= +0: tn = (lo - o) * inv, tf = (hi - o) * inv; d <= -0: tn = (hi - o) * inv, tf = (lo - o) * inv.
 *    tn is then multiplied by 1 - 2^-16 when >= 0 and by 1 + 2^-16 otherwise, tf by 1 + 2^-16 when >= 0 and by 1 - 2^-16
 *    otherwise.  near = fmax(fmax(fmax(tmin, tn_x), tn_y), tn_z), far = fmin(fmin(fmin(tmax, tf_x), tf_y), tf_z): a NaN (0 times
 *    infinity: the ray runs in a plane of the box) constrains nothing.  The face is ACCEPTED when it passes rule 3, t is finite and
 *    near <= t && t <= far.  Every step is monotone in lo and hi, so a box that encloses the face's gives an interval that encloses
 *    [near, far]: culling by node boxes never changes an answer.
 * 5. Answers per valid ray.  mode 0 (closest): the accepted face of minimum t, the lowest face index on equal t: t, face (index
 *    inside its mesh), bary = (b1, b2), back; a miss or an invalid ray gives +inf, -1, (0, 0), 0.  mode 1 (any): occluded = 1 when a face
 *    is accepted, else 0.  mode 2 (count): crossings = the number of accepted faces.  A ray through a shared edge or vertex is
 *    accepted by every face that touches it: the count is then higher than the number of crossings of the surface.
 *
 * The hierarchy: one binary tree per mesh over its n used faces, in a caller-owned buffer of bdm_mesh_bvh_bytes(b, sum_f) bytes:
 *   b records of 4 int32 (n, faces dropped, 0, 0), padded to 16 bytes, then 2 sum F nodes of 32 bytes, those of mesh m from node
 *   2 face_first[m] on.  A node = lo (3 float32), hi (3 float32), link, skip (int32).  Nodes 0 .. n - 2 are internal (link = the left
 *   child), nodes n - 1 .. 2 n - 2 leaves (link = the face, box = the face's own); node 0 is the root; skip = the node a walk goes
 *   to when it leaves the subtree, -1 at the end.  A walk "visit node; enter link when its interval is not empty, else go to skip"
 *   visits every node at most once and needs no stack.  An internal box is the min / max of its children's.
 *   Build: bdm_mesh_bvh_keys writes one int64 key per face, (m << 32) | (dropped << 30) | the 30-bit Morton code of
 *   ((a + b) + c) * (1 / 3 as float32) in the box of the mesh's finite vertices, 10 bits per axis: q = fmin(fmax((c - lo) * s, 0), 1023)
 *   truncated, s = 1024 / (hi - lo), or 0 where hi - lo is not positive and finite.  The caller sorts the keys ascending with a
 *   STABLE sort (ties keep the face order) and hands the sorted keys and the permutation (int64 packed face rows) to
 *   bdm_mesh_bvh_build: the tree is the radix tree of (key, position) of Karras 2012, the boxes are fitted bottom-up, one arrival
 *   counter per internal node.  counts (b, 2) int32: faces used, faces dropped.
 * bdm_mesh_raycast walks the tree, bdm_mesh_raycast_exhaustive tests every face (staged through LDS): both give the same bits.
 *   Outputs, each (sum R) rows: t float32, face int32, bary (sum R, 2) float32, back uint8 (mode 0); occluded uint8 (mode 1); crossings
 *   int32 (mode 2).  Any of them may be NULL and only those of the mode are written.  counts (b, 5) int32, never NULL: valid rays,
 *   invalid rays, rays with an accepted face, faces used, faces dropped.
 * Limits: 0 <= b <= 65535, sum V < 2^31, 3 sum F < 2^31, sum R < 2^31, offsets non-decreasing from 0, mode 0 .. 2, no NULL pointer
 *   other than the per-ray outputs, the workspace and the hierarchy 16-byte aligned, no output and no part of the workspace
 *   overlapping an input or another output.  b == 0 returns 0 and launches nothing; anything else outside the limits returns 1,
 *   launches nothing and leaves the outputs untouched; the _bytes functions return 0 outside the limits.
 * workspace: bdm_mesh_bvh_workspace_bytes(b, sum_v, sum_f) for the two build calls (the offsets, six floats per mesh, 24 bytes per
 *   face), bdm_mesh_raycast_workspace_bytes(b) for the queries (the offsets); contents irrelevant before each call.
 * Determinism: min / max of floats and integer adds are the only atomics; no spin-wait, no grid barrier, no loop that waits for
 *   another workgroup: the first thread to arrive at an internal node leaves, the second fits it.  The walk of a ray ends after at
 *   most 2 n nodes whatever the buffer holds, and a link outside the mesh ends it.  Mesh j of a batch has the bits of that mesh
 *   alone, and so has a repeated call. */
size_t bdm_mesh_bvh_bytes(int b, long long sum_f);
size_t bdm_mesh_bvh_workspace_bytes(int b, long long sum_v, long long sum_f);
int bdm_mesh_bvh_keys(int b, const float *verts, const int *faces, const long long *vert_first, const long long *face_first, long long *keys,
                      void *workspace, void *stream);
int bdm_mesh_bvh_build(int b, const float *verts, const int *faces, const long long *vert_first, const long long *face_first,
                       const long long *keys, const long long *order, int *counts, void *bvh, void *workspace, void *stream);
size_t bdm_mesh_raycast_workspace_bytes(int b);
int bdm_mesh_raycast(int mode, int b, const float *verts, const int *faces, const long long *vert_first, const long long *face_first,
                     const void *bvh, const float *rays, const long long *ray_first, float *t, int *face, float *bary, unsigned char *back,
                     unsigned char *occluded, int *crossings, int *counts, void *workspace, void *stream);
int bdm_mesh_raycast_exhaustive(int mode, int b, const float *verts, const int *faces, const long long *vert_first,
                                const long long *face_first, const float *rays, const long long *ray_first, float *t, int *face, float *bary,
                                unsigned char *back, unsigned char *occluded, int *crossings, int *counts, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BDM_HIP_H */
