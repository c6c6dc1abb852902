/*
 * libfv2p_ops — C ABI of the MI355X-native (gfx950) voxel-to-point hot path.
 *
 * This header is the drop-in boundary underneath the reference's pybind/torch extension
 * modules.  Every entry point takes plain device pointers, explicit sizes,
 * a caller-provided workspace and a HIP stream (passed as void*), and returns 0 or a
 * negative FV2P_E* code; fv2p_last_error() gives the message.  Nothing here allocates
 * device memory, touches the legacy default stream or calls exit().
 *
 * Each declaration cites the reference interface it replaces (paths relative to the
 * reference checkout, jialeli1/From-Voxel-to-Point).
 */
#ifndef FV2P_OPS_H_
#define FV2P_OPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FV2P_ABI_VERSION 1

#define FV2P_EINVAL      (-1)  /* bad argument (shape, range, null pointer)            */
#define FV2P_EWORKSPACE  (-2)  /* workspace smaller than the matching *_ws_bytes query */
#define FV2P_EHIP        (-3)  /* a HIP runtime call failed                            */
#define FV2P_ELIMIT      (-4)  /* problem exceeds a documented packing limit           */

typedef void* fv2p_stream_t;   /* hipStream_t */

const char* fv2p_last_error(void);
int fv2p_abi_version(void);

/* ---- primitives (exported for tests; used internally by voxeliser and rulebook) ------- */
size_t fv2p_scan_ws_bytes(int64_t n);
int fv2p_exclusive_scan_i32(const int* in, int* out, int64_t n, int* total, void* ws, size_t ws_bytes,
                            fv2p_stream_t stream);
size_t fv2p_radix_sort_ws_bytes(int64_t n);
int fv2p_radix_sort_u64(uint64_t* keys, uint64_t* tmp, int64_t n, int bit_lo, int bit_hi, void* ws,
                        size_t ws_bytes, fv2p_stream_t stream);

/* ---- A1: points_to_voxel ----------------------------------------------------------------
 * Replaces pcdet/datasets/processor/voxel_generator.py:75-133 (points_to_voxel) and
 * :136-207 (_points_to_voxel_reverse_kernel): first-come voxelisation, coords stored (z,y,x),
 * fp32 floor((p-lo)/vs), the whole scan stops at the first point that would open voxel number
 * max_voxels+1 (:198-199).
 *   points      [n_points, ndim] f32 (device), xyz first
 *   voxel_size  [3] f32 host (x,y,z);  range_lo [3] f32 host;  grid [3] i32 host (x,y,z)
 *   voxels      [max_voxels, max_points, ndim] f32 (device) — rows >= *num_voxels untouched zero
 *   coors       [max_voxels, 3] i32 (z,y,x);  num_points_per_voxel [max_voxels] i32
 *   num_voxels  device int: number of voxels produced (<= max_voxels)
 * All outputs are fully written (zero padded) by the call.
 */
size_t fv2p_points_to_voxel_ws_bytes(int64_t n_points, int max_voxels);
int fv2p_points_to_voxel(const float* points, int64_t n_points, int ndim, const float voxel_size[3],
                         const float range_lo[3], const int grid[3], int max_points, int max_voxels,
                         float* voxels, int* coors, int* num_points_per_voxel, int* num_voxels,
                         void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* Stacked form of A1: B clouds of any sizes, concatenated into one point buffer, voxelised in one pass whose number of kernel
 * launches does not depend on B, written as the collated batch (pcdet/datasets/dataset.py:152-183).  Every sample is voxelised as
 * fv2p_points_to_voxel voxelises it alone (first-come order, the break at its own voxel number max_voxels+1); empty clouds are legal.
 *   points      [n_total, ndim] f32 (device), the clouds one after the other
 *   counts      [batch] i32 HOST: points per cloud, >= 0, summing to n_total
 *   voxel_size, range_lo, grid: as above;  max_voxels applies to every sample on its own
 *   rows_cap    = sum over b of min(counts[b], max_voxels): the rows the caller allocates
 *   voxels      [rows_cap, max_points, ndim] f32;  num_points [rows_cap] i32
 *   coords      [rows_cap, 4] i32 (b, z, y, x);  sample b's M_b = min(distinct voxels of b, max_voxels) rows start at sum of M_a, a < b
 *   voxel_cnt   [batch] device i32: M_b
 *   _mean       features [rows_cap, ndim] f32 instead of voxels / num_points: the sum over a row's point slots in slot order divided
 *               by max(num_points, 1) — MeanVFE (pcdet/models/backbones_3d/vfe/mean_vfe.py:14-31), bit for bit
 *               fv2p_voxel_mean_collate — without the padded tensor
 * All outputs are fully written by the call (rows past the produced total are zero); n_total == 0 zero-fills and returns.
 * Limits (FV2P_ELIMIT): n_total <= 2^24 - 2, batch * grid volume <= 2^40 - 2, batch * max_voxels <= 2^24 - 2; batch >= 1.
 * No host synchronisation: the counts travel as kernel arguments.
 */
size_t fv2p_points_to_voxel_stack_ws_bytes(int64_t n_total, int batch, int max_voxels);
int fv2p_points_to_voxel_stack(const float* points, int64_t n_total, int ndim, int batch, const int* counts,
                               const float voxel_size[3], const float range_lo[3], const int grid[3], int max_points,
                               int max_voxels, float* voxels, int* coords, int* num_points, int* voxel_cnt,
                               void* ws, size_t ws_bytes, fv2p_stream_t stream);
int fv2p_points_to_voxel_stack_mean(const float* points, int64_t n_total, int ndim, int batch, const int* counts,
                                    const float voxel_size[3], const float range_lo[3], const int grid[3], int max_points,
                                    int max_voxels, float* features, int* coords, int* voxel_cnt,
                                    void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* Host entry point of A1: the reference calls VoxelGenerator.generate on numpy arrays inside forked DataLoader workers
 * (pcdet/datasets/processor/data_processor.py:43-81 -> voxel_generator.py:75-207), where HIP cannot be initialised.  All
 * pointers are HOST pointers, the scan runs on the calling thread and makes no HIP call; same outputs as above (voxels,
 * num_points_per_voxel zero-filled by the call), *num_voxels is a host int. */
int fv2p_points_to_voxel_host(const float* points, int64_t n_points, int ndim, const float voxel_size[3],
                              const float range_lo[3], const int grid[3], int max_points, int max_voxels,
                              float* voxels, int* coors, int* num_points_per_voxel, int* num_voxels);

/* ---- A3/A4: sparse-conv rulebook ----------------------------------------------------------
 * Replaces sparse_conv_ext.get_indice_pairs_{2d,3d} (pcdet/ops/spconv/src/all.cc:22-33 ->
 * spconv_ops.h:27-140 getIndicePair<NDim>, kernels indice.cu.h:22-203, CPU geometry.h:24-297).
 * Geometry arrays are host int[3] in (z,y,x) order (2-D problems pass a unit leading dim).
 * subm!=0: stride:=1, padding:=ksize/2 (spconv_ops.h:76-80), out_shape must equal in_shape.
 *
 * The build is split around the one host-visible quantity, the number of output rows:
 *   begin : hashes the active set (subm) or the distinct candidate outputs (conv / transposed);
 *           *n_out_host = number of output rows (conv: synchronises `stream`, like the
 *           reference's numActOut, spconv_ops.h:131-139).
 *   finish: fills   out_indices [n_out,4] (b,z,y,x) sorted by flat index (conv only; null for subm),
 *                   tab_in  [K, n_in ]  output row fed by input row i through offset k, or -1,
 *                   tab_out [K, n_out]  input row feeding output row o through offset k, or -1
 *                                       (may be null: for subm with odd ksize and dilation 1
 *                                        tab_out[k] == tab_in[K-1-k]),
 *                   indice_num [K]      pairs per offset (the reference's indiceNum); may be null and obtained
 *                                       later with fv2p_rulebook_count (the fused conv kernels never read it).
 * begin and finish must be given the same workspace (>= fv2p_rulebook_ws_bytes) and arguments.
 * Kernel offset index k = (kz*Ky + ky)*Kx + kx with k_j = in_j - out_j*s_j + p_j (geometry.h:62-73).
 */
size_t fv2p_rulebook_ws_bytes(int64_t n_in, const int ksize[3], const int stride[3], const int dilation[3],
                              int subm, int transpose);
/* Same, plus room for the bitmap path of strided / transposed rulebooks: when batch * output volume <= 2^28 cells and the
 * workspace has this size, begin/finish rank the output cells with one bit per cell and a popcount scan (ascending
 * flat index = the reference's sorted-unique order) instead of the hash set + radix sort; results are identical. */
size_t fv2p_rulebook_ws_bytes_grid(int64_t n_in, int batch, const int out_shape[3], const int ksize[3],
                                   const int stride[3], const int dilation[3], int subm, int transpose);
/* 0 (default): bitmap path whenever it applies; 1: always the hash set + radix sort. Process-wide; for tests / A-B runs. */
int fv2p_rulebook_set_path(int path);
int fv2p_rulebook_begin(const int* indices, int64_t n_in, int batch, const int in_shape[3],
                        const int out_shape[3], const int ksize[3], const int stride[3], const int padding[3],
                        const int dilation[3], int subm, int transpose, int64_t* n_out_host, void* ws,
                        size_t ws_bytes, fv2p_stream_t stream);
int fv2p_rulebook_finish(const int* indices, int64_t n_in, int batch, const int in_shape[3],
                         const int out_shape[3], const int ksize[3], const int stride[3], const int padding[3],
                         const int dilation[3], int subm, int transpose, int64_t n_out, int* out_indices,
                         int* tab_in, int* tab_out, int* indice_num, void* ws, size_t ws_bytes,
                         fv2p_stream_t stream);
/* 4-D rulebooks (SparseConv4d / SubMConv4d: spconv_ops.h:143-258 and the 4-D instantiations of getIndicePair, all.cc:22-33; Python
 * entry point get_indice_pairs_4d, ops.py:96-150 of the reference).  indices [n_in, 5] = (batch, four coordinates), out_indices
 * [n_out, 5]; the same two-phase hash set + radix sort as above (output rows in ascending (batch, cell) order), no bitmap path and
 * no transposed form (the reference has no SparseConvTranspose4d).  Kernel offset index: row-major over ksize[0..3]. */
size_t fv2p_rulebook4d_ws_bytes(int64_t n_in, const int ksize[4], const int stride[4], const int dilation[4], int subm);
int fv2p_rulebook4d_begin(const int* indices, int64_t n_in, int batch, const int in_shape[4],
                          const int out_shape[4], const int ksize[4], const int stride[4], const int padding[4],
                          const int dilation[4], int subm, int64_t* n_out_host, void* ws, size_t ws_bytes,
                          fv2p_stream_t stream);
int fv2p_rulebook4d_finish(const int* indices, int64_t n_in, int batch, const int in_shape[4],
                           const int out_shape[4], const int ksize[4], const int stride[4], const int padding[4],
                           const int dilation[4], int subm, int64_t n_out, int* out_indices, int* tab_in,
                           int* tab_out, int* indice_num, void* ws, size_t ws_bytes, fv2p_stream_t stream);
/* Rows [n,4] (b,z,y,x) ordered by the residue class of (coordinate + padding) mod stride, stable inside a class:
 * input rows of one class of a strided conv reach the same few kernel offsets.  Strides 1 or 2. */
size_t fv2p_rulebook_class_perm_ws_bytes(int64_t n);
int fv2p_rulebook_class_perm(const int* indices, int64_t n, const int stride[3], const int padding[3], int* perm,
                             void* ws, size_t ws_bytes, fv2p_stream_t stream);
int fv2p_rulebook_count(const int* tab_in, int64_t n_in, int kvol, int* indice_num, fv2p_stream_t stream);
/* Reference-format pair lists indicePairs [K,2,n_in] from tab_in; within one offset pairs are ordered by ascending
 * input row (the CPU reference's order, geometry.h:281-295; the GPU reference's slot order is atomic-order).
 * pad != 0 fills the unused tail with -1 (spconv_ops.h:55-57); pad == 0 leaves it unwritten (enough for
 * fv2p_sparse_conv_wgrad_pairs, which reads pair_num[k] entries).  pair_num [K] (optional) receives indiceNum. */
size_t fv2p_rulebook_pairs_ws_bytes(int64_t n_in, int kvol);
int fv2p_rulebook_pairs(const int* tab_in, int64_t n_in, int kvol, int pad, int* pairs, int* pair_num, void* ws,
                        size_t ws_bytes, fv2p_stream_t stream);
/* Tables from caller-supplied pair lists [K,2,pair_len] + indice_num [K] (device). */
int fv2p_pairs_to_tables(const int* pairs, const int* indice_num, int kvol, int64_t pair_len, int64_t n_in,
                         int64_t n_out, int* tab_in, int* tab_out, fv2p_stream_t stream);

/* ---- A5/A6: fused sparse convolution ------------------------------------------------------
 * Replaces sparse_conv_ext.indice_conv_fp32 / indice_conv_backward_fp32 / fused_indice_conv_fp32
 * (all.cc:34-51 -> spconv_ops.h:260-457, fused_spconv_ops.h:28-131; gather/scatter kernels
 * reordering.cu.h:21-157 and the torch::mm between them).
 *   dst[r,:] = (bias) + sum_k src[tab[k][r],:] . W_k           rows with tab == -1 are skipped
 * weight is the reference parameter layout [K][Cin][Cout] (spconv/conv.py:98-99).
 *   forward        : src=features[n_in,Cin],  tab=tab_out, n_dst=n_out, c_dst=Cout, transpose_w=0
 *   backward data  : src=dOut[n_out,Cout],    tab=tab_in,  n_dst=n_in,  c_dst=Cin,  transpose_w=1
 *   inverse conv   : src=features[n_out,Cin'], tab=tab_in, n_dst=n_in,  transpose_w=0
 * flip_k is a flag word: bit 0 (FV2P_TAB_FLIP) reads table row K-1-k for offset k (subm symmetry, lets subm reuse
 * tab_in as tab_out); bit 1 (FV2P_TAB_PLANNED, conv entry points only) promises that the table's allocation continues
 * with the tiling plan fv2p_conv_plan_build wrote behind it (see below).  The reference has no counterpart of the
 * plan: its gather -> mm -> scatter loop balances by construction (one GEMM per offset, spconv_ops.h:300-357).
 * fp32 in / fp32 accumulate on v_mfma_f32_16x16x4_f32; deterministic (fixed k order, no atomics).
 */
#define FV2P_TAB_FLIP 1
#define FV2P_TAB_PLANNED 2
/* Cost-balanced tiling of a table's destination rows for the fused conv kernels.  A table `tab` [kvol][n_dst] allocated
 * with fv2p_conv_plan_ints(n_dst) extra ints behind it can be given a plan once (it depends on the table only, so every
 * conv that shares the rulebook — forward, flipped submanifold backward, any channel count — reuses it): the rows are cut
 * into contiguous ranges of equal cost, cost(row) = max(pairs of the row, 8), for tile counts 256, 384, 512, 768, ...;
 * a launch picks the level that suits its shape and a workgroup processes one range.  Results are bit-identical with
 * and without a plan (every row's sum still runs over ascending k inside one workgroup); only the work per workgroup
 * changes: equal-row tiles carry up to 2x the median pairs at the 5-20 pairs per row of the backbones' deep levels. */
int64_t fv2p_conv_plan_ints(int64_t n_dst);
size_t fv2p_conv_plan_ws_bytes(int64_t n_dst);
int fv2p_conv_plan_build(int* tab, int kvol, int64_t n_dst, void* ws, size_t ws_bytes, fv2p_stream_t stream);
/* Test / tuning hook: force one kernel variant of fv2p_sparse_conv_rows for the calls that follow
 * (0 = heuristic, 1 = plain dense tile, 2 = compacted tile, 3 = register-staged pipeline).  All variants compute
 * the same sum in the same k order. */
int fv2p_sparse_conv_set_impl(int impl);
/* Test / tuning hook for the two thin-layer kernels the heuristic (impl 0) adds for the full 3 x 3 x 3 kernel: conv_rows_thin
 * (16 -> 16, any row count; with it conv_rows_first: <= 8 source channels that are not a multiple of 4 or fewer than 16, <= 32 destination
 * channels - the backbones' first layer) and conv_rows_res (32 source channels, <= 32 destination channels, <= 65 536 rows).  1 = on, 0 = off
 * (the staged kernels take those launches), -1 = back to the FV2P_CONV_THIN / FV2P_CONV_RES preset (default on).  Same sum, same k order. */
int fv2p_sparse_conv_set_paths(int thin_on, int res_on);
/* Profiling hook: when non-NULL, every workgroup of the LDS-DMA conv kernel writes {HW_ID, XCC_ID, start, end of the
 * offset loop, end of the prologue, clocks spent waiting at the per-offset barrier (wave 0), 0, 0} (shader clock) to
 * trace[8*blockIdx .. +7] (device memory, >= 8*ceil(n_dst/64) entries).  NULL switches it off. */
int fv2p_sparse_conv_set_trace(unsigned long long* trace);
/* Measurement hook (bench.py's roofline.in_step_us): while armed, every conv launch of fv2p_sparse_conv_rows* with exactly these
 * channel counts, kernel volume, destination rows and table direction (flip_k & 1) - forward convs that gather their source rows as
 * they are (not the PRE form of fv2p_sparse_conv_rows_bnfin: another kernel instance) - is bracketed by a pair of HIP events on the
 * launch stream (at most 512 pairs; further launches run unbracketed).  fv2p_sparse_conv_probe_read waits for the recorded pairs,
 * returns their number and the sum of their elapsed times in microseconds, and disarms.  No reference counterpart (its timers are
 * commented out: spconv_ops.h:305-360). */
int fv2p_sparse_conv_probe_arm(int c_src, int c_dst, int kvol, int64_t n_dst, int flip);
int fv2p_sparse_conv_probe_read(double* sum_us, int* launches);

/* fv2p_sparse_conv_rows that also leaves the per-column sum and sum of squares of dst (fp64) in `stats`
 * [fv2p_sparse_conv_stat_slots()][2][c_dst]: the caller passes it zero-filled, the conv epilogue (or, for shapes
 * whose sum takes several launches, a reduce pass after the conv) adds into it; the total over the slots is what
 * BatchNorm1d needs (fv2p_batchnorm_forward_stats).  Declared after fv2p_sparse_conv_rows below. */
int fv2p_sparse_conv_stat_slots(void);
int fv2p_sparse_conv_rows(const float* src, int64_t n_src, int c_src, const float* weight, int kvol,
                          const int* tab, int64_t n_dst, int c_dst, int flip_k, int transpose_w,
                          const float* bias, float* dst, fv2p_stream_t stream);
int fv2p_sparse_conv_rows_stats(const float* src, int64_t n_src, int c_src, const float* weight, int kvol,
                                const int* tab, int64_t n_dst, int c_dst, int flip_k, int transpose_w,
                                const float* bias, float* dst, double* stats, fv2p_stream_t stream);
/* Backward-data conv (no bias) whose result dst is the gradient of a BatchNorm1d(+ReLU) output: `stats` (zero-filled,
 * same slot layout) additionally receives that layer's backward sums, sum dz and sum dz * xhat with
 * dz = dst * [y > 0] and xhat, y recomputed from the BatchNorm input bn_x [n_dst, c_dst] — what
 * fv2p_batchnorm_backward_stats needs (c_src > 128: summed by a pass after the conv instead of in its epilogue). */
int fv2p_sparse_conv_rows_bnbwd(const float* src, int64_t n_src, int c_src, const float* weight, int kvol,
                                const int* tab, int64_t n_dst, int c_dst, int flip_k, int transpose_w, float* dst,
                                const float* bn_x, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                const float* bn_beta, int relu, double* stats, const int* perm, fv2p_stream_t stream);
/* ---- round 6: BatchNorm statistics finalised by the conv launch, BatchNorm (+ReLU) of the source rows on the gather ------------
 * The reference runs conv -> nn.BatchNorm1d -> nn.ReLU as three modules (spconv_backbone.py:8-27, modules.py:86-100) and, inside a
 * residual block, conv1 -> bn1 -> relu -> conv2 (spconv_backbone.py:47-68).  Here
 *   fv2p_sparse_conv_rows_bnfin     = the conv that finalises the BatchNorm statistics of its own output: every workgroup stores its
 *                                     tile's column sums as one row of `stats` (a workspace of fv2p_sparse_conv_fin_ws_bytes(n_dst, c_dst)
 *                                     bytes, no initialisation needed), the launch's last workgroups fold the rows in a fixed order
 *                                     (no float atomics: the statistics are bit-identical from run to run) and when the launch ends
 *                                     mean / invstd [c_dst] (and the running statistics, num_batches_tracked) are final and
 *                                     counter[] (fv2p_sparse_conv_fin_counter_words() zeroed device words the caller keeps per stream
 *                                     and direction) zero again - BatchNorm apply kernels
 *                                     (fv2p_batchnorm_apply_res) and consumer convs read 2 - 4 floats per column instead of folding
 *                                     64 slots in every workgroup.  stats == NULL: no statistics.
 *                                     pre_mean / pre_invstd / pre_gamma / pre_beta [c_src] (NULL = off): every gathered source row passes
 *                                     through relu?((v - mean) * invstd * gamma + beta) on its way into the MFMAs - the producer's
 *                                     BatchNorm(+ReLU) output is never materialised.  Same operations in the same order as
 *                                     fv2p_batchnorm_apply: results are bit-identical to the conv over materialised rows.
 *                                     Kernels with that form: ask fv2p_sparse_conv_prenorm_supported (else FV2P_EINVAL, nothing launched).
 *   fv2p_sparse_conv_rows_bnbwd_fin = fv2p_sparse_conv_rows_bnbwd whose last workgroup leaves dgamma, dbeta [c_dst] and
 *                                     coef [2][c_dst] = (mean dz, mean dz * xhat; zeros when batch_stats == 0) for fv2p_batchnorm_backward_fin.
 *   fv2p_sparse_conv_wgrad(_pairs)_pre = the weight gradient with the same normalisation of the gathered operand. */
int fv2p_sparse_conv_rows_bnfin(const float* src, int64_t n_src, int c_src, const float* weight, int kvol, const int* tab,
                                int64_t n_dst, int c_dst, int flip_k, int transpose_w, const float* bias, float* dst,
                                double* stats, unsigned* counter, float eps, float momentum, float* running_mean,
                                float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd,
                                const float* pre_mean, const float* pre_invstd, const float* pre_gamma, const float* pre_beta,
                                int pre_relu, fv2p_stream_t stream);
int fv2p_sparse_conv_prenorm_supported(int c_src, int c_dst, int kvol, int64_t n_dst, int flip_k, int transpose_w);
int fv2p_sparse_conv_fin_counter_words(void);
size_t fv2p_sparse_conv_fin_ws_bytes(int64_t n_dst, int c_dst);
int fv2p_sparse_conv_rows_bnbwd_fin(const float* src, int64_t n_src, int c_src, const float* weight, int kvol, const int* tab,
                                    int64_t n_dst, int c_dst, int flip_k, int transpose_w, float* dst, const float* bn_x,
                                    const float* bn_mean, const float* bn_invstd, const float* bn_gamma, const float* bn_beta,
                                    int relu, double* stats, unsigned* counter, int batch_stats, float* dgamma, float* dbeta,
                                    float* coef, const int* perm, fv2p_stream_t stream);
int fv2p_sparse_conv_wgrad_pre(const float* src, int64_t n_src, int c_src, const float* grad, const int* tab, int64_t n_dst,
                               int c_dst, int kvol, int flip_k, int dense_k, float* dweight, const float* pre_mean,
                               const float* pre_invstd, const float* pre_gamma, const float* pre_beta, int pre_relu, void* ws,
                               size_t ws_bytes, fv2p_stream_t stream);
int fv2p_sparse_conv_wgrad_pairs_pre(const float* src, int64_t n_src, int c_src, const float* grad, int64_t n_grad, int c_dst,
                                     const int* pairs, const int* pair_num, int kvol, int64_t pair_len, int side_src,
                                     float* dweight, const float* pre_mean, const float* pre_invstd, const float* pre_gamma,
                                     const float* pre_beta, int pre_relu, void* ws, size_t ws_bytes, fv2p_stream_t stream);
/* fv2p_sparse_conv_rows with a row order: perm [n_dst] (NULL = identity) says which destination rows share a 64-row
 * tile; every row's sum is unchanged (bit-identical results), only the work per tile changes — a tile visits just the
 * kernel offsets its rows use.  Meant for the backward-data conv of strided layers with fv2p_rulebook_class_perm's
 * order (also accepted by fv2p_sparse_conv_rows_bnbwd). */
int fv2p_sparse_conv_rows_perm(const float* src, int64_t n_src, int c_src, const float* weight, int kvol,
                               const int* tab, int64_t n_dst, int c_dst, int flip_k, int transpose_w,
                               const float* bias, float* dst, const int* perm, fv2p_stream_t stream);
/* dW_k[c_src][c_dst] = sum_r src[tab[k][r],:]^T grad[r,:]   (dweight [K][c_src][c_dst], fully written here).
 *   forward conv's dW : src=features, grad=dOut [n_out,Cout], tab=tab_out, n_dst=n_out.
 * Per-chunk partial tiles go through the workspace and are summed in a fixed order (deterministic, no atomics).
 * dense_k >= 0 names an offset known to pair (almost) every row — the centre of a submanifold conv — which is then split
 * into many short row chunks of its own so that it does not become the straggler of the launch (-1: none). */
size_t fv2p_sparse_conv_wgrad_ws_bytes(int64_t n_dst, int c_src, int c_dst, int kvol);
int fv2p_sparse_conv_wgrad(const float* src, int64_t n_src, int c_src, const float* grad, const int* tab,
                           int64_t n_dst, int c_dst, int kvol, int flip_k, int dense_k, float* dweight, void* ws,
                           size_t ws_bytes, fv2p_stream_t stream);
/* The same weight gradient from the rulebook's compacted pair lists — the reference's indice_pairs [K][2][pair_len]
 * (-1 padded) and indice_pair_num [K] (spconv_ops.h:403-455 walks the same lists; fv2p_rulebook_pairs / _count build
 * them): dW_k = sum_{p < pair_num[k]} src[pairs[k][side_src][p], :]^T grad[pairs[k][1 - side_src][p], :].
 * side_src = 0 for a forward / submanifold conv (src = features indexed by the input side), 1 for an inverse conv.
 * Work is split by pairs, not rows, so dense and sparse offsets cost what their pair counts say. */
size_t fv2p_sparse_conv_wgrad_pairs_ws_bytes(int64_t pair_len, int c_src, int c_dst, int kvol);
int fv2p_sparse_conv_wgrad_pairs(const float* src, int64_t n_src, int c_src, const float* grad, int64_t n_grad,
                                 int c_dst, const int* pairs, const int* pair_num, int kvol, int64_t pair_len,
                                 int side_src, float* dweight, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* fv2p_sparse_conv_wgrad_pairs with short summation chains: on 64 / 128 channels on both sides (the LDS-DMA kernel's shapes) the MFMA
 * accumulators take the products of 16 pairs and are folded into float64 running sums, rounded to fp32 once per chunk, so a chunk's
 * error is that of its 16-term fp32 chains instead of one chain over its up to 512 pairs (dW of a 3 x 3 conv with 150 pairs per offset:
 * 3.2 x the error of MIOpen's blocked sums with the plain form).  Other shapes run the plain kernels.  Same arguments, same
 * workspace (fv2p_sparse_conv_wgrad_pairs_ws_bytes), fixed order, no atomics. */
int fv2p_sparse_conv_wgrad_pairs_fine(const float* src, int64_t n_src, int c_src, const float* grad, int64_t n_grad,
                                      int c_dst, const int* pairs, const int* pair_num, int kvol, int64_t pair_len,
                                      int side_src, float* dweight, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- the first BEV convolution as a sparse convolution with dense output rows ------------------------------------
 * Replaces HeightCompression's dense map (height_compression.py:10-26: spconv_tensor.dense().view(B, C * D, H, W)) in front of the
 * first ZeroPad2d(1) + Conv2d(C * D -> Cout, 3 x 3) of BaseBEVBackbone (base_bev_backbone.py:27-33): the tables below drive
 * fv2p_sparse_conv_rows / fv2p_sparse_conv_wgrad_pairs(_fine) over the sparse rows themselves, so neither the map nor the products with
 * its zeros exist.  indices [n, 4] (batch, z, y, x) of a tensor with spatial shape (depth, height, width), rows unique per cell;
 * kvol = 9 * depth offsets k = z * 9 + ky * 3 + kx (depth <= 3); destination rows = all batch * height * width BEV cells,
 * cell = (b * height + oy) * width + ox.
 *   tab_out [kvol][batch * height * width]  row at (b, z, oy + ky - 1, ox + kx - 1), the (z, ky, kx) tap of the cell under padding 1,
 *                                           stride 1; -1 where there is none.  Filled here (also when n == 0).  A caller that passes
 *                                           FV2P_TAB_PLANNED allocates fv2p_conv_plan_ints(batch * height * width) ints behind it.
 *   tab_in  [kvol][n]                       the cell a row reaches through offset k; -1 for a cell outside the map and for the
 *                                           offsets of the other z planes
 *   pairs [kvol][2][n], pair_num [kvol]     (both may be NULL) the lists of fv2p_rulebook_pairs(tab_in, pad = 0) for
 *                                           fv2p_sparse_conv_wgrad_pairs: ascending input row inside every offset
 * No hash, no sort, nothing read back by the host; every table and list is the same from run to run.  A row whose coordinates lie
 * outside the grid pairs with nothing.  Workspace (for the pair lists only): fv2p_bev_entry_tables_ws_bytes. */
size_t fv2p_bev_entry_tables_ws_bytes(int64_t n, int depth);
int fv2p_bev_entry_tables(const int* indices, int64_t n, int batch, int depth, int height, int width, int* tab_out, int* tab_in,
                          int* pairs, int* pair_num, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- fused sparse convolution on 16-bit operands ----------------------------------------------
 * What the reference binds as indice_conv_half / indice_conv_backward_half / fused_indice_conv_half (all.cc:36-51), plus
 * bfloat16, which it does not have.  `dtype` names the 16-bit format of EVERY operand and result of a call (features,
 * weight, bias, gradients, outputs): FV2P_DT_F16 = IEEE binary16, FV2P_DT_BF16 = bfloat16; any other value returns
 * FV2P_EINVAL and launches nothing.  The fp32 entry points above are not involved and no operand is converted to fp32 in
 * memory: products run on v_mfma_f32_16x16x32_f16 / _bf16 with fp32 accumulators.
 *   fv2p_sparse_conv_rows_h : the contract of fv2p_sparse_conv_rows,
 *                               dst[r,:] = bias + sum_k src[tab[k][r],:] . W_k     (W_k^T with transpose_w = 1)
 *     on the [K][Cin][Cout] parameter layout; entries with tab == -1 are skipped, flip_k bit 0 (FV2P_TAB_FLIP) reads table
 *     row K-1-k for offset k, FV2P_TAB_PLANNED may be set and is ignored (these kernels take no tiling plan).  Each element
 *     is summed over ascending k (all source channels of an offset before the next offset) inside one workgroup, without
 *     atomics; bias [c_dst] (NULL = none; in the call's dtype) is widened to fp32 and added to the fp32 sum, which is then
 *     rounded to nearest even ONCE, at the store.  Results are bit-identical from run to run.  Any c_src, c_dst >= 1
 *     (counts that are not a multiple of 8, or pointers that are not 16-byte aligned, take an element-wise fetch).
 *     n_dst == 0 returns 0 and launches nothing.
 *   fv2p_sparse_conv_wgrad_h : dW_k[cs][cd] = sum_r src[tab[k][r], cs] . grad[r, cd], table-driven like fv2p_sparse_conv_wgrad
 *     (no dense_k, no pair-list form).  Chunks of destination rows leave fp32 partial tiles in the workspace
 *     (fv2p_sparse_conv_wgrad_h_ws_bytes); the partials are summed in ascending chunk order, no atomics, and rounded once
 *     to the 16-bit dweight [K][c_src][c_dst], which is fully written.  n_dst == 0 returns 0, launches nothing and leaves
 *     dweight as it is. */
#define FV2P_DT_F16 1
#define FV2P_DT_BF16 2
int fv2p_sparse_conv_rows_h(const void* src, int64_t n_src, int c_src, const void* weight, int kvol, const int* tab,
                            int64_t n_dst, int c_dst, int flip_k, int transpose_w, const void* bias, void* dst,
                            int dtype, fv2p_stream_t stream);
size_t fv2p_sparse_conv_wgrad_h_ws_bytes(int64_t n_dst, int c_src, int c_dst, int kvol);
int fv2p_sparse_conv_wgrad_h(const void* src, int64_t n_src, int c_src, const void* grad, const int* tab, int64_t n_dst,
                             int c_dst, int kvol, int flip_k, void* dweight, int dtype, void* ws, size_t ws_bytes,
                             fv2p_stream_t stream);
/* The same two passes for fp32 MASTER weights beside 16-bit rows (mixed precision: pcdet.ops.spconv.set_mixed_precision).  `dtype`
 * names the format of src / dst / grad only; the arguments, checks, coverage and summation orders are those of the entry points
 * above, and there is no 16-bit copy of the weights in memory.
 *   fv2p_sparse_conv_rows_hw32 : weight (same [K][c_src][c_dst] layout, [K][c_dst][c_src] with transpose_w = 1) and bias are fp32.
 *     Every weight element is rounded to nearest even to `dtype` while its slice is staged into LDS; from there on the kernel is
 *     that of fv2p_sparse_conv_rows_h, so with bias == NULL the result is bit for bit fv2p_sparse_conv_rows_h on weight rounded to
 *     `dtype`.  The fp32 bias is added to the fp32 sum as it is (NOT rounded to 16 bits first); the sum is rounded once, at the store.
 *   fv2p_sparse_conv_wgrad_hw32 : dweight [K][c_src][c_dst] is fp32: the sum of the chunk partials in ascending chunk order, without
 *     the final rounding (rounding it to `dtype` gives the bits of fv2p_sparse_conv_wgrad_h).  Workspace: fv2p_sparse_conv_wgrad_h_ws_bytes. */
int fv2p_sparse_conv_rows_hw32(const void* src, int64_t n_src, int c_src, const float* weight, int kvol, const int* tab,
                               int64_t n_dst, int c_dst, int flip_k, int transpose_w, const float* bias, void* dst,
                               int dtype, fv2p_stream_t stream);
int fv2p_sparse_conv_wgrad_hw32(const void* src, int64_t n_src, int c_src, const void* grad, const int* tab, int64_t n_dst,
                                int c_dst, int kvol, int flip_k, float* dweight, int dtype, void* ws, size_t ws_bytes,
                                fv2p_stream_t stream);

/* ---- A7: sparse max-pool / neighbour group over the same tables ------------------------------
 * Replace sparse_conv_ext.indice_maxpool_fp32(+backward) (all.cc:52-63 -> pool_ops.h:25-94; output starts
 * at zero so the result is max(0, .)) and indice_group_fp32(+backward) (all.cc:64-71 -> group_ops.h:29-291):
 *   maxpool fwd : out[o,c]   = max(0, max_k in[tab_out[k][o], c])
 *   maxpool bwd : din[i,c]   = sum_k [in[i,c]==out[o,c]] dout[o,c],  o = tab_in[k][i]
 *   group   fwd : out[k,o,:] = in[tab_out[k][o], :] or 0             ([K, n_out, C])
 *   group   bwd : din[i,:]   = sum_k grad[k, tab_in[k][i], :]
 */
int fv2p_sparse_maxpool_fwd(const float* in, int64_t n_in, int c, const int* tab, int kvol, int64_t n_out,
                            int flip_k, float* out, fv2p_stream_t stream);
int fv2p_sparse_maxpool_bwd(const float* in, const float* out, const float* dout, int64_t n_in, int c,
                            const int* tab_in, int kvol, float* din, fv2p_stream_t stream);
/* The two max-pool passes on 16-bit rows.  `dtype` (FV2P_DT_F16 / FV2P_DT_BF16) names the format of in, out, dout and din; any
 * other value returns FV2P_EINVAL with "dtype" in the message and launches nothing.  Elements are compared on their widened
 * values: the forward result is one of its inputs or 0, so it is exact; the backward sum runs in fp32 over ascending k and
 * is rounded to nearest even once.  One thread takes 8 channels (one 16-byte access) when c % 8 == 0 and the pointers are
 * 16-byte aligned, one channel otherwise.  n_out == 0 (fwd) / n_in == 0 (bwd) returns 0 and launches nothing. */
int fv2p_sparse_maxpool_fwd_h(const void* in, int64_t n_in, int c, const int* tab, int kvol, int64_t n_out,
                              int flip_k, void* out, int dtype, fv2p_stream_t stream);
int fv2p_sparse_maxpool_bwd_h(const void* in, const void* out, const void* dout, int64_t n_in, int c,
                              const int* tab_in, int kvol, void* din, int dtype, fv2p_stream_t stream);
int fv2p_sparse_group_fwd(const float* in, int64_t n_in, int c, const int* tab, int kvol, int64_t n_out,
                          int flip_k, float* out, fv2p_stream_t stream);
int fv2p_sparse_group_bwd(const float* grad, int64_t n_out, int c, const int* tab, int kvol, int64_t n_in,
                          int flip_k, float* din, fv2p_stream_t stream);
/* The group pair on 16-bit rows (the reference has indice_group_fp32 only, all.cc:64-71; these carry the features of a 16-bit
 * backbone).  `dtype` (FV2P_DT_F16 / FV2P_DT_BF16) names the format of in / out (fwd) and grad / din (bwd); any other value returns
 * FV2P_EINVAL with "dtype" in the message and launches nothing.  The forward copies 16-bit elements (zeros where the table holds
 * -1); the backward sums in fp32 over ascending k and rounds to nearest even once.  8 channels per 16-byte access when c % 8 == 0
 * and the pointers are 16-byte aligned, one channel otherwise.  n_out == 0 (fwd) / n_in == 0 (bwd) returns 0 and launches nothing. */
int fv2p_sparse_group_fwd_h(const void* in, int64_t n_in, int c, const int* tab, int kvol, int64_t n_out,
                            int flip_k, void* out, int dtype, fv2p_stream_t stream);
int fv2p_sparse_group_bwd_h(const void* grad, int64_t n_out, int c, const int* tab, int kvol, int64_t n_in,
                            int flip_k, void* din, int dtype, fv2p_stream_t stream);

/* ---- (f).2: bilinear gather of BEV features at key points --------------------------------------------------------
 * Replaces bilinear_interpolate_torch and BEVGridPooling.interpolate_from_bev_features
 * (pcdet/models/backbones_3d/pfe/bev_grid_pooling.py:11-45, 68-83).  bev: [B, C, H, W] (channels_first, the layout the
 * detector holds; transposed once into the workspace) or [B, H, W, C]; x, y [B, n]: pixel coordinates (already divided
 * by voxel size and stride); out [B, n, C].  Corners floor / floor + 1 clamped to the map, weights from the clamped
 * corners, sum order a, b, c, d — the reference's arithmetic, no contraction.  bwd: gradient of the map (zero-filled
 * here, float atomics: unordered like torch's index backward); x, y get no gradient. */
size_t fv2p_bev_interp_ws_bytes(int batch, int c, int h, int w, int channels_first);
int fv2p_bev_interp_fwd(const float* bev, int batch, int c, int h, int w, int channels_first, const float* x,
                        const float* y, int64_t n, float* out, void* ws, size_t ws_bytes, fv2p_stream_t stream);
int fv2p_bev_interp_bwd(const float* grad_out, int batch, int c, int h, int w, int channels_first, const float* x,
                        const float* y, int64_t n, float* grad_bev, void* ws, size_t ws_bytes, fv2p_stream_t stream);
/* bwd in the fixed order of fv2p_scatter_add (4 entries per point, the bilinear weights as coefficients), with its own workspace */
size_t fv2p_bev_interp_bwd_ws_bytes(int batch, int c, int h, int w, int channels_first, int64_t n);
int fv2p_bev_interp_bwd_gather(const float* grad_out, int batch, int c, int h, int w, int channels_first, const float* x,
                               const float* y, int64_t n, float* grad_bev, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* The gather on float16 / bfloat16 maps (`dtype`: FV2P_DT_F16 / FV2P_DT_BF16, the format of bev, out, grad_out and grad_bev; any
 * other value returns FV2P_EINVAL with "dtype" in the message and launches nothing).  x / y stay fp32; no operand is converted to
 * fp32 in memory.  fwd: the four corner rows are widened, ((a * wa + b * wb) + c * wc) + d * wd is formed in fp32 in that order and
 * rounded to nearest even ONCE: bit for bit fv2p_bev_interp_fwd on the widened map, rounded.  Lanes take 8 channels per 16-byte
 * access when c % 8 == 0 and the pointers are 16-byte aligned, one channel otherwise.  Workspace: the channel-last image of a
 * channels_first map in its own format, fv2p_bev_interp_h_ws_bytes (0 otherwise, and for a non-positive size).
 * bwd: the fixed-order form only (the entries of fv2p_bev_interp_bwd_gather summed by the 16-bit form of fv2p_scatter_add: fp32
 * sums in the same association, each cell's total rounded once), then the 16-bit transpose back for a channels_first map.  No
 * atomics.  grad_bev is zero-filled where no point falls; n == 0 only zero-fills it.  Workspace: fv2p_bev_interp_bwd_h_ws_bytes
 * (0 for a non-positive map size or n < 0). */
size_t fv2p_bev_interp_h_ws_bytes(int batch, int c, int h, int w, int channels_first);
int fv2p_bev_interp_fwd_h(const void* bev, int batch, int c, int h, int w, int channels_first, const float* x, const float* y,
                          int64_t n, void* out, int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream);
size_t fv2p_bev_interp_bwd_h_ws_bytes(int batch, int c, int h, int w, int channels_first, int64_t n);
int fv2p_bev_interp_bwd_h(const void* grad_out, int batch, int c, int h, int w, int channels_first, const float* x,
                          const float* y, int64_t n, void* grad_bev, int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- (f).2: SparseConvTensor.dense() and its gradient ---------------------------------------------------------
 * Replaces scatter_nd + permute + contiguous (pcdet/ops/spconv/structure.py:5-18, 57-66; consumer HeightCompression,
 * pcdet/models/backbones_2d/map_to_bev/height_compression.py:10-26).  indices [n, 1+ndim] (batch, z, y, x) or
 * (batch, y, x); dense is [B, C, *spatial] (channels_first) or [B, *spatial, C]; it is zero-filled here.
 * Duplicate coordinates: last writer in thread order wins (the reference's index_put is equally unordered). */
int fv2p_sparse_to_dense(const float* features, const int* indices, int64_t n, int c, int ndim, int batch,
                         const int spatial[3], int channels_first, float* dense, fv2p_stream_t stream);
int fv2p_dense_to_sparse(const float* dense, const int* indices, int64_t n, int c, int ndim, int batch,
                         const int spatial[3], int channels_first, float* rows, fv2p_stream_t stream);
/* The same pair on 16-bit features (SparseConvTensor.dense() of a .half() / .bfloat16() backbone, which the reference sends through
 * scatter_nd + permute + contiguous as well, structure.py:57-66).  `dtype` (FV2P_DT_F16 / FV2P_DT_BF16) names the format of features /
 * rows and dense; any other value returns FV2P_EINVAL and launches nothing.  Elements are moved, never converted: the result is bit
 * for bit the reference's.  The forward zero-fills dense itself (also when n == 0).  channels_last with c % 8 == 0 and 16-byte
 * aligned pointers moves 16-byte pieces of a row; every other case moves single elements, channels_first with neighbouring lanes on
 * neighbouring cells. */
int fv2p_sparse_to_dense_h(const void* features, const int* indices, int64_t n, int c, int ndim, int batch,
                           const int spatial[3], int channels_first, void* dense, int dtype, fv2p_stream_t stream);
int fv2p_dense_to_sparse_h(const void* dense, const int* indices, int64_t n, int c, int ndim, int batch,
                           const int spatial[3], int channels_first, void* rows, int dtype, fv2p_stream_t stream);

/* ---- (f).1: MeanVFE + collate of one voxelised cloud -------------------------------------------------------------
 * feats[v, :] = sum of the zero-padded point slots of voxel v / max(num_points[v], 1)   (vfe/mean_vfe.py:14-31),
 * coords[v, :] = (batch_idx, z, y, x)   (dataset.collate_batch, pcdet/datasets/dataset.py:165-171), for the
 * v < min(*num_voxels, max_voxels) voxels of fv2p_points_to_voxel's output; feats / coords point at this cloud's
 * offset inside the batch tensors.  *num_voxels is read on the device. */
int fv2p_voxel_mean_collate(const float* voxels, const int* coors, const int* num_points, const int* num_voxels,
                            int max_voxels, int max_points, int ndim, int batch_idx, float* feats, int* coords,
                            fv2p_stream_t stream);

/* ---- A16: rotated BEV overlap / IoU, rotated and axis-aligned NMS ----------------------------
 * Replace iou3d_nms_cuda.* (pcdet/ops/iou3d_nms/src/iou3d_nms_api.cpp:11-17):
 *   boxes_overlap_bev_gpu (iou3d_nms.cpp:49-68,  kernel iou3d_nms_kernel.cu:236-249)
 *   boxes_iou_bev_gpu     (iou3d_nms.cpp:70-88,  kernel :251-265)
 *   nms_gpu / nms_normal_gpu (iou3d_nms.cpp:90-187, kernels :267-372, host greedy loop :121-135)
 *   boxes_iou_bev_cpu     (iou3d_cpu.cpp:232-252) — host pointers, runs on the calling thread.
 * boxes are [n,7] f32 (x, y, z, dx, dy, dz, heading).  fv2p_nms expects boxes already sorted by descending
 * score; keep [n] i64 and num_keep [1] i32 are DEVICE buffers (the greedy pass runs on the GPU); survivors
 * are written in ascending index order, exactly the reference's keep list.  normal!=0 ignores headings.
 */
int fv2p_boxes_overlap_bev(const float* boxes_a, int num_a, const float* boxes_b, int num_b,
                           float* ans_overlap, fv2p_stream_t stream);
int fv2p_boxes_iou_bev(const float* boxes_a, int num_a, const float* boxes_b, int num_b, float* ans_iou,
                       fv2p_stream_t stream);
size_t fv2p_nms_ws_bytes(int n);
int fv2p_nms(const float* boxes, int n, float thresh, int normal, int64_t* keep, int* num_keep, void* ws,
             size_t ws_bytes, fv2p_stream_t stream);
/* Batched, truncated form for proposal layers (roi_head_template.py:46-101 loops `class_agnostic_nms` over the samples and
 * keeps `selected[:NMS_POST_MAXSIZE]`, model_nms_utils.py:16-20): boxes [batch, n, 7] sorted by descending score per sample,
 * keep [batch, keep_stride] i64, num_keep [batch] i32, both on the device.  max_keep > 0 stops each sample's greedy pass
 * at its max_keep-th survivor (identical to the head of the full list); max_keep <= 0 keeps all. */
size_t fv2p_nms_batch_ws_bytes(int batch, int n, int max_keep);
int fv2p_nms_batch(const float* boxes, int batch, int n, float thresh, int normal, int max_keep, int64_t* keep,
                   int keep_stride, int* num_keep, void* ws, size_t ws_bytes, fv2p_stream_t stream);
/* boxes_iou3d_gpu (pcdet/ops/iou3d_nms/iou3d_nms_utils.py:454-491) for a batch in one launch: boxes_a [batch, num_a, 7], boxes_b
 * [batch, num_b, b_stride >= 7] (e.g. gt boxes with their class id), ans_iou [batch, num_a, num_b] = BEV overlap x height overlap
 * / max(vol_a + vol_b - overlap, 1e-6), clamped to [0, 1] — the same float operations in the same order as the per-sample
 * composition of boxes_overlap_bev_gpu with torch ops. */
int fv2p_boxes_iou3d_batch(const float* boxes_a, int batch, int num_a, const float* boxes_b, int num_b, int b_stride, float* ans_iou,
                           fv2p_stream_t stream);
int fv2p_boxes_iou_bev_cpu(const float* boxes_a, int num_a, const float* boxes_b, int num_b, float* ans_iou);

/* ---- centre head at test time: heat-map peak decode and detections --------------------------------
 * fv2p_center_peaks replaces CenterAFHeadTemplate.predhm_based_predicted_boxes_generation_ssd
 * (pcdet/models/dense_heads/center_af_head_template.py:518-598; maxpool == 0: ..._nomaxpooling, :600-667) with
 * center_utils._nms / _topk / _transpose_and_gather_feat and box_utils.decode_rot_binres (pcdet/utils/box_utils.py:366-406) for a
 * whole batch.  All maps fp32, NCHW, contiguous: hm [B,nc,H,W], offset [B,2,H,W], height [B,1,H,W], dim [B,3,H,W],
 * rot [B,2*bins,H,W], iouscore [B,1,H,W]; free of NaN.
 *   heat      = hm * keep, keep = 1.0f where hm equals the maximum of its 3x3 neighbourhood in its own class map (cells outside
 *               the map take no part, max_pool2d with padding 1), 0.0f elsewhere: a real multiply, a suppressed negative logit
 *               gives -0.0f.  maxpool == 0: heat = hm.
 *   selection : per sample the k entries of heat over (class c, cell = y*W + x) that come first when sorted by descending value,
 *               ties (-0.0f equals 0.0f) by ascending c*H*W + cell.  The reference (two torch.topk) gives this order wherever the
 *               k+1 best values are distinct; where they are not, torch.topk promises nothing and THIS RULE IS THE OP'S
 *               DEFINITION.  Zeros of suppressed cells outrank negative peaks, as in the reference.
 *   decode    : x = ((x + off_x) * float(stride)) * voxel_x + range_x0 in fp32, every product and sum rounded on its own (no
 *               fused multiply-add); y likewise; height and dim copied; heading from the first maximal bin: bin * per + res *
 *               (per/2), per = 2 pi / bins, torch's remainder by 2 pi, values above pi lowered by 2 pi.
 *   outputs   : boxes [B,k,7], cls [B,k,nc] = heat of all classes at the cell, score [B,k] = raw iouscore logit,
 *               cell [B,k] i64 = y*W + x, cls_id [B,k] i32 = c.
 * Limits: 1 <= k <= 512, k <= H*W, 1 <= nc <= 16, 1 <= bins <= 32, maxpool 0 or 1, stride >= 1, sizes >= 1 and non-null pointers
 * (FV2P_EINVAL otherwise); nc*H*W < 2^31 - 4096 and batch <= 65535 (FV2P_ELIMIT); FV2P_EWORKSPACE below fv2p_center_peaks_ws_bytes
 * (a pure host function; 0 for non-positive sizes).  All checks come before the first launch.
 * TWO launches whatever the batch: the heat keys of all samples, then one workgroup per sample that finds the bin of the k-th key
 * with an LDS histogram of the keys' top 12 bits and either sorts the at most 4096 keys from that bin upwards or, in a crowded bin,
 * finds the k-th key with two more histograms (10 + 10 bits) and collects the larger keys and the ties in index order; then it
 * decodes.  No float atomics, no global atomics, no workgroup waits for another: bit-identical from run to run and on any stream. */
size_t fv2p_center_peaks_ws_bytes(int batch, int nc, int h, int w);
int fv2p_center_peaks(const float* hm, const float* offset, const float* height, const float* dim, const float* rot, const float* iouscore,
                      int batch, int nc, int h, int w, int k, int maxpool, int bins, int stride, float voxel_x, float voxel_y, float range_x0,
                      float range_y0, float* boxes, float* cls, float* score, int64_t* cell, int* cls_id, void* ws, size_t ws_bytes,
                      fv2p_stream_t stream);

/* fv2p_detections_fgscore replaces the single-class-NMS branch of Detector3DTemplate.post_processing_withfgscores
 * (pcdet/models/detectors/detector3d_template.py:318-431, the branch :392-415) with
 * model_nms_utils.class_agnostic_nms_withfgscore (pcdet/models/model_utils/model_nms_utils.py:27-50) for a whole batch, without
 * nonzero() / topk / one host synchronisation per sample.  boxes [B,n,7], cls [B,n,nc], loc_score [B,n], fp32.  Per sample:
 * fg = max over c of cls (of 1 / (1 + exp(-cls)) when normalized == 0), label = first maximal class + 1; candidates with
 * fg >= score_thresh, ordered by descending loc_score (ties, -0.0f equal to 0.0f, by ascending candidate index - where
 * loc scores repeat torch.topk promises nothing and this rule is the op's definition), cut at pre_max; rotated NMS at nms_thresh
 * (fv2p_nms_batch: rejected candidates are ordered last as zero-sized boxes far outside the scene, whose IoU with anything is 0), the
 * first post_max survivors.  out_boxes [B,post_max,7], out_scores [B,post_max] = raw loc_score (src_box_scores[selected]),
 * out_labels [B,post_max] i32, out_index [B,post_max] i64 = index into the n candidates, count [B] i32 on the device; rows past
 * count are zero with out_index -1.  1 <= n <= 4096, 1 <= post_max <= n, pre_max >= 1, nc >= 1, batch >= 1 (FV2P_EINVAL); batch <= 65535
 * (FV2P_ELIMIT).  One ordering-and-gather launch, fv2p_nms_batch (two memsets, then a mask and a greedy launch per chunk of row blocks; one
 * chunk where min(n, pre_max) <= 2 * post_max), one output launch; the number does not depend on the batch. */
size_t fv2p_detections_fgscore_ws_bytes(int batch, int n, int pre_max, int post_max);
int fv2p_detections_fgscore(const float* boxes, const float* cls, const float* loc_score, int batch, int n, int nc, int normalized,
                            float score_thresh, float nms_thresh, int pre_max, int post_max, float* out_boxes, float* out_scores,
                            int* out_labels, int64_t* out_index, int* count, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- (f).4: second-stage target sampling --------------------------------------------------------
 * Replaces ProposalTargetLayer.sample_rois_for_rcnn / subsample_rois
 * (pcdet/models/roi_heads/target_assigner/proposal_target_layer.py:92-217; thresholds of ROI_HEAD.TARGET_CONFIG) for a whole
 * batch in one launch, without nonzero() / .item() round trips.  iou (B,R,G): 3-D IoU of every RoI with every (zero padded)
 * ground-truth box; rois (B,R,7); gt (B,G,gt_w); uniforms (B,R+n) in [0,1): the first R order the foreground set (random
 * permutation), the last n pick with replacement.  Per sample: best box per RoI (first maximum), foreground = overlap >=
 * fg_thresh, hard background = [bg_lo, reg_fg), easy = < bg_lo; min(foreground, fg_quota) foreground RoIs in permuted order
 * (all n picked with replacement when there is no background), the rest hard (floor(rest * hard_ratio), capped) then easy
 * background, with replacement.  Outputs s_rois (B,n,7), s_gt (B,n,gt_w), s_iou (B,n), s_index (B,n) i32. */
int fv2p_roi_sample_targets(const float* iou, const float* rois, const float* gt, const float* uniforms, int batch, int r, int g, int n,
                            int gt_w, float fg_thresh, float bg_lo, float reg_fg, int fg_quota, float hard_ratio, float* s_rois,
                            float* s_gt, float* s_iou, int* s_index, fv2p_stream_t stream);

/* First-stage target assignment for a batch (AxisAlignedTargetAssigner.assign_targets_single,
 * pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:66-210, one class): anchor_bev [A,4] and gt_bev
 * [B,G,4] are the nearest-BEV footprints (x0,y0,x1,y1) of anchors [A,7] and gt [B,G,gt_w] (class id at [7], zero rows = padding).
 * labels [B,A] i32: the best box's class where its overlap >= matched_thr or the anchor attains a box's non-zero maximum, 0 below
 * unmatched_thr, -1 in between; reg [B,A,7]: ResidualCoder target of the positive anchors, zero elsewhere. */
size_t fv2p_anchor_assign_ws_bytes(int batch, int g);
int fv2p_anchor_assign(const float* anchor_bev, const float* anchors, int n_anchor, const float* gt_bev, const float* gt, int batch, int g,
                       int gt_w, float matched_thr, float unmatched_thr, int* labels, float* reg, void* ws, size_t ws_bytes,
                       fv2p_stream_t stream);

/* First-stage losses of a batch in one pass (AnchorHeadTemplate.get_cls_layer_loss / get_box_reg_layer_loss,
 * pcdet/models/dense_heads/anchor_head_template.py:98-206; SigmoidFocalClassificationLoss with gamma = 2, WeightedSmoothL1Loss on
 * the sin-difference encoded residuals, two direction bins): cls [B,A,1], box [B,A,7], dirs [B,A,2] logits, labels [B,A] i32 and
 * reg_t [B,A,7] from fv2p_anchor_assign, anchor_rot [A].  loss4 = {total, cls, loc, dir} (already weighted and divided by B);
 * dcls / dbox / ddirs = d total / d logits. */
size_t fv2p_anchor_loss_ws_bytes(int batch, int n_anchor);
int fv2p_anchor_loss(const float* cls, const float* box, const float* dirs, const int* labels, const float* reg_t, const float* anchor_rot,
                     int batch, int n_anchor, float alpha, float beta, float dir_offset, float w_cls, float w_loc, float w_dir, float* loss4,
                     float* dcls, float* dbox, float* ddirs, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* Second-stage losses in one launch (RoIWithIoUHeadTemplate.get_box_cls_layer_loss / get_box_reg_layer_loss /
 * get_box_iouscore_layer_loss, pcdet/models/roi_heads/roi_withiou_head_template.py:133-265, CLS_SCORE_TYPE roi_iou), the canonical
 * targets of assign_targets (:103-135) formed inside: rois [R,7] and gt [R,gt_w] (gt_w >= 7) are the sampled RoIs and their boxes,
 * iou [R], cls [R] logits, reg [R,8] = [iou score, 7 residuals].  soft_span = cls_fg - cls_bg; iou_label_thr =
 * (reg_fg - 0.5) * 2, the threshold of the IoU-score head on the label (iou - 0.5) * 2; beta of the regression smooth-L1.
 * loss5 = {total, cls, reg, corner, iou}; dcls [R] and dreg [R,8] = d total / d logits; canonical [R,7] (may be null) = the
 * canonical box of every roi.  One workgroup, sums in double in a
 * fixed order; no workspace. */
int fv2p_roi_loss(const float* rois, const float* gt, const float* iou, const float* cls, const float* reg, int r, int gt_w, float cls_fg,
                  float cls_bg, float soft_span, float reg_fg, float iou_label_thr, float beta, float* loss5, float* dcls, float* dreg,
                  float* canonical, fv2p_stream_t stream);

/* Point-head foreground loss (PointHeadSimple, point_head_template.py:47-142): sigmoid focal loss (gamma 2) of logits [N] against
 * labels [N] i64 in {-1 ignored, 0, 1}, weight 1 / max(#positive, 1) per counted point, times `weight`.  loss [1], dlogits [N] =
 * d loss / d logits, score [N] = sigmoid(logits). */
size_t fv2p_point_loss_ws_bytes(int n);
int fv2p_point_loss(const float* logits, const int64_t* labels, int n, float alpha, float weight, float* loss, float* dlogits, float* score,
                    void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* RoI grid geometry in one launch (iouguided_roi_head.py:195-220, feature_adaptor/nn_modules.py:6-60): rois [R,7] -> local [R,g^3,3]
 * grid points in the roi's frame (x slowest), column [R,g^2,3] world position of the lowest grid point of every (x, y) column,
 * corners [R,8,3] half extents in boxes_to_corners_3d order. */
int fv2p_roi_grid(const float* rois, int r, int g, float* local, float* column, float* corners, fv2p_stream_t stream);

/* ---- A15 / A18: point-in-box, RoI-aware voxel pooling, RoI point pooling ------------------------
 * Replace roiaware_pool3d_cuda.{points_in_boxes_gpu, points_in_boxes_cpu, forward, backward}
 * (pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:29-177, kernels roiaware_pool3d_kernel.cu:16-359) and
 * roipoint_pool3d_cuda.forward (pcdet/ops/roipoint_pool3d/src/roipoint_pool3d.cpp:22-56, kernels
 * roipoint_pool3d_kernel.cu:16-165).  boxes: [x,y,z,dx,dy,dz,heading]; MARGIN 1e-5 on the GPU paths, 1e-2 in the
 * host path, as in the reference.
 *   points_in_boxes      boxes (B,T,7), pts (B,M,3) -> box_idx_of_points (B,M): first containing box or -1
 *   points_in_boxes_cpu  host pointers; boxes (N,7), pts (M,3) -> pts_indices (N,M) 0/1
 *   roipoint_pool3d      xyz (B,N,3), boxes3d (B,M,7), pts_feature (B,N,C) -> pooled (B,M,S,3+C) = the first S
 *                        inside points in index order, wrapped when fewer; pooled_empty_flag (B,M)
 *   roiaware_pool3d_fwd  rois (R,7), pts (P,3), pts_feature (P,C) -> pts_idx_of_voxels (R,ox,oy,oz,max_pts)
 *                        [slot 0 = count], argmax (R,ox,oy,oz,C), pooled (R,ox,oy,oz,C); pool_method 0 max / 1 avg
 *   roiaware_pool3d_bwd  grad_in (P,C) must be zeroed by the caller (roiaware_pool3d_utils.py:104), accumulated.
 */
int fv2p_points_in_boxes(const float* boxes, const float* pts, int batch, int boxes_num, int pts_num,
                         int* box_idx_of_points, fv2p_stream_t stream);
int fv2p_points_in_boxes_cpu(const float* boxes, const float* pts, int boxes_num, int pts_num, int* pts_indices);
int fv2p_roipoint_pool3d(const float* xyz, const float* boxes3d, const float* pts_feature, int batch, int pts_num,
                         int boxes_num, int feature_len, int sampled_pts_num, float* pooled_features,
                         int* pooled_empty_flag, fv2p_stream_t stream);
/* roipoint_pool3d with the rows already in the RoI's frame (IoUGuidedRoIHead.roipool3d_gpu, iouguided_roi_head.py:144-195): the
 * same selection on boxes3d (B,M,7, the enlarged boxes), rows [x', y', z', score, depth, features...] (B,M,S,5+C) with
 * (x', y', z') = the point minus the centre of rois (B,M,7, the original boxes) rotated by -heading, score from pts_score (B,N),
 * depth = |point| / depth_normalizer - 0.5.  Empty boxes pool zeros. */
int fv2p_roipoint_pool3d_frame(const float* xyz, const float* pts_score, const float* pts_feature, const float* boxes3d,
                               const float* rois, int batch, int pts_num, int boxes_num, int feature_len, int sampled_pts_num,
                               float depth_normalizer, float* pooled_features, int* pooled_empty_flag, fv2p_stream_t stream);
int fv2p_roiaware_pool3d_fwd(const float* rois, const float* pts, const float* pts_feature, int boxes_num,
                             int pts_num, int channels, int max_pts_each_voxel, int out_x, int out_y, int out_z,
                             int pool_method, int* argmax, int* pts_idx_of_voxels, float* pooled_features,
                             fv2p_stream_t stream);
int fv2p_roiaware_pool3d_bwd(const int* pts_idx_of_voxels, const int* argmax, const float* grad_out, int boxes_num,
                             int out_x, int out_y, int out_z, int channels, int max_pts_each_voxel, int pool_method,
                             float* grad_in, fv2p_stream_t stream);
/* roiaware_pool3d_bwd in the fixed order of fv2p_scatter_add; pts_num = rows of grad_in (P), which is written, not accumulated */
size_t fv2p_roiaware_pool3d_bwd_ws_bytes(int boxes_num, int out_x, int out_y, int out_z, int channels, int max_pts_each_voxel,
                                         int pool_method);
int fv2p_roiaware_pool3d_bwd_gather(const int* pts_idx_of_voxels, const int* argmax, const float* grad_out, int boxes_num,
                                    int out_x, int out_y, int out_z, int channels, int max_pts_each_voxel, int pool_method,
                                    int pts_num, float* grad_in, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- A8-A12: pointnet2 (batch and stacked layouts) ------------------------------------------------
 * Replace pointnet2_batch_cuda.* (pcdet/ops/pointnet2/pointnet2_batch/src/pointnet2_api.cpp:10-24) and
 * pointnet2_stack_cuda.* (pcdet/ops/pointnet2/pointnet2_stack/src/pointnet2_api.cpp:11-23).  Argument order and
 * meaning follow the reference wrappers (ints first, then tensors); outputs are caller-allocated.
 *  batch layouts : xyz (B,N,3), features channel-major (B,C,N), idx (B,M,nsample) / (B,M) / (B,N,3)
 *  stack layouts : rows of all samples concatenated, per-sample row counts in *_batch_cnt (int32 [B], device)
 * ball_query      first `nsample` points with d2 <  r^2 in index order, padded with the first hit
 *                 (ball_query_gpu.cu:15-51; stack: idx[0] = -1 when the ball is empty, :16-66); idx pre-zeroed by caller
 * voxel_query     (2r+1)^3 neighbourhood of a dense (B,Z,Y,X) int volume, d2 <= r^2 (voxel_query_gpu.cu:10-89)
 * furthest_point_sampling  temp (B,N) must hold 1e10 (pointnet2_utils.py:26); first index 0; ties as the reference's
 *                 strided tree reduction (sampling_gpu.cu:93-216); temp holds the final distances on return
 * three_nn        3 smallest squared distances (strict <, lowest index wins) + indices (stack: global rows)
 * *_grad          accumulate into grad buffers the caller zeroed (atomic adds, as the reference)
 */
int fv2p_ball_query_batch(int b, int n, int m, float radius, int nsample, const float* new_xyz, const float* xyz,
                          int* idx, fv2p_stream_t stream);
int fv2p_ball_query_stack(int b, int m, float radius, int nsample, const float* new_xyz,
                          const int* new_xyz_batch_cnt, const float* xyz, const int* xyz_batch_cnt, int* idx,
                          fv2p_stream_t stream);
int fv2p_voxel_query_stack(int m, int r1, int r2, int r3, int nsample, float radius, int z_range, int y_range,
                           int x_range, const float* new_xyz, const float* xyz, const int* new_coords,
                           const int* point_indices, int* idx, fv2p_stream_t stream);
int fv2p_group_points_batch(int b, int c, int n, int npoints, int nsample, const float* points, const int* idx,
                            float* out, fv2p_stream_t stream);
int fv2p_group_points_batch_grad(int b, int c, int n, int npoints, int nsample, const float* grad_out,
                                 const int* idx, float* grad_points, fv2p_stream_t stream);
int fv2p_gather_points(int b, int c, int n, int npoints, const float* points, const int* idx, float* out,
                       fv2p_stream_t stream);
int fv2p_gather_points_grad(int b, int c, int n, int npoints, const float* grad_out, const int* idx,
                            float* grad_points, fv2p_stream_t stream);
int fv2p_group_points_stack(int b, int m, int c, int nsample, const float* features,
                            const int* features_batch_cnt, const int* idx, const int* idx_batch_cnt, float* out,
                            fv2p_stream_t stream);
int fv2p_group_points_stack_grad(int b, int m, int c, int n, int nsample, const float* grad_out, const int* idx,
                                 const int* idx_batch_cnt, const int* features_batch_cnt, float* grad_features,
                                 fv2p_stream_t stream);
/* ws / ws_bytes (fv2p_furthest_point_sampling_ws_bytes, may be NULL): scratch of the bucketed kernel — Morton-sorted
 * point order, per-bucket boxes; with it 2048 <= n <= 16384, m >= 1024 run the lazy variant, whose indices and final
 * `temp` are bit-identical to the plain kernel's (and the reference's, sampling_gpu.cu:100-216). */
size_t fv2p_furthest_point_sampling_ws_bytes(int b, int n);
int fv2p_furthest_point_sampling(int b, int n, int m, const float* dataset, float* temp, int* idxs, void* ws,
                                 size_t ws_bytes, fv2p_stream_t stream);
/* The same sampler on a STACKED batch of unequal clouds, in one call: replaces the reference decoder's per-sample loop
 * (residual_v2p_decoder.py:210-232, voxel_set_abstraction.py:139), which runs B single-cloud calls one after the other.
 *  dataset (N_1 + ... + N_B, 3): the samples' rows concatenated; temp (N_1 + ... + N_B) holds 1e10 on entry and the final
 *  running distances on return; idxs (B, m) int32, rows LOCAL to the sample, each row bit-identical to what
 *  fv2p_furthest_point_sampling gives for that cloud alone with the same m (N_i < m is legal: the caller repairs the
 *  tail, residual_v2p_decoder.py:220-222).  Every N_i >= 1, the total at most INT_MAX rows.
 *  cnt_host: the B counts in HOST memory (the planner reads them: kernel form, register slots, workspace carving);
 *  cnt_dev: the same counts as int32 in device memory, as every other stack op takes them.  The call neither synchronises
 *  the stream nor copies from host memory on it.
 * Every sample runs on the form its own count selects (plain, register-bucket, streaming: as the equal-size call would choose
 * for that cloud alone), one workgroup per sample; the forms present are launched once each, one after the other on `stream`,
 * so a batch whose clouds share a form is ONE sampler launch (the register-bucket form with the slot count of its largest
 * cloud).  ws / ws_bytes as above (fv2p_furthest_point_sampling_stack_ws_bytes, a pure host function; NULL or too small: the
 * plain kernel for every sample). */
size_t fv2p_furthest_point_sampling_stack_ws_bytes(int b, const int* cnt_host);
int fv2p_furthest_point_sampling_stack(int b, const int* cnt_host, const int* cnt_dev, int m, const float* dataset,
                                       float* temp, int* idxs, void* ws, size_t ws_bytes, fv2p_stream_t stream);
/* Profiling hook of the streaming sampler (n > 24 576): when non-NULL (device memory, 16 x 8 entries), sample 0 writes
 * trace[8 * wave + {0..7}] = shader clocks spent in {box test, issuing the loads of a pass over the touched buckets, the first
 * bucket of a pass (wait + distance pass + reduction), the pass's other buckets, wave arg-max, candidate exchange + barrier,
 * winner selection}, the touched buckets summed over the rounds.  NULL switches it off. */
int fv2p_fps_set_trace(unsigned long long* trace);
int fv2p_three_nn_batch(int b, int n, int m, const float* unknown, const float* known, float* dist2, int* idx,
                        fv2p_stream_t stream);
int fv2p_three_nn_stack(int b, int n, int m, const float* unknown, const int* unknown_batch_cnt,
                        const float* known, const int* known_batch_cnt, float* dist2, int* idx,
                        fv2p_stream_t stream);
/* fv2p_three_nn_stack through a hashed uniform grid over the known points (2 table slots per point): the same idx / dist2, bit
 * for bit.  Every distance is the scan's float expression, the three best are kept under the (distance, index) order = "strict <
 * over ascending index", and a query is settled by the 27 cells around its own only when every point outside them is provably
 * farther than its third best; the other queries scan their sample, one wave each.  Time goes with the points near each query
 * instead of all of them.  cell: grid spacing in the points' unit (e.g. two voxel pitches of the level the known points are
 * centres of); <= 0 lets the library estimate one.  n = queries, m = known points.  The reference has no counterpart
 * (interpolate_gpu.cu:16-73 scans). */
size_t fv2p_three_nn_grid_ws_bytes(int b, int64_t n, int64_t m);
int fv2p_three_nn_stack_grid(int b, int n, int m, const float* unknown, const int* unknown_batch_cnt,
                             const float* known, const int* known_batch_cnt, float cell, float* dist2, int* idx,
                             void* ws, size_t ws_bytes, fv2p_stream_t stream);
int fv2p_three_interpolate_batch(int b, int c, int m, int n, const float* points, const int* idx,
                                 const float* weight, float* out, fv2p_stream_t stream);
int fv2p_three_interpolate_batch_grad(int b, int c, int n, int m, const float* grad_out, const int* idx,
                                      const float* weight, float* grad_points, fv2p_stream_t stream);
int fv2p_three_interpolate_stack(int n, int c, const float* features, const int* idx, const float* weight,
                                 float* out, fv2p_stream_t stream);
int fv2p_three_interpolate_stack_grad(int n, int c, const float* grad_out, const int* idx, const float* weight,
                                      float* grad_features, fv2p_stream_t stream);
/* The same gradient without float atomics, without the caller's zero fill and in a FIXED order: the entries e = 3 * query + slot of
 * idx [n, 3] are keyed (known row, e) and radix-sorted in the workspace; the sorted sequence is summed in segments of 32 entries (a lane
 * group each, one lane = four channels), runs that cross segment borders are closed from the segments' partial sums in segment order.
 * Bit-identical from run to run; values equal fv2p_three_interpolate_stack_grad's up to the association of each row's sum (the scatter
 * form adds a row's entries in whatever order its atomics land). */
size_t fv2p_three_interpolate_stack_grad_ws_bytes(int n, int c, int m);
int fv2p_three_interpolate_stack_grad_gather(int n, int c, int m, const float* grad_out, const int* idx, const float* weight,
                                             float* grad_features, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- Deterministic mode: scatter-add in a fixed order, and the backward passes built on it --------------------------------
 * fv2p_scatter_add: for every entry e whose dst_row[e] lies in [0, n_dst),
 *     out[dst_row[e] * c + ch] += coef[e] * src[src_off[e] + ch * src_cs]      (ch < c)
 * coef NULL = 1; src_off NULL = e * c (then src_cs must be 1: src is [entries, c]).  Other entries are dropped.  The association of
 * every sum is a function of the entry list only: the entries of a row are taken in ascending e, at their positions in the (row, e)
 * order of all kept entries; that sequence is cut into segments of 32 positions; the piece of a row inside one segment is summed from
 * zero in order (acc = acc + coef * value, two roundings), the pieces of a row that spans segments are added in segment order (first
 * piece, then the next ones), and the row's total is added to out once.  No float atomics; bit-identical from run to run, whatever the
 * stream or the other work on the device.  entries < 2^31, n_dst < 2^31 - 1.
 * The *_gather backward passes below compute the gradient of the atomic entry point they are named after, in that fixed order, and
 * WRITE their outputs (no zero fill by the caller); index entries outside their range are dropped.  Each needs the workspace of its
 * *_ws_bytes query. */
size_t fv2p_scatter_add_ws_bytes(int64_t entries, int c);
int fv2p_scatter_add(int64_t entries, int c, int64_t n_dst, const int* dst_row, const int64_t* src_off, const float* coef,
                     const float* src, int64_t src_cs, float* out, void* ws, size_t ws_bytes, fv2p_stream_t stream);
size_t fv2p_group_points_batch_grad_ws_bytes(int b, int c, int n, int npoints, int nsample);
int fv2p_group_points_batch_grad_gather(int b, int c, int n, int npoints, int nsample, const float* grad_out, const int* idx,
                                        float* grad_points, void* ws, size_t ws_bytes, fv2p_stream_t stream);
size_t fv2p_gather_points_grad_ws_bytes(int b, int c, int n, int npoints);
int fv2p_gather_points_grad_gather(int b, int c, int n, int npoints, const float* grad_out, const int* idx, float* grad_points,
                                   void* ws, size_t ws_bytes, fv2p_stream_t stream);
size_t fv2p_group_points_stack_grad_ws_bytes(int m, int c, int nsample);
int fv2p_group_points_stack_grad_gather(int b, int m, int c, int n, int nsample, const float* grad_out, const int* idx,
                                        const int* idx_batch_cnt, const int* features_batch_cnt, float* grad_features, void* ws,
                                        size_t ws_bytes, fv2p_stream_t stream);
size_t fv2p_three_interpolate_batch_grad_ws_bytes(int b, int c, int n, int m);
int fv2p_three_interpolate_batch_grad_gather(int b, int c, int n, int m, const float* grad_out, const int* idx, const float* weight,
                                             float* grad_points, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- Stack grouping and interpolation on 16-bit feature rows ----------------------------------------------------------------
 * What GroupingOperation and ThreeInterpolate of pointnet2_stack/pointnet2_utils.py:95-262 (group_points_gpu.cu, interpolate_gpu.cu:
 * float only in the reference) do when the features come from a float16 / bfloat16 backbone.  `dtype` (FV2P_DT_F16 / FV2P_DT_BF16)
 * names the format of the feature, output and gradient rows; idx, the batch counts and the interpolation weight stay int32 / float.
 * Any other dtype, a null pointer or a bad size returns FV2P_EINVAL before anything is launched.  Nothing is converted to fp32 in
 * memory; 8 channels per 16-byte access when c % 8 == 0 and the feature pointers are 16-byte aligned, one element otherwise.
 *   fv2p_group_points_stack_h : features (n, c), idx (m, nsample) sample-local -> out (m, c, nsample), a copy of 16-bit elements;
 *     a row outside [0, n) gives zeros.  m * nsample == 0 returns 0 and launches nothing.
 *   fv2p_three_interpolate_stack_h : features (m, c), idx / weight (n, 3) -> out (n, c) = w0 * f0 + w1 * f1 + w2 * f2 in fp32 in the
 *     order of fv2p_three_interpolate_stack (no contraction), rounded to nearest even once; a row outside [0, m) counts as zeros.
 *   The two gradients exist in the fixed-order form only (the siblings of fv2p_group_points_stack_grad_gather and
 *     fv2p_three_interpolate_stack_grad_gather; there is no atomic form): the 16-bit gradient rows are widened on load and summed in
 *     fp32 in exactly the association of fv2p_scatter_add (entries of a row in ascending e, segments of 32 sorted positions, the
 *     pieces of a row that spans segments added in segment order, products weight * value rounded before they are added), and every
 *     row of grad_features is rounded ONCE.  grad_features is written: rows without entries are zero, entries outside the range are
 *     dropped.  Only the fp32 pieces of rows that span segments live in the workspace (*_ws_bytes), never an fp32 image of a
 *     gradient.  No float atomics; bit-identical from run to run.  Zero feature rows return 0 and launch nothing. */
int fv2p_group_points_stack_h(int b, int m, int c, int n, int nsample, const void* features, const int* features_batch_cnt,
                              const int* idx, const int* idx_batch_cnt, void* out, int dtype, fv2p_stream_t stream);
size_t fv2p_group_points_stack_grad_h_ws_bytes(int m, int c, int nsample);
int fv2p_group_points_stack_grad_h(int b, int m, int c, int n, int nsample, const void* grad_out, const int* idx,
                                   const int* idx_batch_cnt, const int* features_batch_cnt, void* grad_features, int dtype,
                                   void* ws, size_t ws_bytes, fv2p_stream_t stream);
int fv2p_three_interpolate_stack_h(int n, int c, int m, const void* features, const int* idx, const float* weight, void* out,
                                   int dtype, fv2p_stream_t stream);
size_t fv2p_three_interpolate_stack_grad_h_ws_bytes(int n, int c, int m);
int fv2p_three_interpolate_stack_grad_h(int n, int c, int m, const void* grad_out, const int* idx, const float* weight,
                                        void* grad_features, int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- Batch gather, grouping and interpolation on 16-bit feature rows (csrc/pointnet2.hip) -----------------------------------------
 * What GatherOperation, GroupingOperation and ThreeInterpolate of pointnet2_batch/pointnet2_utils.py:46-215 (sampling_gpu.cu:10-98,
 * group_points_gpu.cu, interpolate_gpu.cu:76-160: float only in the reference) do on float16 / bfloat16 features; the PointnetSAModuleMSG
 * of IoUGuidedRoIHead (iouguided_roi_head.py:51-69, 266-278) and PointnetFPModule reach them.  Layouts are the fp32 batch ops':
 * features [B][C][N] channel-major, idx int32, weight fp32.  `dtype` (FV2P_DT_F16 / FV2P_DT_BF16) names the format of the feature,
 * output and gradient elements.  Any other dtype, a null feature / gradient pointer where the sizes are non-zero, or c < 1 returns
 * FV2P_EINVAL before anything is launched; zero-sized calls return 0 without a launch.  Nothing is converted to fp32 in memory.
 *   fv2p_gather_points_h : points (b, c, n), idx (b, npoints) -> out (b, c, npoints);
 *   fv2p_group_points_batch_h : points (b, c, n), idx (b, npoints, nsample) -> out (b, c, npoints, nsample).  Both are copies of 16-bit
 *     elements (one kernel for both formats); an index outside [0, n) gives zeros (the fp32 kernels read it unguarded).
 *   fv2p_three_interpolate_batch_h : points (b, c, m), idx / weight (b, n, 3) -> out (b, c, n) = w0 * f0 + w1 * f1 + w2 * f2 in fp32 on
 *     the widened values, in the order of fv2p_three_interpolate_batch (no contraction), rounded to nearest even once: the bits of the
 *     fp32 op on the widened features, rounded.  A known index outside [0, m) counts as a zero.
 *   8 consecutive outputs of a (b, c) row per 16-byte store (their 8 indices as two 16-byte loads) when the row length (npoints,
 *     npoints * nsample, n) is a multiple of 8 and idx / weight / out are 16-byte aligned; one element at a time otherwise.
 *   The three gradients exist in the fixed-order form only (siblings of the fp32 *_grad_gather entry points; no float atomics): entries
 *     in the order of those entry points, fp32 sums in the association of fv2p_scatter_add, every element of grad_points rounded ONCE -
 *     the bits of the fp32 *_grad_gather result on the widened gradient, rounded.  grad_points is WRITTEN: elements no entry reaches are
 *     zero, entries whose index is out of range are dropped.  The workspace (*_ws_bytes, pure host functions) holds the entry lists and
 *     a 16-bit [b * rows][c] staging image that one 16-bit transpose moves into grad_points, never an fp32 image of the gradient.
 *     FV2P_EWORKSPACE for a workspace that is too small, FV2P_ELIMIT from 2^31 entries or 2^30 rows on. */
int fv2p_gather_points_h(int b, int c, int n, int npoints, const void* points, const int* idx, void* out, int dtype,
                         fv2p_stream_t stream);
size_t fv2p_gather_points_grad_h_ws_bytes(int b, int c, int n, int npoints);
int fv2p_gather_points_grad_h(int b, int c, int n, int npoints, const void* grad_out, const int* idx, void* grad_points, int dtype,
                              void* ws, size_t ws_bytes, fv2p_stream_t stream);
int fv2p_group_points_batch_h(int b, int c, int n, int npoints, int nsample, const void* points, const int* idx, void* out,
                              int dtype, fv2p_stream_t stream);
size_t fv2p_group_points_batch_grad_h_ws_bytes(int b, int c, int n, int npoints, int nsample);
int fv2p_group_points_batch_grad_h(int b, int c, int n, int npoints, int nsample, const void* grad_out, const int* idx,
                                   void* grad_points, int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream);
int fv2p_three_interpolate_batch_h(int b, int c, int m, int n, const void* points, const int* idx, const float* weight, void* out,
                                   int dtype, fv2p_stream_t stream);
size_t fv2p_three_interpolate_batch_grad_h_ws_bytes(int b, int c, int n, int m);
int fv2p_three_interpolate_batch_grad_h(int b, int c, int n, int m, const void* grad_out, const int* idx, const float* weight,
                                        void* grad_points, int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- A11 consumer: fused grid set-abstraction (gather -> shared-MLP layer -> max over the samples) ---------------------
 * The part of PointnetSAModuleMSG.forward (pointnet2_batch/pointnet2_modules.py:30-62) that follows the ball query, for the
 * bn=False module of IoUGuidedRoIHead (iouguided_roi_head.py:52-76) after its first, linear layer has been applied per point
 * and per centre:  out[r, i, :] = max_s relu(W2 relu(per_point[r, idx[r, i, s], :] - per_centre[r, i, :])).
 * per_point [rois, n, c], per_centre [rois, m, c], idx [rois, m, s] i32 (ball query output), w2 [c, c] (Conv2d weight),
 * out / grad_out [rois, m, c]; c = 64, s in {16, 32}.  No grouped tensor exists in either direction.
 * arg [rois, m, c] u8 (forward: optional, may be NULL for inference; backward: required): the sample 0 .. s-1 that attained the
 * maximum of (centre, channel) — the first one in sample order, which is where F.max_pool2d sends the gradient
 * (pointnet2_modules.py:57-59) — or 255 where the maximum is 0 (ReLU inactive for every sample: no gradient).  Backward
 * recomputes relu(per_point - per_centre) only. */
int fv2p_sa_grid_supported(int n, int m, int s, int c);
int fv2p_sa_grid_fwd(const float* per_point, const float* per_centre, const int* idx, const float* w2, int rois, int n, int m,
                     int s, int c, float* out, unsigned char* arg, fv2p_stream_t stream);
size_t fv2p_sa_grid_bwd_ws_bytes(int rois);
int fv2p_sa_grid_bwd(const float* per_point, const float* per_centre, const int* idx, const float* w2, const unsigned char* arg,
                     const float* grad_out, int rois, int n, int m, int s, int c, float* grad_point, float* grad_centre,
                     float* grad_w2, void* ws, size_t ws_bytes, fv2p_stream_t stream);
/* The same backward with the per-point gradient in the fixed order of fv2p_scatter_add: every (RoI, centre, sample) row of dh1 is
 * written out and summed into its point's row (no LDS atomics); dW2, grad_centre and the arg-max routing are fv2p_sa_grid_bwd's. */
size_t fv2p_sa_grid_bwd_gather_ws_bytes(int rois, int m, int s);
int fv2p_sa_grid_bwd_gather(const float* per_point, const float* per_centre, const int* idx, const float* w2, const unsigned char* arg,
                            const float* grad_out, int rois, int n, int m, int s, int c, float* grad_point, float* grad_centre,
                            float* grad_w2, void* ws, size_t ws_bytes, fv2p_stream_t stream);
/* The fused grid set-abstraction on float16 / bfloat16 rows (csrc/sa_fused.hip; dtype = FV2P_DT_F16 / FV2P_DT_BF16): per_point,
 * per_centre, out, grad_out and the row gradients are 16-bit elements of that one format, idx / arg as above.  w2 [c, c] is in the rows'
 * format (wd != 0: wd == dtype) or fp32 (wd == 0, the convention of `pd` above: the master weight beside autocast rows); an fp32 w2 is
 * rounded to nearest even on its way into LDS - the result has the bits of the call on w2.to(dtype), no 16-bit copy is made - and
 * grad_w2 has w2's format.  No fp32 image of a row tensor exists anywhere.
 *   forward : h1 = RNE(max(float(P) - float(Q), 0)) is the operand of v_mfma_f32_16x16x32_{f16,bf16}; the maximum over the samples is
 *     taken over the fp32 accumulators and rounded ONCE at the store; arg is fv2p_sa_grid_fwd's (first sample in sample order whose
 *     accumulator equals the maximum, 255 where the maximum is 0).
 *   backward: h1 recomputed as in forward, dh1 = (W2r^T dh2) [h1 > 0] in fp32 accumulators; grad_centre = -sum_s dh1 rounded once;
 *     grad_point in the fixed-order form only (no atomic form exists, the deterministic switch changes nothing): the dh1 rows are staged
 *     in the workspace IN 16 BITS (one rounding per addend) and summed per point in fp32 - in ascending sample order inside one workgroup
 *     per RoI up to m * s = 8192, in the association of fv2p_scatter_add beyond - the total rounded once; grad_point is WRITTEN (rows no sample names are zero); grad_w2 from fp32 partial tiles folded in a fixed order, one rounding
 *     for a 16-bit w2, none for fp32.  All results are bit-identical from run to run and on any stream.
 *   An index outside [0, n) reads as a row of zeros and its grad_point entry is dropped; it is never dereferenced.
 *   c = 64, s in {16, 32}, any n (there is no dP tile in LDS: the fp32 backward's n <= 884 does not apply), rois <= 65535; every pointer
 *   16-byte aligned.  FV2P_EINVAL before any launch for another dtype or wd, a null pointer, an unsupported shape or alignment;
 *   FV2P_EWORKSPACE for a workspace below fv2p_sa_grid_bwd_h_ws_bytes (a pure host function: the partial tiles, the entry list, the 16-bit
 *   dh1 rows [rois * m * s][64] and the workspace of the scatter-add); FV2P_ELIMIT from 2^31 samples or point rows on. */
int fv2p_sa_grid_supported_h(int n, int m, int s, int c);
int fv2p_sa_grid_fwd_h(const void* per_point, const void* per_centre, const int* idx, const void* w2, int wd, int rois, int n, int m,
                       int s, int c, void* out, unsigned char* arg, int dtype, fv2p_stream_t stream);
size_t fv2p_sa_grid_bwd_h_ws_bytes(int rois, int m, int s);
int fv2p_sa_grid_bwd_h(const void* per_point, const void* per_centre, const int* idx, const void* w2, int wd, const unsigned char* arg,
                       const void* grad_out, int rois, int n, int m, int s, int c, void* grad_point, void* grad_centre, void* grad_w2,
                       int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- A13: modulated deformable convolution (DCNv2; DCNv1 = mask of ones) -------------------------
 * Replace DCN.modulated_deform_conv_forward / _backward and DCN.deform_conv_forward / _backward
 * (pcdet/ops/DeformableConvolutionV2PyTorch/src/vision.cpp:6-12 -> src/modulated_deform_conv.h:10-86 ->
 * src/cuda/modulated_deform_conv_cuda.cu:19-280, kernels src/cuda/modulated_deform_im2col_cuda.cuh:24-328).
 * Forward: fused implicit GEMM, no `columns` buffer.  Backward: the column GRADIENTS do pass through the workspace (below), at
 * most 1.5 GiB of them at a time.  Activations are NHWC on this side of the boundary:
 *   x_nhwc [B,H,W,Cin], y_nhwc / dy_nhwc [B*Ho*Wo, Cout]; the weight [Cout,Cin,kh,kw] arrives permuted: forward takes
 *   wt_oc = [kh*kw][Cout][Cin] (input channels contiguous), backward wt = [kh*kw][Cin][Cout] (output channels contiguous);
 *   offset [B, dg*2*kh*kw, Ho, Wo] ((2k, 2k+1) = (dh, dw)), mask [B, dg*kh*kw, Ho, Wo] — reference layouts.
 * fv2p_dcn_forward / fv2p_dcn_backward: groups == 1, Cin / deformable_group a multiple of 16, Cout <= 256 (backward: Cout a
 * multiple of 4).  The *_grouped entry points further below take conv groups and any Cout.
 * backward (modulated_deform_conv_cuda.cu:127-280): dx_nhwc, doffset, dmask, dwt are FULLY written, nothing to zero
 * (dwt [kh*kw][Cin][Cout]; the bias gradient is a plain column sum done by the caller).  No float atomics: the column
 * gradients go through the workspace ([B*Ho*Wo][kh*kw][Cin], the reference's `columns`), every input pixel then sums the
 * samples that touch it in ascending sample order (lists built with integer atomics), so all four gradients are
 * bit-identical from run to run (lists above 4096 samples on ONE input pixel keep an arbitrary order).
 * Any batch: both entry points cut the call into chunks of whole samples (the reference's im2col_step loop,
 * modulated_deform_conv_cuda.cu:85-118) so that x, y, offset and the column gradients of a chunk stay below the kernels' 32-bit
 * limits and the column gradients below 1.5 GiB; fv2p_dcn_backward_ws_bytes is the workspace of ONE chunk.  dx, doffset, dmask
 * are per sample (identical for every chunking); dwt adds the chunks in ascending order (fixed, run-to-run identical).  Only a
 * single sample above a limit is refused (FV2P_ELIMIT).
 */
int fv2p_dcn_forward(const float* x_nhwc, const float* wt_oc, const float* bias, const float* offset,
                     const float* mask, int batch, int height, int width, int c_in, int c_out, int h_out,
                     int w_out, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                     int deformable_group, float* y_nhwc, fv2p_stream_t stream);
/* Step order of the forward kernel: 0 = (tap, group, 16-channel chunk) - rounds 4 / 5 -, 1 = (group, chunk, tap): the nine taps of a chunk
 * back to back (the chunk's 64-byte segments stay in L1 / L2 across the taps), -1 = the library's choice.  Results are identical
 * term by term only within one order (the sum over (tap, channel) terms is taken in step order); both are within 1e-4 of the oracle. */
int fv2p_dcn_set_forward_order(int order);
/* Test hook: the cap on a chunk's column gradients in bytes (0 = back to the 1.5 GiB default). */
int fv2p_dcn_set_colg_cap(int64_t bytes);
size_t fv2p_dcn_backward_ws_bytes(int batch, int height, int width, int h_out, int w_out, int c_in, int c_out, int kh,
                                  int kw, int deformable_group);
int fv2p_dcn_backward(const float* x_nhwc, const float* wt, const float* offset, const float* mask,
                      const float* dy_nhwc, int batch, int height, int width, int c_in, int c_out, int h_out,
                      int w_out, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                      int deformable_group, float* dx_nhwc, float* doffset, float* dmask, float* dwt, void* ws,
                      size_t ws_bytes, fv2p_stream_t stream);
/* The same operator with `group` conv groups (modulated_deform_conv_cuda.cu:62-113, 171-280: the reference's per-group GEMMs) and any
 * number of output channels.  Input channel c belongs to conv group c / (Cin/G) and samples with the offsets and mask of deformable
 * group c / (Cin/dg); output channel o belongs to conv group o / (Cout/G) and sums over its group's Cin/G input channels only.
 * G divides Cin and Cout, dg divides Cin; Cin/G and Cin/dg must be multiples of 16 (FV2P_ELIMIT otherwise): the caller zero-pads the
 * input channels, in pieces gcd(Cin/G, Cin/dg) wide each padded to a multiple of 16, in x and in the weight's input-channel axis -
 * zero channels add nothing to y, doffset or dmask (pcdet DCN.py does this and slices dx and dwt back).  With group = 1 and a geometry
 * fv2p_dcn_forward / _backward take, both launch the same kernels with the same grids and give the same bits.
 *   forward:  wt_oc = [kh*kw][Cout][Cin/G]: wt_oc[k][o][c] = W[o, c, k] (c within o's group).  Any Cout / G: a workgroup's columns
 *             stay inside one group, in column blocks of at most 256.
 *   backward: wt = [kh*kw][Cin][Cout/G]: wt[k][g*Cin/G + c][o] = W[g*Cout/G + o, c, k]; dwt has the same layout.  Cout / G must be a
 *             multiple of 4 (the caller pads each group's output columns with zeros, in dy and wt, and slices dwt back).  Column
 *             gradients of groups wider than 256 output channels are formed in slices of 256 added in ascending order, and a
 *             deformable group that spans conv groups gets its grad_offset / grad_mask from the groups in ascending order: still no
 *             float atomics, still bit-identical from run to run.  Batch chunking and the workspace rule are those above;
 *             fv2p_dcn_backward_grouped_ws_bytes is the workspace of one chunk. */
int fv2p_dcn_forward_grouped(const float* x_nhwc, const float* wt_oc, const float* bias, const float* offset,
                             const float* mask, int batch, int height, int width, int c_in, int c_out, int h_out,
                             int w_out, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                             int deformable_group, int group, float* y_nhwc, fv2p_stream_t stream);
size_t fv2p_dcn_backward_grouped_ws_bytes(int batch, int height, int width, int h_out, int w_out, int c_in, int c_out, int kh,
                                          int kw, int deformable_group, int group);
int fv2p_dcn_backward_grouped(const float* x_nhwc, const float* wt, const float* offset, const float* mask,
                              const float* dy_nhwc, int batch, int height, int width, int c_in, int c_out, int h_out,
                              int w_out, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                              int deformable_group, int group, float* dx_nhwc, float* doffset, float* dmask, float* dwt,
                              void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* The forward on float16 / bfloat16 maps (csrc/dcn_h.hip): the same implicit GEMM on v_mfma_f32_16x16x32_{f16,bf16}, no fp32 copy of
 * any map.  `dtype` (FV2P_DT_F16 / FV2P_DT_BF16) names the format of x_nhwc [B,H,W,Cin], wt_oc [kh*kw][Cout][Cin] and y_nhwc
 * [B*Ho*Wo][Cout]; bias stays fp32 (Cout floats, may be null); offset and mask, in the reference layouts, are fp32 (om_dtype 0) or in
 * the call's format (om_dtype == dtype) and are widened on load, positions are always formed in fp32.  The dtype / om_dtype checks come
 * first: any other value returns FV2P_EINVAL before any HIP call.  Arithmetic: a sample is w0 v0 + w1 v1 + w2 v2 + w3 v3 of the
 * widened corner values in fp32 (the fp32 kernel's fmaf chain), times the mask, rounded to nearest even once into the MFMA operand;
 * fp32 accumulators in the fixed step order (tap, deformable group, 32-channel chunk); bias added in fp32; one rounding at the store.
 * No atomics: two runs give the same bits.  Geometry: groups == 1, Cin / deformable_group a multiple of 16 (a group 16 mod 32 wide
 * ends in a 32-step whose upper half is zero in both operands), any Cout >= 1, any stride / padding / dilation / kernel size of
 * fv2p_dcn_forward; FV2P_ELIMIT otherwise - fv2p_dcn_forward_h_supported (pure host, no HIP call) answers 1 / 0 for it.  x_nhwc and
 * wt_oc must be 16-byte aligned.  Nothing outside x, wt_oc, offset or mask is read.  Batches are cut into chunks of whole samples
 * as above; a zero-sized call returns 0 without a launch; the work runs on `stream`, takes no workspace and allocates nothing. */
int fv2p_dcn_forward_h(const void* x_nhwc, const void* wt_oc, const float* bias, const void* offset, const void* mask,
                       int batch, int height, int width, int c_in, int c_out, int h_out, int w_out, int kh, int kw,
                       int sh, int sw, int ph, int pw, int dh, int dw, int deformable_group,
                       void* y_nhwc, int dtype, int om_dtype, fv2p_stream_t stream);
int fv2p_dcn_forward_h_supported(int c_in, int c_out, int deformable_group);

/* The backward on float16 / bfloat16 maps (csrc/dcn_bwd_h.hip): the three passes of fv2p_dcn_backward on
 * v_mfma_f32_16x16x32_{f16,bf16}, no fp32 copy of any map.  `dtype` names the format of x_nhwc [B,H,W,Cin], wt [kh*kw][Cin][Cout],
 * dy_nhwc [B*Ho*Wo][Cout], dx_nhwc [B,H,W,Cin] and of the column gradients in the workspace; offset and mask are fp32 (om_dtype 0) or
 * in the call's format (om_dtype == dtype), and doffset / dmask leave in THAT format; dwt [kh*kw][Cin][Cout] is fp32 (the caller
 * casts it: an fp32 master weight gets an unrounded gradient).  The dtype / om_dtype checks come first (FV2P_EINVAL before any HIP
 * call).  Arithmetic: fp32 accumulators everywhere; dcol = wt dy from the 16-bit operands; grad_mask / grad_offset from the fp32 dcol
 * and the widened corners of x with fv2p_dcn_backward's formulas, written once per (pixel, tap, deformable group) with one rounding;
 * colg = dcol * mask rounded once to the format (it reaches dx only); dx = fp32 sums over the sample lists in the fixed key and
 * sample order, rounded once; dwt from the column operand formed as fv2p_dcn_forward_h forms it (one rounding) and dy, per-split
 * fp32 partials folded in ascending split and chunk order.  No float atomics, nothing to zero, two runs give the same bits.
 * Geometry: that of fv2p_dcn_forward_h, and Cout <= 256, Cout a multiple of 8 (the caller zero-pads dy and wt); FV2P_ELIMIT
 * otherwise - fv2p_dcn_backward_h_supported (pure host) answers 1 / 0.  x, wt, dy and dx must be 16-byte aligned; nothing outside
 * x, wt, dy, offset or mask is read.  Batches are cut into chunks of whole samples as above (fv2p_dcn_set_colg_cap governs this
 * route too, and the same value gives the same chunks: the cap counts column gradients at 4 bytes an element on both routes, so
 * this route's 2-byte column gradients take half the capped bytes); fv2p_dcn_backward_h_ws_bytes is the workspace of one chunk.  B = 0: dwt is zeroed, nothing else is touched. */
int fv2p_dcn_backward_h_supported(int c_in, int c_out, int deformable_group);
size_t fv2p_dcn_backward_h_ws_bytes(int batch, int height, int width, int h_out, int w_out, int c_in, int c_out, int kh,
                                    int kw, int deformable_group);
int fv2p_dcn_backward_h(const void* x_nhwc, const void* wt, const void* offset, const void* mask, const void* dy_nhwc,
                        int batch, int height, int width, int c_in, int c_out, int h_out, int w_out, int kh, int kw,
                        int sh, int sw, int ph, int pw, int dh, int dw, int deformable_group,
                        void* dx_nhwc, void* doffset, void* dmask, float* dwt, void* ws, size_t ws_bytes, int dtype,
                        int om_dtype, fv2p_stream_t stream);

/* Layout copies around the NHWC entry points above (and fv2p_bev_interp_*): in [batch][rows][cols] -> out [batch][cols][rows],
 * e.g. NCHW -> NHWC with rows = C, cols = H*W.  The reference does the same copies with at::permute + contiguous
 * (modulated_deform_conv_cuda.cu:78,118). */
int fv2p_transpose_batched(const float* in, int batch, int64_t rows, int64_t cols, float* out, fv2p_stream_t stream);
/* The same copy on 16-bit elements.  Bit patterns are moved, so one entry point serves float16 and bfloat16 and takes no dtype;
 * 16-byte accesses of 8 elements on a side whose extent is a multiple of 8 and whose pointer is 16-byte aligned. */
int fv2p_transpose_batched_h(const void* in, int batch, int64_t rows, int64_t cols, void* out, fv2p_stream_t stream);
/* The layout copy and the dtype copy in one pass (`dtype`: FV2P_DT_F16 / FV2P_DT_BF16, the format of the 16-bit side; any other value
 * returns FV2P_EINVAL): _widen reads 16-bit elements and writes fp32, the bits of .float() followed by fv2p_transpose_batched; _round
 * reads fp32 and rounds to nearest even once at the store, the bits of fv2p_transpose_batched followed by .to(dtype).  They carry the
 * float16 / bfloat16 tensors of the DCN backward to and from its fp32 kernels. */
int fv2p_transpose_batched_widen(const void* in, int dtype, int batch, int64_t rows, int64_t cols, float* out, fv2p_stream_t stream);
int fv2p_transpose_batched_round(const float* in, int batch, int64_t rows, int64_t cols, void* out, int dtype, fv2p_stream_t stream);

/* ---- A14: deformable position-sensitive RoI pooling ----------------------------------------------
 * Replace DCN.deform_psroi_pooling_forward / _backward
 * (pcdet/ops/DeformableConvolutionV2PyTorch/src/vision.cpp:11-12 -> src/deform_psroi_pooling.h ->
 * src/cuda/deform_psroi_pooling_cuda.cu:264-418; kernels :59-147, :149-262; caller functions/deform_psroi_pooling_func.py:15-64).
 * Reference layouts: data / grad_data [B, C, H, W]; rois [R, 5] = (batch index, x1, y1, x2, y2) in image pixels;
 * trans / grad_trans [>=R, 2*num_classes, part, part] (NULL with no_trans, num_classes then counts as 1);
 * out / top_count / grad_out [R, output_dim, pooled, pooled] (top_count = samples that fell on the map, as float).
 * C must equal output_dim * group_size^2 (the reference asserts C == output_dim and reads beyond the map for
 * group_size > 1).  An RoI whose batch index is outside [0, B) pools to zeros with count 0.
 * backward: grad_data and grad_trans must be zeroed by the caller (accumulated with atomics). */
int fv2p_deform_psroi_pool_forward(const float* data, const float* rois, const float* trans, int batch, int channels,
                                   int height, int width, int num_rois, int no_trans, float spatial_scale,
                                   int output_dim, int group_size, int pooled_size, int part_size,
                                   int sample_per_part, float trans_std, int num_classes, float* out,
                                   float* top_count, fv2p_stream_t stream);
int fv2p_deform_psroi_pool_backward(const float* grad_out, const float* data, const float* rois, const float* trans,
                                    const float* top_count, int batch, int channels, int height, int width,
                                    int num_rois, int no_trans, float spatial_scale, int output_dim,
                                    int group_size, int pooled_size, int part_size, int sample_per_part,
                                    float trans_std, int num_classes, float* grad_data, float* grad_trans,
                                    fv2p_stream_t stream);
/* backward in the fixed order of fv2p_scatter_add: grad_data from 4 entries per sample, grad_trans from the bins' sums (each over
 * its samples in order) as 2 entries per bin.  Writes grad_data and the first num_rois rows of grad_trans (no zero fill needed). */
size_t fv2p_deform_psroi_pool_backward_ws_bytes(int num_rois, int output_dim, int pooled_size, int sample_per_part);
int fv2p_deform_psroi_pool_backward_gather(const float* grad_out, const float* data, const float* rois, const float* trans,
                                           const float* top_count, int batch, int channels, int height, int width,
                                           int num_rois, int no_trans, float spatial_scale, int output_dim,
                                           int group_size, int pooled_size, int part_size, int sample_per_part,
                                           float trans_std, int num_classes, float* grad_data, float* grad_trans,
                                           void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- (f).3: BatchNorm1d (+ReLU) over sparse-tensor features [N, C] --------------------------------
 * The pair every conv of the reference backbones is followed by: nn.BatchNorm1d(eps=1e-3, momentum=0.01) + nn.ReLU
 * (pcdet/models/backbones_3d/spconv_backbone.py:8-27, :75), applied to SparseConvTensor.features by
 * SparseSequential (pcdet/ops/spconv/modules.py:86-100).  torch semantics: biased batch variance for the
 * normalisation, unbiased for running_var; running = (1 - momentum) * running + momentum * batch; momentum < 0
 * means momentum=None (cumulative average over num_batches_tracked).  Sums are accumulated in fp64 and folded in a
 * fixed order (deterministic).
 *   fv2p_batchnorm_forward  : training-mode layer: batch mean / invstd of x[n,c] (also returned for the backward
 *                             pass), running_mean / running_var / num_batches_tracked updated in place when
 *                             running_mean != NULL, y = relu?((x - mean) * invstd * gamma + beta).
 *   fv2p_batchnorm_apply    : the same normalisation with given mean / invstd (eval mode: running statistics).
 *                             gamma / beta may be NULL; y may alias x.
 *   fv2p_batchnorm_backward : dz = dy * [y > 0] (mask recomputed from x); dgamma = sum dz * xhat, dbeta = sum dz,
 *                             dx = gamma * invstd * (dz - mean(dz) - xhat * mean(dz * xhat))  when batch_stats != 0,
 *                             dx = gamma * invstd * dz                                          otherwise (eval mode).
 * c <= 1024 (c % 4 == 0) or c <= 256.
 */
size_t fv2p_batchnorm_ws_bytes(int64_t n, int c);
int fv2p_batchnorm_forward(const float* x, int64_t n, int c, float eps, float momentum, const float* gamma,
                           const float* beta, int relu, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, float* mean, float* invstd, float* y, void* ws,
                           size_t ws_bytes, fv2p_stream_t stream);
/* fv2p_batchnorm_forward with the sums already taken (stats as left by fv2p_sparse_conv_rows_stats): one launch.
 * zero_next: NULL, or a second stats buffer whose first zero_count doubles are cleared for the next fused conv on this
 * stream (two buffers alternate: a launch reads one and clears what the other's last user left). */
int fv2p_batchnorm_forward_stats(const float* x, int64_t n, int c, float eps, float momentum, const float* gamma,
                                 const float* beta, int relu, float* running_mean, float* running_var,
                                 int64_t* num_batches_tracked, float* mean, float* invstd, float* y,
                                 const double* stats, double* zero_next, int64_t zero_count, fv2p_stream_t stream);
/* fv2p_batchnorm_backward with (sum dz, sum dz * xhat) already in `stats` (fv2p_sparse_conv_rows_bnbwd): one launch. */
int fv2p_batchnorm_backward_stats(const float* x, const float* dy, int64_t n, int c, const float* mean,
                                  const float* invstd, const float* gamma, const float* beta, int relu,
                                  int batch_stats, float* dx, float* dgamma, float* dbeta, const double* stats,
                                  double* zero_next, int64_t zero_count, fv2p_stream_t stream);
/* round 6: fv2p_batchnorm_apply with an optional residual term, y = relu?(bn(x) + residual) - the tail of a residual block
 * (spconv_backbone.py:63-66: out.features += identity; relu) in the normalisation's own pass; fv2p_batchnorm_backward_fin = the apply
 * half of the backward with c1 / c2 (coef) already finalised by fv2p_sparse_conv_rows_bnbwd_fin; fv2p_batchnorm_backward_res = backward
 * of out = relu(bn(x) + identity): the ReLU mask is read from `out`, dz = dout * [out > 0] (the identity branch's gradient) is written
 * beside dx. */
int fv2p_batchnorm_apply_res(const float* x, int64_t n, int c, const float* mean, const float* invstd, const float* gamma,
                             const float* beta, int relu, const float* residual, float* y, fv2p_stream_t stream);
int fv2p_batchnorm_backward_fin(const float* x, const float* dy, int64_t n, int c, const float* mean, const float* invstd,
                                const float* gamma, const float* beta, int relu, const float* coef, float* dx,
                                fv2p_stream_t stream);
int fv2p_batchnorm_backward_res(const float* x, const float* out, const float* dout, int64_t n, int c, const float* mean,
                                const float* invstd, const float* gamma, const float* beta, int batch_stats, float* dx,
                                float* dz, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, fv2p_stream_t stream);
/* round 6: both passes of a BatchNorm whose sums no conv epilogue takes, as ONE launch each (reduce, grid barrier over <= 128 resident
 * workgroups, apply).  counters: two zeroed device words kept by the caller per stream (zero again when the launch ends); ws as
 * fv2p_batchnorm_one_ws_bytes(c).  residual / mask_y / dz_out as in fv2p_batchnorm_apply_res / _backward_res (NULL = plain layer). */
size_t fv2p_batchnorm_one_ws_bytes(int c);
int fv2p_batchnorm_one_pays(int64_t n, int c, int backward);   /* 1: the one-launch pass is the faster one at this size (measured: tools/bn_time.py) */
int fv2p_batchnorm_forward_one(const float* x, int64_t n, int c, float eps, float momentum, const float* gamma, const float* beta,
                               int relu, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean,
                               float* invstd, const float* residual, float* y, void* ws, size_t ws_bytes, unsigned* counters,
                               fv2p_stream_t stream);
int fv2p_batchnorm_backward_one(const float* x, const float* dy, int64_t n, int c, const float* mean, const float* invstd,
                                const float* gamma, const float* beta, int relu, int batch_stats, const float* mask_y, float* dx,
                                float* dz_out, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, unsigned* counters,
                                fv2p_stream_t stream);
/* round 6: the two-launch passes for large tensors (the decoder's 49 152-row layers) with a WIDE reduce: up to 512 workgroups publish
 * their partial sums as rows, the reduce launch's last workgroups fold them in a fixed order (the protocol of
 * fv2p_sparse_conv_rows_bnfin) and the apply launch reads finished mean / invstd or c1 / c2.  counters:
 * fv2p_batchnorm_wide_counter_words(c) zeroed device words kept by the caller per stream. */
size_t fv2p_batchnorm_wide_ws_bytes(int c);
int fv2p_batchnorm_wide_counter_words(int c);
int fv2p_batchnorm_forward_wide(const float* x, int64_t n, int c, float eps, float momentum, const float* gamma, const float* beta,
                                int relu, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean,
                                float* invstd, const float* residual, float* y, void* ws, size_t ws_bytes, unsigned* counters,
                                fv2p_stream_t stream);
int fv2p_batchnorm_backward_wide(const float* x, const float* dy, int64_t n, int c, const float* mean, const float* invstd,
                                 const float* gamma, const float* beta, int relu, int batch_stats, const float* mask_y, float* dx,
                                 float* dz_out, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, unsigned* counters,
                                 fv2p_stream_t stream);
int fv2p_batchnorm_apply(const float* x, int64_t n, int c, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, int relu, float* y, fv2p_stream_t stream);
int fv2p_batchnorm_backward(const float* x, const float* dy, int64_t n, int c, const float* mean,
                            const float* invstd, const float* gamma, const float* beta, int relu, int batch_stats,
                            float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                            fv2p_stream_t stream);

/* ---- BatchNorm1d (+ residual, + ReLU) on 16-bit rows -------------------------------------------------------------
 * The layers between two fv2p_sparse_conv_rows_h calls (csrc/batchnorm_h.hip).  `dtype` (FV2P_DT_F16 / FV2P_DT_BF16) names
 * the format of x, y, dy, dx, residual, mask_y and dz_out; any other value returns FV2P_EINVAL with "dtype" in the message and
 * launches nothing.  `param_dtype` names the format of gamma, beta, running_mean, running_var, dgamma and dbeta: 0 = fp32 (a
 * module kept in fp32 under a 16-bit activation stream) or the call's dtype (module.half() / .bfloat16()); any other value
 * returns FV2P_EINVAL and launches nothing.  mean and invstd are ALWAYS fp32.  No tensor is converted to fp32 in memory.
 * Two launches per pass (reduce with one fp64 partial per workgroup, then apply: every workgroup folds the partials in the
 * same fixed order), no float atomics, no grid barrier: results are bit-identical from run to run.  Per element, in fp32
 * and in this order, (x - mean) * invstd * gamma + beta (+ residual), then the ReLU (NaN passes through), then ONE rounding to
 * nearest even at the store.  16-bit parameters are widened on read; a new running value, dgamma and dbeta are computed in
 * fp64 (from the widened old value) and rounded once on write.
 * Rows travel as 16-byte accesses of 8 elements when c % 8 == 0 and every tensor is 16-byte aligned (c <= 1024), element by
 * element otherwise (c <= 256); a larger c returns FV2P_ELIMIT.  Every entry point returns 0 and launches nothing for n == 0.
 *   fv2p_batchnorm_forward_h  : the contract of fv2p_batchnorm_forward (batch statistics, running statistics moved with
 *                               `momentum`, < 0 = cumulative average over num_batches_tracked, which is advanced), with the
 *                               optional residual of fv2p_batchnorm_apply_res.  Workspace: fv2p_batchnorm_h_ws_bytes.
 *   fv2p_batchnorm_apply_h    : the same normalisation with given mean / invstd (eval mode).  One launch.
 *   fv2p_batchnorm_backward_h : dz = dy * [y > 0], the mask recomputed from x, or read from mask_y > 0 when given (the residual
 *                               form relu(bn(x) + identity): mask_y is that block's output); dz_out (NULL = not wanted) receives
 *                               dz, the identity branch's gradient; dx = gamma * invstd * (dz - c1 - xhat * c2) in fp32, rounded
 *                               once, c1 = mean dz and c2 = mean dz * xhat (both 0 when batch_stats == 0); dgamma = sum dz * xhat
 *                               and dbeta = sum dz, folded in fixed order. */
size_t fv2p_batchnorm_h_ws_bytes(int64_t n, int c);
int fv2p_batchnorm_forward_h(const void* x, int64_t n, int c, float eps, float momentum, const void* gamma, const void* beta,
                             int relu, const void* residual, void* running_mean, void* running_var,
                             int64_t* num_batches_tracked, float* mean, float* invstd, void* y, int dtype, int param_dtype,
                             void* ws, size_t ws_bytes, fv2p_stream_t stream);
int fv2p_batchnorm_apply_h(const void* x, int64_t n, int c, const float* mean, const float* invstd, const void* gamma,
                           const void* beta, int relu, const void* residual, void* y, int dtype, int param_dtype,
                           fv2p_stream_t stream);
int fv2p_batchnorm_backward_h(const void* x, const void* dy, int64_t n, int c, const float* mean, const float* invstd,
                              const void* gamma, const void* beta, int relu, int batch_stats, const void* mask_y, void* dx,
                              void* dz_out, void* dgamma, void* dbeta, int dtype, int param_dtype, void* ws, size_t ws_bytes,
                              fv2p_stream_t stream);

/* ---- BatchNorm2d (+ReLU) on contiguous fp32 NCHW maps [n, c, hw] ---------------------------------------------------------
 * The pair behind every Conv2d / ConvTranspose2d of the reference's BEV backbones: nn.BatchNorm2d(eps=1e-3, momentum=0.01) +
 * nn.ReLU() (pcdet/models/backbones_2d/base_bev_backbone.py:35-46, :53-70; dcn_bev_backbone.py:40-83), which torch runs as a
 * spatial BatchNorm and an elementwise clamp (5 passes over the map forward, 8 backward).  Here (csrc/batchnorm2d.hip) each
 * direction is two launches: a reduce over (sample, channel, chunk of the plane) that writes one pair of fp64 partial sums per
 * workgroup, and an apply on the same grid in which every workgroup folds the partials of its channel in one fixed order - 3
 * passes forward, 5 backward, no atomics, no counters, results bit-identical from run to run.  torch semantics as for
 * fv2p_batchnorm_forward (biased variance for the normalisation, unbiased for running_var, momentum < 0 = cumulative average
 * over num_batches_tracked, which is read before it is advanced).  hw = H * W; planes are read with 16-byte accesses when
 * hw % 4 == 0 and the tensors are 16-byte aligned, element by element otherwise.  gamma / beta may be NULL.
 *   fv2p_batchnorm2d_forward  : training-mode layer: mean / invstd [c] of the batch (returned for the backward pass), running
 *                               statistics moved in place when running_mean != NULL, y = relu?((x - mean) * invstd * gamma + beta).
 *   fv2p_batchnorm2d_apply    : the same expression with given mean / invstd (eval mode).  One launch; n == 0 launches nothing.
 *   fv2p_batchnorm2d_backward : dy = dz * [y > 0] with y recomputed from x by the forward's own expression (y is not read);
 *                               dgamma = sum dy * xhat, dbeta = sum dy, dx = gamma * invstd * (dy - mean(dy) - xhat * mean(dy * xhat))
 *                               when batch_stats != 0, dx = gamma * invstd * dy otherwise.
 * Workspace for _forward and _backward: fv2p_batchnorm2d_ws_bytes(n, c, hw) (0 for a shape that cannot be launched: FV2P_ELIMIT). */
size_t fv2p_batchnorm2d_ws_bytes(int64_t n, int c, int64_t hw);
int fv2p_batchnorm2d_forward(const float* x, int64_t n, int c, int64_t hw, float eps, float momentum, const float* gamma,
                             const float* beta, int relu, float* running_mean, float* running_var,
                             int64_t* num_batches_tracked, float* mean, float* invstd, float* y, void* ws, size_t ws_bytes,
                             fv2p_stream_t stream);
int fv2p_batchnorm2d_apply(const float* x, int64_t n, int c, int64_t hw, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, int relu, float* y, fv2p_stream_t stream);
int fv2p_batchnorm2d_backward(const float* x, const float* dz, int64_t n, int c, int64_t hw, const float* mean,
                              const float* invstd, const float* gamma, const float* beta, int relu, int batch_stats,
                              float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- BatchNorm2d (+ReLU) on contiguous float16 / bfloat16 NCHW maps [n, c, hw] ------------------------------------------------
 * The layer above on the 16-bit volume that fv2p_sparse_to_dense_h writes and the BEV backbones' convolutions keep
 * (csrc/batchnorm2d.hip: the same kernels in a 16-bit format), with the conventions of the 16-bit row op: `dtype` (FV2P_DT_F16 /
 * FV2P_DT_BF16) names the format of x, y, dz and dx; `param_dtype` is 0 (fp32) or equal to `dtype` and names the format of gamma, beta, running_mean, running_var,
 * dgamma and dbeta; mean and invstd are ALWAYS fp32.  The dtype checks come first: any other value returns FV2P_EINVAL with
 * "dtype" in the message.  Every argument check returns before anything is launched and leaves the outputs untouched
 * (FV2P_EINVAL, FV2P_ELIMIT, FV2P_EWORKSPACE).  No map is converted to fp32 in memory: the workspace holds the fp64 partials and
 * the counter copy only.
 * Same two launches per direction, same grid and same fixed-order fold as the fp32 entry points: no float atomics, no grid
 * barrier, bit-identical from run to run.  Elements are widened on load; sums are fp64; per element, in fp32 and in this order,
 * (x - mean) * invstd * gamma + beta, then the ReLU (NaN passes through), then ONE rounding to nearest even at the store.  16-bit
 * parameters are widened on read; a new running value, dgamma and dbeta go from their fp64 value to 16 bits in one rounding.
 * A thread moves 8 elements per 16-byte access when hw % 8 == 0 and the maps are 16-byte aligned, one element otherwise.
 *   fv2p_batchnorm2d_forward_h  : the contract of fv2p_batchnorm2d_forward.
 *   fv2p_batchnorm2d_apply_h    : the same expression with given mean / invstd (eval mode).  One launch; n == 0 launches nothing.
 *   fv2p_batchnorm2d_backward_h : dy = dz * [y > 0] where y is the STORED output, the forward's fp32 value rounded to the format,
 *                                 recomputed from x (y is not read): a float16 pre-activation below 2^-25 was stored as 0 and gets
 *                                 no gradient.  dx = gamma * invstd * (dy - c1 - xhat * c2) in fp32 in that order, rounded once;
 *                                 c1 = mean dy, c2 = mean dy * xhat (both 0 when batch_stats == 0); dgamma = sum dy * xhat,
 *                                 dbeta = sum dy.
 * Workspace for _forward_h and _backward_h: fv2p_batchnorm2d_h_ws_bytes(n, c, hw) (0 for a shape that cannot be launched). */
size_t fv2p_batchnorm2d_h_ws_bytes(int64_t n, int c, int64_t hw);
int fv2p_batchnorm2d_forward_h(const void* x, int64_t n, int c, int64_t hw, float eps, float momentum, const void* gamma,
                               const void* beta, int relu, void* running_mean, void* running_var,
                               int64_t* num_batches_tracked, float* mean, float* invstd, void* y, int dtype, int param_dtype,
                               void* ws, size_t ws_bytes, fv2p_stream_t stream);
int fv2p_batchnorm2d_apply_h(const void* x, int64_t n, int c, int64_t hw, const float* mean, const float* invstd,
                             const void* gamma, const void* beta, int relu, void* y, int dtype, int param_dtype,
                             fv2p_stream_t stream);
int fv2p_batchnorm2d_backward_h(const void* x, const void* dz, int64_t n, int c, int64_t hw, const float* mean,
                                const float* invstd, const void* gamma, const void* beta, int relu, int batch_stats, void* dx,
                                void* dgamma, void* dbeta, int dtype, int param_dtype, void* ws, size_t ws_bytes,
                                fv2p_stream_t stream);

/* ---- Multi-head 1x1 convolution over a contiguous fp32 NCHW map, outputs position-major ---------------------------------------
 * The three 1x1 nn.Conv2d of the reference's anchor head (conv_cls, conv_box, conv_dir_cls: pcdet/models/dense_heads/
 * anchor_head_single.py:21-37) and the `permute(0, 2, 3, 1).contiguous()` its forward() applies to each output (:48-60), as one
 * kernel per direction (csrc/head1x1.hip; forward and backward data on v_mfma_f32_16x16x4_f32).  x is [b, cin, hw] (hw = H * W) and is read as it stands, once
 * per direction; head k has the module's own weight w_k [c_k, cin] and bias_k [c_k] (NULL: no bias) - nothing is repacked or kept
 * between calls; y_k, dy_k are [b * hw, c_k].  One to three heads, packed to the front (c1 == 0: one head; c2 == 0: two), with
 * c0 + c1 + c2 <= 64 and b * hw < 2^30 (FV2P_ELIMIT otherwise); absent heads pass NULL pointers.  Any cin >= 1 and any hw: maps
 * with hw % 4 == 0 and a 16-byte aligned base move 16 bytes per lane, others one element.
 *   fv2p_head1x1_forward          : y_k[g][j] = sum_c x[n][c][p] * w_k[j][c] + bias_k[j], g = n * hw + p.
 *   fv2p_head1x1_backward_data    : dx[n][c][p] = sum_k sum_j w_k[j][c] * dy_k[g][j], written once.
 *   fv2p_head1x1_backward_weights : dw_k[j][c] = sum_g dy_k[g][j] * x[n][c][p] and db_k[j] = sum_g dy_k[g][j] (db_k NULL: not
 *                                   wanted).  Two launches: partial tiles over a fixed split of the positions, accumulated on
 *                                   v_mfma_f64_16x16x4_f64 (exact products, fp64 sums), then a fold of the fp64 partials in split
 *                                   order with one rounding to fp32.  No atomics: bit-identical from run to run.
 * Workspace for _backward_weights: fv2p_head1x1_ws_bytes(b, cin, hw, c0, c1, c2) (a pure host function; 0 for a shape the op does
 * not take). */
size_t fv2p_head1x1_ws_bytes(int64_t b, int cin, int64_t hw, int c0, int c1, int c2);
int fv2p_head1x1_forward(const float* x, int64_t b, int cin, int64_t hw, const float* w0, const float* w1, const float* w2,
                         const float* bias0, const float* bias1, const float* bias2, int c0, int c1, int c2, float* y0, float* y1,
                         float* y2, fv2p_stream_t stream);
int fv2p_head1x1_backward_data(const float* dy0, const float* dy1, const float* dy2, int64_t b, int cin, int64_t hw, const float* w0,
                               const float* w1, const float* w2, int c0, int c1, int c2, float* dx, fv2p_stream_t stream);
int fv2p_head1x1_backward_weights(const float* x, const float* dy0, const float* dy1, const float* dy2, int64_t b, int cin,
                                  int64_t hw, int c0, int c1, int c2, float* dw0, float* dw1, float* dw2, float* db0, float* db1,
                                  float* db2, void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- nn.Linear(bias=False) -> nn.BatchNorm1d [-> nn.ReLU] over fp32 point rows as one op --------------------------------------
 * The triple of the voxel-to-point decoder and of BEVGridPooling.point_bev_feature_compress (csrc/linear_bn.hip; every product on
 * v_mfma_f32_16x16x4_f32: fp32 in, fp32 accumulate).  Everything is fp32 and row-major: x [n][cin], w [cout][cin] (the module's own
 * weight: nothing is repacked or kept between calls), z = x * w^T [n][cout], y and dy [n][cout].  n >= 1, cin 1 .. 1024 and
 * cout 1 .. 512, any value (FV2P_EINVAL outside); 16-byte loads where the row lengths are multiples of 4 and the bases 16-byte
 * aligned, element by element otherwise.  gamma, beta, running_mean and running_var may be NULL as in fv2p_batchnorm_forward;
 * momentum < 0 is momentum=None.  No float atomics and no workgroup waits for another: every sum across workgroups is a row of
 * partials in the workspace that a LATER launch of the same call folds in a fixed order, so statistics, running statistics and every
 * gradient are bit-identical from run to run.  Every call enqueues all of its launches on `stream` and returns.
 *   fv2p_linear_bn_forward      : training mode (n >= 2).  GEMM that stores z and leaves sum z / sum z^2 per workgroup (formed in fp64
 *                                 from the fp32 accumulators); fold -> mean, invstd (biased variance), running statistics with
 *                                 torch's semantics (unbiased running_var, num_batches_tracked += 1); apply ->
 *                                 y = relu?((z - mean) * invstd * gamma + beta).  Three launches.
 *   fv2p_linear_bn_forward_eval : given mean / invstd; scale, shift and the ReLU in the GEMM's epilogue.  One launch; z is stored
 *                                 only when a buffer is passed (a backward pass through the frozen BatchNorm needs it).
 *   fv2p_linear_bn_backward     : dz = dy * [y > 0] recomputed from z; dgamma = sum dz * xhat, dbeta = sum dz;
 *                                 du = gamma * invstd * (dz - mean(dz) - xhat * mean(dz * xhat)) (batch_stats = 0: gamma * invstd * dz)
 *                                 into the caller's du [n][cout]; dx = du * w (dx NULL: skipped); dw = du^T * x over a fixed split of
 *                                 the rows, fp64 partial tiles folded in split order (dw NULL: GEMM and fold skipped).
 * Workspace: fv2p_linear_bn_ws_bytes(n, cin, cout), enough for either direction (0 for a shape the op does not take);
 * fv2p_linear_bn_splits: the row chunks of the weight-gradient pass; fv2p_linear_bn_pays: 1 where the op measured faster, forward +
 * backward, than rocBLAS + fv2p_batchnorm_* (profiles/linear_bn.txt).  All three are pure host functions. */
size_t fv2p_linear_bn_ws_bytes(int64_t n, int cin, int cout);
int fv2p_linear_bn_splits(int64_t n, int cin, int cout);
int fv2p_linear_bn_pays(int64_t n, int cin, int cout);
int fv2p_linear_bn_forward(const float* x, int64_t n, int cin, const float* w, int cout, float eps, float momentum,
                           const float* gamma, const float* beta, int relu, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, float* z, float* mean, float* invstd, float* y, void* ws, size_t ws_bytes,
                           fv2p_stream_t stream);
int fv2p_linear_bn_forward_eval(const float* x, int64_t n, int cin, const float* w, int cout, const float* mean,
                                const float* invstd, const float* gamma, const float* beta, int relu, float* z, float* y,
                                fv2p_stream_t stream);
int fv2p_linear_bn_backward(const float* x, const float* z, const float* dy, int64_t n, int cin, const float* w, int cout,
                            const float* mean, const float* invstd, const float* gamma, const float* beta, int relu,
                            int batch_stats, float* du, float* dx, float* dw, float* dgamma, float* dbeta, void* ws,
                            size_t ws_bytes, fv2p_stream_t stream);

/* ---- The same triple on float16 / bfloat16 point rows (the 16-bit formats of csrc/linear_bn.hip; every product on v_mfma_f32_16x16x32_{f16,bf16}) ----
 * `dt` (FV2P_DT_F16 / FV2P_DT_BF16) names the format T of x [n][cin], z, y, dy, du [n][cout] and dx; `wd` is 0 (w and dw are fp32: a
 * master weight, rounded ONCE to T on its way into LDS - the bits of w.to(T), no 16-bit copy in memory) or equal to dt; `pd` is 0
 * (fp32) or equal to dt and names the format of gamma, beta, running_mean, running_var, dgamma and dbeta.  Any other value returns
 * FV2P_EINVAL with "dtype" in the message.  mean and invstd are fp32.  Limits as the fp32 op: n >= 1 (training mode: n >= 2),
 * cin 1 .. 1024, cout 1 .. 512, FV2P_EINVAL outside, judged before any pointer is touched; 16-byte accesses where the row lengths
 * are multiples of 8 and the bases 16-byte aligned, element by element otherwise.  With u the unit roundoff of T:
 *   1. pre-activation  acc = sum_k x * w: products of two T values are exact, fp32 accumulators in a fixed order;
 *                      z = round_T(acc), stored [n][cout] in T, IS the op's pre-activation everywhere: everything downstream reads
 *                      the stored 16-bit z, widened (torch's bn(linear(x)) on 16-bit rows), so the forward pass and the ReLU mask the
 *                      backward pass recomputes agree by construction.
 *   2. training mode   sum z / sum z^2 of the ROUNDED z per channel from the GEMM's epilogue, fp64 partials per row tile folded in
 *                      a fixed order of the tiles by a later launch; mean / invstd fp32; running statistics (momentum, momentum < 0 = None, unbiased
 *                      variance) and num_batches_tracked in the parameters' format with one rounding;
 *                      y = round_T(relu?((z - mean) * invstd * gamma + beta)) in fp32.  Three launches.
 *   3. eval mode       one launch; z is stored only when a buffer is passed; y from the widened z with the caller's fp32 mean / invstd.
 *   4. backward        the ReLU mask from z with the forward's expression; dgamma, dbeta, c1, c2 from fp64 sums in a fixed order;
 *                      du = gamma * invstd * (dz - c1 - xhat * c2) in fp32, rounded ONCE to T into the caller's du (the staging
 *                      buffer and the MFMA operand); dx = du * w, fp32 accumulators, one rounding to T (dx NULL: skipped);
 *                      dw = du^T * x over a fixed split of the rows: at most 128 rows per fp32 accumulator chain, chains summed in
 *                      fp64, partial tiles folded in split order, ONE rounding into a T weight or an fp32 store for wd = 0 (dw NULL:
 *                      skipped); dgamma / dbeta in the parameters' format.
 *   5. determinism     no float atomics, no workgroup waits for another, no fp32 copy of any [n, .] tensor: bit-identical results
 *                      from run to run.
 * Host-only queries (no device needed): fv2p_linear_bn_h_supported: 1 for a shape inside the limits with valid dt / wd / pd, else 0;
 * fv2p_linear_bn_h_ws_bytes: the workspace of either direction (0 outside the limits); fv2p_linear_bn_h_splits: the row chunks of
 * the weight-gradient pass; fv2p_linear_bn_h_pays: 1 where the op measured faster, forward + backward, than the library's 16-bit
 * product + fv2p_batchnorm_*_h (profiles/linear_bn_half.txt). */
int fv2p_linear_bn_h_supported(int64_t n, int cin, int cout, int dt, int wd, int pd);
size_t fv2p_linear_bn_h_ws_bytes(int64_t n, int cin, int cout);
int fv2p_linear_bn_h_splits(int64_t n, int cin, int cout);
int fv2p_linear_bn_h_pays(int64_t n, int cin, int cout, int dt);
int fv2p_linear_bn_forward_h(const void* x, int64_t n, int cin, const void* w, int cout, float eps, float momentum,
                             const void* gamma, const void* beta, int relu, void* running_mean, void* running_var,
                             int64_t* num_batches_tracked, void* z, float* mean, float* invstd, void* y, int dt, int wd, int pd,
                             void* ws, size_t ws_bytes, fv2p_stream_t stream);
int fv2p_linear_bn_forward_eval_h(const void* x, int64_t n, int cin, const void* w, int cout, const float* mean,
                                  const float* invstd, const void* gamma, const void* beta, int relu, void* z, void* y, int dt,
                                  int wd, int pd, fv2p_stream_t stream);
int fv2p_linear_bn_backward_h(const void* x, const void* z, const void* dy, int64_t n, int cin, const void* w, int cout,
                              const float* mean, const float* invstd, const void* gamma, const void* beta, int relu,
                              int batch_stats, void* du, void* dx, void* dw, void* dgamma, void* dbeta, int dt, int wd, int pd,
                              void* ws, size_t ws_bytes, fv2p_stream_t stream);

/* ---- Voxel R-CNN RoI-grid pooling: NeighborVoxelSAModuleMSG between mlps_in and mlps_out as one op ----------------------------
 * What a grouper of the module does after its voxel query with pool_method 'max_pool' (csrc/voxel_pool.hip), on fp32 rows (16-bit rows: the *_h forms below), without a
 * tensor proportional to m * c * s.  f [n][c] the mlps_in rows, xyz [n][3], new_xyz [m][3], idx [m][s] GLOBAL rows of the voxel
 * query (int32), empty [m] one byte per query (non-zero: the query found nothing), w [c][3] the Conv2d(3, c, 1, bias=False)
 * weight, gamma / beta / running_mean / running_var [c] and num_batches_tracked of its BatchNorm2d.  With
 * d[i][j] = xyz[idx[i][j]] - new_xyz[i] (formed in fp32; zero for an empty query):
 *     out[i][ch] = max_j relu(f[idx[i][j]][ch] + BN(w d[i][j])[ch])        (empty query: relu of the BatchNorm of zero)
 * BN with batch statistics over the m * s positions (training != 0: biased variance, running statistics moved with torch's
 * semantics - unbiased running_var, momentum < 0 is momentum=None, num_batches_tracked += 1 - when running_mean is not NULL) or
 * with the running statistics (training == 0: nothing but out / arg / saved is written).  The statistics follow in fp64 from nine
 * sums over d (sum d, sum d d^T), never from the c-channel tensor.  arg [m][c] (NULL: no backward will follow) receives the winning
 * sample: the lowest j on ties, as max_pool2d scans; a NaN candidate makes the output NaN.  saved: fv2p_voxel_pool_saved_bytes(c)
 * bytes the backward reads (the nine sums, mean and invstd per channel, all fp64).
 * An idx entry outside [0, n) in a non-empty query reads as a zero row of f AND of xyz and receives no gradient: no input makes a
 * kernel leave its buffers.
 *   fv2p_voxel_pool_supported : 1 when c % 4 == 0, 4 <= c <= 128, 1 <= s <= 64, m >= 1 and m * s < 2^31 (FV2P_ELIMIT otherwise)
 *   fv2p_voxel_pool_blocks    : the fixed query blocks of the two partial-sum passes; depends on m only, 0 for m < 1
 *   fv2p_voxel_pool_ws_bytes / _backward_ws_bytes : pure host functions, 0 outside the limits (backward: also from m * c or n * c
 *                               = 2^31 on, the 32-bit entry numbers of fv2p_scatter_add), never decreasing in m
 *   fv2p_voxel_pool_forward   : moments (training) -> fold -> pool: three launches
 *   fv2p_voxel_pool_backward  : g = grad_out * [out > 0]; grad_f [n][c] is WRITTEN (zero fill, then fv2p_scatter_add with one
 *                               channel per entry: fixed order); grad_w [c][3], grad_gamma, grad_beta [c] from per-block fp64
 *                               partials folded in block order and the closed forms of DESIGN "Voxel pooling".  Any of the four may
 *                               be NULL and is then not computed.  `training` as in the forward call that wrote `saved`.
 * f, out and grad_out must be 16-byte aligned.  No float atomics, no workgroup waits for another: every output is bit-identical
 * from run to run.  Every call enqueues all of its launches on `stream` and returns. */
int fv2p_voxel_pool_supported(int64_t m, int s, int c);
int fv2p_voxel_pool_blocks(int64_t m);
size_t fv2p_voxel_pool_saved_bytes(int c);
size_t fv2p_voxel_pool_ws_bytes(int64_t m, int s, int c);
size_t fv2p_voxel_pool_backward_ws_bytes(int64_t m, int s, int c, int64_t n);
int fv2p_voxel_pool_forward(const float* f, const float* xyz, const float* new_xyz, const int* idx, const unsigned char* empty,
                            int64_t n, int64_t m, int s, int c, const float* w, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                            int training, float* out, unsigned char* arg, double* saved, void* ws, size_t ws_bytes,
                            fv2p_stream_t stream);
int fv2p_voxel_pool_backward(const float* xyz, const float* new_xyz, const int* idx, const unsigned char* empty, int64_t n,
                             int64_t m, int s, int c, const float* w, const float* gamma, const float* out,
                             const unsigned char* arg, const double* saved, const float* grad_out, int training, float* grad_f,
                             float* grad_w, float* grad_gamma, float* grad_beta, void* ws, size_t ws_bytes,
                             fv2p_stream_t stream);

/* The same op on float16 / bfloat16 rows, what torch.autocast hands the module (`dtype`: FV2P_DT_F16 / FV2P_DT_BF16, the format T of
 * f, out, grad_out and grad_f; any other value returns FV2P_EINVAL).  Everything that comes from coordinates and parameters stays
 * fp32 / fp64 as above: xyz, new_xyz, w, gamma, beta, the running statistics, the nine moment sums, the coefficients, saved, grad_w,
 * grad_gamma, grad_beta.  The kernels are the fp32 ones instantiated for T:
 *     out[i][ch] = round_T(max_j relu(widen(f[idx[i][j]][ch]) + BN(w d[i][j])[ch]))
 * with the sum, the ReLU, the maximum and arg taken in fp32 and ONE rounding to nearest even at the store.  backward: a cell is live
 * when the stored out, widened, is > 0; g = grad_out there and 0 elsewhere is staged in T (exact); the fp64 sums run in the order of the
 * fp32 op; grad_f [n][c] is WRITTEN by the 16-bit form of fv2p_scatter_add (its fp32 association, every element rounded once).  No
 * float atomics and no fp32 buffer of m * c or n * c elements in either direction.  The limits, fv2p_voxel_pool_supported, _blocks,
 * _saved_bytes and the forward workspace (_ws_bytes) are those of the fp32 op; fv2p_voxel_pool_backward_h_ws_bytes (g in T, the int32
 * destinations, the scatter-add's own workspace) is at least 2 m c bytes below fv2p_voxel_pool_backward_ws_bytes, 0 where that is 0
 * and never decreasing in m.  f, out and grad_out must be 8-byte aligned (a lane moves 4 channels of 2 bytes per access). */
size_t fv2p_voxel_pool_backward_h_ws_bytes(int64_t m, int s, int c, int64_t n);
int fv2p_voxel_pool_forward_h(const void* f, const float* xyz, const float* new_xyz, const int* idx, const unsigned char* empty,
                              int64_t n, int64_t m, int s, int c, const float* w, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                              int training, void* out, unsigned char* arg, double* saved, void* ws, size_t ws_bytes, int dtype,
                              fv2p_stream_t stream);
int fv2p_voxel_pool_backward_h(const float* xyz, const float* new_xyz, const int* idx, const unsigned char* empty, int64_t n,
                               int64_t m, int s, int c, const float* w, const float* gamma, const void* out,
                               const unsigned char* arg, const double* saved, const void* grad_out, int training, void* grad_f,
                               float* grad_w, float* grad_gamma, float* grad_beta, void* ws, size_t ws_bytes, int dtype,
                               fv2p_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FV2P_OPS_H_ */
