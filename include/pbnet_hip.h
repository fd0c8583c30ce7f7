/*
 * include/pbnet_hip.h -- C ABI of libpbnet_hip.so, the MI355X (gfx950) hot path of PBNet.
 *
 * Every entry point takes raw DEVICE pointers, sizes and a hipStream_t; nothing here knows about torch.
 * All functions return PBN_OK (0) or a negative error code and never call exit() (the reference does:
 * lib/PB_lib/src/pbnet/binary.cuh:22-27).  No entry point allocates or frees device memory or synchronises the
 * stream unless stated: scratch comes from the caller (`workspace`), sized by the matching *_workspace_bytes().
 * Citations are relative to /root/reference/.
 */
#ifndef PBNET_HIP_H
#define PBNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pbn_stream_t; /* hipStream_t */

enum {
    PBN_OK = 0,
    PBN_ERR_ARG = -1,        /* bad argument (null pointer, negative size, unsupported shape) */
    PBN_ERR_WORKSPACE = -2,  /* workspace too small */
    PBN_ERR_HIP = -3,        /* a HIP runtime call failed; see pbn_last_hip_error() */
    PBN_ERR_RANGE = -4,      /* a value is outside the supported range (coordinates, class ids) */
    PBN_ERR_UNSUPPORTED = -5
};

/* element types of feature slabs */
enum { PBN_F32 = 0, PBN_BF16 = 1, PBN_F16 = 2 };

/* Scenes (batch elements) of one merged forward: the bound of pbn_sem_argmax_table's population table, of pbn_scene_table
 * and of pbnet_amd/serving.py's max_batch. */
#define PBN_MAX_SCENES 8

const char* pbn_version(void);
/* hipError_t of the last failing HIP call on this thread, as int (0 = none). */
int pbn_last_hip_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Grouping: point-wise binarization + neighbour clustering.
 * Replaces PB_lib.binary_cluster (lib/PB_lib/src/PB_lib_api.cpp:7, lib/PB_lib/src/pbnet/cluster.h:13-18,
 * cluster.cu:16-119) and the Solver pipeline behind it (binary.cu:19-415, binary_cuda_functions.cu:29-308).
 *
 *  off_xyz   [n,3] f32  offset-shifted coordinates (x,y,z of pbnet_ops.py:16-18 as one AoS slab)
 *  org_xyz   [n,3] f32  original coordinates (xo,yo,zo of pbnet_ops.py:27-29)
 *  sem       [n]   i32  predicted class per point, each in [2,19]
 *  seg_len   [n_seg] i32 points per batch segment (ins_bp of PBNet.py:172; "batch_index" of cluster.h:16);
 *                       segments are contiguous slices in order, empty segments allowed
 *  radius, min_pts      scalars: the reference broadcasts one value to all 18 classes (pbnet_ops.py:33-36)
 *  para_f, nv_flag      pbnet_ops.py:70-71 (0.05, true)
 *  general_sem          0: every segment holds ONE class (how PBNet.forward calls it, PBNet.py:154,176);
 *                       1: classes may be mixed inside a segment ("component x class" rule, cluster.cu/binary.cu:206)
 *  cluster_id [n]  i32 out  global ids across segments (cluster.cu:91-93,108), -1 = unassigned
 *  cluster_num[n_seg] i32 out
 *  den        [n]  i32 out  neighbour count EXCLUDING self (binary.cu:148); the Python op returns den+1.
 *                       With general_sem bit 2 set: min(that count, min_pts) -- exact wherever it decides
 *                       den >= min_pts, which is all the grouping reads; the count stops once it is reached
 *  centers    [3*n] f32 out capacity; first 3*C valid (cluster.cu:112-114 resizes instead)
 *  clt_sem    [n]  i32 out  capacity; first C valid (cluster.cu:116-118)
 *  n_clusters [1]  i32 out  C, in DEVICE memory (no host sync inside)
 *  member_start [n+1] i32 out, optional (NULL to skip): CSR offsets of the members of each final cluster
 *  member_idx   [n]   i32 out, optional: point indices grouped by final cluster id, ascending index inside a
 *                       cluster (= torch.nonzero(cluster_id == c) of PBNet.py:204); unassigned points are absent
 *
 * Arithmetic contract (identical to oracle/pb_cluster_ref.c): d2 = (dx*dx + dy*dy) + dz*dz in unfused binary32,
 * test d2 <= r*r; centre = sequential running mean M += (p-M)/N in index order with IEEE division.
 * Results are bit-exact and independent of scheduling.
 */
size_t pbn_cluster_workspace_bytes(int n_points, int n_segments, int general_sem);

int pbn_binary_cluster(const float* off_xyz, const float* org_xyz, const int32_t* sem, const int32_t* seg_len,
                       int n_points, int n_segments, float radius, int min_pts, float para_f, int nv_flag,
                       int general_sem /* bit 0: general (mixed-class) rule; bit 1: n_points is a CAPACITY -- the points that
                       exist are the first sum(seg_len) rows, a count that stays on the device (capacity-planned forward:
                       no host read-back between class selection and grouping); bit 2: den is not needed beyond
                       den >= min_pts (den = min(count, min_pts), every other output unchanged) */, int32_t* cluster_id, int32_t* cluster_num, int32_t* den, float* centers,
                       int32_t* clt_sem, int32_t* n_clusters, int32_t* member_start, int32_t* member_idx,
                       void* workspace, size_t workspace_bytes, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Proposal x instance IoU.  Replaces PB_lib.get_iou (lib/PB_lib/src/iou/get_iou.h:15, get_iou.cu:12-38).
 *  proposals_idx [S] i32, proposals_offset [P+1] i32, instance_labels [N] i64, instance_pointnum [I] i32,
 *  proposals_iou [P,I] f32 out.  iou = (f32)inter / ((f64)(f32)(len_p + len_i - inter) + 1e-5) rounded to f32.
 */
int pbn_get_iou(const int32_t* proposals_idx, const int32_t* proposals_offset, const int64_t* instance_labels,
                const int32_t* instance_pointnum, float* proposals_iou, int n_instance, int n_proposal,
                pbn_stream_t stream);

/* Replaces PB_lib.cal_iou_and_masklabel (lib/PB_lib/src/cal_iou_and_masklabel/cal_iou_and_masklabel.h:14-16,
 * cal_iou_and_masklabel.cu:15-107).  Exported by the reference but never called by its Python; kept so the
 * module symbol table is identical.  mask_label must be pre-filled with -1 by the caller (pbnet_ops.py:121). */
int pbn_cal_iou_and_masklabel(const int32_t* proposals_idx, const int32_t* proposals_offset,
                              const int64_t* instance_labels, const int32_t* instance_pointnum,
                              float* proposals_iou, int n_instance, int n_proposal,
                              const float* mask_scores_sigmoid, float* mask_label, int mode, pbn_stream_t stream);


/* ------------------------------------------------------------------------------------------------------------
 * Sparse-voxel backbone: coordinate hashing and kernel maps.
 * Re-creates the coordinate-manager behaviour the reference obtains from MinkowskiEngine, an un-vendored,
 * un-pinned third-party dependency (README.md:15-27): ME.SparseTensor construction (network/PBNet.py:117,240-247,
 * 265-271), ME.utils.sparse_quantize (datasets/scannetv2/dataset_preprocess.py:269-272), strided / transposed
 * coordinate maps and kernel maps behind MinkowskiConvolution(Transpose) (network/Mink.py:221-288).
 * Coordinates are int32 rows (batch, x, y, z); batch in [0,65534], x/y/z in [-32768,32767].
 * Hash tables are caller-owned: keys uint64[capacity], vals int32[capacity], capacity = pbn_hash_capacity(n).
 * Data-dependent row counts are written to DEVICE ints; a count of -1 flags an out-of-range coordinate.
 * `n_*_dev` inputs may be NULL (then the *_max value is the exact count).
 */
int pbn_hash_capacity(int n);
size_t pbn_coords_workspace_bytes(int n_max);

/* De-duplicate rows: first occurrence survives, survivors keep ascending original order.
 * unique_index[n_unique] (original row of each survivor), inverse[n] (survivor id of every input row, may be NULL),
 * unique_coords[n_unique,4] (may be NULL).  The table maps coordinate -> survivor id afterwards. */
int pbn_coords_unique(const int32_t* coords, const int32_t* n_dev, int n_max, uint64_t* table_keys, int32_t* table_vals,
                      int capacity, int32_t* unique_index, int32_t* inverse, int32_t* unique_coords, int32_t* n_unique,
                      void* workspace, size_t workspace_bytes, pbn_stream_t stream);

/* Coarser coordinate set floor(c / stride_out) * stride_out (first-occurrence order) of a unique fine set whose
 * tensor stride is stride_out/2.  parent_row[n_fine], child_k[n_fine] in [0,8) (kernel index of the k=2,s=2
 * convolution, x fastest), nbr_down[n_coarse,8] child rows (-1 = absent).  The table maps coarse coordinate -> row. */
int pbn_coords_stride(const int32_t* fine_coords, const int32_t* n_fine_dev, int n_fine_max, int stride_out,
                      uint64_t* table_keys, int32_t* table_vals, int capacity, int32_t* coarse_coords,
                      int32_t* parent_row, int32_t* child_k, int32_t* nbr_down, int32_t* n_coarse, void* workspace,
                      size_t workspace_bytes, pbn_stream_t stream);

/* Output-stationary kernel map: nbr[row, k] = row of (out_coords[row] + offsets[k]) in the table, or -1.
 * offsets int32[n_offsets,3] (already multiplied by the tensor stride). */
int pbn_kernel_map(const int32_t* out_coords, const int32_t* n_out_dev, int n_out_max, const int32_t* offsets,
                   int n_offsets, const uint64_t* table_keys, const int32_t* table_vals, int capacity, int32_t* nbr,
                   pbn_stream_t stream);

/* Kernel map of a K^3 hyper-cube whose offsets are generated on the fly: odd K centred, even K not, offsets scaled by
 * tensor_stride, first spatial dimension fastest when x_fastest != 0 (the MinkowskiEngine convention assumed here). */
int pbn_kernel_map_cube(const int32_t* out_coords, const int32_t* n_out_dev, int n_out_max, int kernel_size,
                        int tensor_stride, int x_fastest, const uint64_t* table_keys, const int32_t* table_vals,
                        int capacity, int32_t* nbr, pbn_stream_t stream);

/* Table of the transposed k=2,s=2 convolution: nbr_up[fine_row, k] = parent row for k == child_k[fine_row], else -1. */
int pbn_up_table(const int32_t* parent_row, const int32_t* child_k, const int32_t* n_fine_dev, int n_fine_max,
                 int32_t* nbr_up, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Sparse convolution forward (implicit GEMM on MFMA), replacing MinkowskiConvolution / MinkowskiConvolutionTranspose /
 * MinkowskiLinear forward as used at network/Mink.py:293-350 and network/PBNet.py:43-82,121-123,249,273-277:
 *     out[o, c] = act( (sum_k sum_ci in[nbr[o,k], ci] * W[k, ci, c]) * scale[c] + shift[c] + residual[o, c] )
 *  in_feat   [n_in, ld_in] T  input slab (pointer already advanced to the first input column); padding columns
 *                            up to vecs_per_offset*(16/sizeof(T)) must be readable and finite.  Rows are gathered
 *                            with 32-bit byte offsets: n_in*ld_in*sizeof(T) must be < 2 GiB, else PBN_ERR_RANGE
 *                            (entries of nbr outside [0, n_in) read zeros, never memory outside the slab)
 *  nbr       [n_out, n_offsets] i32 or NULL (identity: 1x1 convolution / linear, n_offsets must be 1)
 *  row_perm  optional processing order (tile position p computes output row row_perm[p])
 *  w_packed  weights in MFMA fragment order: [n_steps][cout_padded/16][64 lanes][16 bytes] where lane l of
 *            (step s, tile t) holds W_flat[(4*s + l/16)*E + j, 16*t + l%16], j < E = 16/sizeof(T), and W_flat is
 *            W[k, ci, c] flattened over (k, ci) with ci padded to vecs_per_offset*E; zero outside the real extent
 *  scale/shift [cout_padded] f32 or NULL (folded eval-mode BatchNorm / bias)
 *  residual  [*, ld_res] T or NULL;  relu != 0 applies max(.,0);  out_feat [*, ld_out] T, cout_padded columns written
 *  dtype     PBN_F32 (v_mfma_f32_16x16x4_f32, exact fp32: the parity configuration), PBN_BF16, PBN_F16
 *  rows_per_wave 0 = automatic choice of kernel family and tile (production); 16 / 32 = the workgroup-tile family of
 *                csrc/spconv.hip with that many rows per wave; >= 100 = the wave-autonomous family of
 *                csrc/spconv_wave.hip in configuration 1000*ksplit + 100*NF + NT (NF 16-row fragments per wave, NT
 *                16-channel tiles per workgroup; PBN_ERR_UNSUPPORTED for a combination that is not built) -- the explicit
 *                values exist for tests and tuning.
 *  workspace     optional scratch (16-byte aligned) for split-K launches: when the row count is too small to fill the
 *                256 CUs the reduction axis is cut into slices whose fp32 partial sums go through this buffer and are
 *                combined in a fixed order by a second kernel; NULL / too small => single-pass launch.
 *  fp32 accumulation, fixed summation order: results are deterministic (bit-identical run to run).
 */
int pbn_spconv_forward(const void* in_feat, int ld_in, int n_in, const int32_t* nbr, int n_offsets, const int32_t* row_perm,
                       const int32_t* n_out_dev, int n_out, const void* w_packed, int vecs_per_offset, int n_steps,
                       int cout_padded, const float* scale, const float* shift, const void* residual, int ld_res,
                       int relu, void* out_feat, int ld_out, int dtype, int rows_per_wave, void* workspace,
                       size_t workspace_bytes, pbn_stream_t stream);

/* The same convolution with a SECOND SOURCE folded into its reduction (round 4): a BasicBlock's 1x1 shortcut
 * (network/Mink.py:77-87: `downsample` = 1x1 convolution + BatchNorm on the block input, added before the last ReLU)
 * becomes extra reduction steps of the block's second convolution --
 *     out[o, c] = act( (sum_k sum_ci in[nbr[o,k], ci] W[k, ci, c] + sum_cj in2[o, cj] W2[cj, c]) * scale[c] + shift[c] + ... )
 * -- one launch and no residual slab instead of two launches.  w_packed holds the steps of the map followed by the steps of
 * the second source: vecs_second / 4 of them, zero-padded by the caller to a whole number of barrier groups of the first
 * source (largest divisor <= 4 of vecs_per_offset / 4), n_steps = the total.  BatchNorm scales of the two branches differ:
 * the caller folds them into the packed weights (scale NULL) and passes the summed shifts.  Both sources: vectors per row a
 * multiple of 4; in2 has at least n_out rows (row o pairs with output row o). */
int pbn_spconv_forward_dual(const void* in_feat, int ld_in, int n_in, const int32_t* nbr, int n_offsets,
                            const int32_t* n_out_dev, int n_out, const void* w_packed, int vecs_per_offset, int n_steps,
                            int cout_padded, const float* scale, const float* shift, const void* residual, int ld_res,
                            int relu, void* out_feat, int ld_out, int dtype, int rows_per_wave, void* workspace,
                            size_t workspace_bytes, const void* in2_feat, int ld_in2, int n_in2, int vecs_second,
                            pbn_stream_t stream);

/* Which kernel family pbn_spconv_forward's automatic choice (rows_per_wave = 0) gives a launch of this shape: 0 workgroup-tile
 * (csrc/spconv.hip), 1 wave-autonomous (spconv_wave.hip), 2 row-stationary (spconv_rs.hip); the experiments library with
 * PBN_CONV_PC set may answer 3, pair-compacted.  No launch; for reports. */
int pbn_spconv_family(int n_out, int n_offsets, int vecs_per_offset, int n_steps, int cout_padded, int dtype, int has_map);

/* out[i, :] = in[idx[i], :] on 16-byte multiples (voxel -> point gathers, network/PBNet.py:130-134,250); a negative
 * index gives a zero row (padding slots of the compacted weight-gradient operands). */
int pbn_gather_rows(const void* in, int ld_in_bytes, const int64_t* idx, int n, int row_bytes, void* out,
                    int ld_out_bytes, pbn_stream_t stream);

/* Per-batch global max and/or average pooling of a slab whose rows are grouped by batch index
 * (MinkowskiGlobalMaxPooling / MinkowskiGlobalAvgPooling of the score branch, network/PBNet.py:67-68,274-276).
 * seg_start int32[n_seg+1] row offsets; out_max / out_avg f32 [n_seg, channels] (either may be NULL).
 * An empty segment yields -inf / NaN exactly like the reductions it replaces.  Deterministic.
 * workspace (optional, pbn_segment_pool_workspace_bytes): lets long segments be reduced by many workgroups in two
 * fixed-order passes; without it every (segment, 32-channel chunk) is one workgroup. */
size_t pbn_segment_pool_workspace_bytes(int n_seg, int channels);
int pbn_segment_pool(const void* feats, int ld, int channels, int dtype, const int32_t* seg_start, int n_seg,
                     float* out_max, float* out_avg, void* workspace, size_t workspace_bytes, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Stage glue of PBNet.forward (csrc/front.hip, csrc/heads.hip): each call replaces a run of small tensor ops of the
 * reference by one launch with identical integer results and the same fp32 arithmetic.  Where a size is followed by a
 * device count (n_dev, n_ent_dev, n_rows_dev: the first int32 word is read on the device) the size is a CAPACITY and the
 * launch covers min(count, capacity); a NULL count means the size is exact (capacity-planned inference, below).
 *
 * pbn_local_scene_rows -- rows of every local scene (network/PBNet.py:182-247).  Entry e (one grouping cluster taking
 * part in one local scene) owns rows [ent_row_start[e], ent_row_start[e+1]); row j of it is the point
 * ins_ind[member_idx[ent_member_start[e] + j]].  Per row: point_idx, row_scene = ent_scene[e], the mask-branch voxel
 * coordinate (scene, floor(xyz * inv_voxel)) -- the reference divides a device tensor by a host scalar, which is a
 * multiplication by the fp32 reciprocal -- and the mask-branch input row
 *   [point_feat[p, 0:channels], sem_score[p, sem_pred[p]], ent_weight[e], 0 ... 0]   (ld_out elements of `dtype`);
 * sem_pred NULL = column 0 (sem_score is then the per-point own-class score of pbn_sem_argmax_table).
 * n_ent_dev / n_rows_dev: both NULL or both given (PBN_ERR_ARG otherwise).
 *
 * pbn_gather_pad_rows -- out[i, 0:row_bytes] = in[idx2[idx[i]], 0:row_bytes] (either index NULL = identity), the rest of
 * the output row zero-filled: builds a 16-byte-aligned, zero-padded input slab in one pass.  All byte counts multiples of 4. */
int pbn_local_scene_rows(const int32_t* ent_row_start, const int32_t* ent_member_start, const int32_t* ent_scene,
                         const float* ent_weight, int n_ent, int n_rows, const int32_t* n_ent_dev,
                         const int32_t* n_rows_dev, const int32_t* member_idx, const int64_t* ins_ind, const float* xyz,
                         float inv_voxel, const void* point_feat, int ld_feat, int channels, const void* sem_score,
                         int ld_sem, const int64_t* sem_pred, int dtype, int64_t* point_idx, int64_t* row_scene,
                         int32_t* coords, void* feat_out, int ld_out, pbn_stream_t stream);
int pbn_gather_pad_rows(const void* in, int ld_in_bytes, int row_bytes, const int64_t* idx, const int64_t* idx2, int n,
                        const int32_t* n_dev, void* out, int ld_out_bytes, pbn_stream_t stream);

/* pbn_pack_weight -- fp32 master weights [n_offsets, dim_a, dim_b] (the reference's `kernel` layout [K, Cin, Cout]) into
 * the `w_packed` fragment order pbn_spconv_forward reads, in one launch.  flip mirrors the offsets (K-1-k), transpose
 * swaps the channel roles: flip + transpose of a centred forward kernel are its input-gradient weights.
 * vecs_per_offset / n_steps / cout_padded as for pbn_spconv_forward with (Cin, Cout) = transpose ? (dim_b, dim_a) :
 * (dim_a, dim_b).  out: n_steps * cout_padded/16 * 1024 bytes. */
int pbn_pack_weight(const float* src, int n_offsets, int dim_a, int dim_b, int flip, int transpose, int dtype,
                    int vecs_per_offset, int n_steps, int cout_padded, void* out, pbn_stream_t stream);

/* pbn_pack_weights_batch -- the same packing for many layers in ONE launch (a training step repacks every layer's forward
 * and input-gradient weights once): `jobs` is a DEVICE array of n_jobs descriptors with pbn_pack_weight's arguments
 * (cin / cout / cin_p = vecs_per_offset * elements-per-16-bytes spelled out), max_vectors = the largest job's
 * n_steps * cout_p/16 * 64 (sizes the grid).  All jobs share `dtype`. */
typedef struct pbn_pack_job {
    const float* src;      /* fp32 master [n_offsets, dim_a, dim_b] */
    void* out;             /* n_steps * cout_p/16 * 1024 bytes */
    int32_t n_offsets, dim_a, dim_b, flip, transpose, cin, cout, cin_p, cout_p, n_steps;
    int32_t reserved[2];
} pbn_pack_job;
int pbn_pack_weights_batch(const pbn_pack_job* jobs, int n_jobs, int max_vectors, int dtype, pbn_stream_t stream);

/* Train-mode batch normalisation of a feature slab x[n, channels] (row stride ld_* elements, rows 16-byte aligned;
 * ME.MinkowskiBatchNorm = torch.nn.BatchNorm1d on .F, /root/reference/network/Mink.py:71-73,224; training, configs[2]).
 *   forward : save_mean / save_invstd f32[channels] from the batch (biased variance), running_mean / running_var (NULL =
 *             not tracked) updated with `momentum` and the unbiased variance, y = (x - mean) * invstd * weight + bias
 *             (weight / bias NULL = 1 / 0).  fp32 arithmetic, sums merged in a fixed order (double for the final merge).
 *   backward: dx, dweight = sum dy * xhat, dbias = sum dy (either may be NULL).
 * workspace: pbn_bn_workspace_bytes(channels), 16-byte aligned; its FIRST 16 BYTES must be zero when a workspace is used for the
 * first time (a ticket counter of the fused merge step -- small slabs merge their block sums in the last workgroup to
 * finish instead of a second launch -- which every call leaves at zero again); one workspace per stream.
 * PBN_ERR_UNSUPPORTED when channels is not a multiple of the 16-byte
 * vector width of `dtype` or a row is not 16-byte aligned (the caller then uses the framework's batch norm). */
size_t pbn_bn_workspace_bytes(int channels);
int pbn_bn_train_forward(const void* x, int ld_x, int n, int channels, int dtype, const float* weight, const float* bias,
                         float eps, float momentum, float* running_mean, float* running_var, void* y, int ld_y,
                         float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, pbn_stream_t stream);
int pbn_bn_train_backward(const void* x, int ld_x, const void* dy, int ld_dy, int n, int channels, int dtype,
                          const float* weight, const float* save_mean, const float* save_invstd, void* dx, int ld_dx,
                          float* dweight, float* dbias, void* workspace, size_t workspace_bytes, pbn_stream_t stream);

/* The same passes with the tail of the reference's blocks fused in (Mink.py:293-350, resnet block: conv -> bn -> relu and
 * conv -> bn -> += residual -> relu):
 *   forward : y = act(bn(x) [+ residual]) with act = max(., 0) when relu != 0 (residual NULL = none);
 *   backward: g = dy where y > 0 else 0 (y = the forward output; NULL = no activation), dx / dweight / dbias from g,
 *             dres (NULL = not wanted) = g, the gradient of the residual branch.
 * Statistics, running buffers, workspace, summation order and error codes as pbn_bn_train_forward / _backward. */
int pbn_bn_act_train_forward(const void* x, int ld_x, int n, int channels, int dtype, const float* weight, const float* bias,
                             float eps, float momentum, float* running_mean, float* running_var, const void* residual,
                             int ld_res, int relu, void* y, int ld_y, float* save_mean, float* save_invstd, void* workspace,
                             size_t workspace_bytes, pbn_stream_t stream);
int pbn_bn_act_train_backward(const void* x, int ld_x, const void* dy, int ld_dy, const void* y, int ld_y, int n, int channels,
                              int dtype, const float* weight, const float* save_mean, const float* save_invstd, void* dx,
                              int ld_dx, void* dres, int ld_dres, float* dweight, float* dbias, void* workspace,
                              size_t workspace_bytes, pbn_stream_t stream);

/* Offset-major pair lists of an output-stationary map (training, BASELINE configs[2]): the rule pairs of ME's
 * convolution weight gradient, dW[k] = sum over pairs (i, o) of offset k of x[i]^T g[o].
 *   pbn_rulebook_pair_counts : table int32[pbn_rulebook_pair_blocks(n), K] (per-block prefix counts, kept for the fill)
 *                              and totals int32[K] (pairs per offset) -- the caller reads the totals back, gives every
 *                              offset ceil(total/seg) segments of `seg` pairs and passes their first-segment indices
 *   pbn_rulebook_pair_fill   : in_idx / out_idx int32[n_segments * seg] (-1 = padding; int64 until round 3), seg_offset int64[n_segments]
 *                              the caller passes n_segments >= the segments the map needs; a surplus segment reads -1 / offset 0
 * nbr[o, k] >= 0 is a pair; EVERY negative value (not only -1) is "no pair".  Pairs of an offset keep ascending output-row
 * order; positions are prefix counts (no atomics): deterministic.  More than 512 offsets: the counts succeed, the fill answers
 * PBN_ERR_UNSUPPORTED.  A refused fill has written nothing. */
int pbn_rulebook_pair_blocks(int n);
int pbn_rulebook_pair_counts(const int32_t* nbr, int n, int n_offsets, int32_t* table, int32_t* totals, pbn_stream_t stream);
int pbn_rulebook_pair_fill(const int32_t* nbr, int n, int n_offsets, const int32_t* table, const int32_t* seg_start, int seg,
                           int n_segments, int32_t* in_idx, int32_t* out_idx, int64_t* seg_offset, pbn_stream_t stream);

/* pbn_rulebook_pair_fill_dev -- the same lists with NO host knowledge of the pair counts (no read-back between
 * pbn_rulebook_pair_counts and the fill: a training step builds ~40 maps): seg_begin int32[n_offsets + 1] is computed on the
 * device from `totals`, in_idx / out_idx / seg_offset must hold the worst case of n * n_offsets / segment + n_offsets
 * segments, only the segments below seg_begin[n_offsets] are written and may be read.  The tail of an offset's last segment
 * is NOT padded -- the slots behind an offset's pair count are not written at all --: the consumer bounds every offset by its
 * pair count (pbn_spconv_wgrad: pair_counts = `totals`).  One launch (every block derives seg_begin from the totals itself);
 * n_offsets <= 512, beyond that PBN_ERR_UNSUPPORTED with nothing written. */
int pbn_rulebook_pair_fill_dev(const int32_t* nbr, int n, int n_offsets, const int32_t* table, const int32_t* totals,
                               int segment, int32_t* seg_begin, int32_t* in_idx, int32_t* out_idx, int64_t* seg_offset,
                               pbn_stream_t stream);

/* pbn_rulebook_pairs_multi -- counts + device-side fill (the two calls above) of up to 16 maps in THREE launches: the
 * training executor needs the lists of all 14 maps of a lineage, most of them small (a launch costs more than their work).
 * Per job the buffers of pbn_rulebook_pair_counts / _fill_dev (table int32[max(pbn_rulebook_pair_blocks(n), 1) * n_offsets]; an
 * empty map keeps one block, which zeroes its table row and publishes its seg_begin).  n_jobs outside 1..16, segment < 1 or a NULL
 * among a job's buffers: PBN_ERR_ARG; a job of more than 512 offsets: PBN_ERR_UNSUPPORTED; either way nothing is launched. */
typedef struct {
    const int32_t* nbr;
    int32_t n, n_offsets;
    int32_t* table;
    int32_t* totals;
    int32_t* seg_begin;
    int32_t* in_idx;
    int32_t* out_idx;
    int64_t* seg_offset;
} pbn_pair_job;
int pbn_rulebook_pairs_multi(const pbn_pair_job* jobs, int n_jobs, int segment, pbn_stream_t stream);

/* Weight gradient of the sparse convolution on the matrix cores (csrc/wgrad.hip), ME's convolution backward w.r.t. the
 * kernel (reached from train.py:57 loss.backward()):  dw[k, ci, co] = sum over the pairs (i, o) of offset k of
 * x[i, ci] * g[o, co].  in_idx / out_idx / seg_begin: the lists of pbn_rulebook_pair_fill, seg_begin int32[K+1] = first
 * `segment`-pair segment of every offset, read on the DEVICE (with lists n_pairs_total only sizes the pair splits: an estimate
 * will do); pair_counts int32[K] (device, may be NULL) = pairs of every offset: without it a workgroup walks the -1 padding of
 * its offset's last segment as well (a stride-16 level holds ~450 pairs per offset in segments of 4096); all lists NULL = identity pairs (1x1 convolution / linear layer; n_offsets 1, n_pairs_total rows).  x [*, ld_x], g [*, ld_g] of `dtype` (widened exactly), dw f32[K, cin, cout], any cin / cout.
 * fp32 accumulation in a fixed order (deterministic).  workspace: pbn_spconv_wgrad_workspace_bytes (pair splits). */
size_t pbn_spconv_wgrad_workspace_bytes(int n_offsets, int cin, int cout);
int pbn_spconv_wgrad(const void* x, int ld_x, const void* g, int ld_g, int dtype, const int32_t* in_idx,
                     const int32_t* out_idx, const int32_t* seg_begin, const int32_t* pair_counts, int segment,
                     int n_pairs_total, int n_offsets, int cin, int cout, float* dw, void* workspace, size_t workspace_bytes,
                     pbn_stream_t stream);
/* The same with the caller's row counts: PBN_ERR_RANGE when a slab reaches 4 GiB (the kernels address rows with 32-bit byte
 * offsets) or the lists 2^30 pairs, PBN_ERR_ARG for device-built (unpadded) lists without pair_counts unless the caller declares
 * them padded (pbn_rulebook_pair_fill pads with -1), or for more identity pairs than rows.  What the package itself calls. */
int pbn_spconv_wgrad_checked(const void* x, int ld_x, long long n_x_rows, const void* g, int ld_g, long long n_g_rows, int dtype,
                             const int32_t* in_idx, const int32_t* out_idx, const int32_t* seg_begin, const int32_t* pair_counts,
                             int lists_padded, int segment, int n_pairs_total, int n_offsets, int cin, int cout, float* dw,
                             void* workspace, size_t workspace_bytes, pbn_stream_t stream);
/* What pbn_spconv_wgrad launches for a call of this shape (csrc/wgrad_plan.h; the launch follows the same function under the
 * same PBN_WGRAD_* environment, so the answer is the plan of the next launch).  form 0: k_wgrad<T> (f32 MFMA; wa = wb = 0),
 * 1: k_wgrad_ring<T, wa, wb, identity>; small_level: quarter tiles instead of pair splits; strips = channel-tile strips of
 * one offset, co_groups of them per input-channel group; splits > 1: partial slabs in the workspace + k_wgrad_reduce;
 * grid = workgroups of the main launch.  aligned16: both slab bases are 16-byte aligned; identity: no pair lists;
 * has_workspace: a workspace pointer is passed.  Host code, no HIP call: answers without a GPU.  PBN_ERR_ARG where the
 * launch refuses the same arguments (sizes < 1, n_pairs_total < 0, unknown dtype, identity with n_offsets != 1); with
 * n_pairs_total = 0 the launch only zero-fills dw. */
typedef struct {
    int32_t form, wa, wb, small_level, strips, co_groups, splits;
    int64_t grid;
} pbn_wgrad_plan;
int pbn_spconv_wgrad_plan(int dtype, int ld_x, int ld_g, int aligned16, int identity, int n_offsets, int n_pairs_total, int cin,
                          int cout, int has_workspace, size_t workspace_bytes, pbn_wgrad_plan* out);

/* ------------------------------------------------------------------------------------------------------------
 * Capacity-planned inference (csrc/plan.hip): the data-dependent sizes of PBNet.forward stay on the device.  Every buffer
 * is allocated at a CAPACITY chosen by the caller (pbnet_amd/planned.py takes them from a previous forward of a scene of the
 * same size class); kernels read the true counts from `counts` (int32[PBN_CNT_WORDS]) and raise bits of
 * counts[PBN_CNT_OVERFLOW] instead of writing past a capacity (the caller then falls back to the size-exact path).
 * The stage kernels (csrc/front.hip, csrc/heads.hip) take (capacity, pointer to the device-side count).
 *   pbn_class_gate       network/PBNet.py:151-160,172-173: classes with (float)count < thr05[c] are dropped; class_base[c]
 *                        = first output slot of class c (-1 dropped), seg_len[(c-2)*nb + b] = points of (class, batch)
 *                        (0 for dropped classes: the grouping skips empty segments), counts[PBN_CNT_POINTS].
 *   pbn_local_plan       network/PBNet.py:182-234 for task 'test': one local scene per cluster; entry table in the layout
 *                        pbn_local_scene_rows reads; counts[ENTRIES, ROWS, SCENES, CLUSTERS].  kNN of the cluster centres:
 *                        ascending (d^2, id) with d^2 = (dx^2+dy^2)+dz^2 in unfused fp32.
 *                        cluster_num / member_start / centers describe all *n_clusters clusters; scenes are made for the first
 *                        C = min(*n_clusters, c_cap) (PBN_OVF_CLUSTERS beyond), whose neighbours may be clusters >= C.
 *                        Written: ent_row_start[0 .. n_ent], the other three entry arrays [0 .. n_ent), nothing beyond.
 *                        counts[CLUSTERS] = C on EVERY path.  More entries than e_cap (PBN_OVF_ENTRIES): ENTRIES = ROWS =
 *                        SCENES = 0, ent_row_start[0] = 0 and no other entry word is written.  More rows than r_cap
 *                        (PBN_OVF_ROWS): the same three counts are 0, the entry arrays are written all the same.
 *   pbn_proposal_offsets network/PBNet.py:330-345: proposals_offset i64[s_cap+1], surviving scene ids, dense renumbering;
 *                        counts[PROPOSALS, PROPOSAL_ROWS].
 *   pbn_batch_starts     seg_start[s] = first row of a batch-sorted [n,4] coordinate list whose batch index is >= s. */
enum {
    PBN_CNT_POINTS = 0, PBN_CNT_CLUSTERS = 1, PBN_CNT_ENTRIES = 2, PBN_CNT_ROWS = 3, PBN_CNT_SCENES = 4,
    PBN_CNT_PROPOSAL_ROWS = 5, PBN_CNT_PROPOSALS = 6, PBN_CNT_OVERFLOW = 7, PBN_CNT_WORDS = 16
};
enum {
    PBN_OVF_POINTS = 1, PBN_OVF_CLUSTERS = 2, PBN_OVF_ENTRIES = 4, PBN_OVF_ROWS = 8, PBN_OVF_SEGMENT = 16,
    PBN_OVF_BATCH = 32, PBN_OVF_LEVEL = 64,
    PBN_OVF_CDIST = 128     /* pbn_local_plan: a (class, batch) segment with more than 25 clusters needed its neighbours ranked --
                             * torch.cdist (PBNet.py:201) switches to its matrix-multiply distance there, whose rounding can rank near-ties
                             * differently from the direct d^2 of this plan: the caller takes the reference's own call (host plan) */
};
int pbn_class_gate(const int32_t* table, const float* thr05, int n_classes, int nb, int m_cap, int n_points,
                   int32_t* class_base, int32_t* seg_len, int32_t* counts, pbn_stream_t stream);
size_t pbn_local_plan_workspace_bytes(int c_cap);
int pbn_local_plan(const int32_t* cluster_num, int n_segments, int nb, const int32_t* member_start, const float* centers,
                   const int32_t* n_clusters, const float* thr02, const int32_t* kmax, int c_cap, int e_cap, int r_cap,
                   int32_t* ent_row_start, int32_t* ent_member_start, int32_t* ent_scene, float* ent_weight,
                   int32_t* counts, void* workspace, size_t workspace_bytes, pbn_stream_t stream);
int pbn_proposal_offsets(const int32_t* per_scene, int s_cap, int64_t* proposals_offset, int64_t* alive_ids,
                         int32_t* dense_of, int32_t* counts, pbn_stream_t stream);
int pbn_batch_starts(const int32_t* coords, const int32_t* n_dev, int n_cap, int n_segments, int32_t* seg_start,
                     pbn_stream_t stream);

/* pbn_mlp_rows (csrc/heads.hip) -- the two-layer heads of network/PBNet.py:43-82 in eval mode, one launch per head:
 *   out[i, 0:n_out] = act( W2 . prelu( (W1 . x) * scale + shift ) + b2 ),   x = in[row(i), 0:channels],
 *   row(i) = idx_b[idx_a[i]] (either index level may be NULL), act = sigmoid or identity.
 * W1 f32[hidden, channels], scale/shift = eval-mode BatchNorm folded (f32[hidden]), slope f32[hidden] (PReLU),
 * W2 f32[n_out, hidden], b2 f32[n_out] or NULL.  fp32 arithmetic, one rounding to `dtype` at the end.
 * in_rows: the row capacity of `in`; a resolved row index outside [0, in_rows) reads as a row of zeros (an index table of a
 * level that overflowed its capacity names rows that were never computed).  in_rows < 0: the rows are not bounded.
 * n_dev: device count of the rows (NULL = n is exact).
 * channels must be 32 and hidden 16 or 32 (the shapes PBNet builds); anything else returns PBN_ERR_UNSUPPORTED. */
int pbn_mlp_rows(const void* in, int ld_in, int in_rows, int channels, const int64_t* idx_a, const int64_t* idx_b, int n,
                 const int32_t* n_dev, const float* w1, const float* scale, const float* shift, const float* slope, int hidden,
                 const float* w2, const float* b2, int n_out, int sigmoid, void* out, int ld_out, int dtype,
                 pbn_stream_t stream);

/* pbn_sem_argmax_table -- network/PBNet.py:134,151-163: per point the arg-max class (first maximum), the softmax score
 * of that class (1 / sum exp(s - max), fp32, rounded to `dtype`; may be NULL) and the [n_cls, nb] population table
 * (zeroed here; points whose batch index is outside [0, nb) are not counted).  block_hist int32[pbn_select_blocks(n),
 * n_cls] receives the per-block class histogram pbn_select_points needs.
 *
 * pbn_select_points -- network/PBNet.py:151-170: the points of the kept classes in class-major order, ascending point
 * index inside a class (what a stable sort by class yields), written straight to the grouping inputs:
 *   position(i) = class_base[c] + #(j < i with class c);   class_base[c] < 0 drops the class.
 *   ins_ind[pos] = i, ins_orig[pos] = xyz[i], ins_off[pos] = xyz[i] + float(offset[i]) (fp32 add), ins_sem[pos] = c.
 * A negative sem_pred belongs to no class (not selected, no position); labels >= n_cls are not allowed.  class_base need not
 * ascend with the class: the kept classes' ranges must be disjoint, in any order.  Positions no point is sent to are not written. */
int pbn_select_blocks(int n);
int pbn_sem_argmax_table(const void* score, int ld, int n_cls, const int32_t* batch, int nb, int n, int dtype,
                         int64_t* sem_pred, void* sem_prob, int32_t* table, int32_t* block_hist, pbn_stream_t stream);
int pbn_select_points(const int64_t* sem_pred, int n, int n_cls, const int32_t* class_base, const int32_t* block_hist,
                      const float* xyz, const void* offset, int ld_off, int dtype, int64_t* ins_ind, float* ins_orig,
                      float* ins_off, int32_t* ins_sem, pbn_stream_t stream);

/* get_proposal (network/PBNet.py:317-347) and the score-branch inputs (:240-252) as an order-preserving compaction:
 *   pbn_mask_count    : rows with mask_score > thd per local scene (per_scene, zeroed here) and per block of rows
 *                       (block_cnt int32[pbn_select_blocks(n)]); the host turns per_scene into the dense renumbering
 *                       of the surviving scenes ("remove null proposals", :342-345) and the proposal offsets;
 *   pbn_proposal_rows : for every kept row, in row order: proposals_idx = (dense_of[row_scene], point_idx),
 *                       proposals_ms = its mask score and, optionally, the score-branch voxel coordinate
 *                       (dense id, floor(xyz[p] * scale * inv_voxel)) and input feature row point_feat[p, 0:channels].
 * n_dev: device count of the input rows (NULL = n is exact); n_scenes may be a capacity either way. */
int pbn_mask_count(const void* mask_score, int ld, float thd, const int64_t* row_scene, int n, const int32_t* n_dev,
                   int n_scenes, int dtype, int32_t* per_scene, int32_t* block_cnt, pbn_stream_t stream);
int pbn_proposal_rows(const void* mask_score, int ld, float thd, const int64_t* row_scene, const int64_t* point_idx, int n,
                      const int32_t* n_dev, const int32_t* dense_of, const int32_t* block_cnt, const float* xyz, float scale,
                      float inv_voxel, const void* point_feat, int ld_feat, int channels, int dtype, int64_t* proposals_idx,
                      void* proposals_ms, int32_t* coords, void* feat_out, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation-time post-processing (csrc/post.hip) -- eval_map.py:55-123, the step right after PBNet.forward
 * (SURVEY.md 8f rank 1).  A proposal is a bitset over the n_fold = N/3 folded points (pbn_post_words(n_fold) 32-bit
 * words per row) instead of the reference's dense [P, N/3] int mask; all results are integers or fp32 quotients of
 * exact integers, i.e. identical to the reference's tensors.
 *   pbn_proposal_bitmask  : eval_map.py:67-70 (TTA fold `% (point_num/3)`, mask rows) + row sizes (:80)
 *   pbn_mask_iou          : eval_map.py:90-96 for the rows listed in `rows` (NULL = all): iou f32[n_rows, n_rows]
 *   pbn_superpoint_refine : eval_map.py:104-116 + tools/getins.py:72-98: per-point label of the picked clusters (the
 *                           last one containing the point), per-superpoint label histogram hist[n_sp, n_pick+1] (bucket
 *                           n_pick = unlabelled), first arg-max label per superpoint, refined per-point labels and the
 *                           rebuilt cluster bitsets masks_out[n_pick, words] with their sizes (0 = cluster vanished)
 *   pbn_bitmask_to_dense  : int32[n_rows, n_fold] 0/1 tensor of selected rows (the reference's `clusters`)
 * The greedy NMS between the two (tools/mIOU.py:77-87) runs on the host on a [P, P] matrix, as in the reference (the device-
 * resident form below runs it on the device). */
int pbn_post_words(int n_fold);
int pbn_proposal_bitmask(const int64_t* proposals_idx, int n_entries, int n_fold, int n_prop, uint32_t* masks,
                         int32_t* counts, pbn_stream_t stream);
int pbn_mask_iou(const uint32_t* masks, const int32_t* rows, int n_rows, int n_fold, const int32_t* counts, float* iou,
                 pbn_stream_t stream);
int pbn_superpoint_refine(const uint32_t* masks, const int32_t* pick, int n_pick, int n_fold, const int64_t* superpoint,
                          int n_sp, int64_t* seg, int32_t* hist, int64_t* sp_label, int64_t* seg_refined,
                          uint32_t* masks_out, int32_t* counts_out, pbn_stream_t stream);
int pbn_bitmask_to_dense(const uint32_t* masks, const int32_t* rows, int n_rows, int n_fold, int32_t* dense,
                         pbn_stream_t stream);

/* The device-resident form of the same step: every count lives in a device scalar (n_rows, n_pick, n_keep: int32[1]) and every
 * table has the capacity n_prop = P, so no call reads anything back, takes a launch argument computed from device data or sizes an
 * allocation from it.  Called in this order after pbn_proposal_bitmask; P <= pbn_post_max_proposals() (4096: k_post_nms keeps
 * the survivors' scores, order and suppress flags in LDS), above it PBN_ERR_UNSUPPORTED.
 *   pbn_post_select           : rows[P] = ascending proposals with clt_score > score_t (fp32 compare) and counts > npoint_t
 *                               (eval_map.py:74-84), tail -1; writes n_rows and CLEARS status (the first launch of a call)
 *   pbn_mask_iou_dev          : pbn_mask_iou for the first n_rows entries of rows; iou f32[P, P] with row stride P, entries
 *                               outside [n_rows, n_rows) are left as they are
 *   pbn_post_nms              : tools/mIOU.py:77-87 in one workgroup.  Walk order: score descending, among EQUAL scores the
 *                               LOWER survivor index first (the reference's argsort()[::-1] leaves ties to numpy's sort); a
 *                               survivor is picked when no earlier pick has iou[pick][it] > nms_t (fp32 `>`).  pick[P] =
 *                               survivor positions in pick order, pick_rows[P] = their proposal indices, tails -1; n_pick
 *   pbn_superpoint_refine_dev : pbn_superpoint_refine for the n_pick clusters of pick_rows.  hist int32[n_sp_cap, P + 1] (row
 *                               stride P + 1, columns 0..n_pick live, bucket n_pick = unlabelled), sp_label int64[n_sp_cap],
 *                               masks_out uint32[P, words], counts_out int32[P] (0 from row n_pick on).  A superpoint id >=
 *                               n_sp_cap ORs 1 into status and takes no part (its point keeps -100); nothing is written
 *                               outside the tables.  Negative ids take no part, as in pbn_superpoint_refine
 *   pbn_post_compact          : keep[P] = the picked clusters with counts2 > 0 in order (eval_map.py:113-118), tail -1; n_keep;
 *                               scores_out[k] = clt_score[pick_rows[keep[k]]], semantic_id_out[k] = label_table[pred_sem[first
 *                               member]] (:63-65; proposals_offset / pred_sem are int64 or int32 per their flag; a missing
 *                               member or a class outside [0, n_labels) gives -1 and ORs 2 into status), tails 0 / -1;
 *                               clusters int32[P, n_fold] = the kept bitsets as 0/1 rows, rows from n_keep on zero.
 *                               PBN_ERR_RANGE when P * n_fold reaches 2^39 elements */
int pbn_post_max_proposals(void);
int pbn_post_select(const float* clt_score, const int32_t* counts, int n_prop, float score_t, int npoint_t, int32_t* rows,
                    int32_t* n_rows, int32_t* status, pbn_stream_t stream);
int pbn_mask_iou_dev(const uint32_t* masks, const int32_t* rows, const int32_t* n_rows, int n_prop, int n_fold,
                     const int32_t* counts, float* iou, pbn_stream_t stream);
int pbn_post_nms(const float* clt_score, const int32_t* rows, const int32_t* n_rows, int n_prop, const float* iou, float nms_t,
                 int32_t* pick, int32_t* pick_rows, int32_t* n_pick, pbn_stream_t stream);
int pbn_superpoint_refine_dev(const uint32_t* masks, const int32_t* pick_rows, const int32_t* n_pick, int n_prop, int n_fold,
                              const int64_t* superpoint, int n_sp_cap, int64_t* seg, int32_t* hist, int64_t* sp_label,
                              int64_t* seg_refined, uint32_t* masks_out, int32_t* counts_out, int32_t* status,
                              pbn_stream_t stream);
int pbn_post_compact(const int32_t* counts2, const int32_t* pick_rows, const int32_t* n_pick, int n_prop, int n_fold,
                     const float* clt_score, const int64_t* proposals_idx, int n_entries, const void* proposals_offset,
                     int offset_i64, const void* pred_sem, int sem_i64, int64_t n_sem, const int64_t* label_table, int n_labels,
                     const uint32_t* masks2, int32_t* keep, float* scores_out, int64_t* semantic_id_out, int32_t* clusters,
                     int32_t* n_keep, int32_t* status, pbn_stream_t stream);

/* The batched, segmented form (csrc/post_batch.hip): the post-processing of ONE merged forward over all its scenes, without
 * the TTA fold and without a dense [P, n] table.  Every proposal of a merged forward lies in one scene (PBNet.py:167-176); the
 * scene of a proposal is the scene of its first member.  The scene table is host data known at merge time and travels by value:
 *   n_scenes B in [1, PBN_MAX_SCENES]; point_start[0] = 0 <= ... <= point_start[B] = n_points_total (scene j owns the points
 *   point_start[j] .. point_start[j + 1] of the merged arrays); sp_start likewise over the flat vote table: scene j's superpoint
 *   capacity is sp_start[j + 1] - sp_start[j], 0 = the scene brings no superpoints and is refined as if every point were its own
 *   (the vote is skipped).  `superpoint` int64[n_points_total] holds scene-LOCAL ids and is never read on the rows of a scene
 *   without superpoints (NULL when no scene has any).
 * Per scene the steps are those of pbn_post_select .. pbn_post_compact with the same tie rule (score descending, lower position in
 * the scene's own ascending survivor list first); bitsets are over point - point_start[scene] with a row pitch of
 * pbn_post_words(largest scene).  clt_score has element type score_dtype (PBN_F32 / PBN_BF16 / PBN_F16) and is compared in fp32.
 * Outputs (B = n_scenes, P = n_prop):
 *   point_instance int32[n_points_total] : scene-local number of the kept instance that owns the point, or -100
 *   scores f32[B, P], semantic_id int64[B, P], npoints int32[B, P] : scene j's kept instances in pick order in the first n_keep[j]
 *                                          entries of row j; tails 0 / -1 / 0
 *   scalars int32[2 * B]                 : n_keep[B], then status[B] (bit 1: a superpoint id >= the scene's capacity -- the id
 *                                          takes no part and writes nothing; bit 2: a kept proposal's class is outside the label
 *                                          table), per scene
 * pbn_post_batch_workspace_bytes sizes the workspace for (P, n_points_total, B, sp_start[B]) and, when layout is not NULL, reports
 * where the tables lie in it (byte offsets; votes int32[sp_total, P + 1], rows / pick_rows / counts2 / renumber int32[B, P],
 * n_rows / n_pick int32[PBN_MAX_SCENES], seg / seg_refined int32[n_points_total], masks uint32[P, words(n_points_total)], iou
 * f32[P, P]: scene j's block starts at row sum(n_rows[:j]), row stride P).  0 for sizes outside the supported range.
 * pbn_post_batch: thirteen launches, no read-back, no allocation, no launch argument computed from device data.  n_prop = 0 is
 * served (every point -100, n_keep and status 0).  PBN_ERR_UNSUPPORTED above pbn_post_max_proposals() proposals, PBN_ERR_ARG for
 * a scene table that is not as stated, PBN_ERR_WORKSPACE for a workspace that is too small -- all before any launch. */
typedef struct pbn_scene_table {
    int32_t n_scenes;
    int32_t point_start[PBN_MAX_SCENES + 1];
    int32_t sp_start[PBN_MAX_SCENES + 1];
} pbn_scene_table;
typedef struct pbn_post_batch_layout {
    int64_t masks, counts, prop_scene, score, rows, pick_rows, n_rows, n_pick, iou, votes, sp_label, seg, seg_refined, counts2,
        renumber, total_bytes;
} pbn_post_batch_layout;
size_t pbn_post_batch_workspace_bytes(int n_prop, int n_points_total, int n_scenes, int n_sp_total, pbn_post_batch_layout* layout);
int pbn_post_batch(const int64_t* proposals_idx, int n_entries, const void* proposals_offset, int offset_i64, int n_prop,
                   const void* clt_score, int score_dtype, const void* pred_sem, int sem_i64, int n_points_total,
                   pbn_scene_table scenes, const int64_t* superpoint, float score_t, int npoint_t, float nms_t,
                   const int64_t* label_table, int n_labels, int32_t* point_instance, float* scores, int64_t* semantic_id,
                   int32_t* npoints, int32_t* scalars, void* workspace, size_t workspace_bytes, pbn_stream_t stream);

/* The same pass WITH the TTA fold: the merged forward holds `copies` rotated copies of every scene (eval_map.py:48-70,
 * dataset_preprocess.py:308-385: three copies as a batch of 3), and the proposals of all copies of a scene are refined together
 * over the scene's n_j points, exactly as post.hip's single-scene device form does with n_fold = n_j.  The table is over FOLDED
 * points:
 *   n_scenes B >= 1, copies >= 1, B * copies <= PBN_MAX_SCENES (the merged forward's batch elements); point_start[0] = 0 <= ... <=
 *   point_start[B]; scene j has n_j = point_start[j + 1] - point_start[j] points and occupies the merged (unfolded) points
 *   copies * point_start[j] .. copies * point_start[j + 1], copy after copy, as valMerge concatenates them; n_points_merged =
 *   copies * point_start[B].  sp_start as in pbn_scene_table.
 * A proposal belongs to the scene of its first member (merged numbering).  A member's bit is (pt - copies * point_start[j]) % n_j:
 * a member in another copy of the proposal's scene is folded in like any other (eval_map.py:67), a member outside the scene is
 * dropped; duplicate bits after the fold are harmless (atomicOr, sizes from popcount).  Everything else is over folded points:
 * superpoint int64[point_start[B]] (one id per folded point), point_instance int32[point_start[B]], scores / semantic_id / npoints
 * [B, P], scalars = n_keep[B], status[B], and the workspace is pbn_post_batch_workspace_bytes(P, point_start[B], B, sp_start[B]).
 * The class of a kept instance is pred_sem at its UNFOLDED first member through the label table (eval_map.py:64 reads it before the
 * fold), so pred_sem holds n_points_merged entries.  Same tie rule, status bits, proposal limit and launch count (thirteen) as
 * pbn_post_batch, integer atomics only; copies = 1 is pbn_post_batch, byte for byte.  PBN_ERR_ARG for a table that is not as
 * stated, before any launch. */
typedef struct pbn_tta_table {
    int32_t n_scenes;
    int32_t copies;
    int32_t point_start[PBN_MAX_SCENES + 1];
    int32_t sp_start[PBN_MAX_SCENES + 1];
} pbn_tta_table;
int pbn_post_batch_tta(const int64_t* proposals_idx, int n_entries, const void* proposals_offset, int offset_i64, int n_prop,
                       const void* clt_score, int score_dtype, const void* pred_sem, int sem_i64, int n_points_merged,
                       pbn_tta_table units, const int64_t* superpoint, float score_t, int npoint_t, float nms_t,
                       const int64_t* label_table, int n_labels, int32_t* point_instance, float* scores, int64_t* semantic_id,
                       int32_t* npoints, int32_t* scalars, void* workspace, size_t workspace_bytes, pbn_stream_t stream);

/* The scene summary (csrc/summary.hip): what a caller still computes from the results of pbn_post_batch[_tta], in one pass over
 * the FOLDED points of the merged forward, on the same stream and without a read-back.  `units` is the table of
 * pbn_post_batch_tta (copies = 1: the plain merged forward); B = units.n_scenes, P = n_prop, n_j the folded points of scene j,
 * N = point_start[B]; point_instance int32[N] and post_scalars (n_keep[B], ...) are that pass's outputs, n_keep[j] =
 * post_scalars[j] stays on the device (clamped so that the scenes' counts sum to at most P).
 *   sem_fold int32[N]        : sem_score is the forward's score table [n_points_merged, n_cls], row stride ld elements, element type
 *                              score_dtype; the copies of point i of scene j are rows copies * point_start[j] + c * n_j + i.  Per
 *                              class s = widen(copy 0), then s = s + widen(copy c) for c = 1 .. copies - 1, each ONE float32
 *                              addition in that order; the label is the first maximum (`v > best`, as pbn_sem_argmax_table: a NaN
 *                              never wins, an all-NaN row gives class 0).  copies = 1 equals pbn_sem_argmax_table's sem_pred.
 *   class_vote int64[B, P],
 *   class_points int32[B, P] : for the n_keep[j] kept instances of scene j (the rows of scores / semantic_id / npoints): the class
 *                              with the most points among the instance's points, counted on sem_fold, ties to the lower class,
 *                              through label_table (eval_map.py:142-155), and that count.  A class outside [0, n_labels) gives -1
 *                              and ORs 2 into status[j].  Tails -1 / 0.
 *   box f32[B, P, 6],
 *   centroid f32[B, P, 3]    : min xyz then max xyz, and the mean, of the instance's points; xyz f32[N, 3] in the scene's own frame
 *                              (NULL: both tables are left untouched).  Minima and maxima are reduced as order-preserving integer
 *                              keys of the float32 bits; the centre is exact and independent of the order of summation: q =
 *                              (int64) rint(x * 65536.0f) per coordinate (ties to even), summed with integer atomics, centroid =
 *                              (float)((double) sum q / (double) count / 65536.0).  A point with a NaN coordinate or |x| >= 32768
 *                              takes no part in box or centre (it still votes) and ORs 4 into status[j], whether or not it belongs
 *                              to an instance; an instance without a
 *                              valid point gets NaN.  Tails 0.
 *   status int32[B]          : cleared by the first launch; bit 2 and bit 4 as above, bit 8: a point_instance value >= n_keep[j] or
 *                              negative other than -100 (the point counts for no instance).
 * Three launches (clear, fold + accumulate with one lane per folded point, finalise), integer atomics only, so two runs give the
 * same bytes.  A workgroup keeps the accumulators of the scene of its first point in LDS when that scene has at most
 * pbn_scene_summary_lds_instances(n_cls) kept instances (0 = no such path) and adds to the workspace directly otherwise.  The
 * workspace holds one accumulator row per proposal (pbn_scene_summary_workspace_bytes; 0 for sizes outside the supported range),
 * 8-byte aligned.  All before any launch: PBN_ERR_ARG for a table that is not as stated, n_cls outside [1, 32], ld < n_cls, an
 * unknown dtype or a missing pointer; PBN_ERR_UNSUPPORTED above pbn_post_max_proposals(); PBN_ERR_WORKSPACE for a workspace that
 * is too small.  n_prop = 0 is served: sem_fold and status are written, the tables are empty (point_instance, post_scalars,
 * label_table, the tables and the workspace may then be NULL). */
size_t pbn_scene_summary_workspace_bytes(int n_prop, int n_cls);
int pbn_scene_summary_lds_instances(int n_cls);
int pbn_scene_summary(const void* sem_score, int ld, int n_cls, int score_dtype, int n_points_merged, pbn_tta_table units,
                      const int32_t* point_instance, const int32_t* post_scalars, int n_prop, const float* xyz,
                      const int64_t* label_table, int n_labels, int32_t* sem_fold, int64_t* class_vote, int32_t* class_points,
                      float* box, float* centroid, int32_t* status, void* workspace, size_t workspace_bytes, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * ScanNet AP evaluator, the association step of /root/reference/tools/eval.py:205-250
 * (`assign_instances_for_scan`).  The reference counts, for every (prediction, ground-truth instance) pair, the points
 * both contain with one pass over the scene per pair (:239) plus one for the void overlap (:235); here ONE pass per
 * prediction fills a row of the overlap table: inter[p][gt_index[i]] += 1 for every point i with masks[p][i] != 0.
 *   masks    : int32[n_pred, n_pts], any non-zero value = inside (eval.py:226 `np.not_equal(pred_mask, 0)`)
 *   gt_index : int32[n_pts], the point's ground-truth id as an index into the scene's sorted unique id list
 *              (0 <= index < n_gt; the ids themselves -- class*1000+instance+1, 0 = unannotated,
 *              datasets/scannetv2/get_val_gt.py:26-39 -- stay on the host)
 *   inter    : int32[n_pred, n_gt] out (zeroed here).  Row sums are the predictions' vertex counts (:227), columns of
 *              non-benchmark ids sum to the void intersection (:235), the rest are the `intersection` fields (:239).
 * Matching and the precision/recall integration (eval.py:27-190) are integer bookkeeping on these counts: on the host in
 * pbnet_amd/evaluate.py (evaluate_matches, the default), or on the device from the epoch log (pbn_ap_table_*, below). */
int pbn_instance_overlap(const int32_t* masks, int n_pred, int n_pts, const int32_t* gt_index, int n_gt, int32_t* inter,
                         pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The same association without a host stop (csrc/apassoc.hip; pbnet_amd/evaluate.py AssociationLog).  Capacities (p_cap,
 * u_cap, id_cap, n_inst_cap, log_words) come from the host; the live counts n_keep and n_gt are device scalars.  Grids are
 * sized by capacity or fixed and striding, work past a live count leaves, only integer atomics are used (bit-identical from
 * run to run) and nothing waits for the host.  Status bits are ORed into a device word; pbn_ap_record_append consumes it.
 *   pbn_gt_encode_dev        : get_val_gt.py:26-37.  sem / ins: int32 or int64 [n_pts] per their flag; first int32[n_inst_cap]
 *                              is working memory (lowest point index per instance, by atomicMin); ids int32[n_pts] =
 *                              label_table[sem of that point] * 1000 + instance + 1 (semantic -100 = class 0), 0 where
 *                              ins < 0.  An instance id >= n_inst_cap ORs INSTANCE_CAP, a semantic label other than -100
 *                              outside [0, n_labels) ORs SEMANTIC_RANGE; such points get id 0, nothing is written out of bounds
 *   pbn_gt_index_dev         : np.unique(ids, return_inverse=True) through a direct table int32[id_cap] (id_cap <= 2^20, above
 *                              it PBN_ERR_UNSUPPORTED): cleared, filled with the vertex count per id, then walked in ascending
 *                              id order by one workgroup: uid[u_cap], gt_vert[u_cap], n_gt, table[id] = the id's slot;
 *                              gt_index[i] = table[ids[i]].  An id < 0 or >= id_cap ORs ID_RANGE and its point gets -1; more
 *                              than u_cap distinct ids OR ID_COUNT, the ids past the capacity get no slot (index -1) and n_gt
 *                              = u_cap.  ids: int32 or int64 per its flag
 *   pbn_instance_overlap_dev : pbn_instance_overlap on clusters int32[p_cap, n_pts] for the rows p < min(*n_keep, p_cap)
 *                              (n_keep NULL = all rows) and the bins g < min(*n_gt, u_cap); inter int32[p_cap, u_cap] with row
 *                              stride u_cap, cleared over that live rectangle only, the rest left as it is.  LDS histogram for
 *                              u_cap <= 8192, global atomics above.  p_cap <= 65535; p_cap * u_cap < 2^31
 *   pbn_ap_record_append     : appends one scene's record to log int32[log_words].  state int32[8] = used | wanted |
 *                              n_records | overflow | offset of the last record (-1 = not written) | spare, zeroed by the
 *                              caller before the first scene.  A single thread sizes the record from n_keep and n_gt, always
 *                              advances `wanted`, and when the record fits and nothing overflowed before advances `used`,
 *                              writes the header and publishes the offset; otherwise it sets `overflow`, which is sticky.  A
 *                              striding grid then writes the body.  Record: header[PBN_AP_RECORD_HEADER] = magic | scene_tag |
 *                              n_keep | n_gt | n_pts | status (*post_status, NULL = 0, ORed with *assoc_status, which is
 *                              cleared) | record words | 0; then uid[n_gt] | gt_vert[n_gt] | label_id[n_keep] (semantic_id
 *                              int64 narrowed; a value that does not fit ORs LABEL_RANGE into the record) | conf[n_keep] as
 *                              float32 bit patterns | inter[n_keep, n_gt] row-major.  n_keep == 0: the header only */
#define PBN_AP_RECORD_MAGIC 0x41504c47
#define PBN_AP_RECORD_HEADER 8
#define PBN_AP_STATUS_ID_RANGE 4          /* bits 1 and 2 are the post-processing's (pbn_post_compact) */
#define PBN_AP_STATUS_ID_COUNT 8
#define PBN_AP_STATUS_LABEL_RANGE 16
#define PBN_AP_STATUS_INSTANCE_CAP 32
#define PBN_AP_STATUS_SEMANTIC_RANGE 64
int pbn_gt_encode_dev(const void* sem, int sem_i64, const void* ins, int ins_i64, int n_pts, const int32_t* label_table,
                      int n_labels, int32_t* first, int n_inst_cap, int32_t* ids, int32_t* status, pbn_stream_t stream);
int pbn_gt_index_dev(const void* ids, int ids_i64, int n_pts, int32_t* table, int id_cap, int32_t* uid, int32_t* gt_vert,
                     int u_cap, int32_t* n_gt, int32_t* gt_index, int32_t* status, pbn_stream_t stream);
int pbn_instance_overlap_dev(const int32_t* clusters, const int32_t* n_keep, int p_cap, int n_pts, const int32_t* gt_index,
                             const int32_t* n_gt, int u_cap, int32_t* inter, pbn_stream_t stream);
int pbn_ap_record_append(int32_t* state, int32_t* log, int64_t log_words, int scene_tag, const int32_t* n_keep, int p_cap,
                         const int32_t* n_gt, int u_cap, int n_pts, const int32_t* post_status, int32_t* assoc_status,
                         const int32_t* uid, const int32_t* gt_vert, const int64_t* semantic_id, const float* conf,
                         const int32_t* inter, pbn_stream_t stream);

/* The same association for ALL scenes of one merged forward (csrc/apassoc_batch.hip; AssociationLog.append_batch), on what
 * pbn_post_batch[_tta] leaves: one label per folded point, no dense [P, n] table.  `units` is the table of that pass (copies = 1:
 * the plain merged forward; B = units.n_scenes, everything here is over FOLDED points, scene j owns point_start[j] ..
 * point_start[j + 1], N = point_start[B]); point_instance int32[N], post_scalars (n_keep[B], status[B]), scores f32[B, P] and
 * semantic_id int64[B, P] are its outputs, left on the device (P = n_prop).  Ground truth over the same N points: `ids` (int32 or
 * int64 per ids_i64), or ids = NULL and a (sem, ins) pair with label_table[n_labels], encoded per scene as pbn_gt_encode_dev does
 * (the lowest point of an instance is the lowest within its scene).
 * Per scene j, in the order 0 .. B - 1, the log receives exactly the record that pbn_gt_encode_dev (optional), pbn_gt_index_dev,
 * pbn_instance_overlap_dev on the densified labels (row k = the points with point_instance == k) and pbn_ap_record_append write:
 * same layout, header words, magic, n_pts = n_j, scene_tag = tags.tag[j], the same used | wanted | n_records | overflow | last
 * offset state machine with the sticky overflow (wanted always advances, the records before the overflow are whole, none after it
 * is written), status = post_scalars[B + j] ORed with this pass's bits 4 / 8 / 16 / 32 / 64.  n_keep[j] is clamped as
 * pbn_scene_summary does (the scenes' counts sum to at most P); n_keep[j] == 0 gives the header alone.  A point counts for
 * inter[k][g] only when its label k lies in [0, n_keep[j]) and its id has a slot g >= 0; -100 and every other label outside that
 * range count for no prediction and are no error here.
 * Six launches whatever B is (eight with the (sem, ins) form; four / six when n_prop == 0, which is served: B header-only
 * records), no read-back, grids sized by capacity, integer atomics only (two runs give the same log bytes).  One direct table per
 * scene (B x id_cap words, id_cap <= 2^20), walked in ascending id order by one workgroup per scene; uid, gt_vert and n_gt per
 * scene in the workspace.  The overlap counters are the record's own inter words: a workgroup keeps the counters of the scene of
 * its first point in LDS when n_keep * n_gt <= pbn_ap_assoc_batch_lds_counters() and adds to the record directly otherwise, as
 * do its lanes beyond a scene boundary.  pbn_ap_assoc_batch_workspace_bytes(N, B, u_cap, id_cap, n_inst_cap): n_inst_cap = 0 sizes
 * it for the `ids` form only; 0 for sizes outside the supported range.
 * All before any launch: PBN_ERR_ARG for a table that is not as stated, B * copies > PBN_MAX_SCENES, a missing pointer, neither
 * form of the ground truth, or a capacity below 1; PBN_ERR_UNSUPPORTED above pbn_post_max_proposals() proposals or with id_cap >
 * 2^20; PBN_ERR_RANGE for log_words >= 2^31; PBN_ERR_WORKSPACE for a workspace that is too small. */
typedef struct pbn_ap_scene_tags {
    int32_t tag[PBN_MAX_SCENES];
} pbn_ap_scene_tags;
size_t pbn_ap_assoc_batch_workspace_bytes(int n_points_total, int n_scenes, int u_cap, int id_cap, int n_inst_cap);
int pbn_ap_assoc_batch_lds_counters(void);
int pbn_ap_assoc_batch(pbn_tta_table units, const int32_t* point_instance, const int32_t* post_scalars, const float* scores,
                       const int64_t* semantic_id, int n_prop, const void* ids, int ids_i64, const void* sem, int sem_i64,
                       const void* ins, int ins_i64, const int32_t* label_table, int n_labels, int u_cap, int id_cap,
                       int n_inst_cap, pbn_ap_scene_tags tags, int32_t* state, int32_t* log, int64_t log_words, void* workspace,
                       size_t workspace_bytes, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The AP table on the device (csrc/apeval.hip; pbnet_amd/evaluate.py APTable): the reference's tools/eval.py:27-190
 * (`evaluate_matches`) on association logs where they lie -- what comes back is ap[n_classes, n_overlaps] instead of the logs.
 * The table accumulates in a caller-owned workspace (pbn_ap_table_workspace_bytes(rec_cap, entry_cap), host-only, 0 for
 * capacities outside the supported range): rec_cap records over all logs of the epoch, entry_cap (score, true) entries over all
 * cells; the predictions of ONE log's usable records need a row each in the same capacity.  A prediction emits at most one
 * entry per overlap >= 0.5 and at most three at 0.25 (instances are disjoint and IoU > th forces inter > th * vertices), so
 * 12 * (sum of n_keep) entries are always enough.  Either overflow is sticky, reported in the scalar block with the wanted count
 * and never a write out of bounds; the results are then not valid.
 *   pbn_ap_table_reset   : clears the accumulated state (one launch).
 *   pbn_ap_table_add_log : one log (log_state = the int32[8] state block of pbn_ap_record_append, read on the device: the
 *                          used words, and its overflow flag, with which the log is refused as AssociationLog.read_log refuses
 *                          it).  Three launches: (a) ONE wave walks the record headers and appends offset | tag + tag_base |
 *                          status | n_keep per record to the directory (offset = the record's word in the concatenation of the
 *                          logs added so far); a record that is not whole stops the walk (scalar `malformed` = 1 and its word;
 *                          2 = a record with more than 65535 predictions, which no writer here produces); records with status
 *                          bits or n_keep == 0 are listed and take no part.  (b) per prediction of a usable record: its class
 *                          (index of label_id in `classes`, -1 if absent), its vertex count (row sum over ALL n_gt columns; kept
 *                          when the class is >= 0 and the count >= min_region), and void + too-small same-class overlap; per
 *                          class has_pred (a kept prediction) and has_gt (an instance column -- uid != 0, class of uid / 1000 >=
 *                          0 -- with uid >= 1000 and gt_vert >= min_region).  (c) one wave per (record, overlap): over[q, g] =
 *                          inter > 0 and (double) inter / max(pred_vert + gt_vert - inter, 1) > th for same-class pairs, a
 *                          plain IEEE division and a strict >; for every instance that counts, in column order, predictions in
 *                          prediction order: the first unvisited one with `over` is marked visited and becomes `best`, every
 *                          later hit emits (0, min(best, conf)), raises best and stays unvisited; then (1, best), or one
 *                          hard_fn without a hit.  visited persists over the record's instances at that overlap.  A kept
 *                          prediction without `over` against any same-class instance, small ones included, emits (0, conf)
 *                          when (double)(void + too-small overlap) / vertices <= th.  Entries go to one table as (cell = class *
 *                          n_overlaps + overlap, score bits, true).  A wave keeps visited and the class, instance and counts bits
 *                          of the record's first 4096 columns in LDS; columns beyond are classified where they are met.
 *   pbn_ap_table_finish  : four launches: segment starts, entries into their cells' segments, ONE workgroup per cell, the
 *                          outputs.  A cell's entries are sorted by (score, true) -- in LDS up to pbn_ap_table_lds_entries()
 *                          entries, in place in global memory above, the same network -- and integrated in float64 in ascending
 *                          distinct-score order as eval.py:131-176 does: first position of every distinct score, true matches
 *                          scored strictly lower, tp / fp / fn, precision with the artificial last point 1, recall with 0, the
 *                          [-0.5, 0, 0.5] widths, the sum (each thread its strided terms, then a fixed tree).  ap float32
 *                          [n_classes * n_overlaps]: NaN without has_gt, 0 with has_gt alone or without entries; cells int32
 *                          [n_classes * n_overlaps][4] = entries | true entries | hard_fn | distinct scores; flags int32[2 *
 *                          n_classes] = has_gt | has_pred; directory int32[rec_cap][4], zero past the records; scalars
 *                          int32[PBN_AP_TABLE_SCALARS] = records | records wanted | entries wanted | prediction rows wanted (the
 *                          largest log) | overflow bits (1 records, 2 entries, 4 prediction rows) | malformed | its word | a log
 *                          had overflowed | the words that log wanted | words walked | first record of the last log | logs.
 *                          The table stays as it was: more logs may follow, and a second call gives the same bytes.
 * Integer atomics only; the order in which entries arrive depends on them, the outputs do not (the sort key is total and equal
 * keys are equal entries): two runs give the same bytes.  Nothing waits for the host.  All before any launch: PBN_ERR_ARG for a
 * missing pointer, a capacity below 1, counts outside [1, PBN_AP_MAX_CLASSES] / [1, PBN_AP_MAX_OVERLAPS], a class id below 1 (0 is
 * the unannotated id), a negative tag_base or min_region, an overlap outside [0, 1]; PBN_ERR_RANGE for entry_cap >= 2^30, rec_cap >= 2^29 or log_words >= 2^31;
 * PBN_ERR_WORKSPACE for a workspace that is too small. */
#define PBN_AP_MAX_CLASSES 32
#define PBN_AP_MAX_OVERLAPS 16
#define PBN_AP_TABLE_SCALARS 16
typedef struct pbn_ap_class_ids {
    int32_t n;
    int32_t id[PBN_AP_MAX_CLASSES];
} pbn_ap_class_ids;
typedef struct pbn_ap_overlaps {
    int32_t n;
    int32_t _pad;
    double th[PBN_AP_MAX_OVERLAPS];
} pbn_ap_overlaps;
size_t pbn_ap_table_workspace_bytes(int rec_cap, int64_t entry_cap);
int pbn_ap_table_lds_entries(void);
int pbn_ap_table_reset(void* workspace, size_t workspace_bytes, int rec_cap, int64_t entry_cap, pbn_stream_t stream);
int pbn_ap_table_add_log(void* workspace, size_t workspace_bytes, int rec_cap, int64_t entry_cap, const int32_t* log_state,
                         const int32_t* log, int64_t log_words, int tag_base, pbn_ap_class_ids classes, pbn_ap_overlaps overlaps,
                         int min_region, pbn_stream_t stream);
int pbn_ap_table_finish(void* workspace, size_t workspace_bytes, int rec_cap, int64_t entry_cap, int n_classes, int n_overlaps,
                        float* ap, int32_t* cells, int32_t* flags, int32_t* directory, int32_t* scalars, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * One-call sub-pipelines (csrc/executor.hip): they only sequence the entry points above.
 *
 * pbn_coords_build: everything a MinkUNet needs from one coordinate lineage -- de-duplication, the four coarser
 * levels (tensor strides 2..16), the k=3 maps of all five levels, optionally the k=5 map of level 0, and the four
 * transposed-convolution tables -- laid out in one caller-owned arena.  Every array is sized for n rows (the input
 * size bounds every level); the real row counts are the first five ints at `counts` (device memory, -1 = range error).
 * Layout offsets are bytes from the arena base and are filled by pbn_coords_arena_bytes(). */
typedef struct {
    int64_t counts, unique_index, inverse;
    int64_t keys[5], vals[5], coords[5], k3[5];
    int64_t parent_row[4], child_k[4], nbr_down[4], up[4];
    int64_t k5, workspace, workspace_bytes;
    int32_t capacity[5];
    int32_t _pad;
} pbn_coords_layout;

size_t pbn_coords_arena_bytes(int n, int want_k5, pbn_coords_layout* layout);
int pbn_coords_build(const int32_t* coords, const int32_t* n_dev, int n, int want_k5, int x_fastest, void* arena,
                     size_t arena_bytes, const pbn_coords_layout* layout, pbn_stream_t stream);

/* pbn_coords_prepare: what constructing a SparseTensor and expanding its lineage in Z-order takes, in ONE call
 * (network/PBNet.py:117,240-247,265-271 reach this through ME.SparseTensor): de-duplication of the input rows (first
 * occurrence wins, survivors in ascending input order = the external row order), Z-order sort of the survivors, and the
 * pbn_coords_build expansion of the sorted rows.  Everything lives in one caller-owned arena:
 *   pyramid       the sorted lineage exactly as pbn_coords_build lays it out (counts[0..4] = rows per level, -1 on a
 *                 coordinate range error)
 *   n_unique      int32: survivors (= counts[0])
 *   unique_index  int64[n]: external row -> input row          inverse   int64[n]: input row -> external row
 *   perm          int64[n]: sorted position -> external row    inv_perm  int64[n]: external row -> sorted position
 *   ucoords       int32[n,4]: survivor coordinates in the external order
 * (only the first n_unique entries of the per-survivor arrays are meaningful; the rest of the struct is scratch). */
typedef struct {
    pbn_coords_layout pyramid;
    int64_t n_unique, unique_index, inverse, perm, inv_perm, ucoords;
    int64_t tmp_keys, tmp_vals, uidx32, inv32, sort_keys, sort_vals, sort_temp, sort_temp_bytes;
} pbn_prepare_layout;

size_t pbn_coords_prepare_bytes(int n, int want_k5, pbn_prepare_layout* layout);
int pbn_coords_prepare_dev(const int32_t* coords, const int32_t* n_dev, int n_cap, int want_k5, int x_fastest, void* arena,
                           size_t arena_bytes, const pbn_prepare_layout* layout, pbn_stream_t stream);
int pbn_coords_prepare(const int32_t* coords, int n, int want_k5, int x_fastest, void* arena, size_t arena_bytes,
                       const pbn_prepare_layout* layout, pbn_stream_t stream);
/* The same contract through the hash-table pipeline of pbn_coords_build (one table per level, values renumbered) instead of
 * the sorted, hash-free one: the cross-check of csrc/pyramid.hip (every output array must be equal); n_dev may be null. */
int pbn_coords_prepare_hash(const int32_t* coords, const int32_t* n_dev, int n_cap, int want_k5, int x_fastest, void* arena,
                            size_t arena_bytes, const pbn_prepare_layout* layout, pbn_stream_t stream);

/* Z-order keys (batch-major, then bit-interleaved x, y, z) of coordinate rows; rows at or beyond *n_dev get the largest
 * key.  Sorting rows by this key turns every run of consecutive rows into a compact spatial block: convolution tiles
 * then drop whole offset groups and their gathers stay inside one XCD's L2. */
int pbn_morton_keys(const int32_t* coords, const int32_t* n_dev, int n_max, int64_t* keys, pbn_stream_t stream);

/* pbn_unet_forward: executes a static list of fused convolutions -- MinkUNetBase.forward (network/Mink.py:291-354) with
 * eval-mode BatchNorm, ReLU and residual adds folded into the epilogues and skip concatenations written in place.
 * Buffers are symbolic: buffer 0 is the caller's input slab, buffer b > 0 is [n_rows[level], width] elements inside the
 * arena (offsets from pbn_unet_arena_bytes).  map_kind: 0 identity (1x1 / linear), 1 k=3 at level_out, 2 k=5 (level 0),
 * 3 k=2,s=2 down (level_in = fine level), 4 transposed k=2,s=2 (level_out = fine level). */
typedef struct {
    int32_t map_kind, level_in, level_out;
    int32_t in_buf, in_col, res_buf, res_col, out_buf, out_col;
    int32_t vpo, n_steps, cout_p, relu;
    int32_t in2_buf;            /* >= 0: second source of pbn_spconv_forward_dual (a folded 1x1 shortcut), else -1 */
    int32_t in2_col, vpo2;
    const void* w;
    const float* scale;
    const float* shift;
} pbn_unet_op;

typedef struct {
    int32_t level, width;
} pbn_unet_buf;

size_t pbn_unet_arena_bytes(const pbn_unet_buf* bufs, int n_bufs, const int32_t* n_rows, int dtype, int64_t* buf_offsets);
/* Capacity form: n_rows_cap are capacities, the rows that exist are n_rows_dev[level] (device).  rows_expected (host, 5 ints, read
 * during the call, nothing of the caller's is kept; NULL = choose by the capacities): the rows the caller EXPECTS per level --
 * kernel families and tile shapes are then chosen for them (as the size-exact forward would choose them), grids for the capacities. */
int pbn_unet_forward_dev(const pbn_unet_op* ops, int n_ops, const pbn_unet_buf* bufs, int n_bufs, const int32_t* n_rows_cap,
                         const int32_t* n_rows_dev, const int32_t* rows_expected, const void* input, int ld_input,
                         const int32_t* const* k3, const int32_t* k5, const int32_t* const* down, const int32_t* const* up,
                         void* arena, size_t arena_bytes, int dtype, void* splitk_ws, size_t splitk_bytes, pbn_stream_t stream);
int pbn_unet_forward(const pbn_unet_op* ops, int n_ops, const pbn_unet_buf* bufs, int n_bufs, const int32_t* n_rows,
                     const void* input, int ld_input, const int32_t* const* k3, const int32_t* k5,
                     const int32_t* const* down, const int32_t* const* up, void* arena, size_t arena_bytes, int dtype,
                     void* splitk_ws, size_t splitk_bytes, pbn_stream_t stream);

/* Measurement variant of pbn_unet_forward: brackets every op with HIP events on the launching stream, synchronises the
 * stream before returning and fills op_ms[n_ops] (host) with the per-op durations in milliseconds. */
int pbn_unet_forward_timed(const pbn_unet_op* ops, int n_ops, const pbn_unet_buf* bufs, int n_bufs, const int32_t* n_rows,
                           const void* input, int ld_input, const int32_t* const* k3, const int32_t* k5,
                           const int32_t* const* down, const int32_t* const* up, void* arena, size_t arena_bytes,
                           int dtype, void* splitk_ws, size_t splitk_bytes, pbn_stream_t stream, float* op_ms);

/* ------------------------------------------------------------------------------------------------------------
 * Native TRAINING executor of a MinkUNet body (csrc/train_exec.hip): the train-mode forward of
 * /root/reference/network/Mink.py:291-350 (every convolution but the final 1x1: conv -> bn -> relu, the BasicBlocks with
 * their shortcuts, the skip concatenations written in place) and its backward as ONE call each -- the sequencing that
 * MinkowskiEngine/fused_train.py does from Python in ~330 native calls per network and direction (configs[2] was host-bound).
 * Same kernels, same order, same arithmetic as that path: pbn_spconv_forward (convolutions and input gradients),
 * pbn_bn_act_train_* (batch norm with its tail), pbn_spconv_wgrad.
 *   op       : convolution in (buf, col) -> pre_buf, then y = act(bn(pre) [+ res]) -> (out_buf, out_col).  Buffers are the
 *              pbn_unet_buf list (buffer 0 = the caller's input slab); pbn_unet_arena_bytes lays out BOTH arenas: the
 *              activations (kept for the backward) and, with the same offsets, their gradients.
 *   backward : ops in reverse; the caller has written d(loss)/d(output) into the gradient arena at the output buffer.
 *              dx_accumulate = the gradient of the input view already holds a contribution (a skip, a shortcut): the input
 *              gradient is then added in the convolution's epilogue (residual = out).  The residual gradient of a block is
 *              WRITTEN by the batch-norm backward, so it must be the first contribution of its buffer (the planner checks).
 *   pairs    : the weight gradient's pair lists per map (pbn_rulebook_pair_fill_dev): index 0..4 = k3 of levels 0..4,
 *              5 = k5, 6..9 = down of fine levels 0..3, 10..13 = up of fine levels 0..3; entries of unused maps may be zero.
 *   stats    : f32, per op [mean | invstd] at stat_off; param_grads: f32, per op dW [K, cin, cout] at dw_off, dgamma /
 *              dbeta at their offsets (all in floats). */
typedef struct {
    int32_t map_kind, level_in, level_out;
    int32_t in_buf, in_col, pre_buf, res_buf, res_col, out_buf, out_col;
    int32_t relu, cin, cout;
    int32_t vpo, n_steps, cout_p;            /* forward weights (pbn_pack_weight) */
    int32_t vpo_d, n_steps_d, cout_p_d;      /* input-gradient weights (offsets mirrored for cubes, channel roles swapped) */
    int32_t want_dx, dx_accumulate, _pad;
    const void* w;
    const void* w_d;
    const float* gamma;
    const float* beta;
    float* running_mean;                      /* NULL: statistics not tracked */
    float* running_var;
    float eps, momentum;
    int64_t stat_off, dw_off, dgamma_off, dbeta_off;
} pbn_train_op;

typedef struct {
    const int32_t* in_idx;
    const int32_t* out_idx;
    const int32_t* seg_begin;
    const int32_t* counts;
    int32_t segment, n_pairs_estimate;
} pbn_pair_lists;

int pbn_unet_train_forward(const pbn_train_op* ops, int n_ops, const pbn_unet_buf* bufs, int n_bufs, const int32_t* n_rows,
                           const void* input, int ld_input, const int32_t* const* k3, const int32_t* k5,
                           const int32_t* const* down, const int32_t* const* up, void* act_arena, size_t arena_bytes,
                           float* stats, int dtype, void* splitk_ws, size_t splitk_bytes, void* bn_ws, size_t bn_ws_bytes,
                           pbn_stream_t stream);
int pbn_unet_train_backward(const pbn_train_op* ops, int n_ops, const pbn_unet_buf* bufs, int n_bufs, const int32_t* n_rows,
                            const void* input, int ld_input, const int32_t* const* k3, const int32_t* k5,
                            const int32_t* const* down, const int32_t* const* up, const pbn_pair_lists* pairs,
                            const void* act_arena, void* grad_arena, size_t arena_bytes, const float* stats,
                            float* param_grads, void* dinput, int ld_dinput, int dtype, void* splitk_ws, size_t splitk_bytes,
                            void* bn_ws, size_t bn_ws_bytes, void* wgrad_ws, size_t wgrad_ws_bytes, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Batch construction (csrc/augment.hip): trainMerge / valMerge of datasets/scannetv2/dataset_preprocess.py:178-385.
 * Rows of a batch form one range; a unit (one dataAugment call) and a scene (primary + mix-up partner) are contiguous
 * row segments given by int32 offsets [n+1].  ext = double[n,6] (min xyz, max xyz).  workspace: pbn_aug_workspace_bytes
 * (n_units or n_scenes).  max_*_rows sizes the grid only.  The ext row of a segment without rows is unspecified.  Every
 * entry refuses a count <= 0 of units or scenes and a null pointer with PBN_ERR_ARG before it writes anything.
 * ------------------------------------------------------------------------------------------------------------ */
int pbn_aug_chunks(int n_rows);
size_t pbn_aug_workspace_bytes(int n_segments);
/* out = ((pre_min ? f32(x - f32 min) : x) @ mats[u]) - its min, times scale[u] where has_scale[u]; ext = extent of out. */
int pbn_aug_affine(const float* xyz, const int32_t* unit_off, int n_units, int max_unit_rows, const int32_t* pre_min,
                   const double* mats, const double* scale, const int32_t* has_scale, double* out, double* ext,
                   void* workspace, pbn_stream_t stream);
/* One elastic pass (gran, mag) on the units of desc int32[n_el,5] = (unit, b0, b1, b2, first float of its 3 grids):
 * 6 box-blur passes of the float32 grids in noise (tmp: the same size; both are overwritten), then
 * x += RegularGridInterpolator(g)(x) * mag; ext = extent per unit after the pass.  Rows of units outside desc keep their
 * bits; the ext rows of those units are overwritten with unspecified values (pass flags 0 for them to pbn_aug_sub_min). */
int pbn_aug_elastic(double* xyz, const int32_t* unit_off, int n_units, int max_unit_rows, const int32_t* desc, int n_el,
                    int total_cells, float* noise, float* tmp, int gran, double mag, double* ext, void* workspace,
                    pbn_stream_t stream);
/* x -= ext min for the units with flags[u] != 0. */
int pbn_aug_sub_min(double* xyz, const int32_t* unit_off, int n_units, int max_unit_rows, const int32_t* flags,
                    const double* ext, pbn_stream_t stream);
/* The crop loop of trainMerge (5 tries of crop(), each up to 17 shrink levels) for scenes with mode 0 (mode 1: keep every
 * point).  triples double[n_scenes,85,3] consumed in order (n_triples valid per scene), levels double[17,3] the full_scale
 * of each shrink.  One launch pair per try; state int32[n_scenes,8] (done, next triple, triples used, last try's start,
 * its level, success, error, tries); counts int32[5,n_scenes,17].  ext_pre = extent before, ext_post = after the
 * offset, over all points (before the mask selects rows).  A point is kept when 0 <= x + o and x + o < level on every
 * axis.  counts[t][s][k] is meaningful for the levels k that try t of scene s visits (up to and including the level it
 * stops at); the other levels of a try that ran hold counts of candidates the loop never takes, tries that did not run
 * and mode-1 scenes hold 0.  error 1: a try found no level with at most max_crop_p points (not reachable while
 * levels[16][0] is 0 and max_crop_p >= 0); error 2: the try needed a triple at or beyond n_triples -- the words triples
 * used, last try's start and its level are then unspecified, next triple and tries describe the tries that completed. */
int pbn_aug_crop(const double* xyz, const int32_t* scene_off, int n_scenes, int max_scene_rows, const int32_t* mode,
                 const double* triples, const int32_t* n_triples, const double* levels, int max_crop_p, int min_crop_p,
                 int32_t* counts, int32_t* state, double* ext_pre, double* ext_post, void* workspace, pbn_stream_t stream);
/* Mask + compaction in input order (xyz - ext_post min, f32(rgb + shift[unit]) | nl, sem) and the instance relabelling
 * loop; labels of unit u are shifted by ins_shift[u] (-100 stays).  label_map / present: int32[n_labels]
 * (label_off[n_scenes+1]), scene_i32: int32[2*n_scenes], scan: int32[pbn_aug_chunks(n_rows)+1].
 * scene_info int32[n_scenes,4] = (rows kept, instance_num, first output row, 0); instance_num is the maximum kept label
 * + 1 after relabelling (-99 when every kept label is -100) and 0 for a scene that keeps no row.  Output rows at and
 * beyond the total kept count are not written; scan[0 .. chunks] is the exclusive scan of the kept rows per 2048-row
 * chunk.  n_rows 0 is valid. */
int pbn_aug_compact(const double* xyz, const float* rgb, const float* nl, const int64_t* sem, const int32_t* ins,
                    const double* shift, const int32_t* ins_shift, const int32_t* unit_off, int n_units,
                    const int32_t* scene_off, int n_scenes, const int32_t* mode, const double* triples, const double* levels,
                    const int32_t* state, const double* ext_pre, const double* ext_post, const int32_t* label_off,
                    int32_t* label_map, int32_t* present, int32_t* scene_i32, int32_t* scan, double* xyz_out,
                    float* feat_out, int64_t* sem_out, int32_t* label_out, int32_t* scene_info, int n_rows, int n_labels,
                    pbn_stream_t stream);
/* getInstanceInfo: per instance mean / min / max (float64, fixed-order reduction) and point count; inst_info f32[n,9]
 * (-100 outside an instance), ins = label + inst_off[scene] (-100 stays).  out_start / inst_start: [n_scenes+1].
 * pointnum / stats f32[n_inst,9] (mean, min, max) are not written when n_inst is 0, nothing is when n_rows is 0 too. */
int pbn_aug_instances(const double* xyz, const int32_t* label, const int32_t* out_start, int n_scenes,
                      const int32_t* inst_start, const int32_t* inst_off, int n_inst, int n_rows, int32_t* pointnum,
                      float* stats, float* inst_info, int64_t* ins, pbn_stream_t stream);
/* coords int32[n,4] = (scene, floor(xyz / voxel_size)) of the float64 coordinates; xyz_f32 = float32(xyz). */
int pbn_aug_quantize(const double* xyz, const int32_t* out_start, int n_scenes, int n_rows, double voxel_size,
                     int32_t* coords, float* xyz_f32, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Mesh decode (csrc/mesh.hip): the per-vertex normals of datasets/scannetv2/decode_scannet.py:76-96 and the superpoints of
 * lib/segmentator (csrc/segmentator.cpp:154-252 segment_mesh, :282-357 segment_point, main.py:17's unique relabel), float32
 * operation by operation.  xyz / normals f32[V,3]; faces [F,3] and edges [E,2] are int32 (idx_i64 = 0) or int64 (1).
 * workspace: pbn_mesh_workspace_bytes(mode, V, F for modes 0/1 or E for mode 2); 0 = sizes out of range.
 * ------------------------------------------------------------------------------------------------------------ */
enum { PBN_MESH_NORMALS = 0, PBN_MESH_SEGMENT = 1, PBN_MESH_SEGMENT_POINT = 2 };
size_t pbn_mesh_workspace_bytes(int mode, int n_vertices, int n_elems);
/* nl f32[V,3]: vertex_normal(xyz, faces); a face naming a vertex twice adds to it once, unreferenced vertices get 0.
 * status int32[1] (device): 0, or 1 when an index lies outside [0, V) (nl is then undefined).  Asynchronous. */
int pbn_mesh_vertex_normals(const float* xyz, int n_vertices, const void* faces, int faces_i64, int n_faces, float* nl,
                            int32_t* status, void* workspace, size_t workspace_bytes, pbn_stream_t stream);
/* sup int64[V]: segment_mesh(xyz, faces, k_thresh, seg_min_verts) relabelled to 0..S-1 in ascending root order; nl
 * (optional) as pbn_mesh_vertex_normals.  Edges sort by (w, edge index), NaN weights last.  SYNCHRONISES the stream (the
 * Felzenszwalb sweep runs on the host); PBN_ERR_RANGE when an index lies outside [0, V).  times_ms (optional, host
 * float[7]): incidence, normals, weights, sort, read-back, host sweep, relabel. */
int pbn_mesh_segment(const float* xyz, int n_vertices, const void* faces, int faces_i64, int n_faces, float k_thresh,
                     int seg_min_verts, int64_t* sup, float* nl, void* workspace, size_t workspace_bytes, float* times_ms,
                     pbn_stream_t stream);
/* sup int64[V]: segment_point(xyz, normals, edges, k_thresh, seg_min_verts), as pbn_mesh_segment. */
int pbn_mesh_segment_point(const float* xyz, const float* normals, int n_points, const void* edges, int edges_i64, int n_edges,
                           float k_thresh, int seg_min_verts, int64_t* sup, void* workspace, size_t workspace_bytes,
                           pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Scans without a mesh (csrc/cloud.hip): the exact k nearest neighbours of every point over a uniform grid, and PCA normals
 * over them -- the edges and normals pbn_mesh_segment_point takes.  xyz f32[n,3].  Argument checks run on the host before
 * any launch; neither pbn_cloud_knn nor pbn_cloud_normals synchronises.
 * ------------------------------------------------------------------------------------------------------------ */
/* bytes of workspace for pbn_cloud_knn; 0 = sizes out of range (n_points < 0 or too large, k outside 1..pbn_cloud_max_k()) */
size_t pbn_cloud_workspace_bytes(int n_points, int k);
int pbn_cloud_max_k(void);                                      /* 32 */
/* idx int32[n,k], d2 f32[n,k], in the caller's point order.  d2(i,j) = ((dx*dx + dy*dy) + dz*dz), dx = x[j] - x[i], each
 * operation rounded to float32 (no FMA).  Row i holds the k points j != i with the smallest key (bits of d2 as u32, j) in
 * ascending key order: coincident points are neighbours at distance 0, self is excluded by index.  When n - 1 < k a row
 * ends in idx = -1, d2 = +inf.  cell > 0 is the grid's cell size, anything else lets the library pick it on the device; it
 * is enlarged until an axis has at most 1024 cells and the grid fits the cell table, and the result never depends on it.
 * status int32[1] (device): 0, or bit 1 when a coordinate is not finite and bit 8 when the sort gave up; no row is
 * trusted (none is written) then. */
int pbn_cloud_knn(const float* xyz, int n_points, int k, float cell, int32_t* idx, float* d2, int32_t* status,
                  void* workspace, size_t workspace_bytes, pbn_stream_t stream);
/* Measurement variant: HIP events around the stages, SYNCHRONISES; times_ms (host float[4]): box + grid, keys + sort,
 * cell table, search. */
int pbn_cloud_knn_timed(const float* xyz, int n_points, int k, float cell, int32_t* idx, float* d2, int32_t* status,
                        void* workspace, size_t workspace_bytes, pbn_stream_t stream, float* times_ms);
/* nl f32[n,3]: for point i, S = i followed by its valid neighbours (0 <= idx < n) in rank order; float64 mean, then the six
 * float64 covariance sums; the unit eigenvector of the smallest eigenvalue (fixed-count cyclic Jacobi in float64), flipped
 * when n . (viewpoint - p_i) < 0, rounded to float32.  |S| < 3 gives the zero vector.  viewpoint: device float[3]. */
int pbn_cloud_normals(const float* xyz, int n_points, const int32_t* idx, int k, const float* viewpoint, float* nl,
                      pbn_stream_t stream);
/* The same normals, each turned towards its own point's viewpoint: views f32[n_views,3] and view_of int32[n] (device).
 * Mean, covariance, Jacobi and rounding are pbn_cloud_normals'; with v = views[view_of[i]] the normal is flipped when
 * (nx * (double(v.x) - px) + ny * (double(v.y) - py)) + nz * (double(v.z) - pz) < 0, pbn_cloud_normals' expression.  A
 * view_of[i] outside [0, n_views) leaves the eigenvector's sign as the Jacobi sweeps give it (a NaN view does too: the
 * comparison is false).  n_views >= 0; views may be NULL only when n_views == 0. */
int pbn_cloud_normals_views(const float* xyz, int n_points, const int32_t* idx, int k, const float* views, int n_views,
                            const int32_t* view_of, float* nl, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Posed depth frames (csrc/frames.hip): an RGB-D sequence back-projected into one compacted cloud.
 * tests/frames_ref.py restates this contract in numpy.  Every expression is one rounded float64 operation per operator,
 * in the order the brackets give; nothing is fused.
 *   Inputs   depth [F,H,W] (device), depth_is_f32 = 0: uint16, z = double(d) / depth_scale; 1: float32 metres,
 *            z = double(d).  colour uint8[F,H,W,3] (device) on the depth grid, or NULL.  pose double[F,16] on the HOST,
 *            camera to world, row-major 4x4 (r00 r01 r02 t0 | r10 ... | r20 ... | bottom row, which is not read).  intr
 *            double[F,4] on the HOST: fx, fy, cx, cy.  Both are read before the call returns.
 *   Limits   checked on the host before any launch, else PBN_ERR_ARG: F, H, W >= 0; F * H * W <= 2^31 - 1; the sampled
 *            pixels F * ceil(H / stride) * ceil(W / stride) <= 2^28; every fx and fy and depth_scale finite and > 0;
 *            depth_min <= depth_max (neither NaN); stride >= 1.
 *   Sampling pixel (u = column, v = row; the pixel centre IS the integer) is considered when u % stride == 0 and
 *            v % stride == 0.  Its id is (f * H + v) * W + u.
 *   Valid    (a) the 12 numbers of the top three rows of frame f's pose are finite (a lost frame, ScanNet's -inf pose,
 *            contributes nothing); (b) z is measured: finite, z > 0 and depth_min <= z <= depth_max (a uint16 0 is no
 *            measurement); (c) with edge > 0 (a ratio; <= 0 or NaN = off): no pixel (u-1,v), (u+1,v), (u,v-1), (u,v+1) --
 *            at FULL resolution whatever the stride -- that lies inside the image and whose zn is measured by (b) has
 *            fabs(zn - z) > edge * z; a neighbour outside the image or without a measurement makes no edge; (d) the three
 *            float32 world coordinates are finite.
 *   World    xc = ((double(u) - cx) * z) / fx; yc = ((double(v) - cy) * z) / fy;
 *            X = ((r00 * xc + r01 * yc) + r02 * z) + t0, Y and Z likewise from rows 1 and 2; each rounded to float32 once,
 *            on the store.
 *   Outputs  rows in ascending pixel id: xyz f32[N,3]; rgb f32[N,3] = the colour bytes as 0..255 floats (with colour);
 *            pixel int32[N].  frame_start int32[F+1]: frame f owns rows frame_start[f] .. frame_start[f+1] - 1, a skipped
 *            frame none.  result int32[2] (device): [0] status, [1] N -- one read-back gives both.
 * Two calls around that read-back: pbn_frames_count tests every sampled pixel (a wave64 ballot and popcount, one count per
 * workgroup), scans the counts (exclusive, into the workspace) and writes frame_start and result; the caller reads result,
 * allocates exactly N rows, and pbn_frames_write -- same arguments, same workspace, untouched in between -- tests the pixels
 * again and stores every wave's survivors contiguously at the workgroup's offset + the wave's offset + the lane's rank in
 * the ballot.  No atomics touch the order: two runs give the same bytes.  A workgroup's pbn_frames_block_pixels() sampled
 * pixels lie in one frame.  pbn_frames_write writes no row at or beyond n_rows: when its own count says there is one
 * (depth changed between the calls, or n_rows is not result[1]) it sets bit 1 of result[0], and no output is to be trusted.
 * Only the _timed entries synchronise.
 * ------------------------------------------------------------------------------------------------------------ */
/* bytes of workspace for pbn_frames_count / pbn_frames_write; 0 = sizes out of range (see Limits) */
size_t pbn_frames_workspace_bytes(int n_frames, int height, int width, int stride);
int pbn_frames_block_pixels(void);                              /* sampled pixels per workgroup: 1024 */
int pbn_frames_count(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose, const double* intr,
                     int n_frames, int height, int width, double depth_scale, double depth_min, double depth_max, int stride,
                     double edge, int32_t* frame_start, int32_t* result, void* workspace, size_t workspace_bytes,
                     pbn_stream_t stream);
/* n_rows = result[1] as read back; xyz, rgb (NULL exactly when colour is) and pixel hold n_rows rows */
int pbn_frames_write(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose, const double* intr,
                     int n_frames, int height, int width, double depth_scale, double depth_min, double depth_max, int stride,
                     double edge, int n_rows, float* xyz, float* rgb, int32_t* pixel, int32_t* result, void* workspace,
                     size_t workspace_bytes, pbn_stream_t stream);
/* Measurement variants: HIP events around the stages, SYNCHRONISE; times_ms (host): float[2] count, scan + starts for
 * pbn_frames_count_timed; float[1] write for pbn_frames_write_timed. */
int pbn_frames_count_timed(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose, const double* intr,
                           int n_frames, int height, int width, double depth_scale, double depth_min, double depth_max,
                           int stride, double edge, int32_t* frame_start, int32_t* result, void* workspace,
                           size_t workspace_bytes, pbn_stream_t stream, float* times_ms);
int pbn_frames_write_timed(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose, const double* intr,
                           int n_frames, int height, int width, double depth_scale, double depth_min, double depth_max,
                           int stride, double edge, int n_rows, float* xyz, float* rgb, int32_t* pixel, int32_t* result,
                           void* workspace, size_t workspace_bytes, pbn_stream_t stream, float* times_ms);

/* ------------------------------------------------------------------------------------------------------------
 * Depth-frame fusion (csrc/tsdf.hip): the frames of "Posed depth frames" fused into a truncated signed distance volume over
 * blocks of 8 x 8 x 8 voxels, and the volume's zero crossings as points with colours and normals.
 * tests/fuse_ref.py restates this contract in numpy.  Every expression is one rounded float64 operation per operator, in
 * the order the brackets give; nothing is fused; a result is rounded to float32 once, on the store.
 *   Inputs   depth, depth_is_f32, colour, pose, intr, F, H, W, depth_scale, depth_min, depth_max, edge as in "Posed depth
 *            frames" (no stride), with its Limits.  voxel finite and > 0; trunc finite with 0 < trunc <= 8 * voxel;
 *            min_weight >= 1; else PBN_ERR_ARG.  A skipped frame (a non-finite number in its pose's top three rows)
 *            contributes nothing anywhere.
 *   Blocks   pbn_fuse_blocks takes the raw cloud xyz f32[n,3] (pbn_frames_write's, stride 1, same filters).  B = 8 * voxel;
 *            origin g[a] = double(min32[a]) - B with min32 the float32 minimum of axis a; a point's block is
 *            b[a] = max(floor((double(p[a]) - g[a]) / B), 1): the quotient is 1 or more up to its rounding, and a point on the minimum
 *            that comes out a last bit below 1 lies in block 1 all the same.  A block is allocated when it or one of its 26
 *            neighbours holds a point.  key = bz << 42 | by << 21 | bx; blocks are ranked in ascending key.
 *            result int32[8] (device): [0] status -- bit 1 a coordinate is not finite, bit 2 an axis spans 2^21 - 1 blocks or
 *            more, neighbours included (block coordinates are 0 .. 2^21 - 2: a neighbour's key is the key +- 1, 2^21 or 2^42,
 *            and coordinate 2^21 - 1 is where the borrow of coordinate 0's lower neighbour lands, so it is never a block), bit 8 a sort gave up, bit 4 more than pbn_fuse_max_blocks() = 2^21 blocks (the
 *            voxel is too small for the scene); with a status no key is written --, [1] M_b, [2..4] the bits of min32: one
 *            read-back gives all.  n = 0 gives M_b = 0.  pbn_fuse_block_keys -- same n_points, same workspace, untouched in
 *            between -- writes block_key int64[M_b]; n_blocks other than result[1] sets bit 32 and writes nothing.
 *   Volume   pbn_fuse_integrate.  World to camera per frame, on the host: Rt = R transposed,
 *            tc[r] = -((Rt[r,0]*t0 + Rt[r,1]*t1) + Rt[r,2]*t2) (a rigid inverse; a pose that is not rigid is the caller's
 *            error and is not detected).  The voxel (ix, iy, iz) of block (bx, by, bz) has the centre
 *            p[a] = g[a] + (double(8 * b[a] + i[a]) + 0.5) * voxel, origin = g as double[3] on the HOST.  For every frame
 *            that is not skipped, in ascending frame order:
 *              1. pc[r] = ((Rt[r,0]*p0 + Rt[r,1]*p1) + Rt[r,2]*p2) + tc[r]; zc = pc[2]; skip unless zc > 0;
 *              2. uf = (fx * pc[0]) / zc + cx, vf = (fy * pc[1]) / zc + cy, ur = rint(uf), vr = rint(vf) (ties to even); skip
 *                 unless 0 <= ur <= W - 1 and 0 <= vr <= H - 1, compared in float64 (false for NaN);
 *              3. z = the depth at (vr, ur), valid by rules (b) and (c) of "Posed depth frames" (rule (d) is not asked: no
 *                 world point is formed);
 *              4. s = z - zc; skip when s < -trunc;
 *              5. d = min(1.0, s / trunc);
 *              6. S += d, Wt += 1, and with colour C[c] += double(byte c).
 *            tsdf = float32(S / double(Wt)), weight = Wt, rgb[c] = float32(C[c] / double(Wt)); a voxel with Wt = 0 stores
 *            0 everywhere.  tsdf f32[M_b,512], weight int32[M_b,512], rgb f32[M_b,512,3] (NULL exactly when colour is),
 *            in-block index (iz * 8 + iy) * 8 + ix.  One workgroup per block keeps every voxel's sums in registers through
 *            all frames; frames whose frustum cannot meet the block's bounding sphere are passed over, which never changes
 *            a result.  The call waits once for its upload of the cameras; the volume is never read.
 *   Surface  a voxel is observed when weight >= min_weight.  For every observed voxel q in ascending (block rank, in-block
 *            index) and a = 0, 1, 2: n = q + e_a (in another block through the sorted keys; a block that is not allocated
 *            is unobserved) must be observed and (D(q) < 0) != (D(n) < 0) on the stored float32 values as float64.  Then
 *            r = D(q) / (D(q) - D(n)); the point is p(q) with coordinate a replaced by p(q)[a] + r * voxel;
 *            rgb = rgb(q) + r * (rgb(n) - rgb(q)); G(x)[b] = D'(x + e_b) - D'(x - e_b) where an unobserved voxel reads as
 *            D(x) itself; gv[b] = G(q)[b] + r * (G(n)[b] - G(q)[b]); len = sqrt((gv0*gv0 + gv1*gv1) + gv2*gv2); nl = gv / len,
 *            the zero vector when len is 0 or not finite: it points from the surface into free space, towards the sensors.
 *            Rows in that order: xyz, rgb, nl f32[N,3], weight int32[N] = min(weight(q), weight(n)), voxel_id int64[N] =
 *            (block rank * 512 + in-block index) * 3 + a.  pbn_fuse_extract_count writes result int32[2] = (status, N);
 *            the caller reads it and pbn_fuse_extract_write -- same volume, same workspace, untouched in between -- writes
 *            the rows; a row at or beyond n_rows is not written and sets bit 32; the rows below n_rows are written all the same.  n_blocks <= 1398101 (N fits an int32).
 * No atomic touches an order or a float: two runs give the same bytes.  Only the _timed entries (and pbn_fuse_integrate's
 * one wait) synchronise.
 * ------------------------------------------------------------------------------------------------------------ */
int pbn_fuse_max_blocks(void);                                  /* 2^21 */
/* bytes of workspace for pbn_fuse_blocks / pbn_fuse_block_keys; 0 = n_points out of range (< 0 or above 2^28) */
size_t pbn_fuse_blocks_workspace_bytes(int n_points);
int pbn_fuse_blocks(const float* xyz, int n_points, double voxel, int32_t* result, void* workspace, size_t workspace_bytes,
                    pbn_stream_t stream);
/* Measurement variant: SYNCHRONISES; times_ms (host float[3]): box + keys, the points' blocks, dilation + the allocated blocks. */
int pbn_fuse_blocks_timed(const float* xyz, int n_points, double voxel, int32_t* result, void* workspace, size_t workspace_bytes,
                          pbn_stream_t stream, float* times_ms);
int pbn_fuse_block_keys(int n_points, int n_blocks, int64_t* block_key, int32_t* result, void* workspace, size_t workspace_bytes,
                        pbn_stream_t stream);
size_t pbn_fuse_integrate_workspace_bytes(int n_frames);        /* 0 = n_frames < 0 */
int pbn_fuse_integrate(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose, const double* intr,
                       int n_frames, int height, int width, double depth_scale, double depth_min, double depth_max, double edge,
                       double voxel, double trunc, const double* origin, const int64_t* block_key, int n_blocks, float* tsdf,
                       int32_t* weight, float* rgb, void* workspace, size_t workspace_bytes, pbn_stream_t stream);
/* Measurement variant: SYNCHRONISES; times_ms (host float[1]): the integration; stats (host uint64[2], or NULL): [0] the
 * block-frame pairs left by the cull (each stands for 512 voxel-frame pairs), [1] the depth samples gathered in step 3. */
int pbn_fuse_integrate_timed(const void* depth, int depth_is_f32, const uint8_t* colour, const double* pose, const double* intr,
                             int n_frames, int height, int width, double depth_scale, double depth_min, double depth_max,
                             double edge, double voxel, double trunc, const double* origin, const int64_t* block_key, int n_blocks,
                             float* tsdf, int32_t* weight, float* rgb, void* workspace, size_t workspace_bytes, pbn_stream_t stream,
                             float* times_ms, uint64_t* stats);
size_t pbn_fuse_extract_workspace_bytes(int n_blocks);          /* 0 = n_blocks out of range */
int pbn_fuse_extract_count(const float* tsdf, const int32_t* weight, const int64_t* block_key, int n_blocks, int min_weight,
                           int32_t* result, void* workspace, size_t workspace_bytes, pbn_stream_t stream);
int pbn_fuse_extract_write(const float* tsdf, const int32_t* weight, const float* vol_rgb, const int64_t* block_key, int n_blocks,
                           int min_weight, double voxel, const double* origin, int n_rows, float* xyz, float* rgb, float* nl,
                           int32_t* out_weight, int64_t* voxel_id, int32_t* result, void* workspace, size_t workspace_bytes,
                           pbn_stream_t stream);
/* Measurement variants: SYNCHRONISE; times_ms (host float[1]): count + scan; the write. */
int pbn_fuse_extract_count_timed(const float* tsdf, const int32_t* weight, const int64_t* block_key, int n_blocks, int min_weight,
                                 int32_t* result, void* workspace, size_t workspace_bytes, pbn_stream_t stream, float* times_ms);
int pbn_fuse_extract_write_timed(const float* tsdf, const int32_t* weight, const float* vol_rgb, const int64_t* block_key,
                                 int n_blocks, int min_weight, double voxel, const double* origin, int n_rows, float* xyz, float* rgb,
                                 float* nl, int32_t* out_weight, int64_t* voxel_id, int32_t* result, void* workspace,
                                 size_t workspace_bytes, pbn_stream_t stream, float* times_ms);

/* ------------------------------------------------------------------------------------------------------------
 * Raw sensor scans (csrc/thin.hip): grid thinning to the network's pitch, statistical outlier removal over the kNN graph's
 * d2, and the way back from the kept points to the raw ones.  Argument checks run on the host before any launch; only the
 * _timed entry synchronises.  Every output is a pure function of the input (no float atomics): two runs give the same
 * bytes, and tests/thin_ref.py restates each in numpy.
 * ------------------------------------------------------------------------------------------------------------ */
/* bytes of workspace for pbn_thin_points; 0 = n_points out of range (< 0 or above 2^28) */
size_t pbn_thin_workspace_bytes(int n_points);
/* One output row per occupied cell of a grid of `pitch` (finite, > 0; else PBN_ERR_ARG).  xyz f32[n,3]; rgb f32[n,3] or
 * NULL.  Origin o[a] = the float32 minimum of axis a; cell c[a] = floor((double(p[a]) - double(o[a])) / pitch) (correctly
 * rounded float64 division); key = cz << 42 | cy << 21 | cx; rows in ascending key order.  Per row t: out_xyz / out_rgb
 * f32[.,3] = float32(the float64 sum of the members' values, added from 0.0 in ascending point index, / double(count));
 * count[t] = members; first[t] = the lowest member index; inverse int32[n]: the row of every input point.  The arrays
 * out_xyz, out_rgb, count and first hold n rows, of which the first M are written.
 * result int32[2] (device): [0] status -- 0, or bit 1 a coordinate is not finite, bit 2 an axis spans 2^21 cells or more,
 * bit 8 a sort gave up; with a status no output is written -- and [1] M, the number of rows: one read-back gives both. */
int pbn_thin_points(const float* xyz, const float* rgb, int n_points, double pitch, float* out_xyz, float* out_rgb,
                    int32_t* count, int32_t* first, int32_t* inverse, int32_t* result, void* workspace, size_t workspace_bytes,
                    pbn_stream_t stream);
/* Measurement variant: HIP events around the stages, SYNCHRONISES; times_ms (host float[5]): box + keys, low-word sort,
 * high-word keys + sort, run heads + scan, cells. */
int pbn_thin_points_timed(const float* xyz, const float* rgb, int n_points, double pitch, float* out_xyz, float* out_rgb,
                          int32_t* count, int32_t* first, int32_t* inverse, int32_t* result, void* workspace,
                          size_t workspace_bytes, pbn_stream_t stream, float* times_ms);
/* bytes of workspace for pbn_cloud_outlier_mask; 0 = n_points out of range */
size_t pbn_cloud_outlier_workspace_bytes(int n_points);
/* d2 f32[n,k] as pbn_cloud_knn writes it.  m_i = (float64 sum in rank order, from 0.0, of sqrt(double(d2[i,r])) over the
 * finite entries) / their number; a row without a finite entry has no m_i, is not kept and counts nowhere.  Sums over
 * points: blocks of 256 consecutive indices, inside a block the tree v[j] += v[j + s] for s = 128 .. 1 (absent entries
 * 0.0), block partials added in block order.  mu = sum m_i / n_valid; sigma = sqrt(sum (m_i - mu)^2 / n_valid) (a second
 * pass); keep[i] (uint8 0 / 1) = m_i <= mu + ratio * sigma in float64 (a product, then a sum).  stats double[3] (device):
 * mu, sigma, n_valid; without a valid row mu and sigma are NaN; n_points == 0 writes zeros.  ratio finite and >= 0,
 * k in 1..pbn_cloud_max_k(), else PBN_ERR_ARG. */
int pbn_cloud_outlier_mask(const float* d2, int n_points, int k, double ratio, uint8_t* keep, double* stats, void* workspace,
                           size_t workspace_bytes, pbn_stream_t stream);
/* bytes of workspace for pbn_cloud_raw_index; 0 = n_points out of range */
size_t pbn_cloud_raw_index_workspace_bytes(int n_points);
/* raw_index int32[n_raw]: with t = inverse[i] (a row of the n_points points keep and idx speak of) and kept_row = the
 * exclusive scan of keep: kept_row[t] when keep[t]; else kept_row[j] of the first j = idx[t, r] in rank order with keep[j];
 * else -1 (also for t outside [0, n_points)).  idx int32[n_points,k], -1 = no neighbour. */
int pbn_cloud_raw_index(const int32_t* inverse, int n_raw, const uint8_t* keep, const int32_t* idx, int n_points, int k,
                        int32_t* raw_index, void* workspace, size_t workspace_bytes, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fixed-radius queries (csrc/cloud.hip): the neighbour count behind radius outlier removal, and the way back from the kept
 * points to the raw ones without a kNN graph.  pbn_cloud_knn's grid front and d2; rf = `radius` (float32, finite and > 0),
 * r2 = fl(rf * rf); j is a neighbour of i when j != i and d2(i,j) <= r2 (coincident points are neighbours at 0; an r2 that
 * underflows to 0 counts only those).  cell > 0 is the grid's cell size, anything else a hair above the radius; the result
 * never depends on it.  status int32[1] (device): 0, or bit 1 when a coordinate is not finite and bit 8 when the sort gave
 * up; no row is written then.  Argument checks run on the host before any launch (sizes in 0..2^28, radius, cap >= 1,
 * pointers: PBN_ERR_ARG); only the _timed entry synchronises.  No atomics besides the front's: two runs, the same bytes;
 * tests/radius_ref.py restates each output in numpy.
 * ------------------------------------------------------------------------------------------------------------ */
/* bytes of workspace for pbn_cloud_radius_count; 0 = n_points out of range */
size_t pbn_cloud_radius_workspace_bytes(int n_points);
/* count int32[n], in the caller's point order: min(number of neighbours, cap), cap in 1..2^31 - 1; a query stops scanning
 * at cap.  n_points == 0 launches nothing; one point counts 0. */
int pbn_cloud_radius_count(const float* xyz, int n_points, float radius, int cap, float cell, int32_t* count, int32_t* status,
                           void* workspace, size_t workspace_bytes, pbn_stream_t stream);
/* Measurement variant: HIP events around the stages, SYNCHRONISES; times_ms (host float[4]): box + grid, keys + sort,
 * cell table, count. */
int pbn_cloud_radius_count_timed(const float* xyz, int n_points, float radius, int cap, float cell, int32_t* count,
                                 int32_t* status, void* workspace, size_t workspace_bytes, pbn_stream_t stream, float* times_ms);
/* bytes of workspace for pbn_cloud_radius_raw_index; 0 = n_points or n_raw out of range */
size_t pbn_cloud_radius_raw_index_workspace_bytes(int n_points, int n_raw);
/* raw_index int32[n_raw]: with t = inverse[i] (a row of the n_points points xyz and keep speak of) and rank = the exclusive
 * scan of keep (uint8 0 / 1): rank[t] when keep[t]; else rank[j] of the KEPT point j with the smallest key (bits of
 * d2(t,j), j) among those with d2(t,j) <= r2 -- a dropped point is never an answer; else -1 (also for t outside
 * [0, n_points)). */
int pbn_cloud_radius_raw_index(const float* xyz, int n_points, const uint8_t* keep, float radius, float cell,
                               const int32_t* inverse, int n_raw, int32_t* raw_index, int32_t* status, void* workspace,
                               size_t workspace_bytes, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Normal orientation (csrc/orient.hip): the signs of a cloud's normals made consistent over its kNN graph, by propagation
 * along the minimum spanning forest under the weight 1 - |n_i . n_j| (Hoppe et al. 1992).  tests/orient_ref.py restates
 * this contract in numpy with a sequential Kruskal.
 *   Sizes    nl float32[n,3], idx int32[n,k], 1 <= k <= pbn_cloud_max_k(), n >= 0, n * k <= 2^31 - 1; else PBN_ERR_ARG.
 *   Null     a point is null when a component of its normal is not finite or all three are +-0.  It has no edges, its row
 *            is copied unchanged, it is never flipped, and it is a tree of its own.
 *   Edges    slot e = i * k + r is an edge between i and j = idx[i,r] when 0 <= j < n, j != i and neither end is null; any
 *            other j is no neighbour.  The graph is undirected: slots i->j and j->i are two edges, equal weight, two ids.
 *   Key      d_e = (nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j in float32, every operation rounded; w_e = 1.0f - fabsf(d_e);
 *            f_e = d_e < 0.0f; key_e = (u64(order_key(w_e)) << 32) | e, order_key the order-preserving bits of a float32
 *            with NaN last and -0 tied with +0 (pbn_mesh_segment's edge order).  Keys are distinct: the order is strict.
 *   Forest   F = the minimum spanning forest under ascending key (Kruskal's).  It is unique, so nothing below depends on
 *            how it is found.
 *   Signs    within a tree s_i in {0,1} with s_a ^ s_b = f_e for every edge of F, which fixes s up to one flip per tree:
 *            of the two, the one with more points at s_i = 0; on a tie the one that keeps the tree's lowest-index point.
 *   Outputs  nl_out float32[n,3]: the input row with the sign bit of all three components inverted where s_i = 1;
 *            flipped uint8[n] = s_i; tree int32[n] = the lowest point index of i's tree; stats int32[4] = trees among
 *            the non-null points, flipped points, null points, 0.
 *   Status   int32[2] (device): [0] is 0, or bit 16 when a link chain did not end within n hops (an internal error: no
 *            output is to be trusted); [1] = the rounds that merged something.
 * Integer atomics only: two runs give the same bytes.  n_points == 0 is valid.  Argument checks run on the host before any
 * launch; only the _timed entry synchronises.
 * ------------------------------------------------------------------------------------------------------------ */
/* bytes of workspace for pbn_cloud_orient; 0 = sizes out of range */
size_t pbn_cloud_orient_workspace_bytes(int n_points, int k);
int pbn_cloud_orient(const float* nl, int n_points, const int32_t* idx, int k, float* nl_out, uint8_t* flipped, int32_t* tree,
                     int32_t* stats, int32_t* status, void* workspace, size_t workspace_bytes, pbn_stream_t stream);
/* Measurement variant: HIP events around the stages, SYNCHRONISES; times_ms (host float[3]): edge codes, rounds, tail. */
int pbn_cloud_orient_timed(const float* nl, int n_points, const int32_t* idx, int k, float* nl_out, uint8_t* flipped,
                           int32_t* tree, int32_t* stats, int32_t* status, void* workspace, size_t workspace_bytes,
                           pbn_stream_t stream, float* times_ms);

/* ------------------------------------------------------------------------------------------------------------
 * Floor plane and upright frame (csrc/upright.hip): PCL / Open3D's segment_plane -- a RANSAC plane fit and a least-squares
 * refit over the inliers -- and the minimal rotation that takes the plane's normal to +z.  tests/upright_ref.py restates
 * this contract in numpy, stage by stage.  Every expression is one rounded IEEE operation per operator, in the order the
 * brackets give, float32 or float64 as stated; nothing is fused.
 *   Inputs   xyz float32[n,3] (device), 0 <= n <= 2^28; threshold t float32, finite, > 0; n_hyp H in
 *            1..pbn_cloud_upright_max_hyp() (4096); seed uint64; up_hint double[3] on the HOST, a unit vector, or NULL;
 *            cos_tilt double (read only with a hint); max_below int >= -1 (-1 = no floor rule).  Else PBN_ERR_ARG.
 *   Draws    mix(z): z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31, all
 *            modulo 2^64 (the splitmix64 finalizer).  Hypothesis h draws i_j = ((mix(seed + 3h + j) >> 32) * n) >> 32 for
 *            j = 0, 1, 2 (the sum modulo 2^64, the product in 64 bits), and p_j = xyz[i_j] as float64.
 *   Plane    float64: e1 = p1 - p0, e2 = p2 - p0; nx = e1y*e2z - e1z*e2y, ny = e1z*e2x - e1x*e2z, nz = e1x*e2y - e1y*e2x;
 *            q = (nx*nx + ny*ny) + nz*nz.  The hypothesis is DEAD when n < 3, when two of its indices coincide, or when
 *            q > 0 is false or q is not finite.  Otherwise r = sqrt(q), u = (nx/r, ny/r, nz/r),
 *            d = -((ux*p0x + uy*p0y) + uz*p0z).  With a hint: g = (ux*hx + uy*hy) + uz*hz; when g < 0, u and d are
 *            negated; when |g| < cos_tilt the hypothesis is dead.  (a, b, c, d) = float32(ux, uy, uz, d).
 *   Score    for every live hypothesis and every point, float32: s = ((a*x + b*y) + c*z) + d; in[h] counts |s| <= t,
 *            above[h] counts s > t, below[h] = n - in[h] - above[h].  A NaN or infinite coordinate anywhere in xyz sets
 *            bit 1 of status (pbn_cloud_knn's bit); no output is to be trusted then.
 *   Select   without a hint a hypothesis with below > above is negated: the two counts swap and (a, b, c, d) change
 *            sign.  With max_below >= 0 a hypothesis with below > max_below is dead (nothing lies under a floor).  The
 *            winner is the live hypothesis with the most inliers, ties to the lowest h; plane0 float32[4] is its plane.
 *            Without a live hypothesis found = 0: xyz_out = xyz, floor = 0, height = 0, R = I, every other output 0.
 *   Refit    over the points with |s| <= t under plane0: the count, the float64 centroid (three sums of the float64
 *            coordinates, each divided by the count), then with dx = x - cx, ... the six sums of dx*dx, dx*dy, dx*dz,
 *            dy*dy, dy*dz, dz*dz.  Every sum has pbn_cloud_outlier_mask's fixed shape over ALL n indices: blocks of 256
 *            consecutive indices, the tree v[j] += v[j + s] for s = 128 .. 1, absent entries (no inlier, or past n) 0.0,
 *            the block partials added in block order from 0.0.  The normal is pbn_cloud_normals' Jacobi eigenvector of the
 *            symmetric matrix of the six sums: 10 fixed sweeps (01, 02, 12) from V = I, the column of the smallest
 *            diagonal entry (ties to the lowest axis) divided by its length.  It is negated when
 *            (nx*a0 + ny*b0) + nz*c0 < 0 with (a0, b0, c0) = float64(plane0); d = -((nx*cx + ny*cy) + nz*cz).
 *            With fewer than 3 inliers plane = float64(plane0).  plane double[4]; moments double[10] = count, centroid,
 *            the six sums.
 *   R        with (a, b, c) = plane[0..2] and k = 1 + c: when k > 0,
 *            R = [[1 - (a*a)/k, -((a*b)/k), -a], [-((a*b)/k), 1 - (b*b)/k, -b], [a, b, c]]; otherwise diag(1, -1, -1).
 *            R double[9] row-major; a pure rotation, no shift.  R32 = float32(R), (a32, b32, c32, d32) = float32(plane).
 *   Apply    per point, float32: xyz_out row r = (R32[r][0]*x + R32[r][1]*y) + R32[r][2]*z;
 *            height = ((a32*x + b32*y) + c32*z) + d32; floor = |height| <= t.  xyz_out may be NULL (the fit alone).
 *   info     int32[8]: found, winner h, its in, above, below (after the select stage), the refit's inliers, the
 *            hypotheses alive at the arg-max, 0.
 * Integer atomics only: two runs give the same bytes.  Argument checks run on the host before any launch; n_points == 0 is
 * valid (found = 0) and launches nothing that indexes; only the _timed entry synchronises.
 * ------------------------------------------------------------------------------------------------------------ */
/* bytes of workspace for pbn_cloud_upright; 0 = sizes out of range */
size_t pbn_cloud_upright_workspace_bytes(int n_points, int n_hyp);
int pbn_cloud_upright_max_hyp(void);
int pbn_cloud_upright(const float* xyz, int n_points, float threshold, int n_hyp, uint64_t seed, const double* up_hint,
                      double cos_tilt, int max_below, float* xyz_out, uint8_t* floor, float* height, double* plane, float* plane0,
                      double* R, double* moments, int32_t* info, int32_t* status, void* workspace, size_t workspace_bytes,
                      pbn_stream_t stream);
/* Measurement variant: HIP events around the stages, SYNCHRONISES; times_ms (host float[4]): hypotheses, score,
 * select + refit, apply. */
int pbn_cloud_upright_timed(const float* xyz, int n_points, float threshold, int n_hyp, uint64_t seed, const double* up_hint,
                            double cos_tilt, int max_below, float* xyz_out, uint8_t* floor, float* height, double* plane,
                            float* plane0, double* R, double* moments, int32_t* info, int32_t* status, void* workspace,
                            size_t workspace_bytes, pbn_stream_t stream, float* times_ms);
/* The launch geometry of the score kernel, for tests: points per workgroup (pbn_cloud_upright uses
 * pbn_cloud_upright_chunk()), hypotheses per workgroup, and the entry with `chunk` in 1..2048 given.  The geometry changes
 * the speed, never a byte of the result. */
int pbn_cloud_upright_chunk(void);
int pbn_cloud_upright_hyp_block(void);
int pbn_cloud_upright_chunked(const float* xyz, int n_points, float threshold, int n_hyp, uint64_t seed, const double* up_hint,
                              double cos_tilt, int max_below, int chunk, float* xyz_out, uint8_t* floor, float* height,
                              double* plane, float* plane0, double* R, double* moments, int32_t* info, int32_t* status,
                              void* workspace, size_t workspace_bytes, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Annotated raw scans (csrc/vote.hip): the raw points' labels voted down to the kept points.  Integers only: two runs
 * give the same bytes, and tests/vote_ref.py restates the contract in numpy.  Argument checks run on the host before any
 * launch (n_classes in 1..1023, n_raw and m in 0..2^28, else PBN_ERR_ARG); nothing synchronises.
 * ------------------------------------------------------------------------------------------------------------ */
/* bytes of workspace for pbn_cloud_vote_labels; 0 = n_raw or m out of range */
size_t pbn_cloud_vote_workspace_bytes(int n_raw, int m);
/* rows int32[n_raw]: the kept row in [0, m) that speaks for raw point i, or -1 (pbn_cloud_raw_index, or pbn_thin_points'
 * inverse); sem int32[n_raw]; ins int32[n_raw] or NULL.  Codes: s = sem < 0 ? n_classes : sem; q = ins < 0 ? 2^21 - 1 : ins
 * (q = 0 for every point when ins is NULL): any negative label is "unannotated", a label like any other that orders
 * LAST.  Vote key = s << 21 | q.  Per kept row t: members[t] = #{i: rows[i] == t}; the winner is the key with the largest
 * count among them, ties to the LOWEST key; votes[t] = its count; out_sem[t] / out_ins[t] (int64) = its s / q, the two
 * unannotated codes written as -100.  A row without members gets -100, -100, 0, 0; points with rows == -1 vote nowhere.
 * old_id int64[min(m, 2^21)] or NULL.  Not NULL: the instance ids that won a row are renumbered 0 .. I'-1 in ascending
 * old-id order in out_ins, old_id[new] = old for new < I'.  NULL: out_ins keeps the raw ids and I' is 0.
 * result int32[2] (device): [0] status -- 0, or bit 1 a sem >= n_classes, bit 2 an ins >= 2^21 - 1, bit 4 a rows entry
 * outside [-1, m), bit 8 a sort gave up; with a status the outputs are unspecified -- and [1] I': one read-back gives
 * both.  n_raw == 0 fills the m rows and launches nothing else; m == 0 runs the range checks alone. */
int pbn_cloud_vote_labels(const int32_t* rows, const int32_t* sem, const int32_t* ins, int n_raw, int m, int n_classes,
                          int64_t* out_sem, int64_t* out_ins, int32_t* votes, int32_t* members, int32_t* result,
                          int64_t* old_id, void* workspace, size_t workspace_bytes, pbn_stream_t stream);
/* Measurement variant: HIP events around the stages, SYNCHRONISES; times_ms (host float[6]): fill + keys, key sort, row
 * pairs + row sort, run heads + scan + starts, pick, compaction. */
int pbn_cloud_vote_labels_timed(const int32_t* rows, const int32_t* sem, const int32_t* ins, int n_raw, int m, int n_classes,
                                int64_t* out_sem, int64_t* out_ins, int32_t* votes, int32_t* members, int32_t* result,
                                int64_t* old_id, void* workspace, size_t workspace_bytes, pbn_stream_t stream,
                                float* times_ms);

/* ------------------------------------------------------------------------------------------------------------
 * Validation meters (csrc/metrics.hip): the integer counts behind train.py:123-304 (eval_epoch).  No workspace, no
 * synchronisation, integer atomics only (identical counters run to run).  Neither entry writes its inputs.
 * ------------------------------------------------------------------------------------------------------------ */
/* tools/mIOU.py:18-31 (intersectionAndUnionGPU) as counts, ADDED to caller-owned counters.  pred / target: n labels,
 * int32 (flag 0) or int64 (flag 1), element-aligned.  With q_i = ignore_index where target_i == ignore_index and pred_i
 * elsewhere (mIOU.py:24):  intersection[c] += #{q_i == target_i == c},  output[c] += #{q_i == c},  target[c] +=
 * #{target_i == c}, c in [0, K); values outside [0, K) count nowhere (histc drops them), so a target that is out of range
 * but not the ignore value still counts its prediction in `output`.  acc3k int64[3K] = intersection | output | target.
 * conf_kk int64[K*K] (optional): [t*K + p] += 1 for t, p in [0, K), t != ignore_index.  n_class in [2, 64]; n == 0 is
 * PBN_OK and launches nothing; a bad argument is PBN_ERR_ARG before any launch. */
int pbn_sem_confusion(const void* pred, int pred_i64, const void* target, int target_i64, int64_t n, int n_class,
                      int ignore_index, int64_t* acc3k, int64_t* conf_kk, pbn_stream_t stream);
/* train.py:153-168 for one scene, WRITTEN to row8 int64[8] = n, agree, n_pos, pos_pred1, n_neg, neg_pred1, n_nan, 0 with
 * pred1 = pred_mask >= threshold (compared in float32), agree = #{pred1 == gt}, n_pos = #{gt == 1}, n_neg = #{gt == 0},
 * pos_pred1 / neg_pred1 the rows of each with pred1 = 1.  A NaN score counts in n_nan only.  pred_mask: n scores of `dtype`
 * (PBN_F32 / PBN_BF16 / PBN_F16); gt_mask: int32 (gt_i64 0) or int64 (1).  n == 0 writes a zero row. */
int pbn_mask_accuracy(const void* pred_mask, int dtype, const void* gt_mask, int gt_i64, int64_t n, float threshold,
                      int64_t* row8, pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training losses (csrc/losses.hip): the seven terms of model_fn (network/PBNet.py:366-416, diceLoss :463-468) in one
 * forward call and their gradients in one backward call.  Float32 arithmetic per row, float64 sums through per-workgroup
 * partials in the workspace (grids depend on the row counts only, no floating-point atomics: the same inputs give the same
 * bits).  Asynchronous, no host synchronisation.  Every *_dtype is PBN_F32 / PBN_BF16 / PBN_F16.
 *   points   sem_score [n_points, n_class] with leading dimension sem_ld, sem_label / ins_label int64 (-100 = ignore),
 *            offset_pred [n_points, 3], inst_info f32[n_points, 9] (columns 0-2 used), xyz f32[n_points, 3]
 *   mask     pred_mask [n_rows], gt_mask int64[n_rows] with -1 = ignore.  n_rows < 0: only the three point terms exist
 *            (below cluster_epoch) and no mask / proposal argument is read
 *   scores   iou f32[n_prop, n_inst] as pbn_get_iou writes it, clt_scores [n_prop]
 * Return codes, all before any launch: PBN_ERR_ARG (a null required pointer, a misaligned one, a negative n_points / n_prop,
 * n_class outside [2, 64], sem_ld < n_class), PBN_ERR_UNSUPPORTED (an unknown dtype), PBN_ERR_WORKSPACE (workspace too small).
 * ------------------------------------------------------------------------------------------------------------ */
size_t pbn_losses_workspace_bytes(int64_t n_points, int64_t n_rows, int64_t n_prop);
/* terms f32[8] = semantic, offset_norm, offset_dir, mask, dice, score, loss (their sum), 0.  counts int64[4] = rows with
 * ins_label != -100, rows with gt_mask != -1, rows with a class label, rows whose label is neither -100 nor in [0, n_class)
 * (such a row is ignored and never used as an index).  state f64[8]: what the backward needs (n_keep, n_valid + 1e-6, R,
 * 2A + 1, U, P).  gt_mask is REWRITTEN with -1 -> 0 (the reference assigns 0.5 in place into a long tensor) and mask_weight
 * u8[n_rows] receives gt_mask != -1; gt_scores f32[n_prop] = get_segmented_scores(max_i iou[p, i], fg, bg), bit for bit.
 * An empty mean (no class label, n_rows = 0, n_prop = 0) is 0 / 0 = NaN, as torch's.  Unlike torch, a NaN in `iou` is dropped
 * by the row maximum and a NaN pred_mask on an ignored row stays out of the mask term (neither arises from pbn_get_iou or
 * from sigmoid scores).  workspace: 16-byte aligned. */
int pbn_losses_forward(const void* sem_score, int sem_dtype, int sem_ld, const int64_t* sem_label, const void* offset_pred,
                       int offset_dtype, const float* inst_info, const float* xyz, const int64_t* ins_label, int64_t n_points,
                       int n_class, const void* pred_mask, int mask_dtype, int64_t* gt_mask, uint8_t* mask_weight,
                       int64_t n_rows, const float* iou, int n_inst, const void* clt_scores, int clt_dtype, int64_t n_prop,
                       double fg_thresh, double bg_thresh, float* gt_scores, float* terms, int64_t* counts, double* state,
                       void* workspace, size_t workspace_bytes, pbn_stream_t stream);
/* d terms[6] / d (sem_score, offset_pred, pred_mask, clt_scores) times the DEVICE scalar *grad_loss, each written once in its
 * input's dtype: g_sem [n_points, n_class] (contiguous), g_offset [n_points, 3], g_mask [n_rows], g_clt [n_prop].  Inputs as
 * the forward left them (gt_mask rewritten, mask_weight, gt_scores, state); nothing of size n_points x n_class is kept
 * between the calls: the softmax is recomputed. */
int pbn_losses_backward(const void* sem_score, int sem_dtype, int sem_ld, const int64_t* sem_label, const void* offset_pred,
                        int offset_dtype, const float* inst_info, const float* xyz, const int64_t* ins_label, int64_t n_points,
                        int n_class, const void* pred_mask, int mask_dtype, const int64_t* gt_mask, const uint8_t* mask_weight,
                        int64_t n_rows, const void* clt_scores, int clt_dtype, const float* gt_scores, int64_t n_prop,
                        const double* state, const float* grad_loss, void* g_sem, void* g_offset, void* g_mask, void* g_clt,
                        pbn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimizer step and loss meters of the training epoch (csrc/optim.hip; train.py:36-120, :350-357).
 *
 * table: a DEVICE array of n_chunks records, built once by the host and reused while the gradient addresses stay put.  A
 * record covers at most PBN_OPTIM_CHUNK consecutive float32 elements of ONE tensor: its parameter, gradient and state
 * addresses and the element count; vec = 1 when all its addresses are multiples of 16 (16-byte loads and stores), 0 =
 * dword accesses.  float32 only; the chunks of one call must not overlap.  One thread owns one element: no atomics, the
 * same inputs give the same bits on every grid.  Asynchronous, no host synchronisation, no workspace.
 *
 * Every operation is ONE float32 operation (no FMA, correctly rounded '/' and sqrtf), in this order; all scalars are
 * formed by the caller in float64 and rounded to float32 once:
 *   Adam   g' = g + weight_decay * p                 (coupled, weight_decay != 0)
 *          p  = p * (1 - lr * weight_decay), g' = g  (decoupled = 1: AdamW)
 *          m  = m + (g' - m) * one_minus_beta1;  v = v * beta2 + (g' * g') * one_minus_beta2
 *          d  = sqrtf(v) / bc2_sqrt + eps;       p = p - step_size * (m / d)
 *          with step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), t = the step count of the call's tensors
 *   SGD    g' = g + weight_decay * p (weight_decay != 0);  buf = first ? g' : buf * momentum + g';  p = p - lr * buf
 * state0 = exp_avg / momentum_buffer, state1 = exp_avg_sq (unused by SGD).  PBN_ERR_ARG before any launch: n_chunks < 0, a
 * null or misaligned table, a flag outside {0, 1}, a scalar that is not finite, bc2_sqrt <= 0.  n_chunks == 0 is PBN_OK.
 * ------------------------------------------------------------------------------------------------------------ */
#define PBN_OPTIM_CHUNK 4096
typedef struct pbn_optim_chunk_rec {
    void* param;
    const void* grad;
    void* state0;
    void* state1;
    int32_t n;
    int32_t vec;
} pbn_optim_chunk_rec;
int pbn_optim_chunk(void);
int pbn_optim_adam(const void* table, int n_chunks, float lr, float beta1, float one_minus_beta1, float beta2,
                   float one_minus_beta2, float eps, float weight_decay, float step_size, float bc2_sqrt, int decoupled,
                   pbn_stream_t stream);
int pbn_optim_sgd(const void* table, int n_chunks, float lr, float momentum, float weight_decay, int first,
                  pbn_stream_t stream);
/* AverageMeter.update (tools/log.py:26-30) for k terms at once: acc f64[3k] = val | sum | count gets val[j] = terms[j],
 * sum[j] += terms[j] * weights[j], count[j] += weights[j], in float64 (terms f32[k] widened, weights f64[k]).  One launch of
 * one wave, lane j owns term j; k in [0, 1024]. */
int pbn_loss_meter_update(const float* terms, const double* weights, double* acc, int k, pbn_stream_t stream);

/* ---- Self-test entry points ------------------------------------------------------------------------------------------------
 * The device primitives every stage starts from -- the range fill, the two exclusive scans, the 32-bit radix sort -- called
 * on their own, exactly as the stages call them, so that tests/test_prims_gpu.py can pin them at their tile edges.  No
 * product path uses these.  All are asynchronous on `stream`; argument checks run on the host before any launch
 * (PBN_ERR_ARG: a negative or oversized n, a missing pointer; PBN_ERR_WORKSPACE: a workspace that is too small).
 *
 * pbn_selftest_workspace_bytes  what = 0 the three-launch scan, 1 the chained scan, 2 the sort; n elements in 0..2^28.  Host
 *                               only; 0 for a bad argument.
 * pbn_selftest_sort_tile        keys per workgroup of a digit pass of the sort in this build.  Host only.
 * pbn_selftest_fill             ONE fill_ranges call over n_ranges (0..64) ranges base + offset[i], bytes[i], value[i]; the
 *                               three arrays are on the host; offset -1 is a null pointer.  The caller keeps the ranges inside
 *                               its buffer.
 * pbn_selftest_scan             out[i] = in[0] + .. + in[i-1] (int32), *total = the sum when total is not null.  chained = 0:
 *                               the three-launch form; 1: the one-launch form, whose state words and *total this entry zeroes
 *                               first and which ORs 16 into *status (required, cleared by the caller) when a workgroup gives
 *                               up waiting.  in may alias out, total may be out + n; both are passed through as given.
 * pbn_selftest_sort_u32         stable sort of n (key, value) pairs by key: keys_out[i] = the i-th key in ascending order as a
 *                               64-bit word, vals_out[i] its value; ties keep the input order.  ORs 8 into *status (cleared by
 *                               the caller) when a workgroup gives up waiting.  Only the histogram is zeroed here: a second
 *                               call into a used workspace must give the same bytes. */
size_t pbn_selftest_workspace_bytes(int what, int n);
int pbn_selftest_sort_tile(void);
int pbn_selftest_fill(uint8_t* base, const int64_t* offset, const int64_t* bytes, const uint8_t* value, int n_ranges,
                      pbn_stream_t stream);
int pbn_selftest_scan(const int32_t* in, int32_t* out, int n, int chained, int32_t* total, int32_t* status, void* ws,
                      size_t ws_bytes, pbn_stream_t stream);
int pbn_selftest_sort_u32(const uint32_t* keys, const int32_t* vals, int n, uint64_t* keys_out, int32_t* vals_out,
                          int32_t* status, void* ws, size_t ws_bytes, pbn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PBNET_HIP_H */
