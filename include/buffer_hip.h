/* buffer_hip.h -- C ABI of libbuffer_hip.so, the MI355X (gfx950) drop-in for the
 * native operators on BUFFER's registration-inference hot path.
 *
 * Conventions
 *   - every entry point returns 0 on success, a negative BUF_E* code on failure;
 *     buf_last_error() returns a thread-local message for the last failure.
 *   - pointers are DEVICE pointers unless the parameter name ends in _host.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream). All work
 *     is enqueued asynchronously on it unless the comment says "synchronises".
 *   - scratch memory is caller-owned: size it with the matching *_ws_bytes().
 *   - no torch types, no C++ types.  Process state is limited to: the thread-local error message, the per-device
 *     record of raised dynamic-LDS limits (hipFuncSetAttribute is per device; a process may drive several GPUs),
 *     and the optional HIP-event timing registry behind buf_timing_enable (off by default, mutex-guarded).
 *
 * Reference interfaces replaced (paths relative to the BUFFER repository):
 *   cpp_wrappers/cpp_neighbors/wrapper.cpp:58-238        radius_neighbors.batch_query
 *   cpp_wrappers/cpp_subsampling/wrapper.cpp:62-333      grid_subsampling.subsample_batch
 *   cpp_wrappers/cpp_subsampling/wrapper.cpp:338-566     grid_subsampling.subsample
 *   pointnet2_ops.pointnet2_utils (README.md:31)         furthest_point_sample, gather_operation,
 *                                                        ball_query, grouping_operation, three_nn
 *   knn_cuda.KNN (README.md:32)                          brute-force k-NN
 *   torch_batch_svd.svd (README.md:35)                   batched 3x3 SVD
 * and the fused device stages the build adds behind the same boundary
 * (models/point_learner.py, models/patch_embedder.py, models/BUFFER.py call sites
 * are cited per function below).
 */
#ifndef BUFFER_HIP_H
#define BUFFER_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BUF_OK            0
#define BUF_EINVAL       -1   /* bad argument (shape, null pointer, negative size) */
#define BUF_EHIP         -2   /* HIP runtime error (message carries hipGetErrorString) */
#define BUF_EWORKSPACE   -3   /* workspace too small */
#define BUF_ECAPACITY    -4   /* data-dependent capacity exceeded (e.g. voxel table) */
#define BUF_ENODEVICE    -5   /* no gfx950 device visible */

const char* buf_last_error(void);
int         buf_version(void);
/* Number of visible HIP devices (<0 on error); does not create a context. */
int         buf_device_count(void);
/* Measurement aid (off by default): when enabled, buf_grid_query (kernel id 0), buf_cylindrical_net (1) and
 * buf_cost_volume_net (2) bracket their kernel with HIP events on the launch stream.
 * buf_timing_collect_kernel synchronises on the events of one kernel id, returns the number of launches and
 * their summed duration / algorithmic work (bytes for id 0, flops for ids 1 and 2), and drops them.
 * buf_timing_collect = buf_timing_collect_kernel(0, ...). */
#define BUF_TIMED_GRID_QUERY 0
#define BUF_TIMED_CYL_NET    1
#define BUF_TIMED_COST_NET   2
#define BUF_TIMED_SELECT_PATCHES 3   /* A8:  work = 12*Nf + 12*P + 12*P*nsample bytes */
#define BUF_TIMED_PATCH_VOXELIZE 4   /* A10: work = 12*P*npts + 4*P*16*ncentres bytes */
#define BUF_TIMED_FPS            5   /* A6:  work = rounds (m) of the launch; bytes = 12*N' + 4*m per cloud */
#define BUF_TIMED_NN1            6   /* A12: work = 2*Q*N*D flops */
#define BUF_TIMED_VN_GATHER      7   /* A4:  work = 4*N*K + 12*N + 12*N*Cin + 12*N*Cout bytes */
#define BUF_TIMED_GRID_SUBSAMPLE 8   /* A1:  work = 12*N + 12*M(capacity N) + 4*B bytes; spans the whole kernel sequence */
#define BUF_TIMED_DESC_HEAD      9   /* A11 tail: work = (2*32*140*4 + 128) bytes per patch */
#define BUF_TIMED_CYL_NET_SPLIT  10  /* A11 dense, split-f16 form (buf_cylindrical_net_split): work = dense flops, as id 1 */
#define BUF_TIMED_COST_NET_SPLIT 11  /* A13, split-f16 form */
#define BUF_TIMED_SPFH           12  /* N6 k_spfh: work = n * (24 + 4*k_nbr + 24*K + 264) bytes, K = min(max_nn, k_nbr) (an upper bound: rows are shorter) */
#define BUF_TIMED_FPFH           13  /* N6 k_fpfh: work = n * K * 264 bytes, the SPFH gather at full rows (an upper bound as well) */
#define BUF_TIMED_SC2_COMPAT     14  /* N8 k_sc2_gather + k_sc2_compat: work = sum n^2 pairs of rows */
#define BUF_TIMED_SC2_CONF       15  /* N8 the power iteration, k_sc2_conf and k_sc2_seeds: work = power_iterations * sum n^2 */
#define BUF_TIMED_SC2_COUNTS     16  /* N8 k_sc2_counts: work = 8 * sum (seed groups * n * words) bytes of bit rows streamed */
#define BUF_TIMED_SC2_HYP        17  /* N8 k_sc2_hyp: work = seed ranks launched */
#define BUF_TIMED_SC2_REFINE     18  /* N8 k_sc2_refine: work = pairs */
#define BUF_TIMED_CLIQUE_GRAPH   19  /* N10 k_sc2_gather + k_sc2_compat + k_clique_deg: work = sum n^2 pairs of rows */
#define BUF_TIMED_CLIQUE_PEEL    20  /* N10 k_clique_peel: work = pairs */
#define BUF_TIMED_CLIQUE_ORDER   21  /* N10 k_clique_order + the second k_sc2_compat: work = 2 sum n^2 */
#define BUF_TIMED_CLIQUE_WALK    22  /* N10 k_clique_walk: work = seed ranks launched */
#define BUF_TIMED_CLIQUE_POSE    23  /* N10 k_clique_pose (GNC-TLS + voting): work = pairs */
#define BUF_TIMED_CLIQUE_POLISH  24  /* N10 k_clique_polish: work = pairs */
#define BUF_TIMED_ISS_SALIENCY   25  /* N11 k_iss_saliency: work = n * (4*k_sal + 24*K + 32) bytes, K = the columns read (an upper bound: rows are shorter) */
#define BUF_TIMED_ISS_NMS        26  /* N11 k_iss_nms: work = n * (4*k_nms + 8*K + 9) bytes (an upper bound as well) */
#define BUF_TIMED_NKERNELS       27
void        buf_timing_enable(int on);
long long   buf_timing_collect(double* total_ms, double* total_bytes);
long long   buf_timing_collect_kernel(int kernel_id, double* total_ms, double* total_work);

/* ------------------------------------------------------------------------------------------
 * A2  radius neighbours -- cpp_neighbors.batch_query (neighbors.cpp:211-332).
 *
 * d2 = ((dx*dx + dy*dy) + dz*dz) in fp32 without contraction, accept d2 < r*r,
 * rows ascending by (d2, support index), padded with ns_total.  Support indices are
 * global (stacked).  A cell grid (edge >= radius, auto-coarsened to `cells_per_elem`)
 * replaces the reference's KD-tree.
 *
 * buf_grid_t is a plain host struct filled by buf_grid_build and read by buf_grid_query;
 * the grid itself lives in the caller's workspace.
 */
typedef struct buf_grid {
    void*   ws;            /* device workspace handed to buf_grid_build            */
    size_t  ws_bytes;
    int     ns, nb;
    int64_t cells_per_elem;
    float   radius;
    const float* supports; /* the support array the grid was built from (must stay alive while queried) */
    /* device sub-allocations inside ws */
    void*   desc;          /* per-element grid descriptors                         */
    int*    s_off;         /* int32[nb+1] support offsets                          */
    int*    table;         /* int32[nb*cells_per_elem] inclusive cell ends         */
    void*   sorted;        /* float4[ns]: x,y,z,bitcast(global index), cell order  */
    int*    order;         /* int32[ns]: global support index in cell order        */
    void*   scan_tmp;
} buf_grid_t;

int64_t buf_grid_default_cells(int ns, int nb);
size_t  buf_grid_ws_bytes(int ns, int nb, int64_t cells_per_elem);
/* The cell rule of the build, on the host (pure arithmetic, no device): ext f64[3] = extent of an element's box over its finite
 * coordinates (finite, >= 0), cells_per_elem >= 1.  edge = radius * 1.00001 (1.0 for radius <= 0), multiplied by 1.25 until
 * prod(floor(ext / edge) + 1) <= cells_per_elem -- however many steps that takes: it ends at a one-cell table at the latest.
 * -> *edge_out, dim_out int[3] (every dim >= 1, their product <= cells_per_elem): the values buf_grid_build derives, bit for bit. */
int     buf_grid_cell_dims(const double* ext, float radius, int64_t cells_per_elem, double* edge_out, int* dim_out);
int     buf_grid_build(buf_grid_t* g, const float* supports, int ns, const int* s_batches_host, int nb,
                       float radius, int64_t cells_per_elem, void* ws, size_t ws_bytes, void* stream);
/* queries f32[nq,3]; q_order (nullable) int32[nq]: processing order, any permutation of 0..nq-1 (slot t handles query
 * q_order[t]) -- a spatially coherent order keeps a wavefront inside few cells; the result does not depend on it.  The fast
 * kernel takes a slot's batch element from the slot, so an order that keeps every element's queries inside that element's
 * range [q_off[b], q_off[b+1]) runs entirely on it (the grid's own order, or the order of another grid over the same
 * clouds, do); a query placed in another element's range is handed to the slower lane-per-query pass (same result).
 * Passing the grid's own supports with q_order == g->order (a self query in cell order) lets the kernel take index and
 * coordinates from the cell-ordered array in one load.  nbr_out int32[nq,k_out] (k_out may be 0: count only);
 * counts_out (nullable) int32[nq] = untruncated neighbour counts; max_count_out (nullable)
 * int32[1], atomically max-ed (caller zeroes it).  radius may differ from the build radius
 * as long as it is <= the grid's cell edge. */
int     buf_grid_query(const buf_grid_t* g, const float* queries, int nq, const int* q_batches_host,
                       const int* q_order, float radius, int k_out, int* nbr_out, int* counts_out,
                       int* max_count_out, void* todo_ws, void* stream);
/* todo_ws: int32[nq] scratch (rows longer than 64 neighbours -- and, in the cell-centric self query, cells whose 27-cell
 * candidate set exceeds the LDS stage -- are redone by a second, unbounded pass).  It may be null ONLY when k_out == 0 and
 * either q_order is null or the call is a self query (queries == the grid's supports, nq == ns, q_order == g->order); a
 * self query without it runs on the query-centric kernel.  A self query WITH it may write the list in the count-only
 * (k_out == 0) pass as well (stage-overflow queries), so the workspace must hold nq ints there too.
 * Build + query in one call (what batch_query does); ws >= buf_grid_ws_bytes(ns,nb,0) + 4*nq bytes. */
int     buf_radius_neighbors(const float* queries, int nq, const float* supports, int ns,
                             const int* q_batches_host, const int* s_batches_host, int nb, float radius,
                             int k_out, int* nbr_out, int* counts_out, int* max_count_out,
                             void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A1  grid subsampling -- cpp_subsampling.subsample_batch (grid_subsampling.cpp:5-106,109-211).
 *
 * Voxel key and barycentre arithmetic are the reference's, in fp32, summed in input order;
 * rows are emitted per batch element in ascending voxel-key order (the reference emits
 * libstdc++ unordered_map order: same multiset of rows, bit for bit).
 * out_pts f32[n,3] (capacity n rows); out_batches_host int32[nb]; returns M via *out_m_host.
 * `max_cells` bounds the dense voxel table (sum over elements); BUF_ECAPACITY if exceeded.
 * When every element has <= 16384 points the call is one workgroup per element with the sort in LDS (k_vox_fused:
 * no table in global memory, `max_cells` unused, no capacity to exceed); otherwise, or with BUF_VOX_FUSED=0 in the
 * environment, the global-table counting sort.  Both forms emit the same rows.
 * Synchronises `stream` (the row count has to reach the host).
 */
size_t  buf_grid_subsample_ws_bytes(int n, int nb, int64_t max_cells, int fdim);
/* feats (nullable) f32[n,fdim] -> out_feats f32[M,fdim]: per-voxel feature means, summed in input order. */
int     buf_grid_subsample_batch(const float* pts, int n, const int* batches_host, int nb, float dl,
                                 int max_p, const float* feats, int fdim, float* out_pts, float* out_feats,
                                 int* out_batches_host, int* out_m_host,
                                 int64_t max_cells, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * pointnet2_ops.pointnet2_utils surface (external CUDA package, README.md:31; call sites
 * models/BUFFER.py:266-271, models/patch_embedder.py:100-104, utils/common.py:442-455).
 * All tensors contiguous fp32 / int32 in device memory.
 */
/* furthest_point_sample: xyz f32[b,n,3] -> idx int32[b,m]; starts at index 0, skips points with
 * |p|^2 <= 1e-3, arg-max tie rule of the upstream 512-thread kernel.  ws only for n > 32768. */
size_t  buf_fps_ws_bytes(int b, int n);
int     buf_fps(const float* xyz, int b, int n, int m, int* idx_out, void* ws, size_t ws_bytes, void* stream);
/* ragged batch (clouds of different size sampled concurrently, one workgroup each): xyz f32[sum(n),3] stacked,
 * lengths_host int[b] -> idx int32[b,m], indices local to each cloud.  ws sized for (1, sum(n)). */
int     buf_fps_ragged(const float* xyz, const int* lengths_host, int b, int m, int* idx_out, void* ws, size_t ws_bytes,
                       void* stream);
/* gather_operation: feat f32[b,c,n], idx int32[b,m] -> f32[b,c,m] */
int     buf_gather(const float* feat, const int* idx, int b, int c, int n, int m, float* out, void* stream);
/* grouping_operation: feat f32[b,c,n], idx int32[b,m,nsample] -> f32[b,c,m,nsample] */
int     buf_group(const float* feat, const int* idx, int b, int c, int n, int m, int nsample, float* out, void* stream);
/* ball_query: first nsample points (index order) with d2 < radius^2; unused slots = first hit; rows
 * without any hit are all zero.  idx int32[b,m,nsample]. */
int     buf_ball_query(const float* xyz, const float* new_xyz, int b, int n, int m, float radius, int nsample,
                       int* idx, void* stream);
/* three_nn: unknown f32[b,n,3], known f32[b,m,3] -> dist f32[b,n,3] (sqrt of the 3 smallest d2), idx int32[b,n,3] */
int     buf_three_nn(const float* unknown, const float* known, int b, int n, int m, float* dist, int* idx, void* stream);
/* MiniSpinNet.select_patches fused (models/patch_embedder.py:93-121): pts f32[n,3] (already permuted),
 * kpts f32[m,3] -> patches f32[m,nsample,3] with the keypoint in every unused slot and in the last slot. */
int     buf_select_patches(const float* pts, const float* kpts, int n, int m, float radius, int nsample,
                           float* patches, void* stream);
/* The same (models/patch_embedder.py:93-121) for every cloud of a step in one launch: pts f32[sum n_c,3] = the (already permuted) support clouds stacked,
 * lengths_host int[nc], kpts f32[nc*m,3] (m keypoints per cloud) -> patches f32[nc*m,nsample,3].  Builds an A2 cell grid
 * over the stacked clouds in `ws` and walks a per-query bitmask of in-ball points in index order (identical results to
 * buf_select_patches cloud by cloud).  Per query the kernel takes the bitmask or the index-ordered scan, whichever its candidate
 * count makes faster; the development switch BUF_SPB_PATH (environment, read on every call) overrides that for every query of the
 * call: `grid` = the bitmask wherever the call has one (clouds up to 131 072 points), `scan` = the ordered scan, anything else or
 * unset = the kernel's own choice.  The result does not depend on it (tests/test_patch_select_gpu.py runs all three). */
size_t  buf_select_patches_batched_ws_bytes(int n_total, int nc);
int     buf_select_patches_batched(const float* pts, const int* lengths_host, int nc, const float* kpts, int m, float radius,
                                   int nsample, float* patches, void* ws, size_t ws_bytes, void* stream);
/* The random permutation of the support cloud that precedes the ball query (patch_embedder.py:97-98: torch.randperm) for nc
 * clouds in one launch: out[off_c + j] = cloud_c[prp_c(j)], prp_c = a keyed pseudo-random permutation of [0, n_c) (4-round
 * Feistel network, cycle-walked).  clouds_host: nc HOST-side pointers to DEVICE arrays f32[n_c,3]; keys_host: nc keys. */
int     buf_permute_clouds(const float* const* clouds_host, const int* lengths_host, const unsigned long long* keys_host,
                           int nc, float* out, void* stream);

/* A5b  ordered compaction of `x > threshold` (torch.where at models/BUFFER.py:255-259): ascending indices.
 * x f32 read with element stride `stride` (score[:,0] of an [n,1] tensor: stride 1); idx_out int32[n] capacity;
 * count_out int32[1] on the device. */
size_t  buf_compact_ws_bytes(int n);
int     buf_compact_greater(const float* x, int stride, int n, float threshold, int* idx_out, int* count_out,
                            void* ws, size_t ws_bytes, void* stream);

/* knn_cuda.KNN(k, transpose_mode=True) (README.md:32; models/BUFFER.py:347,352):
 * ref f32[b,n,d], query f32[b,q,d] -> dist f32[b,q,k] (Euclidean, ascending), idx int64[b,q,k]. d,k <= 64. */
size_t  buf_knn_ws_bytes(int b, int q, int k);
/* k = 1, d = 32 (the mutual-matching calls): with a workspace of buf_knn1_ws_bytes(b, n, q) bytes buf_knn ranks the pairs on the
 * f16 matrix pipe and forms the reference's fp32 sum only for the pairs it cannot separate from the best one (csrc/pointops.hip,
 * k_nn1f_*): same indices and distances, bit for bit, as the exact scan it falls back to with the smaller workspace. */
size_t  buf_knn1_ws_bytes(int b, int n, int q);
int     buf_knn(const float* ref, const float* query, int b, int n, int q, int d, int k, float* dist,
                long long* idx, void* ws, size_t ws_bytes, void* stream);

/* torch_batch_svd.svd (README.md:35; utils/common.py:715): a f32[n,3,3] -> u,s,v with a = u diag(s) v^T, s descending. */
int     buf_svd3x3_batched(const float* a, int n, float* u, float* s, float* v, void* stream);

/* ------------------------------------------------------------------------------------------
 * A4/A5  Vector-Neuron blocks (models/point_learner.py:315-416,467-582,246-265; models/vn_layers.py:46-75,108-130).
 * Feature rows f32[N,3C] channel-major/xyz-minor.  bn_scale = w/sqrt(var+1e-5), bn_shift = b - mean*bn_scale
 * (both null when Cout == 1: the reference skips VN batch-norm there).
 */
/* gather + VN-linear + VN-BN + VN-leaky + mean over all k slots.  mode 1: [f,delta]; mode 6: [f,delta,f x delta,mean(delta)].
 * idx int32[nq,k] with shadow index >= ns.  wf,wd f32[cout, cin+1 | cin+3]. */
int     buf_vn_gather_block(const float* q_pts, const float* s_pts, const float* feats, const int* idx,
                            int nq, int ns, int k, int cin, int cout, int mode, float scale,
                            const float* wf, const float* wd, const float* bn_scale, const float* bn_shift,
                            float slope, float* out, void* stream);
/* The same for mode '1' with the channel contraction hoisted out of the neighbour loop (csrc/vn.hip: the feature part of both
 * VN-linear maps is formed once per SUPPORT point, a neighbour slot adds the delta column): 4-5 x fewer operations in the resnet
 * blocks, results within half an ulp of a partial sum of buf_vn_gather_block.  ws: buf_vn_gather_pre_ws_bytes(ns, cout) bytes.
 * buf_vn_gather_pre_supported: 1 when the slot stage (16 * 32 * k bytes: k <= 96) and the weight stage (8 * cout * (cin + 1) bytes)
 * each fit the 48 KiB of LDS of a launch, else 0: buf_vn_gather_block_pre then returns BUF_EINVAL with nothing launched, and mode 1
 * of buf_vn_gather_block (any k) is the path to take. */
int     buf_vn_gather_pre_supported(int k, int cin, int cout);
size_t  buf_vn_gather_pre_ws_bytes(int ns, int cout);
int     buf_vn_gather_block_pre(const float* q_pts, const float* s_pts, const float* feats, const int* idx,
                                int nq, int ns, int k, int cin, int cout, float scale,
                                const float* wf, const float* wd, const float* bn_scale, const float* bn_shift,
                                float slope, float* out, void* ws, size_t ws_bytes, void* stream);
/* point-wise VN layer on concat(a[ind_a[i*ind_stride]] , b[i]) (+ residual); ind_a null = identity;
 * rows with index >= na read as zeros (closest_pool shadow); wd null = plain VN linear. */
int     buf_vn_pointwise(const float* a, const int* ind_a, int ind_stride, int na, int ca, const float* b, int cb,
                         int n, int cout, const float* wf, const float* wd, const float* bn_scale,
                         const float* bn_shift, float slope, const float* residual, float* out, void* stream);
/* max_pool (models/KPConv/blocks.py:104-121): out[i,f] = max_k feats_pad[idx[i,k], f], zero shadow row. */
int     buf_gather_max(const float* feats, const int* idx, int nq, int ns, int k, int width, float* out, void* stream);
/* Conv1d(kernel 1) of the score heads (models/point_learner.py:128-136,163-171): out[i] = W x[i] + b, x f32[n,cin],
 * W f32[cout,cin], b f32[cout] (device), cin, cout <= 32; activation 0 none, 1 sigmoid, 2 softplus. */
int     buf_row_linear(const float* x, int n, int cin, int cout, const float* w, const float* b, int activation, float* out,
                       void* stream);
/* InstanceNorm1d (biased variance, no affine) over contiguous row segments: the score heads of
 * models/point_learner.py:128-136,163-171 normalise over the stacked points of ONE pair; lens_host[s] rows per
 * segment (HOST int[nseg], sum = n).  x f32[n,c] -> out f32[n,c].  Deterministic (no atomics). */
size_t  buf_segment_instance_norm_ws_bytes(int nseg, int c);
int     buf_segment_instance_norm(const float* x, int n, int c, const int* lens_host, int nseg, float eps, float* out,
                                  void* ws, size_t ws_bytes, void* stream);
/* VNStdFeature tail (vn_layers.py:213-219): x f32[n,3c], z f32[n,9] -> f32[n,3c] invariant scalars. */
int     buf_vn_std(const float* x, const float* z, int n, int c, float* out, void* stream);
/* One whole score head of models/point_learner.py:128-136 (Ref.inv_layer -> eps) / :163-171 (Keypt.invar_layer -> saliency) in 7
 * launches: VNStdFeature (vn1 -> vn2 -> vn_lin -> x . z, vn_layers.py:169-222) + Conv1d 30 -> 20 | InstanceNorm1d over the pair |
 * Conv1d 20 -> c1 | InstanceNorm1d | Conv1d c1 -> 1 + activation (0 none, 1 sigmoid, 2 softplus).  x f32[n,30] -> out f32[n,1];
 * lens_host: rows per pair (HOST int[nseg], sum = n).  vn*_wf / _wd: map_to_feat / map_to_dir [Cout,Cin]; _bsc / _bsh: folded VN
 * batch-norm (null: none); lin: vn_lin's map_to_feat [3,5]; w* / b*: Conv1d weights [Cout,Cin] / bias.  Only the released
 * widths (10 -> 10 -> 5 -> 3; 30 -> 20 -> c1 <= 10 -> 1); bit-identical to buf_vn_pointwise x 3, buf_vn_std, buf_row_linear and
 * buf_segment_instance_norm called one after the other. */
size_t  buf_score_head_ws_bytes(int n, int nseg);
int     buf_score_head(const float* x, int n, const int* lens_host, int nseg,
                       const float* vn1_wf, const float* vn1_wd, const float* vn1_bsc, const float* vn1_bsh, float vn1_slope,
                       const float* vn2_wf, const float* vn2_wd, const float* vn2_bsc, const float* vn2_bsh, float vn2_slope,
                       const float* lin, const float* w0, const float* b0, const float* w1, const float* b1, int c1,
                       const float* w2, const float* b2, int final_activation, float eps, float* out,
                       void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A9+A10 (+ point MLP of A11) fused: axis alignment, normalisation, cylindrical voxelisation
 * (420 ball queries of `nsample` per patch), azimuth de-rotation, Conv1x1(3->16)+BN+ReLU, max.
 * (models/patch_embedder.py:123-171,74-79; utils/common.py:431-498,501-525)
 * patches f32[np,npts,3] (keypoint in the last slot); axis f32[np,3] or null (KITTI/ETH: R = I);
 * centres f32[ncentres,3]; azi_cs f32[azi_n,2] = cos,sin of -i*2pi/azi_n; mlp_* are HOST arrays
 * (w[16,3], b[16], bn_scale[16], bn_shift[16]).  out_x f32[np,16,ncentres]; out_R f32[np,3,3];
 * out_rand f32[np,3]; out_patches (nullable) f32[np,npts,3].
 * ws: device workspace of buf_patch_voxelize_ws_bytes(ncentres) bytes (the split-f16 operand tables of the distance and
 * MLP matrix instructions, rebuilt by every call; BUF_EWORKSPACE when too small).  The hit decisions are the reference's
 * fp32 test `d2 < r2` bit for bit (csrc/voxelize.hip: matrix-pipe filter + fp32 re-test of the pairs it cannot call).
 */
size_t  buf_patch_voxelize_ws_bytes(int ncentres);
int     buf_patch_voxelize(const float* patches, const float* axis, int npatch, int npts, float des_r,
                           const float* centres, int ncentres, int azi_n, const float* azi_cs, float voxel_r,
                           int nsample, const float* mlp_w_host, const float* mlp_b_host, const float* bn_scale_host,
                           const float* bn_shift_host, float* out_x, float* out_R, float* out_rand, float* out_patches,
                           void* ws, size_t ws_bytes, void* stream);

/* A11 (dense)  Cylindrical_Net (models/patchnet.py:15-85): Conv3d(16->64, 3x3x3) + 7 x Conv2d 3x3, BatchNorms folded, circular
 * azimuth / zero elevation padding (utils/common.py:265-310), as ONE kernel in the Winograd F(2x2,3x3) domain, all fp32
 * (csrc/convnet_wg.hip: 38 instead of 75 matrix instructions per 4 input x 16 output channels; a different fp32 summation
 * order, within 1e-6 of the output scale of a direct-form evaluation: tests/native/convnet_direct.hip is that cross-check).
 * x f32[np,48,140] (= [np,16,3,7,20]) -> y f32[np,32,140] (= [np,32,7,20]); bias_host[l]: DEVICE pointers to [Cout].
 * wt_host[l]: DEVICE pointers to U = G g G^T of the BN-folded filters ([Cout,Cin,3,3]; layer 0: Cin = c16*3 + depth) in the
 * tiling [N-group][i][k-step][n2][lk][li][j] = U[i][j][16 (NG g + n2) + li][4 ks + lk] with NG = buf_winograd_group(Cin, Cout)
 * N-tiles per group (the N-tiles one wavefront owns: its k-steps are contiguous in memory), as buf_winograd_tile_weights lays
 * them out (fp64 on the host; output row 6, whose window ends in the elevation padding, runs in the direct form for its columns
 * 0..15 -- 6 matrix instructions on a full M-tile -- with the six taps formed in registers from U_0, U_1 and U_2).  Cin a multiple of 16 (of 32 for Cout 128), Cout in {32, 64, 128}, last layer 32. */
int     buf_winograd_group(int cin, int cout);                                                   /* host only: NG of a layer: 2 for every width */
int     buf_winograd_tile_weights(const float* w_host, int cout, int cin, float* out_host);   /* host only: [Cout,Cin,3,3] -> 16*Cout*Cin floats */
int     buf_winograd_tile_filters(const float* w_host, int cout, int cin, int ng, int nblk, float* out_host);
                                                   /* host only: the same tiling with N-groups of ng and nblk = 4 | 5 blocks -> 4*nblk*Cout*Cin floats */
/* The F(2x4, 3x3) form of the layers with 128 output channels (csrc/convnet_w24.hip, w24_layer_pair: tiles of 2 x 4 outputs along
 * the azimuth, 30 instead of 38 matrix instructions per 4 input x 16 output channels in those layers; the other layers as above;
 * all fp32).  Opt-in per call through relu_host[l]: bit 0 is the ReLU as before, bit 1 (BUF_CYL_F24) says that wt_host[l] holds,
 * BEHIND the 16*Cout*Cin floats above, the 24*Cout*Cin floats of buf_winograd_f24_tile_weights: U = G2 g G4^T (4 row x 6 column
 * components; points 0, +-1, +-2, infinity; fp64 on the host) tiled [pair][i][k-step][768] with, per (row component i, k-step),
 * the column components j = 0, 1, 2, 5 of the pair's two N-tiles as [n2][lk][li][4] and then j = 3, 4 as [n2][lk][li][2].
 * If any layer carries the bit, every layer with 128 output channels must and no other may (else BUF_EINVAL); with 0 / 1 in
 * every word nothing beyond the first 16*Cout*Cin floats of a buffer is read. */
#define BUF_CYL_F24 2
/* The same form in layers with 64 output channels and Cin a multiple of 64 (csrc/convnet_w24k.hip, kernel k_cyl_net_w24k: the four
 * wavefronts split K and exchange partial sums through LDS; 30 instead of 38 matrix instructions there as well).  Bit 2 (BUF_CYL_F24K)
 * of relu_host[l] says that wt_host[l] holds the 24*Cout*Cin floats of buf_winograd_f24_tile_weights behind its 16*Cout*Cin floats.
 * Allowed only on such layers, and only in a stack that also satisfies the bit-1 rule above (every layer with 128 output channels
 * carries bit 1); words above 7 are rejected (BUF_EINVAL).  buf_cylindrical_net_wg_flags reports what a call would accept. */
#define BUF_CYL_F24K 4
int     buf_cylindrical_net_wg_flags(const int* cin_host, const int* cout_host, const int* relu_host);   /* host only: 0 if these 8 widths and relu words are accepted */
int     buf_winograd_f24_tile_weights(const float* w_host, int cout, int cin, float* out_host);   /* host only: [Cout,Cin,3,3] -> 24*Cout*Cin floats; Cout a multiple of 32 */
int     buf_cylindrical_net_wg(const float* x, int npatch, const float* const* wt_host, const float* const* bias_host,
                               const int* cin_host, const int* cout_host, const int* relu_host, float* y, void* stream);
/* The layers that carry bit 2 have two forms of the same arithmetic up to the order of summation: the K split above (k_cyl_net_w24k) and
 * the pass split (csrc/convnet_w24p.hip, a layer form of k_cyl_net_w25t: each wavefront owns one row component of the F(2,3) row transform for all
 * four N-tiles over the whole K, folds once and hands three N-tiles' partial outputs over through LDS).  Same buffers, same flags;
 * `form` picks one per call (no process-wide state), BUF_CYL_FORM_DEFAULT what buf_cylindrical_net_wg runs: the pass split
 * (profiles/f24p_ab.md).  A form outside -1..1 is
 * BUF_EINVAL; a stack without bit 2 runs as it does through buf_cylindrical_net_wg. */
#define BUF_CYL_FORM_DEFAULT (-1)
#define BUF_CYL_FORM_K_SPLIT 0
#define BUF_CYL_FORM_PASS_SPLIT 1
int     buf_cylindrical_net_wg_form(const float* x, int npatch, const float* const* wt_host, const float* const* bias_host,
                                    const int* cin_host, const int* cout_host, const int* relu_host, int form, float* y, void* stream);
int     buf_cylindrical_net_wg_supports(const int* cin_host, const int* cout_host);   /* host only: 0 if the kernel is built for these 8 widths */
/* F(2x4) tiles in EVERY layer (csrc/convnet_w24a.hip, layer forms of k_cyl_net_w25t): buf_cylindrical_net_wg with one more array.  wt_host,
 * bias_host and relu_host are exactly what buf_cylindrical_net_wg takes (same buffers, same words, same rules and messages for the words).
 * wt24_host[8]: per layer null, or the 24*Cout*Cin floats of buf_winograd_f24_tile_weights ([pair][i][k-step][768]) in a buffer of their
 * own -- allowed on a layer that carries neither BUF_CYL_F24 nor BUF_CYL_F24K and has 64 or 32 output channels, else BUF_EINVAL.  A
 * 64-output layer with a set runs the pass-split form of the bit-2 layers (any Cin that is a multiple of 16: layer 0's 48), a 32-output
 * layer with a set the pass split over its one N-tile pair; a layer without a set runs as it does through buf_cylindrical_net_wg.  The widths rules
 * are those of buf_cylindrical_net_wg_supports with one change: the rule "only 32-output layers follow a 32-output layer" binds from the
 * first 32-output layer WITHOUT a set on, to the end of the stack (its form leaves partial sums in zero words that later, wider layers
 * would read as padding); behind 32-output layers that all have their sets any supported layer may follow.  All checks happen before
 * the first device call; buf_cylindrical_net_wg_all_flags reports on the host what a call would accept (of wt24_host it looks only at
 * which entries are null).  Timed under BUF_TIMED_CYL_NET with the dense flop figure. */
int     buf_cylindrical_net_wg_all_flags(const int* cin_host, const int* cout_host, const int* relu_host, const float* const* wt24_host);
int     buf_cylindrical_net_wg_all(const float* x, int npatch, const float* const* wt_host, const float* const* bias_host,
                                   const int* cin_host, const int* cout_host, const int* relu_host, const float* const* wt24_host,
                                   float* y, void* stream);
/* F(2x5, 3x3) tiles (csrc/convnet_w25.hip, a layer form of k_cyl_net_w25t): tiles of 2 rows x 5 azimuth columns carry the 7 x 20 map with 4 x 4
 * regular tiles, 28 matrix instructions per 4 input x 16 output channels and no direct round of row 6 (F(2x4): 24 + 6).
 * buf_cylindrical_net_wg_all with one more array, wt25_host[8]: per layer null, or the 28*Cout*Cin floats of
 * buf_winograd_f25_tile_weights -- U = G2 g G5^T (4 row x 7 column components; points 0, +-1, +-2, +-1/2; fp64 on the host) tiled
 * [i][k-step][N-tile][448] with, per (row component, k-step, N-tile), the column components j = 0..3 as [lk][li][4], j = 4, 5 as
 * [lk][li][2] and j = 6 as [lk][li] -- in a buffer of their own.  Allowed on a layer with 64 or 32 output channels and Cin a multiple of
 * 16, whatever F(2x4) bit its relu word or entry of wt24_host it carries (the F(2x5) set wins); else BUF_EINVAL.  A layer without
 * one runs as in buf_cylindrical_net_wg_all, and with no F(2x5) set at all the result is that entry point's, bit for bit.  A 32-output
 * layer with an F(2x5) set counts as one with a set in the widths rule above.  buf_cylindrical_net_w25_flags: host only. */
int     buf_winograd_f25_tile_weights(const float* w_host, int cout, int cin, float* out_host);   /* host only: [Cout,Cin,3,3] -> 28*Cout*Cin floats; Cout a multiple of 16 */
int     buf_cylindrical_net_w25_flags(const int* cin_host, const int* cout_host, const int* relu_host, const float* const* wt24_host,
                                      const float* const* wt25_host);
int     buf_cylindrical_net_w25(const float* x, int npatch, const float* const* wt_host, const float* const* bias_host,
                                const int* cin_host, const int* cout_host, const int* relu_host, const float* const* wt24_host,
                                const float* const* wt25_host, float* y, void* stream);
/* Host-formed row-6 taps and the direct round first in the layers with 128 output channels (csrc/convnet_w25t.hip, kernel k_cyl_net_w25t).
 * buf_cylindrical_net_w25 with one more array and one more word.  taps_host[8]: per layer null, or the 6*Cout*Cin floats of
 * buf_cyl_row6_tile_taps -- the filter rows 0 and 1 as they are, tiled [pair][k-step][q = 0..2][lk][li][4] with float 4 q + e =
 * 6 n2 + 3 a + b of a lane -- in a buffer of their own; allowed on a layer with 128 output channels that carries BUF_CYL_F24, else
 * BUF_EINVAL.  order: 0, or BUF_CYL_ROW6_FIRST: the direct round of row 6 runs in front of the Winograd round in every such layer.
 * A layer without a tap set forms its taps as in buf_cylindrical_net_w25; with no set and order = 0 the result is that entry point's,
 * bit for bit. */
#define BUF_CYL_ROW6_FIRST 1
int     buf_cyl_row6_tile_taps(const float* w_host, int cout, int cin, float* out_host);   /* host only: [Cout,Cin,3,3] -> 6*Cout*Cin floats; Cout a multiple of 32 */
int     buf_cylindrical_net_w25t(const float* x, int npatch, const float* const* wt_host, const float* const* bias_host,
                                 const int* cin_host, const int* cout_host, const int* relu_host, const float* const* wt24_host,
                                 const float* const* wt25_host, const float* const* taps_host, int order, float* y, void* stream);

/* A11 (dense), split-f16 form -- the same stack with fp32-EQUIVALENT arithmetic on the f16 matrix pipe (csrc/convnet_h3.hip; opt-in,
 * the all-fp32 kernel above stays the default): every fp32 operand is split once into hi = f16(x) and lo' = f16((x - hi) 2^11)
 * (x = hi + 2^-11 lo' to one fp32 ulp), a product sum is [sum hi hi] + 2^-11 [sum hi lo' + sum lo' hi] in two fp32 accumulators:
 * three v_mfma_f32_16x16x32_f16 per (16 outputs x 16 positions x 32 channels), direct 9-tap form.  Measured against the float64
 * stack: not worse than the fp32 kernels (tests/test_model_gpu.py, profiles/r04_f16_split.txt).  Requires every activation and
 * weight below 65504 in magnitude (f16 range): weights are checked by the tiler, an activation that leaves the range sets bit 0
 * of *status_dev (DEVICE int32, nullable; the caller clears and reads it) -- the BARE kernel: a caller that does not manage the range
 * itself uses buf_cylindrical_net_split_safe below, which re-runs such patches on the fp32 kernel.
 * x f32[np,Cin0,140] -> y f32[np,32,140]; bias_host[l]: DEVICE f32[Cout]; wt_host[l]: DEVICE u16 planes as buf_split_tile_filters
 * lays them out from the BN-folded filters [Cout,Cin,3,3]:
 *   out[((((g 9 + tap) KS + ks) 2 + n2) 2 + plane) 512 + (kg 16 + row) 8 + i] = plane(w[32 g + 16 n2 + row][32 ks + 8 kg + i][tap]),
 *   tap = 3 ky + kx, KS = ceil(Cin / 32) (channels beyond Cin zero), plane 0 = hi, plane 1 = lo'; buf_split_filter_count u16 values.
 * Cin a multiple of 16, <= 128, not in 65..96; Cout in {32, 64, 128}; last layer 32. */
long long buf_split_filter_count(int cout, int cin);                                             /* host only */
int     buf_split_tile_filters(const float* w_host, int cout, int cin, unsigned short* out_host);   /* host only */
int     buf_cylindrical_net_split(const float* x, int npatch, const void* const* wt_host, const float* const* bias_host,
                                  const int* cin_host, const int* cout_host, const int* relu_host, float* y, int* status_dev, void* stream);
/* The same stack with buf_descriptor_head fused behind its last layer (the [32][140] map stays in LDS): head_params = DEVICE
 * f32[545] as for buf_descriptor_head -> desc f32[np,32], equi f32[np,32,140]; bit-identical to the two calls in sequence. */
int     buf_cylindrical_net_split_head(const float* x, int npatch, const void* const* wt_host, const float* const* bias_host,
                                       const int* cin_host, const int* cout_host, const int* relu_host, const float* head_params,
                                       float* desc, float* equi, int* status_dev, void* stream);

/* The split form made SAFE BY CONSTRUCTION (csrc/split_safe.hip; what buffer_amd.ops.CylindricalNetSplit calls): flags_ws (DEVICE
 * int32[np], scratch) is cleared, the split kernel sets flags_ws[p] for every patch whose input or hidden activation left the f16 range
 * (NaN included), then buf_cylindrical_net_wg's kernel runs over the same grid with the flags as a mask -- workgroups of clear patches
 * return at once, flagged patches are recomputed in fp32 and overwrite their result (bit-identical to buf_cylindrical_net_wg [+
 * buf_descriptor_head] for those patches).  Same stream, no host round trip; nothing is returned from behind an overflow.
 * head_params null: y_or_equi = y f32[np,32,140]; else desc f32[np,32] and y_or_equi = equi f32[np,32,140].
 * wt_split_host as buf_cylindrical_net_split, wt_wg_host as buf_cylindrical_net_wg (relu_host may carry BUF_CYL_F24 / BUF_CYL_F24K for it: the
 * split kernel sees bit 0 only), bias_host shared.  Replaces the model's
 * torch layers of models/patchnet.py:15-85 exactly like the two entry points it combines. */
int     buf_cylindrical_net_split_safe(const float* x, int npatch, const void* const* wt_split_host, const float* const* wt_wg_host,
                                       const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                                       const float* head_params, float* y_or_equi, float* desc, int* status_dev, int* flags_ws, void* stream);

/* The same with the form of the fp32 re-run stated (BUF_CYL_FORM_*, as for buf_cylindrical_net_wg_form) */
int     buf_cylindrical_net_split_safe_form(const float* x, int npatch, const void* const* wt_split_host, const float* const* wt_wg_host,
                                            const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                                            int form, const float* head_params, float* y_or_equi, float* desc, int* status_dev, int* flags_ws,
                                            void* stream);
/* The same with the fp32 re-run through k_cyl_net_w25t_rerun: wt24_host as for buf_cylindrical_net_wg_all (a flagged patch is bit-identical
 * to that entry point's result) */
int     buf_cylindrical_net_split_safe_all(const float* x, int npatch, const void* const* wt_split_host, const float* const* wt_wg_host,
                                           const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                                           const float* const* wt24_host, const float* head_params, float* y_or_equi, float* desc,
                                           int* status_dev, int* flags_ws, void* stream);
/* The same with wt24_host and wt25_host as for buf_cylindrical_net_w25 */
int     buf_cylindrical_net_split_safe_w25(const float* x, int npatch, const void* const* wt_split_host, const float* const* wt_wg_host,
                                           const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                                           const float* const* wt24_host, const float* const* wt25_host, const float* head_params,
                                           float* y_or_equi, float* desc, int* status_dev, int* flags_ws, void* stream);
/* The same with the fp32 re-run through k_cyl_net_w25t_rerun: taps_host and order as for buf_cylindrical_net_w25t */
int     buf_cylindrical_net_split_safe_w25t(const float* x, int npatch, const void* const* wt_split_host, const float* const* wt_wg_host,
                                            const float* const* bias_host, const int* cin_host, const int* cout_host, const int* relu_host,
                                            const float* const* wt24_host, const float* const* wt25_host, const float* const* taps_host,
                                            int order, const float* head_params, float* y_or_equi, float* desc, int* status_dev,
                                            int* flags_ws, void* stream);

/* A11 (head)  attention pooling + normalisation (models/patch_embedder.py:66-72,81-84): pool_layer
 * (Conv2d 1x1 32->16 + BN + ReLU, Conv2d 1x1 16->1 + BN + ReLU), desc = normalize(mean(y * w)),
 * equi = normalize(y, channel).  y f32[np,32,140] -> desc f32[np,32], equi f32[np,32,140].
 * params: DEVICE f32[545] = w0 [16][32], b0 [16], w3 [16], b3 [1] with the BatchNorms folded. */
int     buf_descriptor_head(const float* y, int npatch, const float* params, float* desc, float* equi, void* stream);

/* ------------------------------------------------------------------------------------------
 * A13  CostVolume + CostNet (models/BUFFER.py:37-66, models/patchnet.py:88-147) fused on fp32 MFMA: the
 * [m,32,20,5,20] cost tensor is never built.  s_eq,t_eq f32[m,32,5,20] (elevation rows 1..ele_n-2 of the
 * equivariant maps) -> ind f32[m] (expected azimuth shift).  wt_host/bias_host: HOST arrays of 10 DEVICE
 * pointers, BN folded; layers 6..9: weights W[K][Cout] with K = ((dn*KH + dk)*KW + dl)*Cin + c, the last layer (20
 * outputs) zero-padded to 32 columns / biases.  Layers 1..5 run in the Winograd F(2x2,3x3) domain as 3x3 correlations over
 * (n, l): buf_winograd_tile_filters(w2d, Cout, Cin2d, ng, 4, out) with ng = buf_cost_winograd_group(layer) N-tiles per group
 * (16*Cout*Cin2d floats each), w2d = the (3,1,3) filters [Cout,Cin,3(dn),3(dl)]
 * for layers 2..5 and, for layer 1 (which collapses k: 3 -> 1), [64][dk*32 + c][dn][dl] = W1[o][c][dn][dk][dl], Cin2d = 96.  Layer 0 is linear in cost = S(shifted) - T and is passed SEPARATED
 * (exact up to fp32 re-association): wt_host[0] = Ws[480][32] followed by Wt[288][32],
 *   Ws[(dk*5 + e+2)*32 + c][o] = sum over dl-dn=e of W0[o][c][dn][dk][dl],  Wt[(dk*3 + dl)*32 + c][o] = sum over dn of W0
 * (buffer_amd.ops.separate_cost_layer0).  Every [K][Cout] matrix is stored in the MFMA B-operand tiling: blocks
 * [K/16][Cout/16] of 256 floats, block (g, n) laid out [lk 0..3][li 0..15][p 0..3] = W[16g + 4lk + p][16n + li]
 * (buffer_amd.ops.mfma_tile_weights(w, lk_major=True) is the host-side re-layout). */
int     buf_cost_winograd_group(int layer);           /* host only: ng of layers 1..5 = 2, 2, 2, 2, 1 (0 for the others) */
int     buf_cost_volume_net(const float* s_eq, const float* t_eq, int m, const float* const* wt_host,
                            const float* const* bias_host, float* ind_out, void* stream);
/* The same with the row gather of models/BUFFER.py:285-292 (ss_equi = src_equi[s_mids], [:, :, 1:ele_n-1]) fused in:
 * equi f32[rows,32,ele_n,20] = the full equivariant maps of all keypoints (ele_n = 7),
 * match i pairs row s_rows[i] with row t_rows[i] (DEVICE int64[m]); elevation rows 1..ele_n-2 are read inside the kernel. */
int     buf_cost_volume_net_gather(const float* equi, int ele_n, const long long* s_rows, const long long* t_rows, int m,
                                   const float* const* wt_host, const float* const* bias_host, float* ind_out, void* stream);
/* The twins with the layer forms of csrc/costnet_w24.hip: F(2x4, 3x3) tiles in layers 2 and 4, the Winograd F(2x2) form in layer 6.
 * f24_host: HOST array of 3 DEVICE pointers, each nullable -- [0], [1]: buf_winograd_f24_tile_weights of the [Cout][Cin][3][3] filters
 * of layers 2 and 4, [2]: buf_winograd_tile_filters(w2d, 64, 64, 1, 4, out) of layer 6.  A layer without a set runs as in
 * buf_cost_volume_net from wt_host (all ten matrices are still required).  The timed span is BUF_TIMED_COST_NET with the same work figure. */
int     buf_cost_volume_net_w24(const float* s_eq, const float* t_eq, int m, const float* const* wt_host, const float* const* bias_host,
                                const float* const* f24_host, float* ind_out, void* stream);
int     buf_cost_volume_net_w24_gather(const float* equi, int ele_n, const long long* s_rows, const long long* t_rows, int m,
                                       const float* const* wt_host, const float* const* bias_host, const float* const* f24_host,
                                       float* ind_out, void* stream);
/* The twins with the layer forms of csrc/costnet_w24b.hip: beside the forms above, layer 1 on F(2x4) tiles (one k' plane resident at a
 * time) and layer 3 as F(2x4) rows with an F(2x2) tail.  f24_host: HOST array of 5 DEVICE pointers, each nullable -- [0..2] as above,
 * [3]: buf_winograd_f24_tile_weights of layer 1's collapsed filter [64][96 = (dk, c)][dn][dl], [4]: the same of layer 3's [128][64][3][3].
 * A layer without a set runs as in buf_cost_volume_net_w24.  The timed span is BUF_TIMED_COST_NET with the same work figure. */
int     buf_cost_volume_net_w24b(const float* s_eq, const float* t_eq, int m, const float* const* wt_host, const float* const* bias_host,
                                 const float* const* f24_host, float* ind_out, void* stream);
int     buf_cost_volume_net_w24b_gather(const float* equi, int ele_n, const long long* s_rows, const long long* t_rows, int m,
                                        const float* const* wt_host, const float* const* bias_host, const float* const* f24_host,
                                        float* ind_out, void* stream);

/* A13, split-f16 form -- the same network with fp32-EQUIVALENT arithmetic on the f16 matrix pipe (csrc/costnet_h3.hip; opt-in, see
 * buf_cylindrical_net_split for the operand split): layer 0 separated as above, every layer a direct-form correlation.
 * wt_host: HOST array of 11 DEVICE pointers to u16 planes laid out by buf_split_tile_gemm(w [Cout][Cin][ntaps], Cout, Cin, ntaps, nt, out):
 *   [0] layer 0 S-term [32][32][15 taps = dk*5 + e+2] = Ws, nt 2      [1] layer 0 T-term [32][32][9 taps = dk*3 + dl] = Wt, nt 2
 *   [2] layer 1 [64][96 = dk*32 + c][9 taps = dn*3 + dl], nt 2         [3..8] layers 2..7 [Cout][Cin][9 taps = dn*3 + dl], nt 2 (layer 7: nt 1)
 *   [9] layer 8, nt 1          [10] layer 9 [20][32][4 taps = dn*2 + dl], nt 1 (20 outputs padded to 32)
 * out[((((g ntaps + tap) KS + ks) nt + n2) 2 + plane) 512 + (kg 16 + row) 8 + i] = plane(w[16 nt g + 16 n2 + row][32 ks + 8 kg + i][tap]).
 * bias_host: 10 DEVICE f32 pointers (layer 9: 32 values, 20 used).  status_dev as in buf_cylindrical_net_split. */
long long buf_split_gemm_count(int cout, int cin, int ntaps, int nt);                               /* host only */
int     buf_split_tile_gemm(const float* w_host, int cout, int cin, int ntaps, int nt, unsigned short* out_host);   /* host only */
int     buf_cost_volume_net_split(const float* s_eq, const float* t_eq, int m, const void* const* wt_host,
                                  const float* const* bias_host, float* ind_out, int* status_dev, void* stream);
int     buf_cost_volume_net_split_gather(const float* equi, int ele_n, const long long* s_rows, const long long* t_rows, int m,
                                         const void* const* wt_host, const float* const* bias_host, float* ind_out,
                                         int* status_dev, void* stream);
/* Safe by construction, as buf_cylindrical_net_split_safe (models/patchnet.py:88-147): per-match flags in flags_ws (DEVICE int32[m]),
 * the fp32 kernel of buf_cost_volume_net[_gather] re-runs the flagged matches in the same stream.  s_rows null: dense s_eq / t_eq
 * f32[m,32,5,20]; else s_eq = t_eq = equi f32[rows,32,7,20] with DEVICE int64 row ids.  wt_split_host / bias_split_host as
 * buf_cost_volume_net_split, wt_f32_host / bias_f32_host as buf_cost_volume_net. */
int     buf_cost_volume_net_split_safe(const float* s_eq, const float* t_eq, int ele_n, const long long* s_rows, const long long* t_rows,
                                       int m, const void* const* wt_split_host, const float* const* bias_split_host,
                                       const float* const* wt_f32_host, const float* const* bias_f32_host, float* ind_out,
                                       int* status_dev, int* flags_ws, void* stream);
/* The same with the masked re-run in the layer forms of buf_cost_volume_net_w24: f24_host as for buf_cost_volume_net_w24, whose bits the flagged matches carry. */
int     buf_cost_volume_net_split_safe_w24(const float* s_eq, const float* t_eq, int ele_n, const long long* s_rows, const long long* t_rows,
                                           int m, const void* const* wt_split_host, const float* const* bias_split_host,
                                           const float* const* wt_f32_host, const float* const* bias_f32_host, const float* const* f24_host,
                                           float* ind_out, int* status_dev, int* flags_ws, void* stream);
/* ... and in those of buf_cost_volume_net_w24b: f24_host[5] as for that entry point. */
int     buf_cost_volume_net_split_safe_w24b(const float* s_eq, const float* t_eq, int ele_n, const long long* s_rows, const long long* t_rows,
                                            int m, const void* const* wt_split_host, const float* const* bias_split_host,
                                            const float* const* wt_f32_host, const float* const* bias_f32_host, const float* const* f24_host,
                                            float* ind_out, int* status_dev, int* flags_ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * A14 hypotheses + all-vs-all scoring (models/BUFFER.py:295-311): ind f32[m] -> R f32[m,3,3], t f32[m,3],
 * inlier_num int32[m], best_out int32[1] (first arg-max), best_mask uint8[m]. */
int     buf_hypotheses_score(const float* ind, const float* ss_kpts, const float* tt_kpts, const float* ss_R,
                             const float* tt_R, int m, int azi_n, float inlier_th, float* R_out, float* t_out,
                             int* inlier_num, int* best_out, unsigned char* best_mask, void* stream);
/* A15  deterministic 3-point RANSAC over `corr` (int32[ncorr] indices into src/tgt, both f32[*,3]);
 * replaces open3d registration_ransac_based_on_correspondence (models/BUFFER.py:314-326).
 * T_out f32[4,4]; info_out (nullable) int32[2] = {inliers of the winner, winner id or -1}. */
size_t  buf_ransac_ws_bytes(int nhyp);
int     buf_ransac_kabsch(const float* src, const float* tgt, const int* corr, int ncorr, int nhyp,
                          unsigned long long seed, float max_dist, float edge_similarity, float* T_out,
                          int* info_out, void* ws, size_t ws_bytes, void* stream);
/* The same on the correspondences selected by mask uint8[m] (best_mask of buf_hypotheses_score): index list and count
 * stay on the device, so a pose recovery is enqueued without a host round trip.  ws: buf_ransac_masked_ws_bytes(m, nhyp). */
size_t  buf_ransac_masked_ws_bytes(int m, int nhyp);
int     buf_ransac_kabsch_masked(const float* src, const float* tgt, const unsigned char* mask, int m, int nhyp,
                                 unsigned long long seed, float max_dist, float edge_similarity, float* T_out,
                                 int* info_out, void* ws, size_t ws_bytes, void* stream);
/* A16  post_refinement (models/BUFFER.py:382-418,424-464): <= iters rounds of weighted Kabsch in one launch.
 * T_init,T_out f32[4,4]; src,tgt f32[m,3]; info_out (nullable) int32[2] = {last inlier count, rounds run}. */
int     buf_post_refine(const float* T_init, const float* src, const float* tgt, int m, float inlier_threshold,
                        int iters, float* T_out, int* info_out, void* stream);
/* A14 + A15 + A16 (models/BUFFER.py:295-311 hypotheses and scoring, :314-326 RANSAC, :382-464 post_refinement) for every pair of
 * a step in one set of launches: the matches of nb pairs stacked (pair p owns seg_host[p]
 * consecutive rows of ind f32[M], ss/tt_kpts f32[M,3], ss/tt_R f32[M,9]); seeds_host u64[nb] (RANSAC sampler seed per pair);
 * refine_iters = 0 skips the post-refinement (KITTI) -> poses f32[nb,4,4] (identity for pairs with fewer than 3 matches).
 * Pair by pair bit-identical to buf_hypotheses_score + buf_ransac_kabsch_masked + buf_post_refine. */
size_t  buf_recover_poses_ws_bytes(int m_total, int nb, int nhyp);
int     buf_recover_poses_batched(const float* ind, const float* ss_kpts, const float* tt_kpts, const float* ss_R, const float* tt_R,
                                  const int* seg_host, int nb, const unsigned long long* seeds_host, int azi_n, float inlier_th,
                                  int nhyp, float max_dist, float edge_similarity, float refine_threshold, int refine_iters,
                                  float* poses_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * N1  pre-processing that feeds the path (ThreeDMatch/dataset.py:93,104,125-153; KITTI/dataset.py): the open3d
 * 0.13.0 calls of the reference's datasets, restated from open3d's published algorithms (parity unpinned).
 *
 * buf_voxel_downsample = PointCloud.voxel_down_sample: voxel index floor((p - (min - voxel/2)) / voxel), one row per
 * occupied voxel = fp64 mean of its points (and normals, not re-normalised), rows in ascending voxel-key order.
 * pts / normals: f32[n,3] (is_f64 = 0) or f64[n,3] (is_f64 = 1), normals nullable; out_pts / out_normals f64[>=n,3];
 * *out_m_host = rows written.  max_cells as in buf_grid_subsample_batch.
 *
 * buf_knn_normals = estimate_normals(KDTreeSearchParamKNN(knn)) + orient_normals_towards_camera_location on the
 * candidate lists of a radius search: cand int32[nq,ncand] = buf_grid_query output (sorted by distance, >= ns = empty),
 * knn <= ncand <= 48.  The knn nearest are re-ranked in fp64; covariance by cumulants, normal = eigenvector of the
 * smallest eigenvalue (open3d FastEigen3x3).  qidx (nullable) maps row -> point (for retries on a subset; null: row = point, nq <= ns);
 * deficient[row] = 1 when the row holds fewer than min(knn, ns) points (its search ball was too small: retry with a
 * larger radius), else the normal of point qidx[row] is written.  camera_host: HOST double[3]. */
size_t  buf_voxel_downsample_ws_bytes(int n, int64_t max_cells);
int     buf_voxel_downsample(const void* pts, const void* normals, int is_f64, int n, double voxel_size, double* out_pts,
                             double* out_normals, int* out_m_host, int64_t max_cells, void* ws, size_t ws_bytes, void* stream);
/* The same for nb clouds stacked in pts (lengths_host int[nb]) in ONE set of launches and one host round trip: out_pts holds the
 * voxel means of cloud 0, then cloud 1, ... (out_lengths_host int[nb]); every cloud has its own bounding box / voxel grid, so the
 * rows equal those of nb separate calls. */
size_t  buf_voxel_downsample_batch_ws_bytes(int n, int nb, int64_t max_cells);
int     buf_voxel_downsample_batch(const void* pts, int is_f64, int n, const int* lengths_host, int nb, double voxel_size,
                                   double* out_pts, int* out_lengths_host, int64_t max_cells, void* ws, size_t ws_bytes, void* stream);
int     buf_knn_normals(const float* pts, int ns, const int* qidx, int nq, const int* cand, int ncand, int knn,
                        const double* camera_host, int orient, float* normals, unsigned char* deficient, void* stream);

/* N2  ICP (KITTI/dataset.py:95-117 open3d registration_icp; open3d 0.13.0 restated, parity unpinned): B pairs per call.
 * src f32[sum src_lengths_host,3] and tgt f32[sum tgt_lengths_host,3] stack the pairs' clouds (pair b owns src_lengths_host[b]
 * / tgt_lengths_host[b] consecutive rows); tgt_normals f32[*,3] (nullable for point-to-point); T_init_f64 f64[B,4,4] (device).
 * buf_icp_batched takes methods 0 and 1; buf_gicp_batched is method 2 with its two further arguments, src_normals f32[*,3] and epsilon.
 * method BUF_ICP_POINT_TO_POINT: rigid update = Kabsch with the det correction of the centred cross-covariance (fp64);
 * method BUF_ICP_POINT_TO_PLANE: J^T J x = -J^T r (J = [p x n, n], r = (p - q) . n, absolute coordinates, fp64 Cholesky),
 *   dT = [Rz(x2) Ry(x1) Rx(x0) | x3..5] (open3d TransformVector6dToMatrix4d, restated, unpinned).
 * method BUF_ICP_GENERALIZED (plane-to-plane, Segal et al.; open3d registration_generalized_icp restated, unpinned): per match, in
 *   fp64, d = p - q, S = C(n_q) + R C(n_s) R^T with C(n) = I - (1 - epsilon) n n^T (R = the rotation block of the running T), M = S^-1
 *   (symmetric 3x3, by cofactors), J = [-[p]x | I]; H = sum J^T M J, g = sum J^T M d, H x = -g by the point-to-plane Cholesky and the
 *   same dT.  A normal row counts if | |n|^2 - 1 | < 1e-3 in fp64 (which a non-finite component fails); any other row is taken as
 *   zero, C = I: clouds without usable normals take isotropic (point-to-point Gauss-Newton) steps.  epsilon = 1 does the same.
 *   inlier_rmse stays Euclidean (open3d reports the Mahalanobis residual): the three methods share fitness, rmse and stopping rules.
 * Correspondence of a source point: p = T s in fp64, rounded to fp32; the nearest target point of its pair with fp32 d2 < max_dist^2
 * (buf_grid_query's arithmetic, ties to the lowest index = column 0 of the buf_grid_query row); non-finite points never match.
 * Per pair: fitness = matches / source points, rmse = sqrt(sum d2 / matches) (0 without matches), d2 Euclidean in fp64.
 * The loop of buffer_amd/icp.py::icp_point_to_point: the iteration count is the number of updates applied; a pair stops before an
 * update with fewer than 3 (point-to-point) / 6 (point-to-plane, generalized) matches or a system that is not positive definite (T unchanged),
 * after an update when |d fitness| < rel_fitness and |d rmse| < rel_rmse, and after max_iteration updates.  T_out f64[B,4,4],
 * fitness_out / rmse_out f64[B] and iters_out int32[B] (device) belong to the last correspondence pass, as does nn_out
 * (nullable, int32[sum src_lengths]: global target row of every source point, sum tgt_lengths_host = no match).  An empty pair
 * returns T_init, fitness 0, 0 iterations.  Results are bitwise reproducible and independent of the other pairs of the batch.
 * Synchronises: one int is read back after every 8th round (at most ceil((max_iteration + 1) / 8) readbacks).
 * BUF_EINVAL before any device work for max_dist <= 0 or not finite, point-to-plane without normals, negative lengths, a method
 * other than 0 / 1 in buf_icp_batched (it has no source normals: method 2 is buf_gicp_batched), and in buf_gicp_batched a null normal
 * array or an epsilon outside (0, 1] or not finite.  buf_icp_ws_bytes takes all three methods. */
#define BUF_ICP_POINT_TO_POINT 0
#define BUF_ICP_POINT_TO_PLANE 1
#define BUF_ICP_GENERALIZED 2
size_t  buf_icp_ws_bytes(int n_src_total, int n_tgt_total, int npairs, int method);
int     buf_icp_batched(const float* src, const int* src_lengths_host, const float* tgt, const float* tgt_normals,
                        const int* tgt_lengths_host, int npairs, int method, float max_dist, const double* T_init_f64,
                        int max_iteration, double rel_fitness, double rel_rmse, double* T_out_f64, double* fitness_out,
                        double* rmse_out, int* iters_out, int* nn_out, void* ws, size_t ws_bytes, void* stream);
int     buf_gicp_batched(const float* src, const float* src_normals, const int* src_lengths_host, const float* tgt,
                         const float* tgt_normals, const int* tgt_lengths_host, int npairs, float max_dist, double epsilon,
                         const double* T_init_f64, int max_iteration, double rel_fitness, double rel_rmse, double* T_out_f64,
                         double* fitness_out, double* rmse_out, int* iters_out, int* nn_out, void* ws, size_t ws_bytes, void* stream);

/* N6  FPFH descriptors (Rusu, Blodow, Beetz 2009; open3d compute_fpfh_feature with KDTreeSearchParamHybrid restated from its
 * published form, parity unpinned: this text is the specification).  One call for any number of stacked clouds.
 * pts, normals f32[n,3]; nbr int32[n,k_nbr] = a buf_grid_query row per point (ascending by (d2, index), padded with values >= n:
 * the rows stay inside a point's cloud, so no lengths are needed); fpfh_out f64[n,33]; spfh_out f64[n,33] (nullable: the table is
 * then kept in ws, buf_fpfh_ws_bytes(n) bytes; with spfh_out given no workspace is read).
 * Row of point i: the entries < n (and >= 0) among the first min(max_nn, k_nbr) columns, m_i of them.  Column 0 is taken to be the
 *   point itself and is skipped, whatever it holds (open3d's k = 1..).  m_i < 2: both output rows of i are zero.
 * Pair feature of (i, j), all fp64 on the fp32 inputs promoted, no FMA, dot products as (x + y) + z:
 *   d = p_j - p_i, L = sqrt(d . d); L == 0: f = (0, 0, 0).  a1 = n_i . d / L, a2 = n_j . d / L.  If |a1| < |a2| (open3d tests
 *   acos|a1| > acos|a2|: the same decision without the transcendental): (n1, n2, d) = (n_j, n_i, -d), f2 = -a2; else (n1, n2) =
 *   (n_i, n_j), f2 = a1.  v = d x n1; |v| == 0: f = (0, 0, 0); else v /= |v|, w = n1 x v, f1 = v . n2, f0 = atan2(w . n2, n1 . n2).
 * Bins: x0 = 11 (f0 + pi) / (2 pi), x1 = 11 (f1 + 1) / 2, x2 = 11 (f2 + 1) / 2; bin(x) = 0 if !(x >= 0), 10 if x >= 11, else (int)x
 *   (NaN and -inf: bin 0, +inf: bin 10).  Feature c counts in slot 11 c + bin; a zero feature is binned too (slots 5, 16, 27).
 * SPFH: integer counts, spfh[i][s] = count * (100.0 / (m_i - 1)).  (open3d adds the increment 100 / (m_i - 1) once per pair: the
 *   product differs from that sum by rounding only and can be tested exactly.)
 * FPFH: acc[s] = sum over the row's columns 1.. in column order of spfh[j][s] * w_ij with w_ij = 1.0 / d2_ij (formed once per
 *   neighbour; open3d divides by d2 per slot: rounding only), d2 = d . d as above; j is skipped unless 0 < d2 < inf.  For each block
 *   of 11 slots S_c = the sum of acc over the block in ascending slot order; S_c != 0: the block is multiplied by 100.0 / S_c.
 *   fpfh[i][s] = acc[s] + spfh[i][s].
 * No float atomics, every sum has a fixed order: a point's rows are the same bits alone, in any batch and on reruns.
 * BUF_EINVAL before any device work for n < 0, k_nbr < 1, max_nn < 2 or > 128, a null input or fpfh_out with n > 0, and, when
 * spfh_out is null, a workspace that is null or smaller than buf_fpfh_ws_bytes(n).  n == 0 succeeds and touches nothing. */
size_t  buf_fpfh_ws_bytes(int n);
int     buf_fpfh(const float* pts, const float* normals, int n, const int* nbr, int k_nbr, int max_nn,
                 double* fpfh_out /* f64[n,33] */, double* spfh_out /* f64[n,33], nullable = use ws */,
                 void* ws, size_t ws_bytes, void* stream);

/* N11  ISS keypoints (Intrinsic Shape Signatures, Zhong 2009, in the simplified form of open3d's compute_iss_keypoints, restated
 * from its published form, parity unpinned: this text is the specification).  One call for any number of stacked clouds, two
 * launches (saliency, then non-maximum suppression, which reads saliency_out), no workspace, nothing read back.
 * pts f32[n,3]; nbr_sal int32[n,k_sal] / nbr_nms int32[n,k_nms] = a buf_grid_query row per point at the salient / the non-max radius
 * (ascending by (d2, index), padded with values >= n: the rows stay inside a point's cloud, so no lengths are needed; the two may be
 * one array).  saliency_out f64[n]; eig_out f64[n,3] (nullable); mask_out u8[n]: 1 = keypoint.
 * Rows: the valid entries of a row are those with 0 <= idx < n among its first min(max_nn, k) columns (max_nn == 0: all k columns);
 *   the point itself is one of them (column 0 is not skipped: the covariance is taken over the whole support, as open3d does).
 * Saliency of point i, m_i = the valid entries of its salient row.  m_i < min_neighbors: eigenvalues and saliency are 0.  Otherwise,
 *   all fp64 on the fp32 coordinates promoted, no FMA: mu = (sum p_j) / m_i and C_ab = (sum (p_j,a - mu_a)(p_j,b - mu_b)) / m_i, six
 *   entries, every sum over the valid entries in column order.  lambda1 >= lambda2 >= lambda3 = the eigenvalues of C: cyclic Jacobi,
 *   pivots (0,1), (0,2), (1,2), until the off-diagonal absolute sum is <= 1e-20 of the diagonal's or 12 sweeps are done: a
 *   deterministic function of the six entries (backward stable: each lambda is within a few ulp of lambda1 of the exact one).
 *   s_i = lambda3 if lambda1 > 0 and lambda2 < gamma_21 * lambda1 and lambda3 < gamma_32 * lambda2, else 0 (products: open3d divides;
 *   lambda1 > 0 restates its cov.isZero() exit).  eig_out[i] = (lambda1, lambda2, lambda3).
 * Non-maximum suppression: mask_i = 1 iff s_i > 0, the non-max row of i has at least min_neighbors valid entries, and no valid entry j
 *   of it has s_j > s_i.  Ties keep both points (open3d's IsLocalMaxima).
 * Further deviations from open3d: its radius search is in fp64 on a KD-tree, the rows here come from the caller (buf_grid_query: fp32
 *   d2 < r*r); it takes the resolution heuristic and the cloud, here both radii arrive as rows.
 * A NaN or infinite point has an empty row in the grid, so it falls under the first rule, and it is in no other row: every output is
 * finite.  No float atomics, every sum has a fixed order: a point's outputs are the same bits alone, in any batch and on reruns.
 * BUF_EINVAL before any device work, buf_last_error naming the argument, for n < 0, k_sal or k_nms < 1, max_nn < 0,
 * min_neighbors < 1, a gamma that is not finite or not positive, and with n > 0 a null pts, nbr_sal, nbr_nms, saliency_out or
 * mask_out.  n == 0 succeeds and touches nothing. */
int     buf_iss_keypoints(const float* pts, int n, const int* nbr_sal, int k_sal, const int* nbr_nms, int k_nms, int max_nn,
                          double gamma_21, double gamma_32, int min_neighbors, double* saliency_out /* f64[n] */,
                          double* eig_out /* f64[n,3], nullable */, unsigned char* mask_out /* u8[n] */, void* stream);

/* N13  Normals and covariances of radius and hybrid neighbourhoods (open3d estimate_normals / estimate_covariances with
 * KDTreeSearchParamRadius / KDTreeSearchParamHybrid, restated from the published form, parity unpinned: this text is the
 * specification).  One call for any number of stacked clouds, one launch, no workspace, nothing read back.
 * pts f32[n,3]; nbr int32[n,k_nbr] = a buf_grid_query row per point (ascending by (d2, index), padded with values >= n: the rows stay
 * inside a point's cloud, so no lengths are needed).  normals_out f32[n,3], cov_out f64[n,6] = (c00, c01, c02, c11, c12, c22),
 * count_out int32[n]: each nullable, not all three.
 * Rows: the valid entries of row i are those with 0 <= idx < n among its first min(max_nn, k_nbr) columns, wherever they sit
 *   (max_nn == 0: all k_nbr columns); m_i is their number.  The point itself is one of them, as the grid returns it: nothing is skipped.
 * Arithmetic, all fp64 on the fp32 coordinates promoted, no FMA: q = p_i.  For each valid entry j in column order d = p_j - q,
 *   S1_a += d_a and S2 += (dx dx, dx dy, dx dz, dy dy, dy dz, dz dz).  m_i >= 3: mu = S1 / m_i, E = S2 / m_i, cov_ab = E_ab - mu_a * mu_b;
 *   the normal is the eigenvector of the smallest eigenvalue as open3d's FastEigen3x3 finds it (the solver of buf_knn_normals: the same
 *   function of the six entries), a zero vector from it becomes (0, 0, 1).  m_i < 3: cov = (1, 0, 0, 1, 0, 1) (open3d's identity) and
 *   the normal is (0, 0, 1).  orient != 0: the normal is flipped when n . (camera - q) < 0, the products summed left to right as
 *   buf_knn_normals sums them.  count_out[i] = m_i.
 * Deviations from open3d: the moments are taken about the query point, not the origin (the same covariance up to rounding, far better
 *   conditioned for clouds away from the origin: the cancellation in E - mu mu^T is of the order of the neighbourhood's radius squared,
 *   not of the cloud's distance squared); the rows come from the fp32 grid search (d2 < r*r in fp32), not from an fp64 KD-tree.
 * Non-finite points: a NaN or infinite point has an empty row in the grid and lies in no other row, so it takes the m_i < 3 rule.  A
 *   hand-made row of three or more entries that names a non-finite point has a covariance with non-finite entries: cov_out holds them
 *   as computed and the normal is (NaN, NaN, NaN); nothing else follows from it.  Indices are range-checked: nothing is read out of bounds.
 * order (nullable) int32[n], a permutation of the points: slot t of the launch handles point order[t] (an entry outside [0, n) is
 *   skipped).  Speed only: with the grid's cell order (buf_grid_t.order) the gathers of a wavefront stay inside a few cells.  The result
 *   does not depend on it.
 * No float atomics, every sum has a fixed order: a point's outputs are the same bits alone, in any batch, with any order and on reruns.
 * BUF_EINVAL before any device work, buf_last_error naming the argument, for n < 0, k_nbr < 1, max_nn < 0, all three outputs null,
 * orient != 0 with a null camera_host (f64[3], host), and with n > 0 a null pts or nbr.  n == 0 succeeds and touches nothing. */
int     buf_row_normals(const float* pts, int n, const int* nbr, int k_nbr, int max_nn, const int* order /* nullable */,
                        const double* camera_host, int orient, float* normals_out /* f32[n,3], nullable */,
                        double* cov_out /* f64[n,6], nullable */, int* count_out /* int32[n], nullable */, void* stream);

/* N14  Exact k nearest neighbours in 3-D on the cell grid (open3d KDTreeSearchParamKNN).  One launch for any number of stacked clouds,
 * no workspace beyond the grid's, nothing read back.
 * g: a grid of buf_grid_build, at whatever radius it was built (the cell edge affects speed only).  queries f32[nq,3], element b of the
 * grid owning the next q_batches_host[b] of them: a query's candidates are the supports of its own element.
 * Distance: d2 = (dx*dx + dy*dy) + dz*dz in fp32 without contraction, buf_grid_query's.  A pair whose d2 is not finite -- a NaN or
 * infinite coordinate on either side, or an overflow -- matches nothing (buf_grid_query's d2 < r*r never accepts one either): a
 * non-finite support is in no row and a non-finite query has a fully padded row.
 * Row qi of nbr_out int32[nq,k]: the k smallest keys (bits of d2, global support index) in ascending order, so ties go to the lower
 * index exactly as in a buf_grid_query row -- wherever such a row at some radius holds k entries or more, its first k are this row.
 * Fewer than k matches: the tail is padded with ns (g->ns).  d2_out (nullable) f32[nq,k]: the d2 of every entry, +inf in the padding.
 * 1 <= k <= 64.  q_order (nullable) int32[nq]: slot t of the launch handles query q_order[t], as in buf_grid_query (an entry outside
 * [0, nq) is skipped); the result does not depend on it.
 * Search: rings of cells at Chebyshev distance 0, 1, 2, ... around the query's cell (a query outside the box starts from the nearest
 * border cell), closed once the k-th d2 lies strictly below the squared distance from the query to the nearest face of the visited
 * cube inside the grid (taken in fp64 from the build's cell arithmetic, reduced by a margin that covers the fp32 rounding of d2), or
 * once the cube covers the element's grid.  At most max(dim) + 1 rings on any input.
 * No atomics: a query's row is the same bits alone, in any batch, under any q_order and on reruns.
 * BUF_EINVAL before any device work, buf_last_error naming the value, for a null g or q_batches_host, nq < 0, k outside [1, 64],
 * lengths that are negative or do not sum to nq, and with nq > 0 a null queries or nbr_out.  nq == 0 succeeds and writes no output;
 * the queries of an empty element get padded rows. */
int     buf_grid_knn(const buf_grid_t* g, const float* queries, int nq, const int* q_batches_host, const int* q_order /* nullable */,
                     int k, int* nbr_out /* int32[nq,k] */, float* d2_out /* nullable f32[nq,k] */, void* stream);

/* N15  The sums of open3d's remove_statistical_outlier (0.13, restated from the published form, parity unpinned: this text is the
 * specification) on k-NN rows: nc stacked clouds per call, two launches, no float atomics, nothing read back.
 * d2 f32[n,k]: a buf_grid_knn d2 row per point (self query, the point itself in column 0, +inf padding at the tail); cloud c owns
 * the next lengths_host[c] rows.
 *   mean_i  = the fp64 sum, in column order, of sqrt((double) d2_ij) over the row's entries before the first that is not finite,
 *             divided by their number; -1 for a row without entries.                                         -> mean_out f64[n]
 *   V       = the cloud's number of rows with entries; mu = (sum of the mean_i > 0) / V;
 *   sd      = sqrt(sum over mean_i > 0 of (mean_i - mu)^2 / (V - 1)); thr = mu + std_ratio * sd.     -> stats_out f64[nc,3] = mu, sd, thr
 *   keep_i  = mean_i > 0 && mean_i < thr.                                -> keep_out u8[n], kept_out int32[nc] = kept rows per cloud
 * The rule is followed literally: a cloud of one point has V - 1 = 0, sd = NaN and keeps nothing; a cloud of two points has sd = 0,
 * thr = mu = both means and keeps nothing; an empty cloud has mu = NaN.
 * Sums per cloud: thread t of 256 adds the cloud's rows t, t + 256, ... in that order, the 256 partial sums are folded by a binary
 * tree with strides 128, 64, ..., 1.  The order depends on the cloud's length alone: a cloud's numbers are the same bits alone or stacked.
 * ws: int32[nc + 1] device scratch (buf_outlier_statistical_ws_bytes).  BUF_EINVAL for n < 0, k < 1, nc < 1, a NaN std_ratio, lengths
 * that are negative or do not sum to n, a null lengths_host, stats_out, kept_out or ws, and with n > 0 a null d2, mean_out or keep_out. */
size_t  buf_outlier_statistical_ws_bytes(int nc);
int     buf_outlier_statistical(const float* d2, int n, int k, const int* lengths_host, int nc, double std_ratio,
                                double* mean_out /* f64[n] */, double* stats_out /* f64[nc,3] */, unsigned char* keep_out /* u8[n] */,
                                int* kept_out /* int32[nc] */, void* ws, size_t ws_bytes, void* stream);

/* N12  Batched descriptor matching with a mutual and a ratio filter: exact, ragged, `pairs` pairs per call.  One scan launch for both
 * directions of all pairs, two small launches for the filters and the ordered output; no atomics; the host reads nothing back.
 * Pair p owns a_lengths_host[p] / b_lengths_host[p] consecutive rows of fa / fb (f32[., d], device, 1 <= d <= 64): A_p and B_p.
 * Distance of rows (i, j): ssd = the fp32 sum over the dimensions IN ORDER of (a_c - b_c)^2, formed with __fsub_rn, __fmul_rn and
 *   __fadd_rn, never contracted (the operations of buf_knn): ssd(i, j) is the same bits as ssd(j, i), and a zero dimension appended to
 *   both rows changes nothing.
 * Ranking: by the 64-bit key (float bits of ssd) << 32 | row index, as buf_knn ranks.  The nearest row has the smallest key, the
 *   second nearest the second smallest; ties go to the lower row.
 * Forward match of row i of A_p: its nearest row j of B_p.
 * mutual != 0: the row stays only if i is the nearest row of A_p to j.
 * 0 < ratio < 1: the row stays only if ssd1 <= r2 * ssd2, with ssd1 / ssd2 the FORWARD nearest and second-nearest sums (the ratio test
 *   looks at the forward direction only: at the neighbours in B_p of the row of A_p, never at those of j in A_p),
 *   r2 = (float)((double)ratio * ratio) and the product one __fmul_rn: the squared form of Lowe's test, no square root.  Without a
 *   second neighbour (one row in B_p, or one ranked row) the test passes.  ratio <= 0 switches the test off.
 * Non-finite rows: a row with a NaN or infinite component is matched by nobody and matches nobody, on either side (it is not ranked).
 *   Finite rows whose sum overflows to +inf are ranked like any other.
 * Output: the surviving (i, j), pair-local indices, ascending i inside a pair, the pairs stacked in pair order, in corr_out
 *   (int32[na_total, 2] capacity; the rows past the total are not written); counts_out[p] (device int32[pairs]) = the rows of pair p.
 *   nn_out (nullable) int32[na_total, 2] = per row of A its nearest and second-nearest row of B_p, -1 where there is none; ssd_out
 *   (nullable) f32[na_total, 2] = their sums, +inf where there is none.  Both cover the forward direction, filters or not.
 * A pair's rows are the same bits alone, in any batch and at every launch.  With mutual != 0, the ratio off and finite inputs they are
 * the rows of two buf_knn calls at k = 1 and the comparison idx_ba[idx_ab[i]] == i.
 * BUF_EINVAL before any device work for pairs < 0, d outside 1..64, ratio >= 1 or NaN, a null host array or counts_out, a negative
 * length, 2^31 - 1 rows or more on a side, a null input that has rows, a null corr_out when A has rows, and a workspace that is null
 * or smaller than buf_feature_match_ws_bytes(na_total, nb_total, pairs).  pairs == 0 succeeds and touches nothing; without a row in
 * A the counts are zeroed and nothing else is touched; a pair with an empty side yields no rows. */
size_t  buf_feature_match_ws_bytes(long long na_total, long long nb_total, int pairs);
int     buf_feature_match(const float* fa, const int* a_lengths_host, const float* fb, const int* b_lengths_host,
                          int pairs, int d, int mutual, float ratio,
                          int* corr_out /* int32[na_total,2] capacity */, int* counts_out /* device int32[pairs] */,
                          int* nn_out /* optional int32[na_total,2]: nearest, second (-1 if none) */,
                          float* ssd_out /* optional f32[na_total,2], +inf if none */,
                          void* ws, size_t ws_bytes, void* stream);

/* N7  Fast Global Registration (Zhou, Park, Koltun, ECCV 2016; open3d registration_fast_based_on_feature_matching restated from
 * its published form, parity unpinned: this text is the specification).  B pairs per call, two launches, nothing read back.
 * Pair b owns src_lengths_host[b] / tgt_lengths_host[b] consecutive rows of src / tgt (f32[.,3], device) and corr_lengths_host[b]
 * consecutive rows of corr (int32[.,2], device: (src row, tgt row) inside the pair's own clouds), and draws with seeds_host[b].
 * All arithmetic is fp64 on the fp32 inputs promoted, without FMA; dot products are (x + y) + z.
 * Tuple test (AdvancedMatching, step 3), on the coordinates as given, n = the pair's correspondences, ntrial = trial_factor * n:
 *   trial t draws r_k = splitmix64(seed + 3 t + k) % n, k = 0, 1, 2 (the mixer of buf_ransac_kabsch: splitmix64(0) =
 *   0xE220A8397B1DCDAF; with replacement, as open3d draws).  a_e / b_e = the squared lengths of the edges e = (0,1), (1,2), (2,0)
 *   between the three target / source points, d = u - v, (dx*dx + dy*dy) + dz*dz.  With s2 = tuple_scale * tuple_scale (formed once,
 *   on the host) the trial is accepted iff s2 * a_e < b_e and s2 * b_e < a_e for all three edges: strict, so a repeated index or a
 *   coincident point rejects it.  (open3d compares scale * l < l' and l' < l / scale on the lengths, after normalisation: the same
 *   decision up to rounding, without a square root.)  A trial with an index outside its cloud or a non-finite coordinate is rejected.
 *   The accepted trials are kept in ascending trial order, the first max_tuples of them, each adding its three correspondences in the
 *   order k = 0, 1, 2 (duplicates stay).  trials examined = 1 + the trial that filled the list, ntrial when it never filled.
 *   rows_out[b] (nullable) int32[3 max_tuples, 2] = the kept (src row, tgt row), the tail -1.
 * Normalisation (NormalizePointCloud, one scale): c_src, c_tgt = the means of the pair's whole clouds, D = the largest |p - c| over
 *   both; a row with a non-finite coordinate is left out of mean, count and maximum.  The means are fixed-shape sums: lane k of 256
 *   adds the rows k, k + 256, ... in ascending order, then a tree over the lanes.  The points used below are (p - c) / D.  An empty
 *   cloud (no finite row) or D == 0 gives status NOTHING.
 * Optimisation (OptimizePairwiseRegistration).  Fewer than 10 kept rows: status NOTHING.  Else T = I, mu = mu_start, floor = delta
 *   (delta_absolute == 0: open3d's own comparison, in normalised units) or (delta / D)^2 (delta_absolute != 0: the paper's).  For
 *   it = 0 .. iterations - 1, over the kept rows (s, p): q = R s + t per row of T as ((R0*sx + R1*sy) + R2*sz) + t; r = p - q;
 *   w = (mu / (r.r + mu))^2, w = 0 where r.r is not finite (open3d transforms a copy of the cloud step by step instead of
 *   accumulating T: rounding only).  Jacobian rows [0, -qz, qy, -1, 0, 0], [qz, 0, -qx, 0, -1, 0], [-qy, qx, 0, 0, 0, -1];
 *   H += w J J^T, g += w J r, summed in the shape of the means; H x = -g by the LDL^T of buf_icp_batched; T <- dT(x) T with
 *   dT = [Rz(x2) Ry(x1) Rx(x0) | x3..5]; then, if it % decrease_every == 0 and mu > floor, mu /= division_factor.  A system that is
 *   not positive definite or a non-finite solution stops the pair with status FAILED and the T of the last good iterate.
 * Outputs (device).  T_out f64[B,4,4] src -> tgt = [R | D t + c_tgt - R c_src]; a pair without an applied update (NOTHING, FAILED
 *   in the first step, iterations == 0) returns the identity exactly (open3d would return the translation c_tgt - c_src there).
 *   info_out int32[B,4] = status (BUF_FGR_*), tuples kept, trials examined, updates applied.  weights_out[b] (nullable)
 *   f64[3 max_tuples] = w of the last linearisation per kept row (the failed one included), NaN in the tail and everywhere when
 *   nothing was linearised.  No float atomics, every sum has a fixed order: a pair's outputs are the same bits alone, in any batch,
 *   in any batch order and on reruns.
 * BUF_EINVAL before any device work for npairs < 0, negative lengths, a null required argument with npairs > 0 (src / tgt / corr only
 * where their rows are not zero), tuple_scale outside (0, 1], max_tuples outside 1..4096, trial_factor < 1 or trial_factor * n beyond
 * int, mu_start / delta / division_factor not finite and > 0, division_factor <= 1, decrease_every < 1, iterations < 0, and a
 * workspace that is null or smaller than buf_fgr_ws_bytes.  npairs == 0 succeeds and touches nothing; a pair with n == 0 returns the
 * identity, NOTHING and zeros. */
#define BUF_FGR_NOTHING 0
#define BUF_FGR_OK      1
#define BUF_FGR_FAILED  2
size_t  buf_fgr_ws_bytes(int n_corr_total, int npairs, int max_tuples);
int     buf_fgr_batched(const float* src, const int* src_lengths_host, const float* tgt, const int* tgt_lengths_host,
                        const int* corr /* int32[sum corr_lengths,2]: (src row, tgt row), local to the pair's clouds */,
                        const int* corr_lengths_host, int npairs, const unsigned long long* seeds_host,
                        double tuple_scale, int max_tuples, int trial_factor,          /* 0.95, 1000, 100 */
                        double mu_start, double delta, int delta_absolute,             /* 1.0, 0.025, 0 */
                        double division_factor, int decrease_every, int iterations,    /* 1.4, 4, 64 */
                        double* T_out /* f64[B,4,4] src -> tgt */, int* info_out /* int32[B,4] */,
                        int* rows_out /* nullable int32[B,3*max_tuples,2] */, double* weights_out /* nullable f64[B,3*max_tuples] */,
                        void* ws, size_t ws_bytes, void* stream);

/* N8  SC2-PCR (Chen, Sun, Yang, Tao, "SC^2-PCR: A Second Order Spatial Compatibility for Efficient and Robust Point Cloud
 * Registration", CVPR 2022), the single-stage form: a deterministic consensus estimator on given correspondences, the third pose
 * estimator of the classical row.  No SC2-PCR source was at hand: the algorithm is restated from its published form, parity with any
 * other implementation is unpinned and this text is the specification.  The paper's second sampling stage (k2) and its learned
 * variants are not provided.  B pairs per call, 8 + power_iterations launches on the caller's stream, nothing read back.
 * Pair b owns src_lengths_host[b] / tgt_lengths_host[b] consecutive rows of src / tgt (f32[.,3], device) and n = corr_lengths_host[b]
 * consecutive rows of corr (int32[.,2], device: (src row, tgt row) inside the pair's own clouds); row i is (p_i, q_i), promoted to
 * fp64.  A row is DEAD if an index is outside its cloud or a coordinate is not finite: its row and column of both compatibility
 * matrices are zero, the diagonal included, and it is never a seed, a set member or an inlier.  All arithmetic is IEEE fp64, every
 * product, sum, division and square root rounded once in the written order, without FMA.
 *   d(a, b) = sqrt(((ax-bx)^2 + (ay-by)^2) + (az-bz)^2);  e_ij = |d(p_i, p_j) - d(q_i, q_j)|.
 *   Hard compatibility C_ij = (e_ij <= d_thr), kept as a BIT MATRIX of n x ceil(n / 64) 64-bit words per pair (bit j % 64 of word
 *   j / 64 of row i; C is symmetric, so row j serves as column j).  Soft compatibility s_ij = max(0, 1 - (e_ij e_ij) / (d_thr d_thr))
 *   (d_thr d_thr formed once on the host); it is recomputed from the points wherever it is used and is exactly 0 where C_ij = 0.
 *   Confidence: v = 1 on the live rows, then power_iterations times v <- S v and v <- v / max v.  v_i is summed in a fixed shape: the
 *   columns in tiles of 128, tile t into partial sum t % 4 in ascending order, v_i = (s0 + s1) + (s2 + s3).
 *   Non-maximum suppression (nms_radius > 0): c_i = v_i unless a live j with d(p_i, p_j) <= nms_radius has v_j > v_i, then c_i = -1;
 *   nms_radius == 0: c = v.
 *   Seeds: S = min(max_seeds, max(1, ceil(seed_ratio n))) (n = all rows of the pair); the seeds are the S rows of largest c, ties to
 *   the lowest row, only those with c > 0; a seed's rank is its place in that order.
 *   Second-order counts of seed s: K[s, j] = C[s, j] * sum_k C[s, k] C[k, j] = the population count of (row s AND row j), masked by
 *   bit j of row s.  Its consensus set: the k1 columns of largest K, ties to the lowest column, only K > 0, in that order; fewer than
 *   3 members: no hypothesis, count -1.
 *   Hypothesis: weights w = 1 on the set, power_iterations times w <- S_set w (ascending set order), w <- w / max w; with
 *   u = w / sum w: cp = sum u p, cq = sum u q, H = sum u ((p - cp)(q - cq)^T), R = V diag(1, 1, det(V U^T)) U^T of H = U S V^T
 *   (one-sided Jacobi; the identity for H = 0 or a non-finite H), t = cq - R cp.  The sums over the set run over lanes and a tree.
 *   Score = the live rows with |R p + t - q| < inlier_thr, R p per row as ((R0 px + R1 py) + R2 pz) + t.  The winner has the largest
 *   score, ties to the lowest rank.
 *   Refinement, up to refine_iterations passes: the inliers of the current pose; stop if this is not the first pass and their number
 *   did not grow, or if it is below 3; else the unweighted Kabsch pose over them (means, then H, in the fixed shape of 256 lanes and
 *   a tree) is the next pose.  The final count and inliers_out are those of the pose returned.
 * Outputs (device).  T_out f64[B,4,4] src -> tgt.  info_out int32[B,6] = status (BUF_SC2_*), live rows, seeds, the winner's row (-1
 *   without a hypothesis), the winner's score before refinement, the final count.  NOTHING = fewer than 3 live rows, no hypothesis or
 *   a winner with fewer than 3 inliers: the identity exactly, final count 0, no inliers.  Nullable: conf_out f64[sum n] (v after the
 *   last normalisation, NaN on dead rows), seeds_out / hyp_counts_out int32[B,max_seeds] (rows and scores by rank, tail -1),
 *   counts_out int32[max_seeds * sum n] (pair b's block starts at max_seeds * (its first correspondence row), rank r at + r n_b;
 *   ranks without a seed -1), inliers_out uint8[sum n].  No atomics, every sum has a fixed order: a pair's outputs are the same bits
 *   alone, in any batch, in any batch order and on reruns.
 * BUF_EINVAL before any device work for npairs outside 0..65535, negative lengths, more than BUF_SC2_MAX_ROWS correspondences in a pair,
 * a null required argument with npairs > 0 (src / tgt / corr only where their rows are not zero), d_thr / inlier_thr not finite and
 * > 0, seed_ratio outside (0, 1], max_seeds outside 1..1024, k1 outside 3..128, nms_radius negative or not finite, power_iterations
 * outside 0..1000, refine_iterations < 0, and a workspace that is null or smaller than buf_sc2_ws_bytes (sized from the actual
 * lengths: 76 bytes per row, the bit matrices, 4 min(max_seeds, max(1, n)) n bytes of counts and 104 max_seeds + 48 bytes per pair,
 * each array rounded up to 256 bytes; 0 for arguments out of range).  npairs == 0 succeeds and touches nothing. */
#define BUF_SC2_NOTHING 0
#define BUF_SC2_OK      1
#define BUF_SC2_MAX_ROWS 16384
size_t  buf_sc2_ws_bytes(const int* corr_lengths_host, int npairs, int max_seeds);
int     buf_sc2_batched(const float* src, const int* src_lengths_host, const float* tgt, const int* tgt_lengths_host,
                        const int* corr /* int32[sum corr_lengths,2]: (src row, tgt row), local to the pair's clouds */,
                        const int* corr_lengths_host, int npairs,
                        double d_thr, double inlier_thr, double seed_ratio, int max_seeds,     /* -, -, 0.2, 512 */
                        int k1, double nms_radius, int power_iterations, int refine_iterations, /* 30, 0, 10, 20 */
                        double* T_out /* f64[B,4,4] src -> tgt */, int* info_out /* int32[B,6] */,
                        double* conf_out, int* seeds_out, int* hyp_counts_out, int* counts_out, unsigned char* inliers_out /* nullable */,
                        void* ws, size_t ws_bytes, void* stream);

/* N9  Voxelized Generalized ICP (Koide, Yokozuka, Oishi, Banno, "Voxelized GICP for fast and accurate 3D point cloud
 * registration", ICRA 2021) against a reusable map of target voxels.  No VGICP source was at hand: the method is restated from the
 * paper, parity with any other implementation is unpinned and this text is the specification.  Unless stated otherwise all
 * arithmetic is IEEE fp64, every operation rounded once in the written order, without FMA, and every sum runs in a fixed order: a
 * pair's outputs are the same bits alone, in any batch, in reversed order and on reruns.  No float atomics.
 *
 * THE MAP covers nclouds target clouds stacked in pts (f32[sum lengths_host,3], device); normals f32[.,3] is nullable.
 *   Voxel of a point: k_c = floor((double)p_c / voxel) per axis (a division; the origin is absolute, no bounding box enters it).  A
 *   point with a non-finite coordinate or any |k_c| >= 2^20 is left out of the map.
 *   key = ((kz + 2^20) << 42) | ((ky + 2^20) << 21) | (kx + 2^20).
 *   Every occupied voxel of a cloud gives one row: count N; mean = (sum of its points, in input order, each promoted to fp64) / N;
 *   cov = (sum over its points, in input order, of C(n_i)) / N, stored as six values 00 01 02 11 12 22.
 *   C(n)_rc = delta_rc - ((1 - epsilon) n_r) n_c, with (1 - epsilon) formed once; n is the point's normal row promoted to fp64
 *   under N2's rule: it counts if | ((nx nx + ny ny) + nz nz) - 1 | < 1e-3 (which a non-finite component fails), any other row and
 *   every row of a null array is taken as zero, C = I.
 *   Rows of a cloud are in ascending key order, clouds follow one another; row_off int32[nclouds + 1] (device) is each cloud's row
 *   range.  The map remembers voxel and epsilon.
 *   Lookup: a dense table of row indices over each cloud's box of occupied voxel coordinates, the clouds' tables one after the
 *   other, at most max_cells slots in all (BUF_ECAPACITY if the boxes need more: a far outlier inflates its cloud's box).  The same
 *   table is the counting sort's, so where a row lands and what a lookup returns never depend on the run.
 *   The map lives in ONE caller-allocated device buffer of buf_voxel_map_bytes(sum lengths, nclouds, max_cells) bytes (88 bytes per
 *   point and 4 per slot, rounded up); the build also takes a workspace of buf_voxel_map_ws_bytes (12 bytes per point and 4 per
 *   slot) that is free again when it returns.  buf_voxel_map_t is a host handle into that buffer: it stays valid as long as the
 *   buffer does and may serve any number of buf_vgicp_batched calls.  Building synchronises once, to read back one record of two ints
 *   (capacity status, rows).  buf_voxel_map_export writes keys int64[n], counts int32[n], means f64[n,3], covs f64[n,6] (the first
 *   map->nrows rows of each; n = their capacity) and row_off int32[nclouds + 1], all device arrays.
 *   BUF_EINVAL before any device work for voxel <= 0 or not finite, epsilon outside (0, 1] or not finite, nclouds outside 1..65535,
 *   negative lengths, max_cells outside 1..2^31-2; in export for n < map->nrows.  The two size functions answer 0 out of range.
 *
 * REGISTRATION: B pairs per call.  Sources are stacked as in N2 (src f32[sum src_lengths_host,3]); src_normals f32[.,3] is nullable
 *   (C = I).  pair_cloud_host int[B] (nullable: pair b uses cloud b) names the map cloud of each pair; several pairs may name one.
 *   neighbors is 1 (the voxel a point falls into), 7 (that voxel, then +x, -x, +y, -y, +z, -z) or 27 (all offsets, dz outermost and
 *   dx innermost, each running -1, 0, +1).
 *   Per round and source point: p = T s with N2's expression ((T0 x + T1 y) + T2 z) + T3 per row; k = floor(p / voxel); a
 *   non-finite p or a |k_c| >= 2^20 gives no term.  Every OCCUPIED voxel v among the offsets, in offset order, gives one term (there
 *   is no distance test): d = p - mean_v; S_rc = (cov_v,rc + (R R^T)_rc) - ((1 - epsilon) m_r) m_c with R the rotation block of T,
 *   (R R^T)_rc = (R_r0 R_c0 + R_r1 R_c1) + R_r2 R_c2 and m = R n_s (rows as (R_r0 n0 + R_r1 n1) + R_r2 n2), i.e. cov_v + R C(n_s) R^T;
 *   M = S^-1 by cofactors as in N2; J = [-[p]x | I]; H += N_v J^T M J, g += N_v J^T M d (each entry formed as in N2, times N_v, and
 *   added to the point's running sum; the points of a tile of 256 are summed by an xor butterfly inside each wavefront, the four
 *   wavefronts in ascending order, the tiles of a pair by lane and butterfly).
 *   Per pair and round: fitness = source points with at least one term / source points; inlier_rmse = sqrt(sum over all terms of
 *   ((dx dx + dy dy) + dz dz) / terms), 0 without terms: the Euclidean distance to VOXEL MEANS, of the order of the voxel size, not a
 *   surface residual, and comparable only at equal voxel and neighbors.
 *   Update: H x = -g by N2's Cholesky (LDL^T) solve, N2's dT, T <- dT T.  Stopping is N2's with terms in the place of matches:
 *   before an update with fewer than 6 terms or a system that is not positive definite (T unchanged); after an update when
 *   |d fitness| < rel_fitness and |d rmse| < rel_rmse; after max_iteration updates.
 *   Outputs as in buf_gicp_batched (T_out f64[B,4,4], fitness_out / rmse_out f64[B], iters_out int32[B], of the last pass); row_out
 *   (nullable) int32[sum src_lengths]: the cloud-local map row of the voxel the point fell into in the pair's last pass, or -1.  A
 *   pair with an empty source or an empty map cloud returns T_init, fitness 0 and 0 iterations.
 *   Synchronises as N2: one int read back after every 8th round.
 *   BUF_EINVAL before any device work for a null or unbuilt map, neighbors outside {1, 7, 27}, a pair_cloud entry outside the map
 *   (or, with a null pair_cloud, more pairs than map clouds), npairs outside 0..65535, negative lengths, max_iteration < 0, a null
 *   required argument; BUF_EWORKSPACE for a workspace below buf_vgicp_ws_bytes(sum src_lengths, B). */
typedef struct buf_voxel_map {
    void*   buf;                 /* the caller's device buffer */
    size_t  buf_bytes;
    int     nclouds, nrows, n;   /* clouds, rows of all clouds, points given */
    int64_t max_cells;
    double  voxel, epsilon;
    void*   clouds;              /* views into buf: per-cloud box and table offset */
    int*    table;               /* [max_cells + 1] slot -> row of all clouds, -1 = empty voxel */
    double* rows;                /* [nrows,10] mean (3), cov (6), count */
    long long* keys;             /* [nrows] */
    int*    row_off;             /* [nclouds + 1] */
} buf_voxel_map_t;
size_t  buf_voxel_map_bytes(int n_total, int nclouds, int64_t max_cells);
size_t  buf_voxel_map_ws_bytes(int n_total, int nclouds, int64_t max_cells);
int     buf_voxel_map_build(buf_voxel_map_t* map, const float* pts, const float* normals, const int* lengths_host, int nclouds,
                            double voxel, double epsilon, int64_t max_cells, void* buf, size_t buf_bytes, void* ws, size_t ws_bytes,
                            void* stream);
int     buf_voxel_map_export(const buf_voxel_map_t* map, int n, long long* keys, int* counts, double* means, double* covs,
                             int* row_off, void* stream);
size_t  buf_vgicp_ws_bytes(int n_src_total, int npairs);
int     buf_vgicp_batched(const buf_voxel_map_t* map, const float* src, const float* src_normals, const int* src_lengths_host,
                          const int* pair_cloud_host, int npairs, int neighbors, const double* T_init_f64, int max_iteration,
                          double rel_fitness, double rel_rmse, double* T_out_f64, double* fitness_out, double* rmse_out,
                          int* iters_out, int* row_out, void* ws, size_t ws_bytes, void* stream);

/* N10  Maximum-clique inlier selection + truncated-least-squares pose, the method made known by TEASER++ (Yang, Shi, Carlone, "TEASER:
 * Fast and Certifiable Point Cloud Registration", T-RO 2021): the fourth pose estimator of the classical row, for inlier ratios of a few
 * per cent, with a per-pair bound on the size of any consistent set.  No TEASER++ source or paper was at hand: this text is the
 * specification and parity with the authors' code is unpinned.  Deviations: the scale is fixed to 1; the clique comes from a
 * deterministic greedy heuristic with the k-core bound beside it, not from exact branch and bound; there is no certification stage; N8's
 * inlier refit is appended.  B pairs per call, 9 kernels after the upload of the pair table on the caller's stream, nothing read back.  Pairs, rows (p_i, q_i), DEAD rows,
 * d(a, b), e_ij and the arithmetic rules (IEEE fp64, every operation rounded once in the written order, no FMA) are N8's.
 *   Graph: the vertices are the live rows; an edge ij (i != j) iff e_ij <= d_thr; a bit matrix with a ZERO diagonal.  deg_i = the
 *   population count of row i.  Dead rows have deg = core = rank = -1.
 *   Core numbers: core_i = the largest k such that i lies in a subgraph in which every vertex has degree >= k (unique, whatever the
 *   peeling order).  bound = max core + 1 (0 without live rows): no clique of the graph has more vertices.
 *   Order: the live rows sorted by (core descending, deg descending, row ascending); rank_i = the place of row i.
 *   Greedy cliques: the seeds are the first S = min(max_seeds, live rows) rows of the order.  The walk of seed s: members = (s),
 *   candidates = row s; while candidates are left, the candidate of lowest rank becomes the next member and the candidates are ANDed
 *   with its row (rows ranked before s take part like any other).  size[r] = the walk length of the seed of rank r.  The winner has the
 *   largest size, ties to the lowest rank.  K = min(size, max_members); the members m_0 .. m_{K-1} are the first K of the winner's walk
 *   in walk order.  size < 3: NOTHING.
 *   Rotation, GNC-TLS over the translation-invariant measurements: for a < b in lexicographic order alpha = p[m_b] - p[m_a], beta =
 *   q[m_b] - q[m_a], M = K (K - 1) / 2 of them.  c2 = tim_thr tim_thr (formed once on the host).  w = 1; iteration it = 0, 1, ...:
 *   H = sum w alpha beta^T; R from H as in N8 (V diag(1, 1, det(V U^T)) U^T, the identity for H = 0 or a non-finite H); r2 =
 *   |beta - R alpha|^2 with R alpha as ((R0 ax + R1 ay) + R2 az); in iteration 0: g = 2 max(r2) / c2 - 1, g <= 0 stops with all weights
 *   1 and gnc_steps = 1, else mu = 1 / g; hi = ((mu + 1) / mu) c2, lo = (mu / (mu + 1)) c2; the new weight is 0 if r2 >= hi, 1 if
 *   r2 <= lo, else sqrt((c2 (mu (mu + 1))) / r2) - mu; the exact zeros and ones are counted; stop after this iteration if it >= 1 and
 *   zeros + ones == M and (zeros, ones) equal the previous iteration's (before iteration 0: (0, M)), or if it + 1 == gnc_iterations;
 *   mu <- mu gnc_factor.  The rotation is the R of the last iteration run, gnc_steps the number of iterations run.  H and the two
 *   counts are summed over 256 lanes (lane l takes the measurements (a, a + 1 + l + 256 k) of every a, in ascending order) and a tree.
 *   Translation, component-wise TLS voting: x_k = q[m_k] - (R p[m_k]).  Per axis with the values v_k and c = t_thr: the 2K endpoints
 *   v_k - c, v_k + c sorted ascending into e_0 .. e_{2K-1}; candidates h_j = (e_j + e_{j+1}) 0.5; the consensus set I_j = {k : |v_k -
 *   h_j| <= c} (an empty one is skipped); est_j = (sum over I_j of v_k) / |I_j| in member order; cost_j = sum over I_j of (v_k -
 *   est_j)^2 + (K - |I_j|) (c c); the component is the est_j of least cost, ties to the lowest j.
 *   Polish: N8's refinement unchanged, started from (R, t) with inlier_thr and refine_iterations.  Fewer than 3 final inliers: NOTHING.
 * Outputs (device).  T_out f64[B,4,4] src -> tgt.  info_out int32[B,8] = status (BUF_CLIQUE_*), live rows, bound, the winner's size,
 *   the winner's rank (-1 without one), K, gnc_steps, the final inlier count.  NOTHING: the identity exactly, final count 0, no inliers.
 *   Nullable: deg_out / core_out / rank_out int32[sum n]; sizes_out int32[B,max_seeds] (tail -1); members_out int32[B,max_members]
 *   (rows, tail -1); weights_out f64[B, max_members (max_members - 1) / 2] (the last weights computed, NaN tail; all NaN without a
 *   rotation); pose0_out f64[B,12] (R row-major and t before the polish; the identity and 0 without one); inliers_out uint8[sum n].
 *   Integer LDS atomics only, every float sum in a fixed order: a pair's outputs are the same bits alone, in any batch, in any batch
 *   order and on reruns.
 * BUF_EINVAL before any device work for npairs outside 0..65535, negative lengths, more than BUF_SC2_MAX_ROWS correspondences in a
 * pair, a null required argument with npairs > 0 (src / tgt / corr only where their rows are not zero), d_thr / tim_thr / t_thr /
 * inlier_thr not finite and > 0 (tim_thr and t_thr: and so their squares), max_seeds outside 1..1024, max_members outside 3..512,
 * gnc_factor not finite and > 1, gnc_iterations outside 1..1000, refine_iterations < 0, and a workspace that is null or smaller than
 * buf_clique_ws_bytes (sized from the actual lengths: 116 bytes per row, the two bit matrices, 4 max_seeds (max_members + 2) + 192
 * bytes per pair, each array rounded up to 256 bytes; 0 for arguments out of range).  npairs == 0 succeeds and touches nothing; a pair
 * with n == 0 returns the identity, NOTHING and zeros (winner's rank -1). */
#define BUF_CLIQUE_NOTHING 0
#define BUF_CLIQUE_OK      1
size_t  buf_clique_ws_bytes(const int* corr_lengths_host, int npairs, int max_seeds, int max_members);
int     buf_clique_batched(const float* src, const int* src_lengths_host, const float* tgt, const int* tgt_lengths_host,
                           const int* corr /* int32[sum corr_lengths,2]: (src row, tgt row), local to the pair's clouds */,
                           const int* corr_lengths_host, int npairs,
                           double d_thr, double tim_thr, double t_thr, double inlier_thr,          /* -, d_thr, d_thr / 2, d_thr */
                           int max_seeds, int max_members, double gnc_factor, int gnc_iterations,  /* 64, 256, 1.4, 100 */
                           int refine_iterations,                                                   /* 20 */
                           double* T_out /* f64[B,4,4] src -> tgt */, int* info_out /* int32[B,8] */,
                           int* deg_out, int* core_out, int* rank_out, int* sizes_out, int* members_out, double* weights_out,
                           double* pose0_out, unsigned char* inliers_out /* nullable */,
                           void* ws, size_t ws_bytes, void* stream);

/* N4 Pair statistics under a given transform: P pairs over C shared clouds per call (what overlap ratio, inlier RMSE and the 6x6
 * information matrix of a pair are made of; the evaluation half of an ICP round without the loop).
 * pts f32[sum lengths_host,3] stacks the C clouds; pair k = (pair_src_host[k], pair_tgt_host[k], T_f64[k]) with T_f64 f64[P,4,4]
 * (device) mapping the source cloud into the frame of the target cloud.  A cloud may appear in any number of pairs, on either side,
 * and a pair may name one cloud twice.  ONE cell grid over all C clouds is built per call (radius = the correspondence distance,
 * cells_per_elem as in buf_grid_build, <= 0 = its default; a share smaller than a cloud's box coarsens the cell edge by 1.25 until it
 * fits: same results, more candidates per row).
 * Per source row the arithmetic of buf_icp_batched's correspondence: p = T s in fp64, ((T0*sx + T1*sy) + T2*sz) + T3 per row of T,
 * rounded to fp32 for the search; nearest row of the target cloud with fp32 d2 = (dx*dx + dy*dy) + dz*dz < radius^2 (strict, radius^2
 * in fp32), ties to the smaller row; a row whose search point is not finite matches nothing.  A match adds in fp64: 1, |p - u|^2
 * with the unrounded p and the target point u, u, and the upper triangle of u u^T; u is in the target cloud's own frame.
 * matched_out int32[P]; moments_out f64[P,10] = sum d2, sum u (x, y, z), sum u u^T (xx, xy, xz, yy, yz, zz); nn_out (nullable)
 * int32[n_src_rows], pair k owning the next lengths_host[pair_src_host[k]] entries: row inside the target cloud, -1 = no match.
 * n_src_rows = the sum of the pairs' source lengths.  Sums have a fixed order and there are no float atomics: a pair's results are
 * the same bits alone, in any batch, in any pair order and across runs.  Nothing is read back.
 * BUF_EINVAL before any device work for a pair index outside [0, C), radius <= 0 or not finite, negative lengths, null outputs
 * with P > 0.  P == 0 succeeds and touches nothing; empty clouds and pairs with an empty source give zeros. */
size_t  buf_pair_stats_ws_bytes(int n_total, int nclouds, int npairs, int n_src_rows, int64_t cells_per_elem);
int     buf_pair_stats(const float* pts, const int* lengths_host, int nclouds, const int* pair_src_host, const int* pair_tgt_host,
                       int npairs, const double* T_f64, float radius, int64_t cells_per_elem, int* matched_out,
                       double* moments_out, int* nn_out /* nullable */, void* ws, size_t ws_bytes, void* stream);

/* N3  Per-stage ground-truth metrics of B registered pairs (a diagnostic beside the registration path: keypoint repeatability,
 * inlier counts of the putative and the mutual matches, the consensus set of the returned pose).  One launch, nothing read back.
 * kp f32[2*B*P,3]: the keypoints in the batched pipeline's layout, pair b owns rows [2bP, 2bP+P) (source) and [(2b+1)P, (2b+2)P)
 * (target); s_nn / t_nn int32[B,P]: descriptor-space 1-NN of every source keypoint among the pair's target keypoints and the
 * reverse (rows of the pair's own cloud, 0..P-1; an index outside that range matches nothing); T_gt_f64 f64[B,4,4] ground truth
 * src -> tgt; T_est_f32 f32[B,4,4] the returned pose (widened to fp64 exactly).
 * Arithmetic (a numpy restatement gives the same bits, the convention of buf_icp_batched):
 *   p = T s in fp64 without FMA, ((r0*x + r1*y) + r2*z) + t per row, rounded to fp32;
 *   d2 = (dx*dx + dy*dy) + dz*dz in fp32; a point is within tau when d2 < (float)tau * (float)tau (strict);
 *   the inverse of T_gt is formed on the device in fp64 as [R^T, -R^T t] with tinv_i = -((R0i*t0 + R1i*t1) + R2i*t2), and applied
 *   in the same operation order; non-finite points are within nothing (their d2 is NaN or inf and fails every comparison);
 *   the nearest keypoint is the running minimum over ascending rows with a strict <, so the lowest row keeps a tie.
 * out_counts int32[B, BUF_METRICS_NCOUNT], per pair:
 *   REP_SRC     source keypoints whose nearest target keypoint under T_gt is within tau_kp
 *   REP_TGT     target keypoints whose nearest source keypoint under the inverse of T_gt is within tau_kp
 *   NN_INL      source keypoints s with |T_gt kp_s - kp_tgt[s_nn[s]]| within tau_match (putative = 1-NN, no mutual check: the count
 *               behind Feature Matching Recall)
 *   MUTUAL      mutual matches, t_nn[s_nn[s]] == s
 *   MUTUAL_INL  mutual matches within tau_match under T_gt
 *   CONS        mutual matches within dist_th under T_est (the consensus set of the returned pose)
 *   CONS_TRUE   of those, the ones also within tau_match under T_gt
 * out_nn_d2 (nullable) f32[2*B*P]: the fp32 d2 from every keypoint (kp's row order) to its nearest keypoint of the pair's other
 * cloud under the ground truth; +inf where there is none (non-finite points).
 * Integer atomics only: results are bitwise reproducible and independent of the other pairs of the batch.
 * BUF_EINVAL before any device work for npairs < 0 or P < 0, a threshold that is not finite and > 0, and a null required pointer
 * with npairs * P > 0; npairs == 0 or P == 0 succeeds and touches nothing. */
#define BUF_METRICS_NCOUNT     7
#define BUF_METRICS_REP_SRC    0
#define BUF_METRICS_REP_TGT    1
#define BUF_METRICS_NN_INL     2
#define BUF_METRICS_MUTUAL     3
#define BUF_METRICS_MUTUAL_INL 4
#define BUF_METRICS_CONS       5
#define BUF_METRICS_CONS_TRUE  6
int     buf_match_metrics(const float* kp, const int* s_nn, const int* t_nn, int npairs, int P, const double* T_gt_f64,
                          const float* T_est_f32, float tau_kp, float tau_match, float dist_th, int* out_counts,
                          float* out_nn_d2 /* nullable */, void* stream);

/* N5  Pose-graph optimisation with line processes (the multiway registration of Choi, Zhou, Koltun 2015, restated here in full: no
 * library's conventions are pinned), G graphs per call, ONE launch, nothing read back, all arithmetic fp64 without FMA.
 * Graph g owns nodes_host[g] consecutive rows of X_init_f64 / X_out_f64 (f64[N_total,4,4], device) and edges_host[g] consecutive
 * edges: edge_i_host / edge_j_host (graph-local node ids), Z_f64 f64[E,4,4] and info_f64 f64[E,6,6] (device), uncertain_host u8[E];
 * fixed_host[g] = the node that keeps its pose, mu_host[g] = the line-process weight (0 = line process off).  X_out must not
 * overlap X_init.
 * Model.  Node pose X_k = (R_k, p_k) maps fragment k into the world.  Edge e = (i, j, Z, L, u): Z maps fragment j into fragment i (the
 *   gt.log convention, T_ij = inv(W_i) W_j).  E = Z^-1 X_i^-1 X_j, rigid inverses formed as [R^T, -R^T t]; residual r = [phi; tau],
 *   phi = Log(R_E), tau = t_E.  Log goes through the quaternion of R_E (Shepperd's branch on the largest of w, x, y, z; w made >= 0)
 *   and phi = 2 atan2(|v|, w) v / |v| (2 v where |v| = 0): a few ulp on all of [0, pi].  L is the symmetric 6x6 information matrix in the
 *   order [rotation, translation] (the 'open3d' convention of pairs.information_matrix over the matched points of fragment j in j's
 *   frame); q = r^T L r.
 * Line process.  An uncertain edge of a graph with mu > 0 has l = (mu / (mu + q))^2 and the cost term mu q / (mu + q)
 *   (= l q + mu (sqrt(l) - 1)^2); every other edge has l = 1 and the cost term q.  F = the sum of the cost terms.
 * Jacobians, for the update X_k <- X_k (Exp(a_k), b_k), i.e. R <- R Exp(a), p <- p + R b; Exp(a) = I + (sin t / t) [a]x +
 *   ((sin(t/2) / (t/2))^2 / 2) [a]x^2, t = |a|.  With M = X_j^-1 X_i = (R_M, p_M), P = [phi]x and Jri = I + P/2 + P^2/12 (the series
 *   is cut there: part of the contract):
 *     J_i = [[-Jri R_M, 0], [-R_E [p_M]x R_M, -R_E R_M]]        J_j = [[Jri, 0], [0, R_E]]
 * Normal equations.  H = sum l_e J^T L J, g = sum l_e J^T L r with l_e frozen at the linearisation point (IRLS); the six rows and
 *   columns of the fixed node are removed.
 * Loop (Levenberg-Marquardt, Nielsen's damping).  lambda0 = tau0 * max diag H; a graph without a free node, without an edge or with
 *   lambda0 not > 0 returns X_init with status NOTHING.  lambda = lambda0, nu = 2.  Every solve factors H + lambda I by Cholesky and
 *   sets delta = -(H + lambda I)^-1 g; a pivot that is not positive and finite makes the solve a rejected one.  max |delta| <=
 *   eps_step stops with CONVERGED_STEP, delta not applied.  Otherwise X' = X (Exp(a), b) per free node, F' = the cost at X' and
 *   rho = (F - F') / (delta^T (lambda delta - g)).  Accepted when rho > 0 and F' is finite: X <- X', lambda <- lambda * max(1/3,
 *   1 - (2 rho - 1)^3), nu <- 2, and F - F' <= eps_cost * F (the F before the step) stops with CONVERGED_COST.  Otherwise rejected:
 *   lambda <- lambda nu, nu <- 2 nu, and lambda > 1e30 * lambda0 stops with STALLED.  max_iterations counts solves; using them up
 *   gives MAX_ITER (max_iterations == 0: the costs and the edge outputs at X_init).  A graph with a non-finite value in its Z, info
 *   or X_init returns X_init with status FAILED, NaN costs and NaN edge outputs, and does not disturb the other graphs of the call.
 * Outputs (device).  X_out f64[N_total,4,4]; status_out int32[G,3] = status (BUF_PG_*), solves, accepted steps; cost_out f64[G,2] =
 *   F at X_init, F at X_out; edge_out f64[E,2] = (l_e, q_e) at X_out.
 * Shape on the device.  One workgroup per graph runs the whole loop.  Its threads linearise one edge each into a per-edge record;
 *   every node row of H and g is then gathered over the node's incident edges in ascending edge order; H is a dense square of
 *   6 (n - 1) in the workspace, factored by a blocked Cholesky with an LDS panel; every sum is a fixed-shape tree.  No float atomics:
 *   a graph's results are the same bits alone, in any batch, in any graph order and across runs.  At most BUF_PG_MAX_NODES nodes per
 *   graph: more gives BUF_ECAPACITY before any device work.
 * BUF_EINVAL before any device work for negative counts, an edge index outside its graph, i == j, fixed outside its graph, mu < 0
 * or not finite, eps_step / eps_cost / tau0 not finite and > 0, max_iterations < 0, and a null required pointer with work to do.
 * ngraphs == 0 succeeds and touches nothing.  buf_pose_graph_ws_bytes: max_nodes = the largest graph of the call (0 bytes for a
 * negative count, ngraphs == 0 or max_nodes above the capacity). */
#define BUF_PG_MAX_NODES        128
#define BUF_PG_NOTHING          0
#define BUF_PG_CONVERGED_STEP   1
#define BUF_PG_CONVERGED_COST   2
#define BUF_PG_MAX_ITER         3
#define BUF_PG_STALLED          4
#define BUF_PG_FAILED           5
size_t  buf_pose_graph_ws_bytes(int ngraphs, int nodes_total, int edges_total, int max_nodes);
int     buf_pose_graph_optimize(const int* nodes_host, const int* edges_host, int ngraphs, const int* edge_i_host,
                                const int* edge_j_host, const double* Z_f64, const double* info_f64,
                                const unsigned char* uncertain_host, const int* fixed_host, const double* mu_host,
                                const double* X_init_f64, int max_iterations, double eps_step, double eps_cost, double tau0,
                                double* X_out_f64, int* status_out, double* cost_out, double* edge_out, void* ws, size_t ws_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BUFFER_HIP_H */
