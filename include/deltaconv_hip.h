/* deltaconv_hip.h -- C ABI of libdeltaconv_hip.so (MI355X / gfx950).
 *
 * The reference (rubenwiersma/deltaconv) has no FFI boundary on its hot path: it is Python over
 * third-party torch extensions (torch_cluster / torch_sparse / torch_scatter) and ATen.  The entry
 * points below are what a binding for that path binds INSTEAD of those packages; each one cites
 * the reference call site(s) it replaces (paths relative to /root/reference).  INTEGRATION.md
 * shows the ctypes stub and the reference-side edits.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP), fp32 / int32 / uint8 as typed; no torch types.
 *   - `stream` is a hipStream_t (NULL = default stream); all work is enqueued, nothing syncs,
 *     nothing allocates (callers pass workspaces) -> every entry point is hipGraph-capturable.
 *   - return 0 on success, <0 on error (DC_ERR_*); dc_last_error() gives the message.
 *   - layouts: nbr[Nt,k] centre-major (edge e = i*k+s); G,D [Nt,k,2]; scalar fields [Nt, ld];
 *     vector fields [2Nt, ld] with row 2i = u-, row 2i+1 = v-component
 *     (deltaconv/geometry/operators.py:4-21); `ld*` = row stride in floats (>= row length), so
 *     outputs can land directly in a column block of a wider concat buffer.
 *   - clouds of a batch are contiguous; cloud_ptr[B+1] int32 offsets (sorted `batch` vector of
 *     deltaconv/models/deltanet_base.py:44).
 */
#ifndef DELTACONV_HIP_H
#define DELTACONV_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DC_OK 0
#define DC_ERR_ARG (-1)
#define DC_ERR_LAUNCH (-2)
#define DC_ERR_WORKSPACE (-3)
#define DC_FPS_MAX_POINTS (16384) /* points per cloud dc_geodesic_fps_batch takes: 8 bytes of LDS per point in one workgroup */
#define DC_FPS_LARGE_MAX_POINTS (262144) /* points per cloud dc_geodesic_fps_large takes: two bit sets of n / 8 bytes of LDS */
#define DC_FPS_EUCLID_MAX_POINTS (16384) /* points per cloud dc_fps_batch takes: 16 points per thread of a 1024-thread workgroup, in registers */
#define DC_FPS_GRID_MAX_POINTS (262144) /* points per cloud dc_fps_grid takes: one key per 64 of its at most 2 n cells in the LDS of one workgroup (64 KiB) */

int32_t dc_version(void);
const char* dc_last_error(void);
/* Experiment switches for A/B measurements (product defaults: all 0 except key 0).  key 0: XCD-aware block remap
 * (default 1); 1: edge-at-a-time max-aggregation backward; 2: value 2 = weight gradients through the round-1
 * direct-load kernel; 3: value 1 = dense products through the exact fp32 MFMA chain (bitwise an fmaf chain) instead of
 * the bf16 split products (three bf16 planes per fp32 operand, six partial products, fp32 accumulation: error against
 * fp64 no larger than the chain's); 4: first-round phase shift of every second 128 x 128 GEMM workgroup of a CU in
 * percent of a K loop (0 = default 50, negative = off); 5 / 6: force the weight-gradient tile (1..4) / slab count;
 * 7: units (tile x 64-channel slab) per workgroup of the persistent two-piece tiled applies (0 = launcher's choice);
 * 8: value 1 = CSC count / scan / fill by one workgroup per cloud (round 3) instead of eight column ranges per cloud;
 * 9: value 1 = ignore pre-split weight planes (every product splits its weight operand in the K loop, as in round 3);
 * 10: value 1 = cross-entropy of <= 64 rows through the two-launch form (same bits as the one-launch form);
 * 11: value 1 = dense products with fewer than 256 workgroups keep 128-column tiles (round-6 rule off);
 * 12: weight gradients on whole tiles: 0 = the plane-image kernel (operands cut into bf16 planes once, at the LDS store) on the
 * launches it runs faster (128-row tiles, more than one workgroup per CU), 1 = the fp32-tile kernel everywhere (fallback, A/B partner), 2 = the plane-image kernel on every
 * whole tile (lab);
 * 13: plain dense products over pre-split weight planes (forward, input gradient, the statistics epilogues, the paired launch):
 * 0 = the fp32 activation tiles reach LDS by 16-byte LDS-DMA into a ring of three buffers, 1 = through staging registers and
 * ds_write_b128 into two padded buffers (the earlier loop: fallback, A/B partner).  Same floats into the same MFMAs: same bits;
 * 14: the two gradient products of a block through dc_linear_backward_both / dc_linear_bn_backward_both: 0 = ONE launch for the
 * pairs of kernel instantiations in the library's table, 1 = always the two launches of the separate calls (fallback, A/B partner).
 * Same workgroups on the same data: same bits. */
int dc_set_option(int32_t key, int32_t value);

/* Deferred finalisers (round 6): a column reduction is two launches (partials, finaliser).  Between dc_finalisers_begin() and
 * dc_finalisers_end() a call of dc_linear_bn_stats_forward / dc_bn_act_backward_reduce announced by dc_finaliser_defer_next()
 * (one-shot, per call) queues its finaliser instead of launching it; dc_finalisers_end launches ONE kernel for all of them (at
 * most 4; discard != 0: drops them).  The independent products of a DeltaConv layer (max-aggregation stream and s_mlp,
 * deltaconv/nn/deltaconv.py:50-59) share a finaliser launch this way -- same sums, same bits.  The coefficient outputs of the
 * queued calls are valid behind dc_finalisers_end; their workspaces must stay alive until then.  Thread-local host state. */
int dc_finalisers_begin(void);
int dc_finaliser_defer_next(void);
/* with it: the dense product of the announced dc_linear_bn_stats_forward call (weight planes, whole tiles) waits as well; two
 * queued products of one kernel instantiation run as ONE launch at dc_finalisers_end (same arithmetic per element: same bits) */
int dc_gemm_defer_next(void);
int dc_finalisers_end(int32_t discard, void* stream);

/* Measurement aid (bench.py `roofline.frac`): device-clock stamps of the tiled two-piece forward applies and the tiled transposed applies.  After
 * dc_stamp_buffer(buf, slots) every launch of that family takes the next 4 x uint64 record of `buf` AT ENQUEUE TIME (a launch
 * captured into a HIP graph keeps its record across replays): [0] earliest workgroup entry, [1] latest workgroup exit with
 * its stores complete, constant 100 MHz clock; the caller sets [0] = huge, [1] = 0 before a replay.  dc_stamp_tag(record) =
 * 1000 * kind + channels (forward: kind 1 = div|curl|norm, 2 = hodge, 3 = div; transposed: 11 = div|curl|norm^T, 12 = hodge^T,
 * 13 = grad^T (+ sum), 14 = max-aggregation backward, 15 = div^T, 16 = layer-0 edge MLP backward).  buf = NULL disarms (the product default). */
int dc_stamp_buffer(uint64_t* buf, int32_t slots);
int32_t dc_stamp_count(void);
int32_t dc_stamp_tag(int32_t record);

/* ---- graph ------------------------------------------------------------------------------- */
/* knn_graph(pos, k, batch, loop=True, flow='target_to_source')  (torch_cluster via
 * torch_geometric) -- deltaconv/models/deltanet_base.py:52,63.
 * Order: fp32 ((dx*dx+dy*dy)+dz*dz) ascending, ties by lower index, self included; global ids.
 * Every cloud needs >= k points; k <= 64.  lanes_per_query: 0 = auto, 64 = wave-per-query selection
 * kernel (clouds <= 4096 points), 1 or 8 = sorted-insertion kernel. */
int dc_knn(const float* pos, const int32_t* cloud_ptr, int32_t num_clouds, int32_t max_cloud_size, int32_t k,
           int32_t lanes_per_query, int32_t* nbr, void* stream);

/* ---- exact kNN over a uniform cell grid, for large clouds (csrc/knn_grid.hip, csrc/knn_grid_math.h) ------------------------ */
/* The workspace of one dc_knn_grid / dc_knn_cross_grid call: linear in the sizes, a function of the sizes alone.
 *   num_points  HOST: the REFERENCE rows of the call (dc_knn_grid: all points, cloud_ptr[num_clouds] - cloud_ptr[0];
 *               dc_knn_cross_grid: rptr[B] - rptr[0]);  num_clouds  HOST: the clouds / cloud pairs of the call
 * -> bytes: one 48-byte grid record per cloud, 2 * num_points + num_clouds per-cell counters and as many cell starts (+ the scan's
 * block sums), and the points in cell order, 16 bytes each -- about 48 bytes a point.  0: a negative size or more than 2^31 - 1 points. */
size_t dc_knn_grid_workspace_bytes(int64_t num_points, int32_t num_clouds);
/* dc_knn through a uniform cell grid per cloud: the arguments and the OUTPUT of dc_knn, bit for bit -- fp32
 * ((dx*dx+dy*dy)+dz*dz) without contraction, ascending, ties by lower index, self included, global ids; every cloud needs >= k
 * points; k <= 64.  Opt-in: worth it where the n^2 distances of dc_knn dominate (README: measured), never picked by size here.
 *   pos, cloud_ptr, num_clouds (<= 65 535), max_cloud_size, k, nbr   as in dc_knn
 *   target      HOST: the wanted mean number of points per cell (csrc/knn_grid_math.h: make_grid; DEFAULT_TARGET = 1); any positive
 *               finite value gives the same output -- 1e9 one cell per cloud (a brute-force search on one thread per query), 0.25
 *               the cap of 2 n cells
 *   workspace   DEVICE, 16-byte aligned, workspace_bytes >= dc_knn_grid_workspace_bytes(all points of the call, num_clouds)
 * The grid rule, the ring walk and the proof of the stopping bound: csrc/knn_grid_math.h.  Positions with a non-finite coordinate:
 * dc_knn's output is meaningless there and this one need not equal it, but it reads and writes in bounds and emits only ids inside
 * the row's cloud: such a point is never picked, its own row names itself k times, and a slot that no finite point can fill names
 * the query.  A null pointer, k outside 1 .. 64, num_clouds above 65 535, target not positive and finite, a workspace that is
 * missing, misaligned or smaller than that of max_cloud_size points: DC_ERR_ARG with a message, checked before anything touches the
 * device (a workspace smaller than the device-side offsets demand leaves the rows of the clouds past it unwritten).  Seven
 * launches whose sizes depend on the HOST arguments only, stream-ordered, no allocation, no synchronisation, capturable and
 * replayable on new positions written in place; integer atomics on counters, and the outputs are a function of the inputs only. */
int dc_knn_grid(const float* pos, const int32_t* cloud_ptr, int32_t num_clouds, int32_t max_cloud_size, int32_t k, float target,
                int32_t* nbr, void* workspace, size_t workspace_bytes, void* stream);
/* dc_knn_cross through a uniform cell grid per REFERENCE cloud: the arguments, limits and OUTPUT of dc_knn_cross (declared with
 * the propagation stage below), bit for bit in idx and in d2 -- reference ids LOCAL to the pair's reference cloud, ascending d2,
 * ties by lower id, -1 / +inf where fewer than k reference points can be picked; k <= 16, B <= 65 535.  A reference point with a
 * non-finite coordinate belongs to no cell and is never picked; a query with one gets -1 / +inf in every slot; a query outside the
 * box of its reference cloud is searched from the border cell.  The queries are taken as they come (not sorted by cell).
 *   target, workspace   as in dc_knn_grid, workspace_bytes >= dc_knn_grid_workspace_bytes(rptr[B] - rptr[0], B): the capacity
 *               in reference rows is read back from workspace_bytes, and it sizes the build's launches
 * Argument errors as dc_knn_cross, plus target and the workspace as above: DC_ERR_ARG with a message.  B = 0 or
 * max_query_cloud = 0 returns DC_OK.  Seven launches, stream-ordered, capturable, no allocation, no synchronisation. */
int dc_knn_cross_grid(const float* query, const int64_t* qptr, const float* ref, const int64_t* rptr, int32_t B,
                      int64_t max_query_cloud, int32_t k, float target, int32_t* idx, float* d2, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Transposed adjacency of nbr (in-edges per point, ascending edge id).  Stands in for the A^T
 * products torch_sparse autograd performs and torch_scatter's arg-indexed backward. */
size_t dc_csc_workspace_bytes(int32_t num_points);   /* upper bound for any k <= 255; 4*Nt*(k+1) suffices */
int dc_csc_build(const int32_t* nbr, const int32_t* cloud_ptr, int32_t num_clouds, int32_t num_points, int32_t k,
                 int32_t* tptr /*[Nt+1]*/, int32_t* tedge /*[Nt*k]*/, void* workspace, size_t workspace_bytes,
                 void* stream);

/* Same result (identical tptr / tedge) for clouds of at most 4096 points: count, scan and fill of a cloud run in one
 * workgroup on LDS counters (2 launches instead of 5).  workspace: num_points * k int32. */
int dc_csc_build_clouds(const int32_t* nbr, const int32_t* cloud_ptr, int32_t num_clouds, int32_t num_points,
                        int32_t max_cloud, int32_t k, int32_t* tptr, int32_t* tedge, void* workspace,
                        size_t workspace_bytes, void* stream);

/* coefT[t] = coef[tedge[t]]: G or D in CSC order for the transposed applies (once per batch). */
int dc_csc_permute_coef(const float* coef, const int32_t* tedge, int64_t num_edges, float* coefT, void* stream);

/* ---- tangent frames ------------------------------------------------------------------------ */
/* build_tangent_basis -- deltaconv/geometry/grad_div_mls.py:50-69 */
int dc_tangent_basis(const float* normal, int32_t n, float* x_basis, float* y_basis, void* stream);
/* estimate_basis -- deltaconv/geometry/grad_div_mls.py:10-47 (orientation may be NULL).
 * x_basis sign convention: largest-|component| positive (LAPACK's sign is arbitrary). */
int dc_estimate_basis(const float* pos, const int32_t* nbr, int32_t n, int32_t k, const float* orientation,
                      float* normal, float* x_basis, float* y_basis, void* stream);

/* ---- operator assembly ---------------------------------------------------------------------- */
/* build_grad_div (+ coords_projected, gaussian_weights, weighted_least_squares,
 * fit_vector_mapping) -- deltaconv/geometry/grad_div_mls.py:72-277.  Outputs the gradient and
 * divergence operators as G[Nt,k,2], D[Nt,k,2] over nbr (never COO/CSR). */
size_t dc_mls_workspace_bytes(int32_t num_clouds, int32_t num_points);
int dc_mls_assemble(const float* pos, const float* normal, const float* x_basis, const float* y_basis,
                    const int32_t* nbr, const int32_t* cloud_ptr, int32_t num_clouds, int32_t num_points,
                    int32_t max_cloud_size, int32_t k, float kernel_width, float regularizer, int32_t normalized,
                    float* G, float* D, void* workspace, size_t workspace_bytes, void* stream);
/* build_tangent_basis + build_grad_div in one call -- the model's path when normals are given (deltanet_base.py:59-61,69):
 * x_basis / y_basis [Nt,3] are OUTPUTS (written by the assembly's first launch); same values as dc_tangent_basis followed
 * by dc_mls_assemble, two launches fewer. */
int dc_mls_assemble_normals(const float* pos, const float* normal, const int32_t* nbr, const int32_t* cloud_ptr,
                            int32_t num_clouds, int32_t num_points, int32_t max_cloud_size, int32_t k, float kernel_width,
                            float regularizer, int32_t normalized, float* x_basis, float* y_basis, float* G, float* D,
                            void* workspace, size_t workspace_bytes, void* stream);
/* build_grad_div(..., shape_regularizer=s) -- grad_div_mls.py:241-244,266-267 (weighted_least_squares :146-150): the
 * gradient rows come from the fit regularised by `regularizer`, the surface coefficients behind the divergence rows
 * (fit_vector_mapping) from a second fit regularised by `shape_regularizer`. */
int dc_mls_assemble_shape(const float* pos, const float* normal, const float* x_basis, const float* y_basis,
                          const int32_t* nbr, const int32_t* cloud_ptr, int32_t num_clouds, int32_t num_points,
                          int32_t max_cloud_size, int32_t k, float kernel_width, float regularizer,
                          float shape_regularizer, int32_t normalized, float* G, float* D, void* workspace,
                          size_t workspace_bytes, void* stream);

/* The stages of build_grad_div on their own: the reference exports and tests them one by one
 * (deltaconv/geometry/__init__.py:3; test/geometry/test_grad_div_mls.py:58-275).  Same device functions as the
 * fused kernels behind dc_mls_assemble (csrc/point_math.h); fp32 in / fp32 out, fp64 inside.
 * Edges are centre-major in groups of k (edge e belongs to group e / k), as everywhere in the reference
 * (grad_div_mls.py:24-25,85,224). */
/* coords_projected -- grad_div_mls.py:72-97: coords[E,2] = ((p_col - p_row) minus its normal part) . (x, y) of frame e / k */
int dc_mls_coords(const float* pos, const float* normal, const float* x_basis, const float* y_basis,
                  const int32_t* row, const int32_t* col, int64_t num_edges, int32_t k, float* coords, void* stream);
/* gaussian_weights -- grad_div_mls.py:100-116: dist[Nt*k] -> weights[Nt*k]; cloud_ptr[num_clouds+1] delimits the
 * clouds whose mean edge length scales the kernel (batch=None: one cloud); workspace >= 128 * num_clouds bytes
 * (16 ordered fp64 partial sums per cloud) */
int dc_mls_gaussian_weights(const float* dist, const int32_t* cloud_ptr, int32_t num_clouds, int32_t max_cloud_size,
                            int32_t k, float kernel_width, float* weights, void* workspace, size_t workspace_bytes,
                            void* stream);
/* weighted_least_squares -- grad_div_mls.py:119-152: coords[Nt*k,2], weights[Nt*k] -> wls[Nt*k,6] =
 * ((B^T W B + regularizer I)^-1 B^T W)^T per point (the shape_regularizer variant is a second call) */
int dc_mls_wls(const float* coords, const float* weights, int32_t num_points, int32_t k, float regularizer, float* wls,
               void* stream);
/* fit_vector_mapping -- grad_div_mls.py:155-194: mapping[E,2,2] = g^-1 T per edge; row must be constant inside a
 * group of k edges (the scatter_add over row, :165, is the sum over the group in slot order) */
int dc_mls_vector_mapping(const float* pos, const float* normal, const float* x_basis, const float* y_basis,
                          const int32_t* row, const int32_t* col, int64_t num_edges, int32_t k, const float* wls,
                          const float* coords, float* mapping, void* stream);

/* ---- operator applies (SparseTensor @ dense: deltanet_base.py:78; deltaconv.py:57,66;
 *      operators.py:27,33,40,43) -------------------------------------------------------------
 * k: the forward entry points below and dc_knn_max / _max_affine / _max_affine_residual / _sum stage (points per block + 1) * k * 12 + 16
 * bytes of LDS, which must fit 64 KiB: with g = C / V channel groups (V = 4, 2 or 1 floats per access, from C, the leading dimensions and
 * the base pointers) a block holds 64 points for g <= 4, else ceil(256 / g).  k <= 84 works at every C, g = 5 up to k = 103, g = 8 up to
 * k = 165, g >= 16 up to k = 255; beyond that the call returns DC_ERR_LAUNCH.  The transposed forms take every k <= 255 at every C. */
/* out[2Nt,C] = grad @ x[Nt,C] */
int dc_apply_grad(const float* G, const int32_t* nbr, int32_t n, int32_t k, const float* x, int32_t C, int64_t ldx,
                  float* out, int64_t ldo, void* stream);
/* out[Nt,C] = div @ v[2Nt,C] */
int dc_apply_div(const float* D, const int32_t* nbr, int32_t n, int32_t k, const float* v, int32_t C, int64_t ldv,
                 float* out, int64_t ldo, void* stream);
/* out[Nt,3C] = [div v | curl v | norm v]  (deltaconv.py:57 + operators.py:4-7,23-27), v read once */
int dc_apply_div_curl_norm(const float* D, const int32_t* nbr, int32_t n, int32_t k, const float* v, int32_t C,
                           int64_t ldv, float* out, int64_t ldo, void* stream);
/* out[2Nt,C] = hodge_laplacian(v) given dc[Nt,2C] = [div v | curl v]  (operators.py:35-46) */
int dc_apply_hodge(const float* G, const int32_t* nbr, int32_t n, int32_t k, const float* dc, int32_t C, int64_t lddc,
                   float* out, int64_t ldo, void* stream);

/* Transposed forms = backward of the four applies (operators carry no gradient).  The coefficient
 * argument is the operator in CSC order (dc_csc_permute_coef).  accumulate != 0 adds into the
 * destination (gradient accumulation without a separate add). */
int dc_apply_grad_T(const float* GT, const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k, const float* dy,
                    int32_t C, int64_t ldy, float* dx, int64_t ldx, int32_t accumulate, void* stream);
/* out[n, C] = a (+ b when non-null) + grad^T dy: dc_apply_grad_T with the accumulation of the other gradients of x'
 * (autograd's adds for a tensor with several consumers: the next layer and the concatenated embedding input,
 * deltanet_base.py:82-87, deltanet_classification.py:42) folded into the store; `out` is a fresh tensor. */
int dc_apply_grad_T_sum(const float* GT, const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k,
                        const float* dy, int32_t C, int64_t ldy, const float* a, int64_t lda, const float* b,
                        int64_t ldb, float* out, int64_t ldo, void* stream);
int dc_apply_div_T(const float* DT, const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k, const float* dy,
                   int32_t C, int64_t ldy, float* dv, int64_t ldv, int32_t accumulate, void* stream);
int dc_apply_hodge_T(const float* GT, const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k, const float* dh,
                     int32_t C, int64_t ldh, float* ddc, int64_t lddc, int32_t accumulate, void* stream);
int dc_apply_div_curl_norm_T(const float* DT, const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k,
                             const float* dout, int32_t C, int64_t ldo, const float* v, int64_t ldv, float* dv,
                             int64_t lddv, int32_t accumulate, void* stream);

/* ---- forward applies / max aggregation from a TILE PLAN --------------------------------------------------------
 * Same operations as dc_apply_{grad,div,div_curl_norm,hodge} / dc_knn_max[_affine] (same reference call sites:
 * deltanet_base.py:78; nn/deltaconv.py:52-57,66; geometry/operators.py:27-43), results identical bit for bit; the
 * neighbour rows come from LDS instead of the gather path.  The plan groups the points of every cloud into tiles of
 * P (32 or 64) points that are consecutive on a Morton curve through the positions and lists the unique neighbour
 * rows of each tile (layout: deltaconv_amd/csrc/tile_plan.h); it depends on positions + graph only and is built once
 * per batch, like the CSC.  The reference has no counterpart (torch_sparse / torch_scatter gather from global memory).
 * Restrictions: clouds of at most dc_tile_plan_max_cloud() points, k even, k <= 64, P * k <= 2048; the apply entry
 * points need C % 64 == 0 and 16-byte aligned rows and return DC_ERR_ARG otherwise (use the plain entry points).
 * The operator argument is the same G / D as for the plain entry points.  Occupied tile ids are a dense prefix of
 * [0, num_tiles): cloud b owns sum_{c<b} ceil(N_c / P) + [0, ceil(N_b / P)); for equal-sized clouds num_tiles is exact. */
int32_t dc_tile_plan_tiles(int32_t num_points, int32_t num_clouds, int32_t max_cloud, int32_t P);   /* number of tile ids T: the `num_tiles` of every call below */
size_t dc_tile_plan_words(int32_t num_tiles, int32_t k, int32_t P);   /* plan size in int32 words */
int32_t dc_tile_plan_max_cloud(void);
int dc_tile_plan_build(const float* pos, const int32_t* nbr, const int32_t* cloud_ptr, int32_t num_clouds,
                       int32_t num_points, int32_t max_cloud, int32_t k, int32_t P, int32_t* plan, void* stream);
int dc_apply_grad_tiled(const float* G, const int32_t* plan, const int32_t* nbr, int32_t n, int32_t num_tiles,
                        int32_t k, int32_t P, const float* x, int32_t C, int64_t ldx, float* out, int64_t ldo,
                        void* stream);
int dc_apply_div_tiled(const float* D, const int32_t* plan, const int32_t* nbr, int32_t n, int32_t num_tiles,
                       int32_t k, int32_t P, const float* v, int32_t C, int64_t ldv, float* out, int64_t ldo,
                       void* stream);
int dc_apply_div_curl_norm_tiled(const float* D, const int32_t* plan, const int32_t* nbr, int32_t n,
                                 int32_t num_tiles, int32_t k, int32_t P, const float* v, int32_t C, int64_t ldv,
                                 float* out, int64_t ldo, void* stream);
int dc_apply_hodge_tiled(const float* G, const int32_t* plan, const int32_t* nbr, int32_t n, int32_t num_tiles,
                         int32_t k, int32_t P, const float* dc, int32_t C, int64_t lddc, float* out, int64_t ldo,
                         void* stream);
int dc_knn_max_tiled(const int32_t* plan, const int32_t* nbr, int32_t n, int32_t num_tiles, int32_t k, int32_t P,
                     const float* h, int32_t C, int64_t ldh, float* out, int64_t ldo, uint8_t* arg, void* stream);
int dc_knn_max_affine_tiled(const int32_t* plan, const int32_t* nbr, int32_t n, int32_t num_tiles, int32_t k,
                            int32_t P, const float* h, int32_t C, int64_t ldh, const float* scale, const float* shift,
                            float slope, float* out, int64_t ldo, uint8_t* arg, void* stream);
/* The same with the layer's last s_mlp block in its epilogue (round 6): out = act2(scale2 h2 + shift2) + max_j act(scale h_j + shift)
 * = `x = self.s_mlp(x) + x_max` of deltaconv/nn/deltaconv.py:54-59 with both BatchNorm + LeakyReLU pairs folded in; out2 (may be
 * NULL, row stride ldo2) receives a second copy (the layer's block of the heads' torch.cat buffer).  Same bits as
 * dc_knn_max_affine_tiled followed by dc_bn_act2 with the maximum as residual. */
int dc_knn_max_affine_residual_tiled(const int32_t* plan, const int32_t* nbr, int32_t n, int32_t num_tiles, int32_t k,
                                     int32_t P, const float* h, int32_t C, int64_t ldh, const float* scale,
                                     const float* shift, float slope, const float* h2, int64_t ldh2, const float* scale2,
                                     const float* shift2, float slope2, float* out, int64_t ldo, float* out2, int64_t ldo2,
                                     uint8_t* arg, void* stream);

/* ---- transposed applies / max-aggregation backward from the TRANSPOSED TILE PLAN (round 4) -----------------------
 * Same operations as dc_apply_{grad,grad_T_sum,div,hodge,div_curl_norm}_T and dc_knn_max_backward, i.e. the backward of
 * the reference's `SparseTensor @ dense` (torch_sparse autograd spmm with A^T: nn/deltaconv.py:57,66,
 * geometry/operators.py:27,33,40,43) and of torch_scatter.scatter(reduce='max') (nn/deltaconv.py:52,54); results
 * identical bit for bit (same sums, ascending edge id per target, no floating-point atomics).  The plan keeps the tiles
 * of the forward plan, orders the targets of a tile by in-degree (the four targets of a wavefront finish together),
 * lists the unique SOURCE rows of the tile (staged in LDS by LDS-DMA) and stores the tile's in-edge lists contiguously
 * (layout: deltaconv_amd/csrc/tile_plan.h, second half).  It is built once per batch from the forward plan + the CSC.
 * Operator argument: the coefficients in TILE order (dc_tile_plan_T_permute_coef: [dc_tile_plan_T_edges(...), 2] floats).  Same restrictions as the forward tiled entry points (C % 64 == 0, 16-byte rows). */
size_t dc_tile_plan_T_words(int32_t num_points, int32_t num_clouds, int32_t num_tiles, int32_t k, int32_t P);
int64_t dc_tile_plan_T_edges(int32_t num_points, int32_t num_clouds, int32_t num_tiles, int32_t k);
int64_t dc_tile_plan_T_edge_offset(int32_t num_points, int32_t num_clouds, int32_t num_tiles, int32_t k, int32_t P);
int dc_tile_plan_T_build(const int32_t* plan, const int32_t* tptr, const int32_t* tedge, const int32_t* cloud_ptr,
                         int32_t num_clouds, int32_t num_points, int32_t max_cloud, int32_t k, int32_t P, int32_t* planT,
                         void* stream);
int dc_tile_plan_T_permute_coef(const float* coef, const float* coefB, const int32_t* planT, int32_t num_points,
                                int32_t num_clouds, int32_t num_tiles, int32_t k, int32_t P, float* coefTt, float* coefBTt,
                                void* stream);   /* coefB / coefBTt (may be NULL): a second operator of the same graph in the same launch */
int dc_apply_grad_T_tiled(const float* GTt, const int32_t* planT, int32_t n, int32_t num_clouds, int32_t num_tiles,
                          int32_t k, int32_t P, const float* dy, int32_t C, int64_t ldy, float* dx, int64_t ldx,
                          int32_t accumulate, void* stream);
int dc_apply_grad_T_sum_tiled(const float* GTt, const int32_t* planT, int32_t n, int32_t num_clouds, int32_t num_tiles,
                              int32_t k, int32_t P, const float* dy, int32_t C, int64_t ldy, const float* a, int64_t lda,
                              const float* b, int64_t ldb, float* out, int64_t ldo, void* stream);
int dc_apply_div_T_tiled(const float* DTt, const int32_t* planT, int32_t n, int32_t num_clouds, int32_t num_tiles,
                         int32_t k, int32_t P, const float* dy, int32_t C, int64_t ldy, float* dv, int64_t ldv,
                         int32_t accumulate, void* stream);
int dc_apply_hodge_T_tiled(const float* GTt, const int32_t* planT, int32_t n, int32_t num_clouds, int32_t num_tiles,
                           int32_t k, int32_t P, const float* dh, int32_t C, int64_t ldh, float* ddc, int64_t lddc,
                           int32_t accumulate, void* stream);
int dc_apply_div_curl_norm_T_tiled(const float* DTt, const int32_t* planT, int32_t n, int32_t num_clouds,
                                   int32_t num_tiles, int32_t k, int32_t P, const float* dout, int32_t C, int64_t ldo,
                                   const float* v, int64_t ldv, float* dv, int64_t lddv, int32_t accumulate, void* stream);
int dc_knn_max_backward_tiled(const int32_t* planT, int32_t n, int32_t num_clouds, int32_t num_tiles, int32_t k,
                              int32_t P, const uint8_t* arg, const float* dout, int32_t C, int64_t ldo, float* dh,
                              int64_t ldh, int32_t accumulate, void* stream);

/* ---- max aggregation (torch_scatter.scatter(reduce='max'): deltaconv/nn/deltaconv.py:52,54) -- */
/* out[i,c] = max_s h[nbr[i,s],c]; arg[Nt,C] = first maximal slot (k <= 255) */
int dc_knn_max(const int32_t* nbr, int32_t n, int32_t k, const float* h, int32_t C, int64_t ldh, float* out,
               int64_t ldo, uint8_t* arg, void* stream);
/* out[i,c] = max_s leaky_slope(scale_c * h[nbr[i,s],c] + shift_c): the BatchNorm + activation of s_mlp_max
 * (nn/mlp.py:9) folded into the max-aggregation gather (nn/deltaconv.py:54); same values, ties and slots
 * as dc_bn_act followed by dc_knn_max.  Backward: dc_knn_max_backward then dc_bn_act_backward. */
int dc_knn_max_affine(const int32_t* nbr, int32_t n, int32_t k, const float* h, int32_t C, int64_t ldh,
                      const float* scale, const float* shift, float slope, float* out, int64_t ldo, uint8_t* arg,
                      void* stream);
/* The same with the layer's last s_mlp block in its epilogue (round 6; tiled twin: dc_knn_max_affine_residual_tiled):
 * out = act2(scale2 h2 + shift2) + max_s act(scale h[nbr[i,s]] + shift) = `x = self.s_mlp(x) + x_max` of nn/deltaconv.py:54-59 with both
 * BatchNorm + LeakyReLU pairs folded in; out2 (may be NULL): second copy.  Same bits as dc_knn_max_affine + dc_bn_act2(residual). */
int dc_knn_max_affine_residual(const int32_t* nbr, int32_t n, int32_t k, const float* h, int32_t C, int64_t ldh,
                               const float* scale, const float* shift, float slope, const float* h2, int64_t ldh2,
                               const float* scale2, const float* shift2, float slope2, float* out, int64_t ldo, float* out2,
                               int64_t ldo2, uint8_t* arg, void* stream);
int dc_knn_max_backward(const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k, const uint8_t* arg,
                        const float* dout, int32_t C, int64_t ldo, float* dh, int64_t ldh, int32_t accumulate,
                        void* stream);
/* The other aggregations of DeltaConv(aggr=...) -- torch_scatter.scatter(reduce='sum' | 'add' | 'mean') at
 * nn/deltaconv.py:52,54: out[i,c] = scale * sum_s h[nbr[i,s],c] (scale = 1, or 1/k for the mean: every point has
 * exactly k neighbours incl. itself), slots in order; backward over the CSC in ascending edge order (no atomics).
 * ('min' runs as -max(-h) through dc_knn_max.) */
int dc_knn_sum(const int32_t* nbr, int32_t n, int32_t k, const float* h, int32_t C, int64_t ldh, float scale, float* out,
               int64_t ldo, void* stream);
int dc_knn_sum_backward(const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k, const float* dout, int32_t C,
                        int64_t ldo, float scale, float* dh, int64_t ldh, int32_t accumulate, void* stream);

/* ---- parallel transport between tangent frames ------------------------------------------------
 * build_transport                                       deltaconv/geometry/connection.py:6-47
 * out[m] = (r00, r01, r10, r11), the 2 x 2 matrix (row-major) that takes a vector's coordinates in the source frame
 * (sn, sx, sn x sx) to the target frame (tn, tx, ty); all arrays fp32 rows of 3, out [M,4].  nbr == NULL: the pair form
 * (row m of all five arrays, the reference's call shape; k is ignored).  nbr given (int32 [N,k], M = N * k): the graph
 * form, target = row m / k, source = row nbr[m]; sn / sx may be tn / tx.  One launch, one thread and one 16-byte store
 * (out 16-byte aligned, else four dword stores) per edge, no [E,3] expansion.  The reference's cos / sin of atan2 are
 * taken as x / r, y / r (csrc/connection_math.h), so the result has one fp32 value on every build. */
int dc_build_transport(const float* tn, const float* tx, const float* ty, const float* sn, const float* sx,
                       const int32_t* nbr, int32_t k, int64_t M, int32_t non_oriented, float* out, void* stream);
/* angle_in_plane                                        deltaconv/geometry/connection.py:50-59
 * out[m] = the angle from u to v in the plane orthogonal to normal (atan2f: tolerance only). */
int dc_angle_in_plane(const float* u, const float* v, const float* normal, int64_t M, float* out, void* stream);
/* rotate_around                                         deltaconv/geometry/connection.py:62-76
 * out[m] = v turned about axis by angle[m] (sincosf: tolerance only); out [M,3]. */
int dc_rotate_around(const float* v, const float* axis, const float* angle, int64_t M, float* out, void* stream);
/* Sum of the neighbours' vectors brought into the centre's frame -- what the reference composes from build_transport
 * (connection.py:40-47, one matrix per edge) and a scatter over edge_index[0]; no call site of its own in the models.
 * Vector rows as in dc_apply_div: rows 2i, 2i+1 of v / out are the two components at point i.  coef [n*k,4] (16-byte
 * aligned) holds one connection per edge.  out[2i+a,c] = scale * acc_a with acc_a = +0, then for slots s ascending,
 * j = nbr[i,s]: acc_a = (acc_a + coef[i,s,a,0] * v[2j,c]) + coef[i,s,a,1] * v[2j+1,c], every operation rounded to fp32.
 * The backward runs over the CSC (dc_csc_build), in-edges e = i*k + s ascending:
 * dv_b = (dv_b + coef[e,0,b] * g[2i,c]) + coef[e,1,b] * g[2i+1,c], dv[2j+b,c] (+)= scale * dv_b.  No atomics. */
int dc_transport_sum(const int32_t* nbr, int32_t n, int32_t k, const float* coef, const float* v, int32_t C, int64_t ldv,
                     float scale, float* out, int64_t ldo, void* stream);
int dc_transport_sum_backward(const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k, const float* coef,
                              const float* g, int32_t C, int64_t ldg, float scale, float* dv, int64_t ldv,
                              int32_t accumulate, void* stream);

/* ---- scalar / vector MLP stream around the dense GEMM -------------------------------------------
 * Linear -> BatchNorm1d(over rows) -> LeakyReLU(0.2)   deltaconv/nn/mlp.py:7-11, nn/nonlin.py:11-35
 * Linear -> VectorNonLin(BatchNorm1d)                  deltaconv/nn/mlp.py:13-17, nn/nonlin.py:38-86
 * (ATen native_batch_norm / leaky_relu / linalg_vector_norm / mul / div in the reference).
 * Column reductions are ordered two-stage sums (bit-reproducible).  Workspace: dc_bn_workspace_bytes. */
size_t dc_bn_workspace_bytes(int64_t rows, int32_t C);
/* batch statistics of h[R,C] -> mean, invstd, scale = gamma*invstd, shift = beta - mean*scale;
 * running_mean/var (may be NULL) updated with momentum (unbiased variance), as nn.BatchNorm1d */
int dc_bn_stats(const float* h, int64_t R, int32_t C, int64_t ldh, const float* gamma, const float* beta, float eps,
                float momentum, float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                float* shift, void* workspace, size_t workspace_bytes, void* stream);
/* inference coefficients from the running statistics */
int dc_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, int32_t C, float* mean, float* invstd, float* scale, float* shift, void* stream);
/* y = leaky_slope(scale*h + shift) (+ residual);  slope 1 = identity, 0 = ReLU */
int dc_bn_act(const float* h, int64_t R, int32_t C, int64_t ldh, const float* scale, const float* shift, float slope,
              const float* residual, int64_t ldr, float* y, int64_t ldy, void* stream);
/* dc_bn_act with a second destination y2 (may be NULL): a layer output that is also a column block of the
 * concatenated embedding input (`torch.cat(conv_out, dim=1)`, models/deltanet_classification.py:42) */
int dc_bn_act2(const float* h, int64_t R, int32_t C, int64_t ldh, const float* scale, const float* shift, float slope,
               const float* residual, int64_t ldr, float* y, int64_t ldy, float* y2, int64_t ldy2, void* stream);
/* backward of dc_bn_act (through the batch statistics when training != 0); dgamma/dbeta may be NULL */
int dc_bn_act_backward(const float* dy, int64_t lddy, const float* h, int64_t ldh, int64_t R, int32_t C,
                       const float* scale, const float* shift, const float* mean, const float* invstd,
                       const float* gamma, float slope, int32_t training, float* dh, int64_t lddh, float* dgamma,
                       float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* vector block.  in: combine != 0 -> [2n, 2co] = [P | Q], the Linear applied to v_cat (NOT to
 * I_J(v_cat)) with the weight halves stacked, y_u = P_u - Q_v, y_v = P_v + Q_u
 * (deltaconv/geometry/operators.py:9-21 folded into the epilogue); combine == 0 -> [2n, co] = y;
 * combine == 2 -> P and Q interleaved (column 2c = P_c, 2c+1 = Q_c), i.e. v_cat @ W.view(2co, K)^T for the
 * reference's [co, 2K] weight of the first VectorMLP layer, no re-stacking of W.
 * combine == 3 (dc_vn_backward, dc_vn_backward_sums, dc_vn_backward_apply only): in = y[2n, co] as stored by
 * dc_linear_vn_stats_forward(interleaved = 2), ld >= co; din = the interleaved d(P, Q) [2n, 2co] of combine == 2
 * (lddi >= 2co), the operand of the block's gradient products.  Same bits as combine == 2 on the matching PQ. */
int dc_vn_stats(const float* in, int64_t n, int32_t co, int64_t ld, int32_t combine, const float* gamma,
                const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                float* invstd, float* scale, float* shift, void* workspace, size_t workspace_bytes, void* stream);
/* out[2n,co] = y * relu(scale*|y| + shift) / max(|y|, 1e-8) */
int dc_vn_apply(const float* in, int64_t n, int32_t co, int64_t ld, int32_t combine, const float* scale,
                const float* shift, float* out, int64_t ldo, void* stream);
int dc_vn_backward(const float* dout, int64_t lddo, const float* in, int64_t ld, int32_t combine, int64_t n,
                   int32_t co, const float* scale, const float* shift, const float* mean, const float* invstd,
                   const float* gamma, int32_t training, float* din, int64_t lddi, float* dgamma, float* dbeta,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- layer-0 ("centralized") edge MLP + max aggregation without the [E,C] tensor ------------------
 * scatter(s_mlp_max(x[col] - x[row]), row, reduce='max') -- deltaconv/nn/deltaconv.py:50-52 with a
 * depth-1 s_mlp_max (nn/mlp.py:7-11).  y = Linear(x) [Nt,C]; edge pre-activation a_e = y_j - y_i.
 * Derivation in deltaconv_amd/csrc/edge_math.h.  amax/amin/s1pt/dzs: [Nt,C] fp32 contiguous,
 * argmax/argmin/arg: uint8 [Nt,C].  Workspace: dc_bn_workspace_bytes(Nt, C). */
int dc_edge_gather_stats(const float* y, int64_t ldy, const int32_t* nbr, int32_t n, int32_t k, int32_t C,
                         int32_t compute_stats, const float* gamma, const float* beta, float eps, float momentum,
                         float* running_mean, float* running_var, float* amax, float* amin, uint8_t* argmax,
                         uint8_t* argmin, float* s1pt, float* mean, float* invstd, float* scale, float* shift,
                         void* workspace, size_t workspace_bytes, void* stream);
int dc_edge_max_apply(const float* amax, const float* amin, const uint8_t* argmax, const uint8_t* argmin, int32_t n,
                      int32_t C, const float* scale, const float* shift, float slope, float* out, int64_t ldo,
                      uint8_t* arg, void* stream);
/* dc_edge_max_apply with the layer's last s_mlp block in its epilogue (round 6): out = act2(scale2 h2 + shift2) + x_max
 * (`x = self.s_mlp(x) + x_max`, deltaconv/nn/deltaconv.py:59), second copy in out2 (may be NULL).  Same bits as
 * dc_edge_max_apply followed by dc_bn_act2 with x_max as residual. */
int dc_edge_max_apply_residual(const float* amax, const float* amin, const uint8_t* argmax, const uint8_t* argmin, int32_t n,
                               int32_t C, const float* scale, const float* shift, float slope, const float* h2,
                               int64_t ldh2, const float* scale2, const float* shift2, float slope2, float* out,
                               int64_t ldo, float* out2, int64_t ldo2, uint8_t* arg, void* stream);
int dc_edge_max_backward(const float* dout, int64_t lddo, const float* y, int64_t ldy, const int32_t* tptr,
                         const int32_t* tedge, int32_t n, int32_t k, int32_t C, const float* amax, const float* amin,
                         const uint8_t* argmax, const uint8_t* argmin, const float* s1pt, const float* scale,
                         const float* shift, const float* mean, const float* invstd, float slope, int32_t training,
                         float* dzs, float* dy, int64_t lddy, float* dgamma, float* dbeta, void* workspace,
                         size_t workspace_bytes, void* stream);
/* dc_edge_max_backward with its CSC pass running from the transposed tile plan (rows (y_i, dz*_i) of the in-edges' sources
 * and the selected slot bytes in LDS); argsel = the `arg` output of dc_edge_max_apply; y, dzs, amax, amin, s1pt contiguous
 * [Nt, C], C % 64 == 0.  Same results bit for bit (same reference lines: nn/deltaconv.py:50-52 backward). */
int dc_edge_max_backward_tiled(const float* dout, int64_t lddo, const float* y, const int32_t* planT, int32_t n,
                               int32_t num_clouds, int32_t num_tiles, int32_t k, int32_t P, int32_t C, const float* amax,
                               const float* amin, const uint8_t* argsel, const float* s1pt, const float* scale,
                               const float* shift, const float* mean, const float* invstd, float slope, int32_t training,
                               float* dzs, float* dy, int64_t lddy, float* dgamma, float* dbeta, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- general form of the centralised edge MLP: materialised edge tensor --------------------------------------------------
 * x_edge = x[col] - x[row] and scatter(h, row, reduce=aggr) of deltaconv/nn/deltaconv.py:50-52 for the shapes the two fused
 * forms do not cover (depth >= 3, other widths, aggr != 'max'): edges are centre-major with k contiguous slots
 * (grad_div_mls.py:24-25), so the scatter is a reduction over k consecutive rows.  mode: 0 max, 1 min, 2 sum, 3 mean;
 * max / min ties keep the first slot. */
int dc_edge_diff(const float* x, int64_t ldx, const int32_t* nbr, int32_t n, int32_t k, int32_t C, float* out, void* stream);
int dc_edge_diff_backward(const float* dE, const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k, int32_t C,
                          float* dx, int64_t lddx, void* stream);
int dc_seg_reduce(const float* h, int32_t n, int32_t k, int32_t C, int32_t mode, float* out, uint8_t* arg, void* stream);
int dc_seg_reduce_backward(const float* dout, int64_t lddo, const uint8_t* arg, int32_t n, int32_t k, int32_t C, int32_t mode,
                           float* dh, void* stream);

/* ---- depth-2 centralised edge MLP + max aggregation (first layer of the part-segmentation net) ------------------------
 * out[i] = max_s act2(bn2(W2 act1(bn1(W1 (x_j - x_i))))), BatchNorm statistics over all E = n k edges:
 * deltaconv/nn/deltaconv.py:50-52 with s_mlp_max = MLP([ci, 64, 64]) (experiments/train_shapenet.py:77-89, mlp_depth = 2),
 * i.e. index_select, two addmm, two native_batch_norm, two leaky_relu and scatter_max on [E, 64] tensors + their autograd.
 * Here (deltaconv_amd/csrc/edge2.hip): z = x W1^T on n rows (own GEMM), statistics of z_j - z_i by dc_edge_gather_stats, then
 * ONE pass over the edges on v_mfma_f32_16x16x4_f32 (exact fp32) that keeps, per (point, channel), the selected
 * pre-BatchNorm-2 value `ysel`, its first slot `arg`, and the BatchNorm-2 sums; out = act2(scale2 ysel + shift2) is a
 * dc_bn_act call.  Backward: ONE recompute pass (three chained MFMA products: y2, du1 = (dy2 W2) act1', dW2 += dy2^T h1)
 * + a CSC closing pass; bit-reproducible (ordered reductions, in-edges in ascending edge id).  64 channels in both blocks.
 * stats_mode: 1 = batch statistics -> mean2 / invstd2 / scale2 / shift2 (+ running statistics), 2 = fp64 sums only
 * (sums = double [2][2*64 + 1] = 258 doubles: two identical records [sum y2 | sum y2^2 | rows = n k], the layout of
 * dc_bn_sums; finished by dc_bn_coeffs_from_sums after the all-reduce: synchronised BatchNorm), 0 = none.  coef1 / coef2 = [mean | invstd | scale | shift]
 * rows (4 x 64).  x [n, ci] / W1 [64, ci] (may be NULL): for ci <= 3 the edge pre-activation is evaluated as W1 (x_j - x_i)
 * per edge, the reference's own order of operations, instead of z_j - z_i.  Workspace: dc_edge2_workspace_bytes(n, k, backward). */
size_t dc_edge2_workspace_bytes(int32_t n, int32_t k, int32_t backward);
/* BatchNorm-1 of that block for ci <= 3 WITHOUT z: y1 = W1 (x_j - x_i) is linear in the edge difference, so its batch statistics
 * follow from the ci + ci (ci + 1) / 2 first and second moments of the differences (ordered fp64 sums); sd [n, ci] = sum_s
 * (x_j - x_i) per point feeds the closed forms of the backward pass.  With it dc_edge2_forward / dc_edge2_backward take z = NULL
 * and `s1pt` = sd. */
int dc_edge2_bn1_stats(const float* x, int64_t ldx, int32_t ci, const float* W1, const int32_t* nbr, int32_t n, int32_t k,
                       const float* gamma1, const float* beta1, float eps, float momentum, float* running_mean,
                       float* running_var, float* sd, float* mean1, float* invstd1, float* scale1, float* shift1,
                       void* workspace, size_t workspace_bytes, void* stream);
int dc_edge2_forward(const float* z, const float* x, int64_t ldx, int32_t ci, const float* W1, const int32_t* nbr,
                     int32_t n, int32_t k, const float* W2, const float* scale1,
                     const float* shift1, float slope1, int32_t stats_mode, const float* gamma2, const float* beta2,
                     float eps, float momentum, float* running_mean, float* running_var, float* ysel, uint8_t* arg,
                     float* mean2, float* invstd2, float* scale2, float* shift2, double* sums, void* workspace,
                     size_t workspace_bytes, void* stream);
int dc_edge2_backward(const float* dout, int64_t lddo, const float* z, const float* x, int64_t ldx, int32_t ci,
                      const float* W1, const int32_t* nbr, const int32_t* tptr,
                      const int32_t* tedge, int32_t n, int32_t k, const float* W2, const float* coef1, const float* coef2,
                      const float* gamma2, float slope1, float slope2, int32_t training1, int32_t training2,
                      const float* ysel, const uint8_t* arg, const float* s1pt, float* dz, int64_t lddz, float* dW2,
                      float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- weight-gradient GEMM on the fp32 matrix cores ---------------------------------------------------
 * C[M,N] (+)= A^T B,  A [R,M], B [R,N], R >> M,N  (dW = dY^T X of every per-point Linear layer: ATen mm in the
 * autograd of deltaconv/nn/mlp.py:9,15).  v_mfma_f32_32x32x2_f32 through the LDS-staged kernel (any M, N, leading
 * dimension < 2^21), reduction split over row slabs (one resident wave of workgroups), ordered reduction kernel:
 * deterministic.  Workspace: dc_gemm_tn_workspace_bytes. */
size_t dc_gemm_tn_workspace_bytes(int64_t R, int32_t M, int32_t N);
int dc_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t R, int32_t M, int32_t N, float* C,
               int64_t ldc, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* The same product with the slab reduction deferred: an autograd node that forms several weight gradients (a DeltaConv layer:
 * v_mlp, s_mlp and max-aggregation Linear of deltaconv/nn/deltaconv.py:35-47) writes the partial tiles [slabs][M][N] of each into
 * its own workspace (dc_gemm_tn_slabs; *slabs <- their number, a HOST int) and sums them all with ONE dc_gemm_tn_reduce_many at
 * the end: C_i[rows_i, cols_i] (ldc_i) (+)= ordered sum of the slabs of entry i, i < count (host arrays of device addresses /
 * sizes) -- the bits dc_gemm_tn writes, in one launch instead of one per weight. */
int dc_gemm_tn_slabs(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t R, int32_t M, int32_t N,
                     void* workspace, size_t workspace_bytes, int32_t* slabs, void* stream);
int dc_gemm_tn_reduce_many(const int64_t* partials, const int64_t* outs, const int64_t* ldc, const int32_t* rows,
                           const int32_t* cols, const int32_t* slabs, const int32_t* accumulate, int32_t count,
                           void* stream);

/* ---- split statistics for synchronised BatchNorm (data parallel) ----------------------------------------
 * Same arithmetic as dc_bn_stats / dc_vn_stats / dc_bn_act_backward / dc_vn_backward (nn/nonlin.py:24-35, 63-79),
 * cut at the reduction so that the host can all-reduce the fp64 column sums across ranks in between
 * (deltaconv_amd/dp.py).  sums: double [2][2*C + 1] = two identical records
 * (sum_0[C] | sum_1[C] | rows of this rank): the host all-reduces the FIRST record in place, the second stays this rank's own
 * (dgamma / dbeta are local sums): no fill, no clone.  dc_sync_means: m1 = sum_0 / rows, m2 = sum_1 / rows from the reduced
 * record, dbeta / dgamma (may be NULL) from the local one.
 *   forward : dc_bn_sums | dc_vn_sums -> all-reduce -> dc_bn_coeffs_from_sums(count = rows of ALL ranks; count <= 0:
 *             the count is on the device at sums[2*C], all-reduced together with the sums -- no host sync)
 *   backward: dc_*_backward_sums -> all-reduce -> m1 = sum_0 / count, m2 = sum_1 / count -> dc_*_backward_apply;
 *             dc_bn_act_backward_sums takes the all-reduced FORWARD record (forward_sums = [sum x | sum x^2 | rows]) and eps
 *             instead of the fp32 mean / invstd: xhat = (h - mean) invstd in fp64, so that the cancellation in h - mean
 *             does not cost dgamma and the second mean |mean| invstd 2^-24 per addend;
 *             dbeta = local sum_0, dgamma = local sum_1 (averaged with the other gradients afterwards). */
int dc_bn_sums(const float* h, int64_t R, int32_t C, int64_t ldh, double* sums, void* workspace,
               size_t workspace_bytes, void* stream);
int dc_vn_sums(const float* in, int64_t n, int32_t co, int64_t ld, int32_t combine, double* sums, void* workspace,
               size_t workspace_bytes, void* stream);
int dc_bn_coeffs_from_sums(const double* sums, int64_t count, int32_t C, const float* gamma, const float* beta,
                           float eps, float momentum, float* running_mean, float* running_var, float* mean,
                           float* invstd, float* scale, float* shift, void* stream);
int dc_bn_act_backward_sums(const float* dy, int64_t lddy, const float* h, int64_t ldh, int64_t R, int32_t C,
                            const float* scale, const float* shift, const double* forward_sums, float eps,
                            float slope, double* sums, void* workspace, size_t workspace_bytes, void* stream);
int dc_sync_means(const double* sums, int32_t C, float* m1, float* m2, float* dgamma, float* dbeta, void* stream);
int dc_bn_act_backward_apply(const float* dy, int64_t lddy, const float* h, int64_t ldh, int64_t R, int32_t C,
                             const float* scale, const float* shift, const float* mean, const float* invstd,
                             const float* gamma, float slope, int32_t training, const float* m1, const float* m2,
                             float* dh, int64_t lddh, void* stream);
int dc_vn_backward_sums(const float* dout, int64_t lddo, const float* in, int64_t ld, int32_t combine, int64_t n,
                        int32_t co, const float* scale, const float* shift, const float* mean, const float* invstd,
                        double* sums, void* workspace, size_t workspace_bytes, void* stream);
int dc_vn_backward_apply(const float* dout, int64_t lddo, const float* in, int64_t ld, int32_t combine, int64_t n,
                         int32_t co, const float* scale, const float* shift, const float* mean, const float* invstd,
                         const float* gamma, int32_t training, const float* m1, const float* m2, float* din,
                         int64_t lddi, void* stream);

/* ---- pre-split weight planes (round 4) -----------------------------------------------------------------------------
 * The split products cut every fp32 operand into three bfloat16 planes.  For the WEIGHT operand of the Linear layers
 * (nn/mlp.py:9,15) that work is the same in every workgroup of every product of a step: dc_presplit_weights cuts all
 * registered weight matrices once (one launch; table = device records {src, fwd planes | NULL, bwd planes | NULL, rows, cols,
 * row stride}, chunk_start = prefix of ceil(rows * cols / 1024) per record), dc_gemm_next_b_planes hands the planes of the
 * next dc_linear_* product of the calling thread to the library (transposed = planes of W^T, for dc_linear_backward_input).
 * `weight` is the fp32 matrix the planes were cut from: the hint is dropped unless the next product's weight operand is that
 * pointer (a hint left behind by a call that failed before its product cannot reach another product of the same shape).
 * Same bits as the in-loop split; the hint is ignored where it does not apply. */
int dc_presplit_weights(const int64_t* table, const int32_t* chunk_start, int32_t n_entries, int32_t total_chunks, void* stream);
int dc_gemm_next_b_planes(const void* weight, const void* planes, int64_t plane_elems, int64_t ld, int32_t transposed);

/* ---- forward / input-gradient GEMMs of the per-point Linear layers on the fp32 matrix cores -------------
 * Replace ATen addmm / mm behind every `Linear(bias=False)` of deltaconv/nn/mlp.py:9,15 (forward product and the
 * input-gradient product of its autograd).  v_mfma_f32_32x32x2_f32 (exact fp32), LDS-staged, any M, N, K and
 * leading dimensions (an unguarded fast path when everything is tile-aligned).  tile: 0 = automatic,
 * 1..4 = 128x128, 128x64, 64x64, 64x128 (measurement).
 *   dc_linear_forward           Y[M,N]  = X[M,K] W[N,K]^T
 *   dc_linear_backward_input    dX[M,K] (+)= dY[M,N] W[N,K]
 * and the forward product fused with the statistics of the layer that follows it (nn/nonlin.py:24-35, 63-79):
 *   dc_linear_bn_stats_forward  Y = X W^T  + BatchNorm batch statistics of Y (== dc_bn_stats on Y)
 *   dc_linear_vn_stats_forward  interleaved: PQ[2n,2co] = V[2n,K] Wst[2co,K]^T (columns interleaved (P_c, Q_c)) +
 *                               statistics of |y| over the n points (== dc_vn_stats(combine = 2) on PQ); otherwise
 *                               Y[2n,co] = V W[co,K]^T + statistics of |(Y_2i, Y_2i+1)| (== dc_vn_stats(combine = 0)).
 *                               interleaved == 2: product and statistics of interleaved == 1, but PQ receives the combined
 *                               y[2n,co] (y_u = P_u - Q_v, y_v = P_v + Q_u; ldpq >= co) -- the bits the dc_vn_* kernels
 *                               rebuild from a stored PQ with combine = 2, at half the bytes.  Consumers: dc_vn_apply /
 *                               dc_vn_stats / dc_vn_sums with combine = 0, the dc_vn_backward* family with combine = 3.
 *                               (dc_linear_vn_sums_forward takes the same three values.)
 * The statistics come out of the GEMM epilogue (fp64 tile sums, ordered final stage): no pass over Y.
 * Workspace: dc_linear_stats_workspace_bytes(M, N, K, tile)  (vn: M = 2n, N = 2co). */
int dc_linear_forward(const float* X, int64_t ldx, const float* W, int64_t ldw, int64_t M, int32_t N, int32_t K,
                      float* Y, int64_t ldy, int32_t tile, void* stream);
int dc_linear_backward_input(const float* dY, int64_t lddy, const float* W, int64_t ldw, int64_t M, int32_t N,
                             int32_t K, float* dX, int64_t lddx, int32_t accumulate, int32_t tile, void* stream);
size_t dc_linear_stats_workspace_bytes(int64_t M, int32_t N, int32_t K, int32_t tile);
int dc_linear_bn_stats_forward(const float* X, int64_t ldx, const float* W, int64_t ldw, int64_t M, int32_t N,
                               int32_t K, float* Y, int64_t ldy, const float* gamma, const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                               float* scale, float* shift, int32_t tile, void* workspace, size_t workspace_bytes,
                               void* stream);
int dc_linear_vn_stats_forward(const float* V, int64_t ldv, const float* Wst, int64_t ldw, int64_t n, int32_t co,
                               int32_t K, float* PQ, int64_t ldpq, int32_t interleaved, const float* gamma,
                               const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                               float* scale, float* shift, int32_t tile, void* workspace, size_t workspace_bytes,
                               void* stream);

/* the two statistics products with the reduction cut open (synchronised BatchNorm): sums = double [2][2*C + 1], the fp64 column sums of this
 * rank's rows (two records, as above), to be all-reduced and finished by dc_bn_coeffs_from_sums -- the fused layer nodes keep their GEMM epilogues
 * when BatchNorm statistics span the ranks of a data-parallel group. */
int dc_linear_bn_sums_forward(const float* X, int64_t ldx, const float* W, int64_t ldw, int64_t M, int32_t N, int32_t K,
                              float* Y, int64_t ldy, double* sums, int32_t tile, void* workspace, size_t workspace_bytes,
                              void* stream);
int dc_linear_vn_sums_forward(const float* V, int64_t ldv, const float* Wst, int64_t ldw, int64_t n, int32_t co, int32_t K,
                              float* PQ, int64_t ldpq, int32_t interleaved, double* sums, int32_t tile, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- BatchNorm/activation backward folded into the GEMMs that consume it --------------------------------
 * Backward of one MLP block y = leaky(batch_norm(x W^T)) (nn/mlp.py:7-11, nn/nonlin.py:24-35): instead of
 * dc_bn_act_backward (reduce + a pass that writes dh) followed by two products that read dh,
 *   dc_bn_act_backward_reduce     dgamma, dbeta, coefs[5*C]  (c_sc | c_sh | c_g | c_a | c_b)
 *   dc_linear_bn_backward_input   dX[M,K] (+)= dh W,    dc_linear_bn_backward_weight   dW[N,K] (+)= dh^T X
 * rebuild dh = c_g * dy * act'(c_sc h + c_sh) + c_a h + c_b inside their operand loaders: dh is never materialised
 * (one launch and 3 passes over [M,N] less per block).  Workspaces: dc_bn_workspace_bytes(R, C) and
 * dc_gemm_tn_workspace_bytes(R, N, K). */
int dc_bn_act_backward_reduce(const float* dy, int64_t lddy, const float* h, int64_t ldh, int64_t R, int32_t C,
                              const float* scale, const float* shift, const float* mean, const float* invstd,
                              const float* gamma, float slope, int32_t training, float* dgamma, float* dbeta,
                              float* coefs, void* workspace, size_t workspace_bytes, void* stream);
/* the coefficient rows of that prologue from ALL-REDUCED sums (dc_bn_act_backward_sums on every rank -> all-reduce):
 * coefs[5 C] from global_sums and the global row count (count <= 0: on the device at global_sums[2 C]); dgamma / dbeta
 * from local_sums (this rank's share; gradients are averaged afterwards). */
int dc_bn_backward_coefs_from_sums(const double* global_sums, int64_t count, const double* local_sums, int32_t C,
                                   const float* gamma, const float* scale, const float* shift, const float* mean,
                                   const float* invstd, int32_t training, float* dgamma, float* dbeta, float* coefs,
                                   void* stream);
int dc_linear_bn_backward_input(const float* dy, int64_t lddy, const float* h, int64_t ldh, const float* coefs,
                                float slope, const float* W, int64_t ldw, int64_t M, int32_t N, int32_t K, float* dX,
                                int64_t lddx, int32_t accumulate, int32_t tile, void* stream);
int dc_linear_bn_backward_weight(const float* dy, int64_t lddy, const float* h, int64_t ldh, const float* coefs,
                                 float slope, const float* X, int64_t ldx, int64_t R, int32_t N, int32_t K, float* dW,
                                 int64_t lddw, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                 void* stream);
/* partial tiles [slabs][N][K] only; the ordered sum comes later from dc_gemm_tn_reduce_many (see dc_gemm_tn_slabs) */
int dc_linear_bn_backward_weight_slabs(const float* dy, int64_t lddy, const float* h, int64_t ldh, const float* coefs,
                                       float slope, const float* X, int64_t ldx, int64_t R, int32_t N, int32_t K,
                                       void* workspace, size_t workspace_bytes, int32_t* slabs, void* stream);

/* Both gradients of a block in ONE call: dW[N,K] (lddw) (+)= dh^T X and dX[R,K] (lddx) (+)= dh W for dh [R,N] = dY (plain form:
 * what dc_gemm_tn(dY, X) and dc_linear_backward_input compute) or the BatchNorm-backward prologue of (dy, h, coefs) (what
 * dc_linear_bn_backward_weight and dc_linear_bn_backward_input compute).  Each product picks its tile, load mode, multiply path and
 * slab plan as in those calls (a plane hint of dc_gemm_next_b_planes goes to the input-gradient product); the two read the same dh
 * and write disjoint outputs, so where the library holds their pair of kernel instantiations they run as one launch
 * (gemm_dual_kernel: the weight-gradient workgroups first, the input-gradient workgroups fill the CUs behind them), otherwise --
 * ragged shapes, the exact chain, weight gradients that run the plane-image kernel, option 14 = 1 -- as the two launches of the
 * separate calls.  The same bits either way.  Workspace: dc_gemm_tn_workspace_bytes(R, N, K).  The _slabs forms leave the partial
 * tiles [slabs][N][K] in the workspace for dc_gemm_tn_reduce_many (*slabs: a HOST int). */
int dc_linear_backward_both(const float* dY, int64_t lddy, const float* X, int64_t ldx, const float* W, int64_t ldw, int64_t R,
                            int32_t N, int32_t K, float* dW, int64_t lddw, int32_t accumulate_w, float* dX, int64_t lddx,
                            int32_t accumulate_x, int32_t tile, void* workspace, size_t workspace_bytes, void* stream);
int dc_linear_backward_both_slabs(const float* dY, int64_t lddy, const float* X, int64_t ldx, const float* W, int64_t ldw,
                                  int64_t R, int32_t N, int32_t K, float* dX, int64_t lddx, int32_t accumulate_x, int32_t tile,
                                  void* workspace, size_t workspace_bytes, int32_t* slabs, void* stream);
int dc_linear_bn_backward_both(const float* dy, int64_t lddy, const float* h, int64_t ldh, const float* coefs, float slope,
                               const float* X, int64_t ldx, const float* W, int64_t ldw, int64_t R, int32_t N, int32_t K,
                               float* dW, int64_t lddw, int32_t accumulate_w, float* dX, int64_t lddx, int32_t accumulate_x,
                               int32_t tile, void* workspace, size_t workspace_bytes, void* stream);
int dc_linear_bn_backward_both_slabs(const float* dy, int64_t lddy, const float* h, int64_t ldh, const float* coefs, float slope,
                                     const float* X, int64_t ldx, const float* W, int64_t ldw, int64_t R, int32_t N, int32_t K,
                                     float* dX, int64_t lddx, int32_t accumulate_x, int32_t tile, void* workspace,
                                     size_t workspace_bytes, int32_t* slabs, void* stream);

/* ---- per-cloud term of the segmentation head's first Linear ----------------------------------------------------------------
 * deltaconv/models/deltanet_segmentation.py:59-66: x_max[batch] (+ the category vector) is concatenated in front of the point
 * features and fed to Linear(E + S, 256).  Here Linear([x_max[batch] | conv]) = Linear_a(x_max)[batch] + Linear_b(conv): the
 * per-cloud half runs on B rows; dc_cloud_bias_add joins it to the per-point half (y[i] = h[i] + g[i / mx], equal-size clouds of
 * mx points, y may be h), dc_cloud_colsum is its backward (out[b] = sum of the rows of cloud b: the index_add of `[batch]`),
 * an ordered two-stage fp64 reduction (bit-reproducible).  Workspace: dc_cloud_colsum_workspace_bytes. */
int dc_cloud_bias_add(const float* h, int64_t ldh, const float* g, int64_t ldg, int64_t n, int32_t C, int64_t mx, float* y,
                      int64_t ldy, void* stream);
size_t dc_cloud_colsum_workspace_bytes(int32_t num_clouds, int64_t mx, int32_t C);
int dc_cloud_colsum(const float* x, int64_t ldx, int32_t num_clouds, int64_t mx, int32_t C, float* out, int64_t ldo,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- embedding head fused with the per-cloud pooling -------------------------------------------------
 * MLP([sum c, E]) -> global_max_pool | global_mean_pool  (deltaconv/models/deltanet_classification.py:42-49),
 * -> global_max_pool (deltanet_segmentation.py:58-61).  h = Linear output [B*N, C] (equal-size clouds);
 * the [B*N, C] activation is never written.  pooled[B, ldp] = [max | mean]; argmax[B, C] = row in cloud. */
int dc_bn_act_pool(const float* h, int64_t ldh, int32_t num_clouds, int32_t N, int32_t C, const float* scale,
                   const float* shift, float slope, int32_t with_mean, float* pooled, int64_t ldp, int32_t* argmax,
                   void* stream);
int dc_bn_act_pool_backward(const float* dpooled, int64_t ldp, const int32_t* argmax, const float* h, int64_t ldh,
                            int32_t num_clouds, int32_t N, int32_t C, const float* scale, const float* shift,
                            const float* mean, const float* invstd, const float* gamma, float slope,
                            int32_t with_mean, int32_t training, float* dh, int64_t lddh, float* dgamma, float* dbeta,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- training loss ------------------------------------------------------------------------------
 * Replaces experiments/utils.py:7-24 (`calc_loss`: label-smoothed cross entropy, eps = 0.2, or
 * `F.cross_entropy(..., reduction='mean')` when smoothing = 0) together with its autograd backward:
 *   loss    = mean_r( -sum_c q_rc * log_softmax(logits_r)_c ),  q = 1-smoothing on the label, smoothing/(C-1) elsewhere
 *   dlogits = (softmax(logits_r) - q_r) / num_rows            (multiply by the incoming gradient of the loss)
 * labels int64 in [0, num_classes) (a label outside poisons the loss with NaN).  Deterministic (ordered fp64 sum). */
size_t dc_ce_loss_workspace_bytes(int64_t num_rows);
int dc_ce_loss(const float* logits, int64_t ld_logits, const int64_t* labels, int64_t num_rows, int32_t num_classes,
               float smoothing, float* loss, float* dlogits, int64_t ld_dlogits, void* workspace,
               size_t workspace_bytes, void* stream);

/* ---- MLP blocks on a handful of rows: the classification head, one row per cloud --------------------------------
 * (/root/reference/deltaconv/models/deltanet_classification.py:34-36,51: MLP([2048,512]) -> Dropout -> MLP([512,256]) ->
 * Dropout -> Linear(256, num_classes); blocks = nn/mlp.py:7-11).  One kernel per block and direction: product +
 * BatchNorm statistics over the rows + finalisation + running statistics + activation forward; BatchNorm / activation
 * backward + d gamma / d beta + weight gradient backward (the input gradient dX = dH W is dc_linear_backward_input).
 * mode 0 = Linear (+ bias) only, 1 = BatchNorm with batch statistics, 2 = with running statistics.
 * M <= dc_rowblock_max_rows() (64), K % 4 == 0, rows of X / W / dW 16-byte aligned.  coef[4,N] = mean, invstd, scale,
 * shift (written forward, read backward); H = the Linear output (saved for backward; mode 0: Y may alias H). */
int32_t dc_rowblock_max_rows(void);
int dc_rowblock_forward(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, int32_t M, int32_t N,
                        int32_t K, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                        float* running_var, int32_t mode, float slope, float* H, int64_t ldh, float* coef, float* Y,
                        int64_t ldy, void* stream);
int dc_rowblock_backward(const float* dY, int64_t lddy, const float* H, int64_t ldh, const float* coef, const float* gamma,
                         float slope, int32_t mode, const float* X, int64_t ldx, int32_t M, int32_t N, int32_t K, float* dW,
                         int64_t lddw, float* dbias, float* dgamma, float* dbeta, float* dH, int64_t lddh, void* stream);
/* The block FOLLOWED BY torch.nn.Dropout(p) (deltaconv/models/deltanet_classification.py:34-36: MLP -> Dropout(0.5) -> MLP ->
 * Dropout(0.5) -> Linear) in the block's own launches: forward Y = dropout(act(bn(X W^T))) and mask[M, N] (1 = kept);
 * backward takes the gradient behind the dropout.  Draws: Philox-4x32-10 keyed by `seed`, counter (element, salt, *step);
 * `step` points at the block's BatchNorm num_batches_tracked on the device (a new mask in every training step, also in
 * replays of a captured graph), `salt` tells the dropout layers of a model apart.  mode 1 | 2 as above. */
int dc_rowblock_forward_dropout(const float* X, int64_t ldx, const float* W, int64_t ldw, int32_t M, int32_t N, int32_t K,
                                const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                                float* running_var, int32_t mode, float slope, float* H, int64_t ldh, float* coef, float* Y,
                                int64_t ldy, float p, int32_t seed, const int64_t* step, int32_t salt, uint8_t* mask,
                                void* stream);
int dc_rowblock_backward_dropout(const float* dY, int64_t lddy, const float* H, int64_t ldh, const float* coef,
                                 const float* gamma, float slope, int32_t mode, const float* X, int64_t ldx, int32_t M,
                                 int32_t N, int32_t K, float* dW, int64_t lddw, float* dgamma, float* dbeta, float* dH,
                                 int64_t lddh, const uint8_t* mask, float p, void* stream);

/* ---- optimizer step (step glue: experiments/train_modelnet.py:67, train_scanobjectnn.py:77, train_shapenet.py:95) -------- */
/* torch.optim.SGD(lr, momentum, weight_decay) (dampening 0, no Nesterov) over ALL parameters in one launch (96 tensors per
 * launch):  g' = g + weight_decay p;  buf = momentum buf + g';  p -= lr buf  (buf starts at zero).  params / grads / bufs /
 * numel: HOST arrays of `count` device addresses / element counts (fp32, contiguous); lr: DEVICE scalar (a scheduler writes
 * it between replays of a captured step). */
int dc_sgd_step(const int64_t* params, const int64_t* grads, const int64_t* bufs, const int64_t* numel, int32_t count,
                const float* lr, float momentum, float weight_decay, void* stream);
/* torch.optim.Adam(lr, betas, eps, weight_decay) (no amsgrad; experiments/train_shapeseg.py:82) over ALL parameters in one
 * launch (80 tensors per launch), torch's single-tensor op order:  t = step + 1;  g' = g + weight_decay p;
 * m += (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g'^2;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).
 * Host arrays as in dc_sgd_step; lr: DEVICE scalar; step: DEVICE fp32 scalar shared by all parameters, incremented by one (by
 * the last workgroup to finish); ticket: DEVICE int32 holding zero (left zero). */
int dc_adam_step(const int64_t* params, const int64_t* grads, const int64_t* exp_avgs, const int64_t* exp_avg_sqs,
                 const int64_t* numel, int32_t count, const float* lr, float* step, int32_t* ticket, double beta1, double beta2,
                 float eps, float weight_decay, void* stream);
/* Several small (strided) copies in one launch: the batch load into the inputs of a captured step (`data.to(device)`,
 * experiments/train_modelnet.py:99) and the first layer's operand blocks (the `torch.cat([x, ...])` of deltaconv/nn/deltaconv.py:57,65).
 * srcs / dsts: HOST arrays of `count` device addresses (4-byte aligned); ld_src / ld_dst / rows / cols in 4-byte words. */
int dc_copy_many(const int64_t* srcs, const int64_t* dsts, const int64_t* ld_src, const int64_t* ld_dst, const int32_t* rows,
                 const int32_t* cols, int32_t count, void* stream);

/* ---- device-resident datasets: batch assembly and augmentation in one launch (csrc/batch.hip, csrc/batch_math.h) -------- */
/* Replaces the host side of the reference's input pipelines -- the per-shape `transform` of Dataset.__getitem__, the DataLoader's
 * collate and `data.to(device)`: experiments/train_modelnet.py:37-50,99, train_shapenet.py:36-50, train_scanobjectnn.py:47-62,
 * train_shapeseg.py:37-61, train_shrec.py:37-52.
 * The store holds the prepared dataset on the device: store_pos [Ns,3], store_norm [Ns,3] or NULL, store_x [Ns,F] or NULL,
 * labels store_y_point [Ns] or store_y_cloud [S] (at most one of them non-NULL), store_category [S,Cc] or NULL, offsets
 * store_ptr [S+1].  idx [B]: DEVICE array, the clouds of this batch in slot order.  B, Nt (= sum of their sizes) and max_cloud
 * (>= the largest of them) are known to the host; a workgroup finds the start of its cloud from the sizes of the slots before it.
 * Outputs: pos [Nt,3], norm [Nt,3], x [Nt,F], batch [Nt] (slot of every point), ptr [B+1], y [Nt] or [B], category [B,Cc]; an output
 * whose store counterpart is NULL is not touched (and may be NULL).  Indices outside [0, S) count as empty clouds; rows >= Nt
 * and points beyond max_cloud are never written.
 * Augmentation: op_codes [n_ops] / op_params [n_ops,3] are HOST arrays (n_ops <= 8), applied to every point in list order:
 *   1 scale          (lo, hi, -)           three factors per cloud; pos *= s; norm *= 1/s, re-normalised   (random_scale.py:24-35)
 *   2 rotate         (deg_lo, deg_hi, axis) one angle per cloud; pos @ R, norm @ R                          (random_rotate.py:28-45)
 *   3 translate      (tx, ty, tz)          one offset per cloud and axis, uniform in (-t, t)               (random_translate_global.py)
 *   4 normal jitter  (tx, ty, tz)          per point and axis; norm / max(|norm|, 1e-5)                    (random_normals.py:25-36)
 *   5 point jitter   (tx, ty, tz)          per point and axis, added to pos   (PyG RandomTranslate, train_scanobjectnn.py:49)
 * Draws: Philox-4x32-10, key (seed, 0x6261746B), counter (point in cloud | 0xFFFFFFFF for a per-cloud draw, DATASET index of the
 * cloud, step low word, step bits 32..60 << 3 | op position); output words x, y, z serve axes 0, 1, 2 (an angle: word x);
 * u = (r >> 8) * 2^-24, value = lo + u * (hi - lo) in fp32 without contraction; angle = degrees * (pi / 180) in fp32, sincosf.
 * seed in [0, 2^32), step in [0, 2^61).  A cloud's augmented rows do not depend on its slot or on the rest of the batch.
 * One launch, stream-ordered, capturable. */
int dc_batch_assemble(const float* store_pos, const float* store_norm, const float* store_x, int32_t F,
                      const int64_t* store_y_point, const int64_t* store_y_cloud, const float* store_category, int32_t Cc,
                      const int64_t* store_ptr, int64_t S, const int64_t* idx, int32_t B, int64_t Nt, int32_t max_cloud,
                      const int32_t* op_codes, const float* op_params, int32_t n_ops, int64_t seed, int64_t step, float* pos,
                      float* norm, float* x, int64_t* batch, int32_t* ptr, int64_t* y, float* category, void* stream);

/* ---- device-side evaluation: votes, arg-max, per-class counts and part IoU in one launch (csrc/eval.hip, csrc/eval_math.h) ---- */
/* Replaces the host side of the reference's test loops -- logits and labels copied to the host per batch, np.argmax, the Python
 * loop over shapes and parts: experiments/utils.py:27-51 (calc_shape_IoU), test_shapenet.py:84-103 (vote sum, arg-max, metrics).
 * logits [Nt,P] fp32 with row stride ld_logits >= P; y [Nt] labels; ptr [B+1] cloud offsets (values outside [0, Nt] are clamped).
 * One workgroup per cloud b = rows ptr[b] .. ptr[b+1]; classification is the same entry with the batch as one cloud (ptr = [0, B]).
 *   votes     NULL, or [Nt,P] contiguous: votes[r,c] += logits[r,c] (one fp32 add), and the predictions come from votes
 *   pred      NULL, or [Nt]: first index of the row maximum, numpy's argmax rule (a NaN is the maximum, the first NaN wins)
 *   cnt, hit  [B,P]: rows of the cloud labelled c, and those of them predicted c; a label outside [0, P) is in no class, is
 *             counted in ignored [B] and indexes nothing
 *   iou       NULL, or [B] fp64: the mean over the cloud's parts of (U == 0 ? 1 : I / U), I = #(pred == part and y == part),
 *             U = #(pred == part or y == part): integer counts, the divisions and the sum in part order in fp64.  The parts are
 *             part_start[k] .. part_start[k] + part_count[k] - 1 with k = arg-max of category [B,Cc] row b (part_start, part_count:
 *             DEVICE arrays [Cc]); category NULL: all P classes.  A part outside [0, P) has an empty union (counts as 1).
 * P in 1 .. 256 (else DC_ERR_ARG with a message); B = 0 returns DC_OK.  Integer counters in LDS, no global atomics, no
 * floating-point atomics: the outputs are a function of the inputs only.  One launch, stream-ordered, capturable. */
int dc_eval_metrics(const float* logits, int64_t ld_logits, float* votes, const int64_t* y, const int32_t* ptr, int32_t B,
                    int64_t Nt, int32_t P, const float* category, int32_t Cc, const int32_t* part_start,
                    const int32_t* part_count, int64_t* pred, double* iou, int32_t* hit, int32_t* cnt, int32_t* ignored,
                    void* stream);

/* ---- geodesic farthest-point sampling of a batch of clouds (csrc/fps.hip, csrc/fps_math.h) ---------------------------------- */
/* Bytes of workspace dc_geodesic_fps_batch needs for clouds of N points in all (the k = 10 graph: neighbours and fp64 edge
 * lengths, plus the uploaded offsets and start points).  Reference: deltaconv/transforms/geodesic_fps.py:14-43 and
 * deltaconv/cpp/sampling.cpp:5-81 (the graph of sampling.cpp:9-31 is the only state between its two stages). */
size_t dc_geodesic_fps_workspace_bytes(int64_t N);
/* Replaces the per-shape host call of the reference's data preparation -- deltaconv/transforms/geodesic_fps.py:14-43 over
 * deltaconv/cpp/sampling.cpp:5-81: the k = 10 nearest-neighbour graph of every cloud (fp64, the point itself left out by index,
 * ties towards the lower index), then n_samples - 1 rounds of "shortest graph distances from the last sample into a distance
 * vector that is never reset; the next sample is the FIRST index of its maximum" -- for B clouds in two launches.  The picks are
 * those of the host library (include/deltaconv_host.h: dc_geodesic_fps) started from the same point: rounds relax edges until
 * nothing changes instead of running Dijkstra, which reaches the same fp64 distances bit for bit (csrc/fps.hip).
 *   pos        DEVICE [N,3] contiguous, fp32 (pos_is_f64 = 0) or fp64 (1); fp32 is widened exactly, all arithmetic is fp64
 *   ptr        HOST [B+1] cloud offsets into pos, ptr[0] = 0, every cloud of 1 .. 16 384 points (DC_FPS_MAX_POINTS: the distance
 *              vector of a cloud lives in the LDS of one workgroup)
 *   max_cloud_size  >= the largest cloud, <= 16 384
 *   start      HOST [B] first sample of every cloud, local to the cloud
 *   out        DEVICE [B,n_samples] sample ids local to the cloud; n_samples above a cloud's size repeats index 0 once every
 *              point is taken (the host library does), a disconnected graph takes the first unreached point
 *   workspace  DEVICE, 8-byte aligned, >= dc_geodesic_fps_workspace_bytes(ptr[B]) bytes (else DC_ERR_WORKSPACE)
 * A cloud above the cap, an empty cloud, a start outside its cloud, n_samples < 1 or B above 65 535: DC_ERR_ARG with a message
 * (checked before anything touches the device); B = 0 returns DC_OK.  ptr and start are copied in stream order and may be freed on
 * return.  No global atomics, no floating-point atomics: the output is a function of the inputs only.  Stream-ordered. */
int dc_geodesic_fps_batch(const void* pos, int32_t pos_is_f64, const int64_t* ptr, int32_t B, int32_t max_cloud_size,
                          int32_t n_samples, const int32_t* start, int32_t* out, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Bytes of workspace dc_geodesic_fps_large needs for clouds of N points in all: dc_geodesic_fps_workspace_bytes(N) plus the
 * distance vectors, 8 N bytes, 256-byte aligned (140 bytes per point).  Reference: deltaconv/cpp/sampling.cpp:30-31 (the
 * distance vector the rounds of :42-50 keep lowering). */
size_t dc_geodesic_fps_large_workspace_bytes(int64_t N);
/* dc_geodesic_fps_batch for clouds above its cap -- the same per-shape host call of the reference's data preparation,
 * deltaconv/transforms/geodesic_fps.py:14-43 over deltaconv/cpp/sampling.cpp:5-81, which has no size limit: the same graph
 * launch, then a sampling kernel (one workgroup of 1 024 threads per cloud, every round inside the launch) that keeps the
 * distance vector in the workspace and only the two frontier bit sets in LDS.  Relaxations meet in unsigned 64-bit integer
 * minima at agent scope, and every later access to a distance is an agent-scope atomic load or store; a minimum does not depend
 * on the order of its operands, so the picks are still a function of the inputs only, and for a cloud both entries take they
 * are the same picks.  Arguments, checks and return codes as dc_geodesic_fps_batch, with
 *   ptr        every cloud of 1 .. 262 144 points (DC_FPS_LARGE_MAX_POINTS); any size from 1 up is taken, not only sizes
 *              above DC_FPS_MAX_POINTS
 *   max_cloud_size  >= the largest cloud, <= 262 144
 *   workspace  DEVICE, 8-byte aligned, >= dc_geodesic_fps_large_workspace_bytes(ptr[B]) bytes (else DC_ERR_WORKSPACE)
 * No floating-point atomics.  Stream-ordered. */
int dc_geodesic_fps_large(const void* pos, int32_t pos_is_f64, const int64_t* ptr, int32_t B, int32_t max_cloud_size,
                          int32_t n_samples, const int32_t* start, int32_t* out, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- Euclidean farthest-point sampling inside the step (csrc/fps_euclid.hip, csrc/fps_euclid_math.h) -------------------------- */
/* What torch_cluster.fps(pos, batch, ratio) and the set abstraction of PointNet++ do, for B clouds in ONE launch that reads
 * nothing on the host (the reference ships only the geodesic sampler of its data preparation, deltaconv/transforms/
 * geodesic_fps.py:14-43; its multi-resolution hint is experiments/train_shapenet.py:32).  Rules (csrc/fps_euclid_math.h): the
 * contract's fp32 distance (dx*dx + dy*dy) + dz*dz, every operation rounded on its own; a running minimum per point; the next
 * pick is the FIRST index of its maximum; a point with a non-finite coordinate is picked only after every finite one, in
 * ascending id.  The picks are pairwise distinct and a function of the inputs only; the first m' picks of m are the m'-pick sample.
 *   pos        DEVICE [N,3] contiguous fp32
 *   ptr        DEVICE [B+1] ABSOLUTE row offsets of the clouds into pos
 *   optr       DEVICE [B+1] offsets into rows: cloud b asks for optr[b+1] - optr[b] picks (at most max_samples are written)
 *   max_cloud  HOST: >= the largest cloud, <= 16 384 (DC_FPS_EUCLID_MAX_POINTS: a cloud's positions and minima live in the
 *              registers of one workgroup); it alone picks the kernel instance.  Of a larger cloud only the first rows are sampled
 *   max_samples  HOST: >= the most picks any cloud asks for
 *   start      DEVICE [B] first pick of every cloud, local to the cloud, or NULL for row 0; an id outside its cloud is read as 0
 *   rows       DEVICE [optr[B]]: rows[optr[b] + r] = ptr[b] + pick_r, a GLOBAL row id, in pick order; a pick index r at or above
 *              the cloud's size gets -1
 * A null pointer (pos, ptr, optr, rows), B < 0, max_samples < 0 or max_cloud outside 0 .. 16 384: DC_ERR_ARG with a message;
 * B = 0 returns DC_OK.  No workspace, no atomics; launch sizes depend on B and max_cloud alone, so the call can be captured and a
 * captured call replays on positions written in place.  Stream-ordered. */
int dc_fps_batch(const float* pos, const int64_t* ptr, const int64_t* optr, int32_t B, int32_t max_cloud, int32_t max_samples,
                 const int32_t* start, int64_t* rows, void* stream);

/* ---- exact Euclidean farthest-point sampling on a cell grid, for large clouds (csrc/fps_grid.hip, csrc/fps_grid_math.h) ---------- */
/* The workspace of one dc_fps_grid call: a function of the sizes alone, linear -- the grid build of dc_knn_grid
 * (dc_knn_grid_workspace_bytes: about 48 bytes a point), 4 bytes of md a point and one 8-byte key for each of the
 * 2 * num_points + num_clouds cells: about 68 bytes a point.
 *   num_points  HOST: all points of the call, ptr[B] - ptr[0]
 * 0: a negative size or more than 2^31 - 1 points. */
size_t dc_fps_grid_workspace_bytes(int64_t num_points, int32_t num_clouds);
/* dc_fps_batch for clouds of up to DC_FPS_GRID_MAX_POINTS = 262 144 points: the SAME picks, bit for bit, found on a uniform cell
 * grid.  A pick updates only the points of the cells within Chebyshev distance R of its own, R the smallest radius whose bound
 * (csrc/knn_grid_math.h: bound2) reaches the md the pick held when it was selected; no other point could change.  The rule, its
 * proof and a serial reference: csrc/fps_grid_math.h.  pos, ptr, optr, max_samples, start and rows are dc_fps_batch's.
 *   max_cloud  HOST: >= the largest cloud, <= DC_FPS_GRID_MAX_POINTS; it sizes the LDS table of the launch.  A cloud LARGER than
 *              max_cloud claims, or one that does not lie inside the workspace's capacity, is not sampled: every one of its rows
 *              gets -1 and its stats are 0 (nothing is read or written out of bounds)
 *   target     HOST: the wanted mean number of points per cell (csrc/knn_grid_math.h: make_grid); any positive finite value
 *              gives the same picks, it only moves the time and the stats
 *   stats      DEVICE [B,2] int64 or NULL: per cloud the number of point updates evaluated, summed over its picks (the population
 *              of every pick's box), and the number of cells in those boxes -- functions of the inputs and the target alone
 *   workspace  DEVICE, 16-byte aligned, workspace_bytes >= dc_fps_grid_workspace_bytes(all points of the call, B)
 * One workgroup per cloud; nothing is handed between workgroups.  A null pointer (pos, ptr, optr, rows, workspace), B < 0,
 * max_samples < 0, max_cloud outside 0 .. DC_FPS_GRID_MAX_POINTS, a target that is not positive and finite, a misaligned or too
 * small workspace: DC_ERR_ARG with a message; B = 0 returns DC_OK.  Integer atomics in the grid build only, no floating-point
 * atomics; six launches whose sizes depend on B, max_cloud and workspace_bytes alone, so the call can be captured and a captured
 * call replays on positions written in place.  Stream-ordered. */
int dc_fps_grid(const float* pos, const int64_t* ptr, const int64_t* optr, int32_t B, int32_t max_cloud, int32_t max_samples,
                const int32_t* start, float target, int64_t* rows, int64_t* stats, void* workspace, size_t workspace_bytes,
                void* stream);

/* ---- voxel-grid subsampling of device-resident clouds (csrc/voxel.hip, csrc/voxel_math.h) --------------------------------------- */
/* The workspace of one dc_voxel_subsample call: a function of the sizes alone, linear -- 2 * num_points + num_clouds table slots of
 * 16 bytes, the scan of num_points + 1 entries (+ its block sums), 12 bytes of origin per cloud: about 40 bytes a point.
 * 0: a negative size, more than 2^31 - 1 points or more than 2^24 clouds. */
size_t dc_voxel_subsample_workspace_bytes(int64_t num_points, int32_t num_clouds);
/* What torch_cluster.grid_cluster / torch_geometric.nn.voxel_grid followed by consecutive_cluster compute, plus a representative
 * per cell: one point per occupied cell of edge `size` of every cloud, and for every point the output row of its cell.  The rules
 * (csrc/voxel_math.h): a point takes part iff its coordinates are finite; the origin of a cloud is the fp32 minimum over ITS finite
 * points (a cloud's result does not depend on its batch-mates) or the caller's; per axis the cell is floorf(fl(fl(p - o) / s));
 * the representative of a cell is the member with the smallest key (bits(d2) << 32 | local index), d2 the contract's fp32
 * (dx*dx + dy*dy) + dz*dz to the cell centre fl(fl(fl(t + 0.5) * s) + o) (pick 0) or 0 (pick 1: the first member); the
 * representatives of a cloud come in ascending row order.  A function of the inputs only: the same bits on every run.
 *   pos         DEVICE [num_points,3] contiguous fp32
 *   ptr         DEVICE [B+1] row offsets of the clouds into pos; rows outside every cloud belong to no cell
 *   num_points  HOST: the rows of pos (it sizes the workspace and, with B, every launch);  B <= 2^24
 *   size_x/y/z  HOST: the edge lengths, positive and finite
 *   origin      DEVICE [B,3] fp32, or NULL for every cloud's own minimum
 *   pick        HOST: 0 = the member nearest the cell centre, 1 = the first member
 *   rows        DEVICE [num_points] (capacity; scratch of the scan until the last launch): the first info[0] entries are the
 *               representatives' rows of pos, clouds in order, ascending inside a cloud
 *   optr        DEVICE [B+1]: cloud b's representatives are rows[optr[b] .. optr[b+1])
 *   cluster     DEVICE [num_points]: the output row of the point's cell (rows[cluster[i]] is i's representative), -1 for a point
 *               that belongs to no cell
 *   info        DEVICE [4]: [0] the output rows in all; [1] the first cloud with a finite point whose cell index reaches 2^20 in
 *               magnitude on some axis (its cell does not pack into 63 bits; such a point gets no cell and the outputs are not to
 *               be used), -1 for none; [2] non-zero if a cloud's table slice ran out (cannot happen for offsets that ascend);
 *               [3] 0
 *   workspace   DEVICE, 16-byte aligned, workspace_bytes >= dc_voxel_subsample_workspace_bytes(num_points, B)
 * A null pointer, a size that is not positive and finite, pick outside {0, 1}, B or num_points out of range, a workspace that is
 * missing, misaligned or too small: DC_ERR_ARG with a message, before anything touches the device.  Seven launches (six with an
 * origin) whose sizes depend on num_points and B alone, stream-ordered, no allocation, no synchronisation; 64-bit integer atomics
 * (compare-and-swap on cells, minimum on keys) in an open-addressing table of which every cloud owns a slice -- the probe loop is
 * bounded by the slice and never waits on another thread, and table collisions cannot reach the outputs. */
int dc_voxel_subsample(const float* pos, const int64_t* ptr, int32_t B, int64_t num_points, float size_x, float size_y,
                       float size_z, const float* origin, int32_t pick, int64_t* rows, int64_t* optr, int64_t* cluster,
                       int64_t* info, void* workspace, size_t workspace_bytes, void* stream);

/* ---- pooling over the cells of a cluster vector (csrc/cluster.hip, csrc/cluster_math.h) ----------------------------------------- */
/* The workspace of one dc_cluster_lists call: counters / fill cursors [num_cells], the scan's block sums and the unordered fill
 * [num_points], 8 bytes each -- linear.  0: a negative size, or more than 2^31 - 1 points or cells. */
size_t dc_cluster_lists_workspace_bytes(int64_t num_points, int64_t num_cells);
/* The member lists of a cluster vector -- the CSR form of torch_scatter's index: row i belongs to cell cluster[i] iff
 * 0 <= cluster[i] < num_cells; any other value (-1: dc_voxel_subsample's "no cell") belongs to none.
 *   cluster     DEVICE int64 [num_points]: dc_voxel_subsample's, or the caller's
 *   cptr        DEVICE int64 [num_cells + 1]: cell j's rows are members[cptr[j] .. cptr[j+1]); cptr[num_cells] = the rows with a cell
 *   members     DEVICE int64 [num_points]: the rows of every cell in ASCENDING order; entries from cptr[num_cells] on are -1
 *   workspace   DEVICE, 8-byte aligned, workspace_bytes >= dc_cluster_lists_workspace_bytes(num_points, num_cells)
 * Count (integer atomics), scan (list_scan.h), unordered fill, then a ranking pass with one thread per fill position: six launches
 * whose sizes depend on num_points and num_cells alone, stream-ordered, no allocation, no synchronisation -- capturable, and a
 * captured call replays on a cluster vector written in place.  Only the place of a row in the unordered fill depends on the race,
 * and the ranks do not: the same bits on every run.  The ranking is QUADRATIC in a list's length (a cell that holds all 262 144
 * rows of a call: 262 144 compares per thread -- slow, not a hang).  Sizes out of range, a null pointer, a workspace that is
 * missing, misaligned or too small: DC_ERR_ARG with a message. */
int dc_cluster_lists(const int64_t* cluster, int64_t num_points, int64_t num_cells, int64_t* cptr, int64_t* members,
                     void* workspace, size_t workspace_bytes, void* stream);
/* torch_scatter.scatter(x, cluster, reduce = "max" | "min" | "sum" | "mean") / torch_geometric's max_pool, avg_pool_x over the lists
 * of dc_cluster_lists, by the rules of csrc/cluster_math.h: the members of a cell in ascending row order, the first copied bit for
 * bit, a later one taken iff strictly larger / smaller (ties keep the lower row, a later NaN is never taken, a first NaN stays) or
 * added with every addition rounded on its own; the mean divides once by the member count; an empty cell gives zeros.
 *   x           DEVICE [num_points, C] fp32, rows ldx >= C apart; C >= 1 (16-byte loads where x, ldx and C allow, scalar otherwise)
 *   mode        0 max, 1 min, 2 sum, 3 mean (the codes of dc_seg_reduce)
 *   out         DEVICE [num_cells, C] fp32, rows ldo apart: every row is written
 *   arg         DEVICE int32 [num_cells, C], rows ldarg apart (max / min; may be NULL for sum / mean, which do not write it): the ROW
 *               of x every channel came from, -1 for an empty cell
 * num_points and num_cells below 2^31, else DC_ERR_ARG (as a bad mode, a leading dimension below C, a null pointer).  One thread
 * per (cell, group of 4 channels), one launch, no atomics, no synchronisation: a function of the inputs only. */
int dc_cluster_pool(const float* x, int64_t ldx, int64_t num_points, int32_t C, const int64_t* cptr, const int64_t* members,
                    int64_t num_cells, int32_t mode, float* out, int64_t ldo, int32_t* arg, int64_t ldarg, void* stream);
/* The gradient of dc_cluster_pool w.r.t. x: every point belongs to one cell, so it is a gather -- one thread per (point, group of 4
 * channels).  max / min: dx[i,c] = arg[cl,c] == i ? g[cl,c] : 0; sum: g[cl,c]; mean: g[cl,c] / (float)(cptr[cl+1] - cptr[cl]), the
 * quotient rounded on its own (as dc_knn_pool_backward's term); a point without a cell gets zeros.  Every row of dx is written.
 *   g           DEVICE [num_cells, C] fp32, rows ldg apart;  cluster  DEVICE int64 [num_points]
 *   cptr        DEVICE int64 [num_cells + 1], read by the mean only (may be NULL otherwise)
 *   arg, ldarg  what dc_cluster_pool wrote; may be NULL for sum / mean
 *   dx          DEVICE [num_points, C] fp32, rows ldx apart
 * The checks of dc_cluster_pool: DC_ERR_ARG.  One launch, no atomics, no synchronisation. */
int dc_cluster_pool_backward(const float* g, int64_t ldg, int64_t num_cells, int32_t C, const int64_t* cluster, int64_t num_points,
                             const int64_t* cptr, const int32_t* arg, int64_t ldarg, int32_t mode, float* dx, int64_t ldx,
                             void* stream);
/* The un-pooling out[i] = x[cluster[i]] (zeros for a point without a cell): x [num_cells, C] -> out [num_points, C].  Its gradient
 * w.r.t. x is dc_cluster_pool in sum mode over the lists: the ordered, atomics-free index_add_.  One launch. */
int dc_cluster_gather(const float* x, int64_t ldx, int64_t num_cells, int32_t C, const int64_t* cluster, int64_t num_points,
                      float* out, int64_t ldo, void* stream);
/* torch_geometric's pool_pos, held to fp64: per cell the sum of its [num_points,3] fp32 rows in member order in fp64, ONE fp64
 * division by the count and ONE rounding to fp32 (an fp32 chain loses the low bits of a cloud shifted by 4 096).  normalize = 1
 * (normals): the fp64 sum divided by its fp64 norm instead, zeros where that norm is zero or not finite.  An empty cell gives zeros.
 *   p  DEVICE [num_points,3] contiguous fp32;  out  DEVICE [num_cells,3] contiguous fp32.  One thread per cell, one launch. */
int dc_cluster_mean3(const float* p, int64_t num_points, const int64_t* cptr, const int64_t* members, int64_t num_cells,
                     int32_t normalize, float* out, void* stream);
/* Per cell the label with the most members, ties to the lowest label; labels outside [0, num_classes) are ignored; a cell without
 * a valid label gets -1.  Integer counting only: per cell the classes between its smallest and largest label times its members.
 *   labels  DEVICE int64 [num_points];  num_classes in [1, 1024], else DC_ERR_ARG;  out  DEVICE int64 [num_cells].  One launch. */
int dc_cluster_majority(const int64_t* labels, int64_t num_points, const int64_t* cptr, const int64_t* members, int64_t num_cells,
                        int32_t num_classes, int64_t* out, void* stream);

/* ---- pooling of tangent-vector features over the cells of a cluster vector (csrc/cluster_vectors.hip, cluster_vectors_math.h) ---- */
/* geometry.cluster_rotation / ClusterPair.rotation: the per-POINT table of parallel transports between every point's frame and the
 * frame of its cell (deltaconv/geometry/connection.py:6-47 as dcconn::transport), 16 bytes per point.
 *   cluster     DEVICE int64 [num_points]; a value outside [0, num_cells) names no cell: four +0.0f
 *   fine_*      DEVICE [num_points,3] contiguous fp32: normal, x-axis, y-axis of the points' frames
 *   coarse_*    DEVICE [num_cells,3] contiguous fp32: those of the cells' frames
 *   to_cell     1 ("down"): entry i = transport(target: cell frame (n, x, y), source: point frame (n, x)); fine_y is not read and may
 *               be NULL.  0 ("up"): entry i = transport(target: point frame (n, x, y), source: cell frame (n, x)); coarse_y may be NULL
 *   rmat        DEVICE [num_points,4] fp32, 16-byte aligned, row-major 2 x 2
 * Sizes out of range, to_cell outside {0, 1}, a null or misaligned pointer: DC_ERR_ARG.  One thread per point, one launch. */
int dc_cluster_rotation(const int64_t* cluster, int64_t num_points, int64_t num_cells, const float* fine_normal, const float* fine_x,
                        const float* fine_y, const float* coarse_normal, const float* coarse_x, const float* coarse_y,
                        int32_t to_cell, int32_t non_oriented, float* rmat, void* stream);
/* geometry.cluster_pool_vectors_rows / ClusterPair.down_vectors: v [2 num_points, C] (rows 2i, 2i+1 = the coefficients at point i
 * in ITS frame) reduced over the lists of dc_cluster_lists, every member first carried into the cell's frame by rmat (the "down"
 * table), by the rules of csrc/cluster_vectors_math.h: members in ascending row order; sum (au + R00 v0) + R01 v1 from +0, mean the
 * sum divided once by the count, max per channel the transported vector of the member of largest squared norm (the first member, a
 * later one iff strictly larger); an empty cell gives zeros.
 *   mode        0 max, 2 sum, 3 mean (1, min, has no vector analogue: DC_ERR_ARG)
 *   out         DEVICE [2 num_cells, C] fp32, rows ldo apart: every row is written
 *   arg         DEVICE int32 [num_cells, C], rows ldarg apart (max; may be NULL for sum / mean, which do not write it): the ROW i
 *               every channel came from, -1 for an empty cell
 * The checks of dc_cluster_pool, and a misaligned rmat: DC_ERR_ARG.  One thread per (cell, group of 4 channels), four members in
 * flight, 16-byte loads where v, ldv and C allow; one launch, no atomics, no synchronisation. */
int dc_cluster_pool_vectors(const float* v, int64_t ldv, int64_t num_points, int32_t C, const int64_t* cptr, const int64_t* members,
                            int64_t num_cells, const float* rmat, int32_t mode, float* out, int64_t ldo, int32_t* arg, int64_t ldarg,
                            void* stream);
/* geometry.cluster_pool_vectors_rows_backward: the gradient of dc_cluster_pool_vectors w.r.t. v, a gather -- one thread per (point,
 * group of 4 channels): with cl = cluster[i], R = rmat[i] (the same "down" table), g0 / g1 rows 2cl, 2cl+1 of g:
 * du = R00 g0 + R10 g1, dw = R01 g0 + R11 g1 -- always (sum), with g0, g1 first divided by (float)(cptr[cl+1] - cptr[cl]) (mean), or
 * where arg[cl,ch] == i and +0 elsewhere (max).  A point without a cell gets zeros; every row of dv is written.
 *   g   DEVICE [2 num_cells, C] fp32, rows ldg apart;  cptr  read by the mean only;  arg, ldarg  what the forward wrote (max)
 *   dv  DEVICE [2 num_points, C] fp32, rows ldv apart
 * DC_ERR_ARG as above.  One launch, no atomics. */
int dc_cluster_pool_vectors_backward(const float* g, int64_t ldg, int64_t num_cells, int32_t C, const int64_t* cluster,
                                     int64_t num_points, const int64_t* cptr, const float* rmat, const int32_t* arg, int64_t ldarg,
                                     int32_t mode, float* dv, int64_t ldv, void* stream);
/* geometry.cluster_unpool_vectors_rows / ClusterPair.up_vectors: the cells' vectors x [2 num_cells, C] carried into every member's
 * frame: out[2i] = R00 x0 + R01 x1, out[2i+1] = R10 x0 + R11 x1 with R = rmat[i] (the "up" table) and x0 / x1 rows 2cl, 2cl+1; zeros
 * for a point without a cell.  out [2 num_points, C].  The same gather kernel through R as it stands.  One launch. */
int dc_cluster_unpool_vectors(const float* x, int64_t ldx, int64_t num_cells, int32_t C, const int64_t* cluster, int64_t num_points,
                              const float* rmat, float* out, int64_t ldo, void* stream);
/* geometry.cluster_unpool_vectors_rows_backward: the gradient of dc_cluster_unpool_vectors w.r.t. x: per cell its members in
 * ascending order from +0, R = rmat[i] (the "up" table), g0 / g1 rows 2i, 2i+1 of g [2 num_points, C]:
 * du = (du + R00 g0) + R10 g1, dw = (dw + R01 g0) + R11 g1 -> dx [2 num_cells, C]; an empty cell gets zeros.  The walk kernel of
 * dc_cluster_pool_vectors in sum mode through the transposed matrices: ordered, atomics-free.  One launch. */
int dc_cluster_unpool_vectors_backward(const float* g, int64_t ldg, int64_t num_points, int32_t C, const int64_t* cptr,
                                       const int64_t* members, int64_t num_cells, const float* rmat, float* dx, int64_t ldx,
                                       void* stream);

/* ---- surface sampling of a batch of triangle meshes (csrc/mesh.hip, csrc/mesh_math.h) ------------------------------------------ */
/* Bytes of workspace dc_mesh_sample needs for meshes of F_total faces in all: the cdf, 8 bytes per face.  Reference:
 * deltaconv/transforms/sample_points.py:22-59 (the area vector of :29-32 is the only state between its stages). */
size_t dc_mesh_sample_workspace_bytes(int64_t F_total);
/* Faces one iteration of the cdf kernel's workgroup scan covers: the sizes around which its tests are placed. */
int32_t dc_mesh_scan_faces(void);
/* Replaces the per-shape host call in front of GeodesicFPS in the reference's data preparation -- deltaconv/transforms/
 * sample_points.py:22-59 as called by experiments/train_modelnet.py:30-34, train_shrec.py:30-34 and train_shapeseg.py:28-34:
 * `num` points on the surface of each of B meshes, faces drawn with a probability proportional to their area, uniform barycentric
 * coordinates with the fold of :36-38, the point as (p0 + f1 e1) + f2 e2 (:46-48), the normal by F.normalize of e1 x e2 (:41-44),
 * the label of corner 0 (:53-54).  Areas are fp64 and cut to integer weights in [0, 2^32] relative to the mesh's largest face;
 * the cdf is their uint64 running sum and a draw picks the first face whose cdf exceeds (u * total) >> 64 -- integer and
 * order-free, so the picks are a function of (mesh, seed, round, dataset index, sample index) only (csrc/mesh_math.h); the
 * division by pos.max() of :26-27 is not restated.  Draws: Philox-4x32-10, key (seed, 0x6D657368), counter (sample index,
 * first_mesh_index + b, round lo, round hi): a mesh's sample does not depend on how meshes are grouped into calls.
 *   vert       DEVICE [Vs,3] fp32 vertex rows of the store
 *   face       DEVICE [Fs,3] vertex ids LOCAL to the mesh, one row per triangle; a row with an id outside [0, V) has weight 0 and
 *              is never indexed
 *   vptr, fptr DEVICE [B+1] ABSOLUTE row offsets of the B meshes of this call into vert / face (a slice of the store's offsets)
 *   y_vert     DEVICE [Vs] per-vertex labels, or NULL (required for y)
 *   pos        DEVICE [B*num,3]; norm [B*num,3], y [B*num], face_id [B*num] (local to the mesh) or NULL
 *   total      DEVICE [B] or NULL: the sum of a mesh's weights; 0 = every face degenerate (such a mesh is sampled uniformly
 *              by face index), -1 = the mesh's cdf did not fit the workspace (the mesh is skipped: zero rows, face_id -1)
 *   workspace  DEVICE, 8-byte aligned, dc_mesh_sample_workspace_bytes(fptr[B] - fptr[0]) bytes; it holds the cdf on return,
 *              mesh b at element fptr[b] - fptr[0]
 * num < 1, B above 65 535, seed outside [0, 2^32), a negative round, dataset indices past 2^32 or y without y_vert: DC_ERR_ARG; a
 * workspace below 8 bytes per mesh: DC_ERR_WORKSPACE; both with a message, checked before anything touches the device.  The
 * offsets are device arrays, so the face count itself is held to the workspace by the kernels (total = -1 above).  B = 0
 * returns DC_OK.  A mesh has at most 2^24 faces (the caller's to check: total < 2^57).  Two launches, stream-ordered, no
 * allocation, no synchronisation, no atomics: the outputs are a function of the inputs only. */
int dc_mesh_sample(const float* vert, const int32_t* face, const int64_t* vptr, const int64_t* fptr, int32_t B,
                   int64_t first_mesh_index, int32_t num, int64_t seed, int64_t round, const int64_t* y_vert,
                   float* pos, float* norm, int64_t* y, int32_t* face_id, int64_t* total,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-shape normalisation of a store of clouds or meshes (csrc/shape_norm.hip, csrc/shape_norm_math.h) ------------------------ */
/* Threads of the workgroup that reduces one shape: the fixed order of the fp64 sums depends on it (csrc/shape_norm_math.h), and the
 * tests place their shape sizes around it. */
int32_t dc_shape_normalize_threads(void);
/* Replaces the per-shape host calls at the head of the reference's pre_transform -- deltaconv/transforms/normalize_scale.py:12-21
 * (experiments/train_modelnet.py:30-34, train_shapenet.py:30-33), normalize_area.py:12-20 and normalize_axes.py:17-26
 * (train_shapeseg.py:28-34): a chain of 1 to 4 ops applied to each of B shapes of a concatenated store.  Every op maps fp32 rows to
 * fp32 rows and the next op sees the rounded result, as the host Compose does.
 *   1 scale  (norm_ord, scaling_factor)  centre on the bounding-box middle, multiply by fl32(fl32(1 / ref) * 0.999999f); ref = the
 *            largest row norm of the centred shape (norm_ord 2: fl32 of the fp64 square root; +inf: the largest |coordinate|), or
 *            the scaling_factor where that is not NaN
 *   2 area   (-, -)   centre, multiply by fl32(1 / sqrt(S / 2)), S the fp64 sum over the shape's face rows of the sampler's doubled
 *            face area (csrc/mesh_math.h) in a fixed order that is a function of the shape alone; a face with an id outside
 *            [0, V) counts 0.  This is the surface area over face ROWS, transforms.NormalizeArea on Data(pos, face=[F,3]);
 *            normalize_area.py indexes data.face[:, 1], which on the [3,F] faces of its dataset reads the ids of face 1 -- in the
 *            ShapeSeg recipe NormalizeAxes follows and rescales uniformly, so only the centring survives and the two agree
 *   3 axes   (-, -)   columns in the stable order of ascending unbiased variance (fp64 sums of x and x*x in the same fixed order; a
 *            tie or a NaN keeps the lower axis first, one row keeps the identity), multiply by fl32(1 / fl32(2 * max)) of the last
 * The centre is fl32(fl32(max + min) / 2) per axis; all of it is csrc/shape_norm_math.h, which a numpy restatement reproduces bit
 * for bit.  Non-finite arithmetic follows IEEE (a zero-area shape gets an infinite scale); nothing is clamped.
 *   pos        DEVICE [N,3] fp32 rows of the store; ptr DEVICE [B+1] ABSOLUTE row offsets of the B shapes of this call (a slice of
 *              the store's offsets); n_rows HOST = ptr[B] - ptr[0]: it sizes the grid only (rows past ptr[B] are not touched)
 *   face, fptr DEVICE [Fs,3] vertex ids LOCAL to the shape and [B+1] ABSOLUTE offsets, the layout of dc_mesh_sample; NULL
 *              unless the chain has an area op
 *   op_codes   HOST [n_ops]; op_params HOST [n_ops,2]
 *   pos_out    DEVICE [N,3], the same rows; may alias pos
 *   norm       NULL, or DEVICE [N,3], in and out: an axes op permutes its columns as it permutes the positions (uniform scaling
 *              leaves unit normals alone).  The reference has no normals at this point: an extension.  Not touched without an axes op
 *   stats      NULL, or DEVICE [B,n_ops,8] fp32 per shape and op: centre 3, scale 1, permutation 3 (as floats), 0.  It is the
 *              table the second launch reads; without it the table lives in workspace (DEVICE, 32 * B * n_ops bytes)
 * An unknown op, n_ops outside 1 .. 4, B above 65 535, an area op without face / fptr, a norm_ord other than 2 or +inf: DC_ERR_ARG;
 * neither stats nor a workspace that holds the table: DC_ERR_WORKSPACE; both with a message, checked before anything touches the
 * device.  B = 0 returns DC_OK.  Two launches (one workgroup per shape builds the table, a grid over the rows of the call applies
 * the chain), stream-ordered, capturable, no allocation, no synchronisation, no atomics: the outputs are a function of the
 * inputs only. */
int dc_shape_normalize(const float* pos, const int64_t* ptr, const int32_t* face, const int64_t* fptr, int32_t B, int64_t n_rows,
                       const int32_t* op_codes, const float* op_params, int32_t n_ops, float* pos_out, float* norm, float* stats,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- propagation from a sampled cloud back to its source: two-set kNN and interpolation (csrc/interp.hip, csrc/interp_math.h) -- */
/* Replaces torch_cluster.knn(x, y, k, batch_x, batch_y) as torch_geometric.nn.knn_interpolate calls it: for each of B cloud
 * pairs, the k nearest REFERENCE points of every QUERY point.  The result carries no gradient: positions and distances are not
 * differentiated (dc_knn_interpolate_backward below is the gradient w.r.t. the interpolated features only).
 * Order (the contract of dc_knn): fp32 ((dx*dx+dy*dy)+dz*dz) without contraction, ascending, ties by lower reference index.
 *   query, ref  DEVICE [*,3] fp32 rows
 *   qptr, rptr  DEVICE [B+1] ABSOLUTE row offsets of the B clouds into query / ref (a slice of a store's offsets serves)
 *   max_query_cloud  HOST, >= the largest query cloud: it sizes the grid only (queries past it are not searched)
 *   idx         DEVICE [*,k] int32, row qptr[b] + i: reference ids LOCAL to the pair's reference cloud, -1 = no such neighbour
 *   d2          DEVICE [*,k] fp32: the value that decided the order, +inf where idx is -1
 * A reference cloud of fewer than k points (0 included) fills its first slots and pads with -1 / +inf.  A candidate whose
 * distance is not below +inf -- a NaN coordinate on either side, or an overflow -- is never picked; nothing is indexed out of
 * the ranges the offsets give.  k outside 1 .. 16, B above 65 535, max_query_cloud outside [0, 2^39) (the grid: at most 2^31 - 1
 * chunks of 256 queries) or a null pointer: DC_ERR_ARG with a message, checked before anything touches the device; B = 0 or
 * max_query_cloud = 0 returns DC_OK.  One launch, stream-ordered, no allocation, no
 * synchronisation, no atomics, capturable: the outputs are a function of the inputs only. */
int dc_knn_cross(const float* query, const int64_t* qptr, const float* ref, const int64_t* rptr, int32_t B,
                 int64_t max_query_cloud, int32_t k, int32_t* idx, float* d2, void* stream);
/* Replaces the arithmetic of torch_geometric.nn.knn_interpolate (PointNet++ feature propagation) on the result of dc_knn_cross:
 * out[qptr[b] + i, c] = sum_s w_s x[rptr[b] + idx_s, c] / sum_s w_s with w_s = 1.0f / fmaxf(d2_s, 1e-16f) (PyG's clamp), fp32,
 * slots in order s = 0 .. k-1, every operation rounded on its own, one division per channel (csrc/interp_math.h).  A slot with
 * idx outside [0, size of the reference cloud) is skipped and indexes nothing; a query with exactly one valid slot gets that row
 * copied bit for bit (k = 1 is an exact gather), one with no valid slot a row of zeros.  Backward w.r.t. x:
 * dc_knn_cross_transpose + dc_knn_interpolate_backward; none w.r.t. positions or distances.
 *   x           DEVICE [*,ldx] fp32 reference rows, C <= ldx; out DEVICE [*,ldo] fp32, C <= ldo
 *   qptr, rptr, max_query_cloud, k, idx, d2   as in dc_knn_cross (the same grid: chunks of 256 queries x cloud pairs)
 * 16-byte loads / stores where the base pointer and the leading dimension allow, scalar otherwise: any C >= 1, the same bits.
 * k outside 1 .. 16, C outside 1 .. 2^20 (a block counts its 256 queries x C/4 channel groups in 32 bits), ldx or ldo below C, B above
 * 65 535, max_query_cloud outside [0, 2^39) (the bound of dc_knn_cross: the same grid) or a null pointer: DC_ERR_ARG with a
 * message, checked before anything touches the device; B = 0 or max_query_cloud = 0 returns DC_OK.  One launch, stream-ordered, no allocation, no synchronisation, no atomics,
 * capturable. */
int dc_knn_interpolate(const float* x, int64_t ldx, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B,
                       int64_t max_query_cloud, int32_t k, const int32_t* idx, const float* d2, float* out, int64_t ldo,
                       void* stream);

/* Replaces what autograd records for torch_geometric.nn.knn_interpolate's gather (y = x[idx]: an index_add_ with floating-point
 * atomics in the backward): the TRANSPOSED lists of a dc_knn_cross result, built once per search.  For every reference row r of
 * the call (ABSOLUTE, as x is indexed: rptr[b] + j), its in-edges: all (q, s) of ITS pair with a valid slot idx[q, s] == j
 * (0 <= idx < size of the reference cloud), named e = q * k + s with q the ABSOLUTE query row (the row of idx / d2), in
 * ASCENDING e, and the coefficient of each (csrc/interp_math.h: 1.0f for the only valid slot of a query, else w_s / den with the
 * forward's den bits).
 *   qptr, rptr  DEVICE [B+1] ABSOLUTE row offsets, as in dc_knn_cross; any B >= 0 (nothing is gridded over the pairs)
 *   num_query   HOST: the rows of idx / d2 (>= qptr[B]); rows outside every pair have no edge.  num_ref  HOST: the rows of x
 *               (>= rptr[B]); a slot that would land past it is dropped
 *   tptr        DEVICE int64 [num_ref + 1], every entry written: the list of row r is [tptr[r], tptr[r+1]); tptr[num_ref] = the
 *               number of valid slots of the call
 *   tedge       DEVICE int64 [num_query * k] (the first tptr[num_ref] entries are written); tcoef fp32, the same positions
 *   workspace   DEVICE, 8-byte aligned, dc_knn_cross_transpose_workspace_bytes(num_query, num_ref, k) bytes (0: sizes out of range)
 * Count (integer atomics), scan, unordered fill (integer atomic cursors), then a ranking pass that sorts every list, one fill
 * position per thread: the outputs are a function of the inputs only.  No floating-point atomics.  k outside 1 .. 16, a negative B or
 * size, num_query * k above 2^39 - 256, a null pointer or a workspace that is null, misaligned or too small: DC_ERR_ARG with a
 * message, checked before anything touches the device.  Six launches, stream-ordered, no allocation, no synchronisation,
 * capturable. */
size_t dc_knn_cross_transpose_workspace_bytes(int64_t num_query, int64_t num_ref, int32_t k);
int dc_knn_cross_transpose(const int64_t* qptr, const int64_t* rptr, int32_t B, int64_t num_query, int64_t num_ref, int32_t k,
                           const int32_t* idx, const float* d2, int64_t* tptr, int64_t* tedge, float* tcoef, void* workspace,
                           size_t workspace_bytes, void* stream);
/* Replaces the backward of torch_geometric.nn.knn_interpolate w.r.t. x (autograd's index_add_ of the weighted rows: floating-point
 * atomics, no run-to-run guarantee) on the lists of dc_knn_cross_transpose: dx[r, c] = 0, then for every in-edge of r in ascending order
 * dx = dx + tcoef * g[e / k - edge_base, c], product and sum each rounded on their own (csrc/interp_math.h).  Every reference row
 * of every pair of the call is written (a row without in-edges gets zeros): no fill pass is needed.  No gradient w.r.t. positions
 * or distances exists.
 *   g           DEVICE [num_g_rows, ldg] fp32, the gradient of the interpolated rows, C <= ldg; an edge whose row
 *               e / k - edge_base falls outside [0, num_g_rows) is skipped
 *   rptr        DEVICE [B+1] ABSOLUTE row offsets of the reference clouds into dx AND tptr; max_ref_cloud HOST, >= the largest
 *               reference cloud: it sizes the grid only (chunks of 256 / ceil(C / 4) reference rows x cloud pairs)
 *   tptr, tedge, tcoef   from dc_knn_cross_transpose; num_edges HOST: the entries of tedge / tcoef (a list is cut to it)
 *   edge_base   a row offset: a contiguous range of clouds runs against lists built once for a whole store by passing
 *               g = the range's rows, edge_base = its first row, tptr + the range's first reference row and rptr relative to it
 *   dx          DEVICE [*, ldx] fp32, C <= ldx
 * 16-byte loads / stores where the base pointer and the leading dimension allow, scalar otherwise: any C >= 1, the same bits.
 * k outside 1 .. 16, C outside 1 .. 2^20, ldg or ldx below C, B above 65 535, max_ref_cloud outside [0, 2^31), a negative size or a
 * null pointer: DC_ERR_ARG with a message, checked before anything touches the device; B = 0 or max_ref_cloud = 0 returns DC_OK.
 * One launch, stream-ordered, no allocation, no synchronisation, no atomics, capturable. */
int dc_knn_interpolate_backward(const float* g, int64_t ldg, int64_t num_g_rows, int32_t C, const int64_t* rptr, int32_t B,
                                int64_t max_ref_cloud, int32_t k, const int64_t* tptr, const int64_t* tedge, const float* tcoef,
                                int64_t num_edges, int64_t edge_base, float* dx, int64_t ldx, void* stream);

/* ---- tangent-vector features between two clouds by parallel transport (csrc/interp_transport.hip, csrc/interp_transport_math.h) -- */
/* Stands in for build_transport (deltaconv/geometry/connection.py:6-47) composed with torch_geometric.nn.knn_interpolate, first
 * half: the table of per-slot matrices of a dc_knn_cross result.  Entry e = q * k + s (q the ABSOLUTE query row, the row of idx / d2)
 * is M = c * R, four fp32 products: c the interpolation coefficient of the slot (the tcoef of dc_knn_cross_transpose: w_s / den in
 * the forward's den bits, exactly 1.0f for the only valid slot of a query, which keeps R's bits) and R the connection of
 * dc_build_transport from the source frame (sn, sx)[rptr[b] + idx[e]] into the target frame (tn, tx, ty)[q].  A slot with idx
 * outside [0, size of the reference cloud) holds four +0.0f and indexes nothing.
 *   qptr, rptr  DEVICE [B+1] ABSOLUTE row offsets, as in dc_knn_cross; tn, tx, ty DEVICE [num_query,3] fp32 rows indexed like idx;
 *               sn, sx DEVICE [*,3] fp32 rows indexed by the rows rptr names
 *   num_query   HOST: the rows of idx / d2 / tmat (>= qptr[B]); max_query_cloud HOST, >= the largest query cloud: it sizes the
 *               grid only (chunks of 256 slots x cloud pairs)
 *   tmat        DEVICE [num_query * k, 4] fp32, 16-byte aligned; rows of queries outside every pair are not written
 * None of it is differentiated.  B above 65 535, k outside 1 .. 16, num_query or max_query_cloud outside [0, 2^35), a null pointer
 * or a misaligned tmat: DC_ERR_ARG with a message, checked before anything touches the device; B = 0, num_query = 0 or
 * max_query_cloud = 0 returns DC_OK.  One launch, one thread and one 16-byte store per slot, stream-ordered, no allocation, no
 * synchronisation, no atomics, capturable. */
int dc_knn_cross_transport(const int64_t* qptr, const int64_t* rptr, int32_t B, int64_t num_query, int64_t max_query_cloud, int32_t k,
                           const int32_t* idx, const float* d2, const float* tn, const float* tx, const float* ty, const float* sn,
                           const float* sx, int32_t non_oriented, float* tmat, void* stream);
/* build_transport (connection.py:6-47) composed with torch_geometric.nn.knn_interpolate, second half: the transported, weighted sum
 * on the table of dc_knn_cross_transport.  Vector rows as in dc_transport_sum: rows 2i, 2i+1 are the two coefficients at point i.
 * For query row q of pair b: au = av = +0, then for slots s = 0 .. k-1 in order, invalid ones (idx outside the reference cloud)
 * skipped, j = rptr[b] + idx[q,s]: au = (au + M00 * v[2j,c]) + M01 * v[2j+1,c], av = (av + M10 * v[2j,c]) + M11 * v[2j+1,c], every
 * operation rounded to fp32 (the order of dc_transport_sum); out[2q,c] = au, out[2q+1,c] = av.  No valid slot: zeros.
 *   v           DEVICE [*,ldv] fp32, two rows per reference point, C <= ldv; out DEVICE [*,ldo] fp32, two rows per query, C <= ldo
 *   qptr, rptr, max_query_cloud, k, idx   as in dc_knn_interpolate (the same grid); tmat 16-byte aligned, indexed like idx
 * 16-byte loads / stores where the base pointer and the leading dimension allow, scalar otherwise: any C >= 1, the same bits.
 * The argument checks of dc_knn_interpolate, and a misaligned tmat: DC_ERR_ARG.  One launch, no atomics, capturable. */
int dc_knn_interpolate_vectors(const float* v, int64_t ldv, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B,
                               int64_t max_query_cloud, int32_t k, const int32_t* idx, const float* tmat, float* out, int64_t ldo,
                               void* stream);
/* The gradient of dc_knn_interpolate_vectors w.r.t. v -- what autograd records for build_transport (connection.py:6-47) composed
 * with torch_geometric.nn.knn_interpolate is an index_add_ with floating-point atomics -- on the lists of dc_knn_cross_transpose
 * (tptr, tedge; its tcoef is not needed, M carries the coefficient).  For reference row r: du = dw = +0, then for every in-edge e
 * of r in ascending order, i = e / k - edge_base, M = tmat[e - edge_base * k]: du = (du + M00 * g[2i,c]) + M10 * g[2i+1,c],
 * dw = (dw + M01 * g[2i,c]) + M11 * g[2i+1,c]; dv[2r,c] = du, dv[2r+1,c] = dw.  Every reference row of every pair is written.
 *   g           DEVICE [2 * num_g_rows, ldg] fp32; an edge whose query row falls outside [0, num_g_rows) or whose table entry falls
 *               outside [0, tmat_rows) is skipped
 *   rptr, max_ref_cloud, tptr, tedge, num_edges, edge_base   as in dc_knn_interpolate_backward (the same grid)
 *   tmat        DEVICE [tmat_rows, 4] fp32, 16-byte aligned: the table from the call's first query row on (a slice of a store-wide
 *               table for a range of clouds)
 *   dv          DEVICE [*, ldv] fp32, two rows per reference point, C <= ldv
 * The argument checks of dc_knn_interpolate_backward, a negative tmat_rows and a misaligned tmat: DC_ERR_ARG.  One launch, no
 * atomics, the same bits on every run, capturable. */
int dc_knn_interpolate_vectors_backward(const float* g, int64_t ldg, int64_t num_g_rows, int32_t C, const int64_t* rptr, int32_t B,
                                        int64_t max_ref_cloud, int32_t k, const int64_t* tptr, const int64_t* tedge,
                                        int64_t num_edges, int64_t edge_base, const float* tmat, int64_t tmat_rows, float* dv,
                                        int64_t ldv, void* stream);

/* ---- scalar features from a cloud DOWN to a sampled one: pooling over a two-set search (csrc/pool.hip, csrc/pool_math.h) --------- */
/* Stands in for a torch_cluster.knn search followed by torch_scatter.scatter(x[col], row, reduce = "max" | "min" | "sum" | "mean"):
 * the set-abstraction step of PointNet++, on the result of dc_knn_cross with the SAMPLED cloud as the query and the full cloud as
 * the reference.  It is no call site of the reference, which pools inside one cloud only; it is what its multi-resolution use
 * (GeodesicFPS, train_shapenet.py:32) needs between two.
 * out[q,c] = reduce over the valid slots s of x[rptr[b] + idx[q,s], c]  (mode: 0 max, 1 min, 2 sum, 3 mean -- the codes of
 * dc_seg_reduce), csrc/pool_math.h: a slot with idx outside [0, size of the reference cloud) is skipped and indexes nothing; the
 * first valid slot is copied bit for bit (k = 1 is an exact gather), a later one replaces it iff it is strictly larger (max) /
 * smaller (min) -- ties keep the nearer slot, a NaN in a later slot is never taken, one in the first valid slot stays -- or is added,
 * every addition rounded on its own, slots in order (sum, mean); mean divides once by (float)cnt.  No valid slot: a row of zeros,
 * arg 255, cnt 0.
 *   x           DEVICE [*,ldx] fp32 reference rows, C <= ldx; out DEVICE [*,ldo] fp32, C <= ldo
 *   qptr, rptr, max_query_cloud, k, idx   as in dc_knn_interpolate (the same grid: chunks of 256 queries x cloud pairs)
 *   arg         DEVICE uint8 [*,ldarg], C <= ldarg: the slot 0 .. k-1 every channel of a max / min came from (one 32-bit store per
 *               group of 4 channels where arg is 4-byte aligned and ldarg a multiple of 4, byte stores otherwise); not written by
 *               sum / mean, for which it may be NULL
 *   cnt         DEVICE uint8 [*]: the number of valid slots of every query row of a pair, written in every mode
 * 16-byte loads / stores where the base pointer and the leading dimension allow, scalar otherwise: any C >= 1, the same bits.
 * The argument checks of dc_knn_interpolate, and: mode outside 0 .. 3, ldarg below C, a NULL cnt, a NULL arg for max / min:
 * DC_ERR_ARG with a message, checked before anything touches the device.  One launch, stream-ordered, no allocation, no
 * synchronisation, no atomics, capturable. */
int dc_knn_pool(const float* x, int64_t ldx, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B,
                int64_t max_query_cloud, int32_t k, const int32_t* idx, int32_t mode, float* out, int64_t ldo, uint8_t* arg,
                int64_t ldarg, uint8_t* cnt, void* stream);
/* The gradient of dc_knn_pool w.r.t. x -- what autograd records for the gather x[col] is an index_add_ with floating-point atomics --
 * on the lists of dc_knn_cross_transpose (tptr, tedge; its tcoef is not needed).  For reference row r: dx[r,c] = 0, then for every
 * in-edge e of r in ascending order, q = e / k, s = e - q * k: max / min add g[q,c] iff arg[q,c] == s (an edge that lost adds
 * nothing), sum adds g[q,c], mean adds g[q,c] / (float)cnt[q]; quotient and sum each rounded on their own (csrc/pool_math.h).
 * Every reference row of every pair is written (a row without in-edges gets zeros).
 *   g           DEVICE [num_g_rows, ldg] fp32, C <= ldg; an edge whose query row falls outside [0, num_g_rows) is skipped
 *   rptr, max_ref_cloud, tptr, tedge, num_edges   as in dc_knn_interpolate_backward (the same grid)
 *   arg, ldarg, cnt   what dc_knn_pool wrote, indexed like g; arg may be NULL for sum / mean
 *   dx          DEVICE [*, ldx] fp32, C <= ldx
 * The argument checks of dc_knn_interpolate_backward and the mode / arg / cnt checks of dc_knn_pool: DC_ERR_ARG.  One launch, no
 * atomics, the same bits on every run, capturable. */
int dc_knn_pool_backward(const float* g, int64_t ldg, int64_t num_g_rows, int32_t C, const int64_t* rptr, int32_t B,
                         int64_t max_ref_cloud, int32_t k, const int64_t* tptr, const int64_t* tedge, int64_t num_edges,
                         int32_t mode, const uint8_t* arg, int64_t ldarg, const uint8_t* cnt, float* dx, int64_t ldx, void* stream);

/* ---- tangent-vector features from a cloud DOWN to a sampled one: transported pooling (csrc/pool_vectors.hip, csrc/pool_vectors_math.h) */
/* The rotation table of a dc_knn_cross result: entry e = q * k + s (q the ABSOLUTE query row, the row of idx) is
 * R = the connection of dc_build_transport from the source frame (sn, sx)[rptr[b] + idx[e]] into the target frame (tn, tx, ty)[q] --
 * the matrix alone, WITHOUT the interpolation coefficient dc_knn_cross_transport multiplies in (it takes no d2).  A slot with idx
 * outside [0, size of the reference cloud) holds four +0.0f and indexes nothing.
 *   qptr, rptr, num_query, max_query_cloud, k, idx, tn, tx, ty, sn, sx, non_oriented   as in dc_knn_cross_transport (the same grid)
 *   rmat        DEVICE [num_query * k, 4] fp32, 16-byte aligned; rows of queries outside every pair are not written
 * The argument checks of dc_knn_cross_transport: DC_ERR_ARG with a message, checked before anything touches the device.  One launch,
 * one thread and one 16-byte store per slot, stream-ordered, no allocation, no synchronisation, no atomics, capturable. */
int dc_knn_cross_rotation(const int64_t* qptr, const int64_t* rptr, int32_t B, int64_t num_query, int64_t max_query_cloud, int32_t k,
                          const int32_t* idx, const float* tn, const float* tx, const float* ty, const float* sn, const float* sx,
                          int32_t non_oriented, float* rmat, void* stream);
/* The set-abstraction step of dc_knn_pool for the vector stream, on the result of dc_knn_cross with the SAMPLED cloud as the query
 * and on the table of dc_knn_cross_rotation: every neighbour's vector is carried into the query's frame, then reduced.  It is no call
 * site of the reference.  Vector rows as in dc_transport_sum: rows 2i, 2i+1 are the two coefficients at point i.  For query row q of
 * pair b, valid slots s = 0 .. k-1 in order (idx outside the reference cloud: skipped), j = rptr[b] + idx[q,s], v0 = v[2j,c],
 * v1 = v[2j+1,c], R = rmat[q*k + s]  (mode: 0 max, 2 sum, 3 mean -- the codes of dc_seg_reduce; 1, min, is refused):
 *   sum    au = av = +0, au = (au + R00*v0) + R01*v1, av = (av + R10*v0) + R11*v1: dc_knn_interpolate_vectors on rmat, bit for bit
 *   mean   the sum, then one division per component by (float)cnt
 *   max    per channel the slot of the largest key v0*v0 + v1*v1 (taken in the source frame): the first valid slot, a later one iff
 *          its key is strictly larger -- ties keep the nearer slot, a NaN key in a later slot is never taken, one in the first valid
 *          slot stays; out = (R00*v0 + R01*v1, R10*v0 + R11*v1) of that slot, arg = the slot
 * every product, sum and quotient rounded to fp32 on its own (csrc/pool_vectors_math.h); out[2q,c] = au, out[2q+1,c] = av.  No valid
 * slot: zeros, arg 255, cnt 0.
 *   v           DEVICE [*,ldv] fp32, two rows per reference point, C <= ldv; out DEVICE [*,ldo] fp32, two rows per query, C <= ldo
 *   qptr, rptr, max_query_cloud, k, idx   as in dc_knn_interpolate (the same grid); rmat 16-byte aligned, indexed like idx
 *   arg         DEVICE uint8 [*,ldarg], one row per QUERY, C <= ldarg: the slot every channel of a max came from (one 32-bit store
 *               per group of 4 channels where arg is 4-byte aligned and ldarg a multiple of 4, byte stores otherwise); not written by
 *               sum / mean, for which it may be NULL
 *   cnt         DEVICE uint8 [*]: the number of valid slots of every query row of a pair, written in every mode
 * 16-byte loads / stores where the base pointer and the leading dimension allow, scalar otherwise: any C >= 1, the same bits.
 * The argument checks of dc_knn_interpolate, and: mode outside {0, 2, 3}, ldarg below C, a NULL cnt, a NULL arg for max, a
 * misaligned rmat: DC_ERR_ARG with a message, checked before anything touches the device.  One launch, stream-ordered, no
 * allocation, no synchronisation, no atomics, capturable. */
int dc_knn_pool_vectors(const float* v, int64_t ldv, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B,
                        int64_t max_query_cloud, int32_t k, const int32_t* idx, const float* rmat, int32_t mode, float* out,
                        int64_t ldo, uint8_t* arg, int64_t ldarg, uint8_t* cnt, void* stream);
/* The gradient of dc_knn_pool_vectors w.r.t. v on the lists of dc_knn_cross_transpose (tptr, tedge; its tcoef is not read).  For
 * reference row r: du = dw = +0, then for every in-edge e of r in ascending order, q = e / k, s = e - q * k, R = rmat[e],
 * g0 = g[2q,c], g1 = g[2q+1,c]: du = (du + R00*g0) + R10*g1, dw = (dw + R01*g0) + R11*g1 -- for every edge (sum), with g0, g1 first
 * divided by (float)cnt[q], each quotient rounded on its own (mean), or iff arg[q,c] == s (max: an edge that lost adds nothing);
 * dv[2r,c] = du, dv[2r+1,c] = dw.  Every reference row of every pair is written (a row without in-edges gets zeros).
 *   g           DEVICE [2 * num_g_rows, ldg] fp32, C <= ldg; an edge whose query row falls outside [0, num_g_rows) is skipped
 *   rptr, max_ref_cloud, tptr, tedge, num_edges   as in dc_knn_interpolate_backward (the same grid)
 *   rmat        DEVICE [num_g_rows * k, 4] fp32, 16-byte aligned, indexed like the rows of g
 *   arg, ldarg, cnt   what dc_knn_pool_vectors wrote, one row per query of g; arg may be NULL for sum / mean
 *   dv          DEVICE [*, ldv] fp32, two rows per reference point, C <= ldv
 * The argument checks of dc_knn_interpolate_backward, the mode / arg / cnt checks of dc_knn_pool_vectors and a misaligned rmat:
 * DC_ERR_ARG.  One launch, no atomics, the same bits on every run, capturable. */
int dc_knn_pool_vectors_backward(const float* g, int64_t ldg, int64_t num_g_rows, int32_t C, const int64_t* rptr, int32_t B,
                                 int64_t max_ref_cloud, int32_t k, const int64_t* tptr, const int64_t* tedge, int64_t num_edges,
                                 const float* rmat, int32_t mode, const uint8_t* arg, int64_t ldarg, const uint8_t* cnt, float* dv,
                                 int64_t ldv, void* stream);

/* ---- per-vertex normals of a store of triangle meshes (csrc/mesh_normal.hip, csrc/mesh_normal_math.h) --------------------------- */
/* First half of what replaces GenerateMeshNormals() in the reference's ShapeSeg pre_transform (experiments/train_shapeseg.py:31,
 * torch_geometric's transform: an index_add_ of the face normals onto their corners): the vertex-to-incident-corner lists of a whole
 * store, built once.  For every vertex row v of the call (ABSOLUTE, as vert is indexed: vptr[b] + id), its corner slots
 * e = 3 * face_row + corner (face_row ABSOLUTE, the row of face) with face[face_row, corner] == id, in ASCENDING e.  A face row
 * with any id outside [0, V) of its mesh has no corner in any list; a face that names a vertex twice is in its list twice.
 *   face        DEVICE [num_faces,3] int32 vertex ids LOCAL to the mesh, one row per triangle (the layout of dc_mesh_sample)
 *   vptr, fptr  DEVICE [B+1] ABSOLUTE row offsets of the B meshes into vert / face (a slice of the store's offsets serves); any
 *               B >= 0 (nothing is gridded over the meshes)
 *   num_verts   HOST: the rows of vert (>= vptr[B]); a row outside every mesh of the call gets an empty list.  num_faces HOST: the
 *               rows of face (>= fptr[B]); a row outside every mesh of the call is in no list
 *   vf_ptr      DEVICE int64 [num_verts + 1], every entry written: the list of row v is [vf_ptr[v], vf_ptr[v+1])
 *   vf_edge     DEVICE int64 [3 * num_faces] (the first vf_ptr[num_verts] entries are written)
 *   workspace   DEVICE, 8-byte aligned, dc_mesh_vertex_faces_workspace_bytes(num_verts, num_faces) bytes (0: sizes out of range)
 * Count (integer atomics), scan, unordered fill (integer atomic cursors), then a ranking pass that sorts every list, one fill
 * position per thread: the outputs are a function of the inputs only.  No floating-point atomics.  A negative B or size,
 * num_verts or 3 * num_faces above 2^39 - 256, a null pointer or a workspace that is null, misaligned or too small: DC_ERR_ARG with
 * a message, checked before anything touches the device.  Six launches, stream-ordered, no allocation, no synchronisation,
 * capturable. */
size_t dc_mesh_vertex_faces_workspace_bytes(int64_t num_verts, int64_t num_faces);
int dc_mesh_vertex_faces(const int32_t* face, const int64_t* vptr, const int64_t* fptr, int32_t B, int64_t num_verts,
                         int64_t num_faces, int64_t* vf_ptr, int64_t* vf_edge, void* workspace, size_t workspace_bytes,
                         void* stream);
/* Second half of what replaces GenerateMeshNormals() of experiments/train_shapeseg.py:31, on the lists of dc_mesh_vertex_faces: per
 * face a = p1 - p0, b = p2 - p0, c = a x b; a face gives c / max(|c|, 1e-12) (weighting 0, "uniform": torch_geometric's) or c
 * itself (weighting 1, "area") to each of its corners; normals[v] = s / max(|s|, 1e-12) with s the sum over the list of v, SEQUENTIAL
 * in list order from +0.  fp32, every operation rounded on its own, |x| = sqrt((x*x + y*y) + z*z) (csrc/mesh_normal_math.h, which
 * a numpy restatement reproduces bit for bit).  A vertex without incident corner or with s = 0 gets the zero vector; a zero-area
 * face gives zero.  The face winding decides the sign: inconsistent winding is not repaired.  A vertex's normal is a function of its
 * mesh alone -- not of B, of the mesh's place in the store or of the grouping into calls; permuting a mesh's faces may change the
 * last bits.
 *   vert        DEVICE [num_verts,3] fp32; face, vptr, fptr, num_verts, num_faces as in dc_mesh_vertex_faces
 *   vf_ptr, vf_edge   from dc_mesh_vertex_faces on the same store (a list is cut to [0, 3 * num_faces); an entry that names a
 *               face row outside the vertex's mesh is skipped)
 *   weighting   0 uniform, 1 area
 *   normals     DEVICE [num_verts,3] fp32; every row of a mesh of the call is written, no other
 *   zero_count  NULL, or DEVICE int32 [B]: per mesh the vertices that got the zero vector (integer atomics on counters zeroed by
 *               the call: order-free)
 * One vertex per thread, the contributions of its faces recomputed from the vertex rows: a thread's cost is its list length (a hub
 * vertex with thousands of faces is correct, not fast).  A negative B or size, a size above 2^39 - 256, an unknown weighting or a
 * null pointer: DC_ERR_ARG with a message, checked before anything touches the device; B = 0 or num_verts = 0 returns DC_OK.  One
 * launch (two with zero_count), stream-ordered, no allocation, no synchronisation, no floating-point atomics, capturable. */
int dc_mesh_vertex_normals(const float* vert, const int32_t* face, const int64_t* vptr, const int64_t* fptr, int32_t B,
                           int64_t num_verts, int64_t num_faces, const int64_t* vf_ptr, const int64_t* vf_edge, int32_t weighting,
                           float* normals, int32_t* zero_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DELTACONV_HIP_H */
