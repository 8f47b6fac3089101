/*
 * pcr.h -- C ABI of libpcr_hip.so, the MI355X (gfx950) implementation of the siamese
 * point-cloud ReID hot path of bentherien/point-cloud-reid.
 *
 * Conventions (all entry points):
 *   - plain `extern "C"`, raw DEVICE pointers, sizes as int, a hipStream_t passed as void*;
 *   - outputs are caller-allocated (as in the reference's pybind11 wrappers, e.g.
 *     mmdet3d/ops/ball_query/src/ball_query.cpp:30-43: dims first, tensors after, outputs
 *     pre-allocated by the Python side);
 *   - the call only ENQUEUES work on `stream`: no allocation, no synchronisation;
 *   - returns a pcr_status (0 = ok).  Unlike the reference launchers, which fprintf + exit(-1)
 *     on a launch error (e.g. ball_query_cuda.cu:73-77), nothing here ever exits the process;
 *   - all float data is IEEE binary32, all index data int32, tensors contiguous, layouts as in
 *     the reference op they replace (cited per function).
 *
 * Section A replaces the reference's native extension modules one for one.
 * Section B are the fused model kernels, which have no native counterpart in the reference
 * (its model path is an unfused chain of ATen calls); each cites the Python it computes.
 */
#ifndef PCR_H_
#define PCR_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef void *pcr_stream_t; /* hipStream_t */

enum pcr_status {
  PCR_OK = 0,
  PCR_ERR_INVALID = 1, /* bad size / null pointer / unsupported configuration */
  PCR_ERR_LAUNCH = 2   /* hipLaunchKernel reported an error (hipGetLastError) */
};

/* ABI version (bumped whenever a signature changes) and human-readable status. */
int pcr_abi_version(void);
#define PCR_PREC_F32 0
#define PCR_PREC_BF16X3 1
#define PCR_PREC_BF16 2
const char *pcr_status_string(int status);

/* ---------------------------------------------------------------- A. point ops ------- */

/* furthest_point_sampling_wrapper (ops/furthest_point_sample/src/furthest_point_sample.cpp:32-43,
 * kernel furthest_point_sample_cuda.cu:25-141).  xyz (B,N,3); temp (B,N) in/out scratch that the
 * caller fills with 1e10 (furthest_point_sample.py:29) and that holds the final min-distances on
 * return; idx (B,M) int32.  Start index 0; tie rule identical to the reference's per-thread scan +
 * halving merge tree for block = min(1024, 2^floor(log2 N)).  Requires 1 <= N < 2^22. */
int pcr_fps_f32(const float *xyz, float *temp, int *idx, int B, int N, int M, pcr_stream_t stream);

/* furthest_point_sampling_with_dist_wrapper (furthest_point_sample.cpp:45-57, kernel .cu:213-331).
 * dist (B,N,N) pairwise distance matrix instead of coordinates. */
int pcr_fps_dist_f32(const float *dist, float *temp, int *idx, int B, int N, int M,
                     pcr_stream_t stream);

/* calc_square_dist (ops/furthest_point_sample/utils.py:4-32): the (B,N,M) matrix the F-FPS / FS samplers hand to
 * pcr_fps_dist_f32 (points_sampler.py:121-157).  a (B,N,C), b (B,M,C) -> out[i][j] = (|a_i|^2 + |b_j|^2) - 2 <a_i,b_j>,
 * sums left to right over the channels, no fma (the reference leaves the order to its matmul); norm: sqrt(.)/C. */
int pcr_pairwise_sqdist_f32(const float *a, const float *b, float *out, int B, int N, int M, int C, int norm,
                            pcr_stream_t stream);

/* ball_query_wrapper (ops/ball_query/src/ball_query.cpp:30-43, kernel ball_query_cuda.cu:11-54).
 * centres (B,M,3), xyz (B,N,3) -> idx (B,M,K): the first K indices k (ascending) with
 * d2 == 0 || (min_r^2 <= d2 < max_r^2), padded with the first hit; rows with no hit are written
 * as zeros (the reference leaves its pre-zeroed buffer untouched; the result is the same). */
int pcr_ball_query_f32(const float *centres, const float *xyz, int *idx, int B, int N, int M,
                       float min_r, float max_r, int K, pcr_stream_t stream);

/* pcr_ball_query_f32 that also returns cnt (B,M): the number of genuine hits (<= K) of every row. */
int pcr_ball_query_cnt_f32(const float *centres, const float *xyz, int *idx, int *cnt, int B, int N, int M,
                           float min_r, float max_r, int K, pcr_stream_t stream);

/* pcr_ball_query_cnt_f32 that ALSO writes the compact row table the wave-autonomous ragged SA kernel reads
 * (pcr_sa_params.row_tab; ABI 12).  rows: pcr_ball_query_rows_floats(B, M, K) floats, 16-byte aligned, = for every
 * (cloud, run of 16 consecutive centres) a region of 16 K entries of 4 floats {bits of the neighbour index, dx, dy, dz}
 * (point - centre): centre after centre its first ceil2(max(cnt, 1)) rows of idx (odd counts and empty balls padded
 * with the row's first entry, exactly as idx pads), then zero entries up to the next multiple of 32 rows; the rest of
 * a region is not written.  idx may be NULL (not written).  Needs pcr_ball_query_rows_ok(N, K, min_r): N <= 1024,
 * K even, min_r == 0 (every ball-query layer of the reference's configs); PCR_ERR_INVALID otherwise. */
long pcr_ball_query_rows_floats(int B, int M, int K);
int pcr_ball_query_rows_ok(int N, int K, float min_r);
int pcr_ball_query_rows_f32(const float *centres, const float *xyz, int *idx, int *cnt, float *rows, int B, int N, int M,
                            float min_r, float max_r, int K, pcr_stream_t stream);

/* pcr_fps_f32 and pcr_ball_query_rows_f32 of the picked centres as ONE launch (round 5): a pick's distances to the cloud
 * are the ball query's distances of that centre, bit for bit, so the query costs one compare per point on top of the
 * sampling.  xyz (B,N,3), temp (B,N) as pcr_fps_f32 -> idx (B,M) the pick order, new_xyz (B,M,3) the centres' coordinates
 * (no gather launch), cnt (B,M) and rows exactly what pcr_ball_query_rows_f32(new_xyz, xyz, NULL, cnt, rows, .., 0, max_r,
 * K) writes.  Needs pcr_fps_ball_query_rows_ok(N, M, K): N <= 1024, 2 <= M <= N, K even.  (The reference runs the two
 * ops back to back: ops/pointnet_modules/point_sa_module.py:166-216 -> points_sampler.py:107-119, ball_query.py:14-47.) */
int pcr_fps_ball_query_rows_ok(int N, int M, int K);
int pcr_fps_ball_query_rows_f32(const float *xyz, float *temp, int *idx, float *new_xyz, int *cnt, float *rows, int B,
                                int N, int M, float max_r, int K, pcr_stream_t stream);

/* The model path's own (dormant) Python samplers / groupers, semantics of the PYTHON code rather than of the CUDA ops:
 *
 * farthest_point_sample (models/pointnet2_utils.py:116-137): first pick = start[b] (the reference draws it with
 * torch.randint; NULL = 0), running distance min(.), next pick = the maximum with ties to the LOWEST index
 * (torch.max), distance (dx^2+dy^2)+dz^2.  temp (B,N) is filled with 1e10 by the caller.  idx (B,M) int32.
 *
 * query_ball_point (:218-240): distances by square_distance's expanded form (-2<c,p> + |c|^2) + |p|^2 (:169-188),
 * a point is kept unless d > radius^2 (i.e. d <= r^2, where the CUDA op uses d < r^2), first K kept indices in index
 * order, padded with the first; a row without a hit is filled with N, as the reference's sort leaves it. */
int pcr_fps_py_f32(const float *xyz, float *temp, const int *start, int *idx, int B, int N, int M,
                   pcr_stream_t stream);
int pcr_query_ball_point_f32(const float *centres, const float *xyz, int *idx, int B, int N, int M, float radius,
                             int K, pcr_stream_t stream);

/* knn_wrapper (ops/knn/src/knn.cpp:28-41, kernel knn_cuda.cu:58-94).  xyz (B,N,3), centres (B,M,3)
 * -> idx (B,M,K) int32 and dist2 (B,M,K), ascending, produced by the same max-heap + heap-sort
 * sequence as the reference (so equal distances come out in the reference's order).
 * 1 <= K <= 100.  (knn.py:62 transposes idx to (B,K,M) on the Python side.) */
int pcr_knn_f32(const float *xyz, const float *centres, int *idx, float *dist2, int B, int N, int M,
                int K, pcr_stream_t stream);

/* gather_points_wrapper / gather_points_grad_wrapper (ops/gather_points/src/gather_points.cpp:28-52,
 * kernels gather_points_cuda.cu:8-26, :51-70).  feat (B,C,N), idx (B,M) -> out (B,C,M);
 * backward ACCUMULATES into grad_feat (B,C,N), which the caller zero-fills (gather_points.py:43). */
int pcr_gather_fwd_f32(const float *feat, const int *idx, float *out, int B, int C, int N, int M,
                       pcr_stream_t stream);
int pcr_gather_bwd_f32(const float *grad_out, const int *idx, float *grad_feat, int B, int C, int N,
                       int M, pcr_stream_t stream);

/* group_points forward / backward (ops/group_points/src/group_points.cpp:31-58, kernels
 * group_points_cuda.cu:56-79, :10-31).  feat (B,C,N), idx (B,S,K) -> out (B,C,S,K);
 * backward accumulates into the caller-zeroed grad_feat (B,C,N). */
int pcr_group_fwd_f32(const float *feat, const int *idx, float *out, int B, int C, int N, int S,
                      int K, pcr_stream_t stream);
int pcr_group_bwd_f32(const float *grad_out, const int *idx, float *grad_feat, int B, int C, int N,
                      int S, int K, pcr_stream_t stream);

/* three_nn_wrapper (ops/interpolate/src/interpolate.cpp:46-58, kernel three_nn_cuda.cu:11-65).
 * unknown (B,N,3), known (B,M,3) -> dist2 (B,N,3) SQUARED distances (three_nn.py:41 takes the
 * sqrt), idx (B,N,3).  Running bests are kept in double and compared with the float distance, as
 * in the reference. */
int pcr_three_nn_f32(const float *unknown, const float *known, float *dist2, int *idx, int B, int N,
                     int M, pcr_stream_t stream);

/* three_interpolate_wrapper / _grad_wrapper (interpolate.cpp:60-86, kernels
 * three_interpolate_cuda.cu:11-35, :61-84).  feat (B,C,M), idx/weight (B,N,3) -> out (B,C,N);
 * backward accumulates into the caller-zeroed grad_feat (B,C,M). */
int pcr_three_interp_fwd_f32(const float *feat, const int *idx, const float *weight, float *out,
                             int B, int C, int M, int N, pcr_stream_t stream);
int pcr_three_interp_bwd_f32(const float *grad_out, const int *idx, const float *weight,
                             float *grad_feat, int B, int C, int N, int M, pcr_stream_t stream);

/* ------------------------------------------- A2. points in boxes, per-box crops ------- */

/* A box is [x, y, z, w, l, h, rz] in LiDAR coordinates, z the BOTTOM face.  Membership restates check_pt_in_box3d /
 * lidar_to_local_coords (ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-49) with that file's widths:
 *   cz = z + h / 2.0 (double sum, rounded to float); outside if fabsf(pz - cz) > h / 2.0 (both z faces are inside);
 *   rot = rz + pi/2 (double sum, rounded to float), sx = px - x, sy = py - y,
 *   local_x = sx*cos(rot) - sy*sin(rot), local_y = sx*sin(rot) + sy*cos(rot) (float, products and sums not contracted);
 *   inside iff -l/2.0 < local_x < l/2.0 and -w/2.0 < local_y < w/2.0 (double compares; the x / y faces are outside).
 *
 * pcr_box_frames_f32: boxes (T,7) -> frames (T,2) = (cosf(rot), sinf(rot)), the pair every kernel of this section derives
 * from a box through one device function.  With this table a host restatement needs no trigonometry of its own and
 * equals the entry points below bit for bit. */
int pcr_box_frames_f32(const float *boxes, float *frames, int T, pcr_stream_t stream);

/* points_in_boxes_batch (roiaware_pool3d/points_in_boxes.py:83-122, kernel points_in_boxes_cuda.cu:79-105).
 * points (B,P,3), boxes (B,T,7) -> out (B,P,T) int32, 1 where box t holds point p and 0 elsewhere; EVERY element is
 * written (the reference zero-fills first and writes the ones).  B <= 65535, T <= 65535 * 256. */
int pcr_points_in_boxes_batch_f32(const float *points, const float *boxes, int *out, int B, int P, int T,
                                  pcr_stream_t stream);

/* points_in_boxes_gpu (points_in_boxes.py:6-49, kernel points_in_boxes_cuda.cu:51-77).  -> out (B,P) int32: the LOWEST
 * index of a box that holds the point, -1 for none; every element is written (the reference pre-fills -1).  B <= 65535. */
int pcr_points_in_boxes_f32(const float *points, const float *boxes, int *out, int B, int P, int T, pcr_stream_t stream);

/* The fused crop: what the reference's tracker does with points_in_boxes_batch, a Python loop over the boxes, a padded
 * batch, a batched affine and one host-side torch.randint per box (models/trackers/deprecated/pc_utils.py:31-96), and
 * what its loader does per object with subsamplePC (datasets/utils.py:606-621), as ONE launch without a host read.
 *
 * points: P rows of `stride` floats, xyz first (a nuScenes sweep is (P,5)); boxes (M,7) -> clouds (M,n,3) f32 and
 * lengths (M) int32, the number of sweep points box m holds (under both rules).  The in-box points of a box are numbered
 * 0 .. len-1 in ascending sweep index; slot s of box m takes in-box point j = ((uint64)u * len) >> 32, u a 32-bit word
 * (torch.randint(high=len) with replacement for every slot, pc_utils.py:84).
 *   u = rand[m*n + s] read as bits when rand != NULL; otherwise the counter-based word of (seed[0], m, s):
 *       mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (uint32)
 *       h = mix((uint32)seed ^ 0x9e3779b9); h = mix(h ^ (uint32)(seed >> 32)); h = mix(h ^ m); u = mix(h ^ s)
 *     seed is a DEVICE pointer to one int64 (NULL = 0): a captured launch draws fresh samples once that word changes.
 *   rule PCR_CROP_RULE_TRACKER: len == 0 -> zeros, otherwise every slot is drawn (pc_utils.py:84-95);
 *        PCR_CROP_RULE_DATASET: len <= 2 -> zeros, len == n -> the in-box points in order, otherwise drawn (subsamplePC).
 *   frame PCR_CROP_FRAME_SENSOR: coordinates as read; _CENTRED: minus (x, y, cz); _BOX: (local_x, local_y, pz - cz), the
 *        values of the membership test (= interpolate_per_frame's affine, INTEGRATION.md "from a sweep and boxes").
 *   z_is_centre != 0: boxes[.][2] is cz itself (gravity-centre boxes, what the tracker holds).
 * One workgroup per box: the sweep is tested in 64-point chunks, the chunks' counts are scanned in LDS, and each slot
 * finds its chunk by binary search and picks by rank inside the chunk's ballot -- no list, no atomics, the same bits on
 * every run.  pcr_crop_boxes_ok(P, M, n, stride): 0 <= P <= PCR_CROP_MAX_POINTS (the count table, one LDS word per 64
 * points plus 64 words of scan scratch, fills the 160 KiB a gfx950 workgroup may take: 64 * (40960 - 64)),
 * 0 <= M <= PCR_CROP_MAX_BOXES, 1 <= n <= PCR_CROP_MAX_SAMPLES, 3 <= stride <= PCR_CROP_MAX_STRIDE; anything else, an
 * unknown frame / rule or a NULL tensor that would be read returns PCR_ERR_INVALID.  M == 0 launches nothing; P == 0
 * gives zero clouds and zero lengths. */
#define PCR_CROP_FRAME_SENSOR 0
#define PCR_CROP_FRAME_CENTRED 1
#define PCR_CROP_FRAME_BOX 2
#define PCR_CROP_RULE_TRACKER 0
#define PCR_CROP_RULE_DATASET 1
#define PCR_CROP_MAX_POINTS 2617344
#define PCR_CROP_MAX_BOXES 65536
#define PCR_CROP_MAX_SAMPLES 65536
#define PCR_CROP_MAX_STRIDE 16
int pcr_crop_boxes_ok(int P, int M, int n, int stride);
int pcr_crop_boxes_f32(const float *points, int stride, const float *boxes, const int *rand, const long long *seed,
                       float *clouds, int *lengths, int P, int M, int n, int frame, int rule, int z_is_centre,
                       pcr_stream_t stream);

/* ------------------------------------------------------------ A3. association --------- */

/* What the reference's tracker does on the host between the matching logits and the track update, as fixed-shape launches
 * without a host read: the class-gated pair list (get_labels_to_compare, trackers/deprecated/tracking_point_reid.py:15-33),
 * the augmented cost matrix (get_cost_mat_margin, tracking_association.py:22-53, :126-128) and the rectangular linear sum
 * assignment it hands to scipy (:141).  Every output is the same bits on every run.  An entry with nothing to do (see each)
 * returns PCR_OK, launches nothing and writes nothing.
 *
 * pcr_assoc_pairs_i32: track_labels (T), det_labels (D), optional track_lengths (T) / det_lengths (D) -> pairs (cap,2)
 * int32 and count (1) int32.  (t, d) is listed iff track_labels[t] == det_labels[d], that label lies in [0, num_classes)
 * and -- when the length pointers are not NULL (use_lengths) -- both lengths are >= min_points.  Order: class ascending,
 * then track index ascending, then detection index ascending (torch.cat of the per-class cartesian_prod).  count is the
 * TRUE number of pairs, also when it exceeds cap (then the first cap pairs are written); slots from count on hold (0, 0).
 * Ranks come from ballots and LDS scans, no atomics.  pcr_assoc_pairs_ok: 0 <= T, D <= PCR_ASSOC_MAX_OBJECTS,
 * 1 <= num_classes <= PCR_ASSOC_MAX_CLASSES, 0 <= cap <= PCR_ASSOC_MAX_OBJECTS^2.  Nothing to do: T == 0 or D == 0 (the
 * list is empty; count and pairs are left as they are). */
#define PCR_ASSOC_MAX_OBJECTS 4096
#define PCR_ASSOC_MAX_CLASSES 32
int pcr_assoc_pairs_ok(int T, int D, int num_classes, int cap);
int pcr_assoc_pairs_i32(const int *track_labels, const int *det_labels, const int *track_lengths, const int *det_lengths,
                        int *pairs, int *count, int T, int D, int num_classes, int min_points, int cap,
                        pcr_stream_t stream);

/* pcr_assoc_cost_f32: cost (T+D, D+T) row-major, EVERY element written (one tracking and one detection decision):
 *   top-left (T,D):     -logits[k] at (t, d) = pairs[k] for k < min(count[0], cap), plus dist_penalty where dist != NULL and
 *                       dist[t*D + d] > dist_max (the distance prior, :26-31); fill elsewhere;
 *   top-right (T,T):    track_miss[t] on the diagonal, fill elsewhere;      bottom-left (D,D): det_new[d] likewise;
 *   bottom-right (D,T): the transpose of the top-left block (:33-38).
 * NULL track_miss / det_new are zeros.  The listed pairs must be distinct (pcr_assoc_pairs_i32's are); a pair outside
 * [0,T) x [0,D) is skipped.  Range as pcr_assoc_pairs_ok(T, D, 1, cap).  Nothing to do: T + D == 0. */
int pcr_assoc_cost_f32(const float *logits, const int *pairs, const int *count, const float *track_miss,
                       const float *det_new, const float *dist, float dist_max, float dist_penalty, float fill,
                       float *cost, int T, int D, int cap, pcr_stream_t stream);

/* pcr_lsa_f32: rectangular linear sum assignment (minimum total) of B problems.  cost (B,R,C) -> col4row (B,R), row4col
 * (B,C) (-1 = unassigned), info (B), and the duals u (B,R), v (B,C) unless NULL.  info 0: solved.  info 1: the problem
 * holds a NaN or an infinity (found by a pre-scan): both index outputs are -1, the duals 0, the solver does not run.
 * info 2: a search found no column (an intermediate value overflowed); outputs as for 1.
 * pcr_lsa_ok: 0 <= R, C <= PCR_LSA_MAX, 0 <= B <= 65535.  Nothing to do: B, R or C == 0.
 *
 * The result is DEFINED by these rules, each operation rounded to binary32, nothing contracted (tests/assoc_ref.py::lsa
 * restates them; the kernel equals it bit for bit, duals included):
 *   transpose   shortest augmenting paths (Jonker-Volgenant) over the rows 0 .. R-1 in order; if R > C the transposed
 *               problem is solved and the outputs are swapped back (col4row <-> row4col, u <-> v);
 *   search      for row cur: minv = 0, short[] = +inf, no column done, i = cur; then repeat:
 *     candidates  every column j not done gets r = ((c[i][j] - u[i]) - v[j]) + minv;
 *     update      if r < short[j] (strict): short[j] = r, pred[j] = i;
 *     selection   the next column is the not-done column with the lowest short, ties (by float comparison, -0 == +0) to
 *                 the LOWEST column index; minv = its short; it is done; if it is unassigned it ends the search (the
 *                 sink), otherwise i = its row;
 *   duals       u[cur] += minv; for every done column j but the sink, with ri its row: u[ri] += (minv - short[j]);
 *               for every done column j: v[j] -= (minv - short[j]);
 *   augment     along pred from the sink back to cur.
 * A search marks one more column done per step, so a problem takes at most min(R,C) * max(R,C) steps; every loop of the
 * kernel is bounded by such an integer count.  One wave per problem: column j lives in lane j % 64 (short / pred / v /
 * row4col and the done bits in registers), u and col4row in LDS, the matrix too when it fits beside them (R*C + 2*min(R,C)
 * words in 160 KiB: 200 x 200 does), otherwise rows are read from global memory. */
#define PCR_LSA_MAX 1024
int pcr_lsa_ok(int B, int R, int C);
int pcr_lsa_f32(const float *cost, int *col4row, int *row4col, float *u, float *v, int *info, int B, int R, int C,
                pcr_stream_t stream);

/* The block rule (additive to ABI 17): pcr_lsa_blocks_f32 solves ONE (R,C) problem block by block.  row_block (R) and
 * col_block (C) are int32 and give every row and column a block id in [0, G); any other value means the row or column
 * takes no part.  For each block g:
 *   sub-problem  cost[rows of g][columns of g], both lists in ascending original index;
 *   solution     exactly pcr_lsa_f32's rules above over the sub-problem: the transpose when the block has more rows than
 *                columns, ties to the LOWEST column index of the sub-problem, the duals;
 *   outputs      col4row (R), row4col (C) hold ORIGINAL indices; a block with no rows or no columns assigns nothing (its
 *                rows and columns get -1, duals 0); rows and columns outside every block get -1, their duals 0;
 *   reads        only entries of the sub-problems are read: a NaN elsewhere is never seen;
 *   info (G)     0 / 1 / 2 per block with pcr_lsa_f32's meanings; the NaN / infinity pre-scan covers the block's own entries
 *                only; a failed block's rows and columns are -1 (duals 0), the other blocks are solved.
 * EVERY element of col4row, row4col, info (and u, v unless NULL) is written.  One launch, one wave per block: the wave
 * compacts the block's rows and columns into two LDS index lists (ballots over 64 ids, ranks from mbcnt, no atomics),
 * gathers the sub-matrix through them into LDS when lists + u + col4row + sub-matrix fit (R + C + 2*min(nr,nc) + nr*nc
 * words in 160 KiB), otherwise reads the gathered rows from global memory, runs the one solver body pcr_lsa_f32 runs,
 * and scatters the results through the lists.  Block sizes are device data: the launch asks for the LDS one block of all
 * R x C could use, capped at 160 KiB.  The blocks run on different CUs at the same time.
 * pcr_lsa_blocks_ok: 0 <= R, C <= PCR_LSA_MAX, 1 <= G <= PCR_ASSOC_MAX_CLASSES + 1.  Nothing to do: never (info is written).
 *
 * pcr_assoc_blocks_i32: track_labels (T), det_labels (D) -> row_block (T + de*D), col_block (D + te*T), the block ids of
 * the matrix pcr_assoc_cost_f32 (de = te = 1) or pcr_assoc_cost_multi_f32 (de / te = dd / td, or [dd > 0] / [td > 0] under
 * reduce) builds.  An object's block is its label when the label lies in [0, num_classes), otherwise the REST block
 * num_classes (free bank slots, padded detections, foreign labels); lengths play no part (an object below min_points
 * stays in its class block: its row is all fill, its decisions are not).  Row t and columns D + j*T + t take track t's
 * block; column d and rows T + i*D + d take detection d's block; G = num_classes + 1.  The top-left block of such a matrix
 * joins only objects of one class (pcr_assoc_pairs_i32 lists no other pair), so the matrix is block-diagonal up to fill
 * and the decoded frame of the block solve equals the full solve's, except that decode info[1] may be smaller (the full
 * solve can be forced to pair leftovers across classes through fill; the blocks are not).  A hand-made matrix with a
 * non-fill entry between two classes does not meet this precondition.
 * Range as pcr_assoc_multi_ok(T, D, de, te, 0) and 1 <= num_classes <= PCR_ASSOC_MAX_CLASSES.  Nothing to do: both
 * outputs empty. */
int pcr_lsa_blocks_ok(int R, int C, int G);
int pcr_lsa_blocks_f32(const float *cost, const int *row_block, const int *col_block, int *col4row, int *row4col, float *u,
                       float *v, int *info, int R, int C, int G, pcr_stream_t stream);
int pcr_assoc_blocks_i32(const int *track_labels, const int *det_labels, int *row_block, int *col_block, int T, int D,
                         int de, int te, int num_classes, pcr_stream_t stream);

/* Any set of decisions per side (additive to ABI 17).  The reference's tracker runs with dd detection decisions and td
 * tracking decisions (VirtualTracker, trackers/deprecated/virtual_tracker.py:80-81, :114-117: by default dd = 2, td = 0);
 * its matrix is (R, C) = (T + dd*D, D + td*T) (tracking_association.py:126).  The two entries below build that matrix by
 * either of its cost rules and turn the solved assignment into per-object decisions and the born / kill masks
 * pcr_bank_plan_i32 takes, as fixed-shape launches without a host read.  Both take a parameter block.
 *
 * pcr_assoc_multi_ok: 0 <= T, D; 0 <= dd, td <= PCR_ASSOC_MAX_DECISIONS; T + dd*D <= PCR_LSA_MAX and D + td*T <=
 * PCR_LSA_MAX; 0 <= cap <= T*D.
 *
 * pcr_assoc_cost_multi_f32: logits (cap), pairs (cap,2), count (1), det_dec (dd,D), trk_dec (td,T) -> cost (R,C) row-major,
 * EVERY element written.  NULL det_dec / trk_dec are zeros.  Layout (:22-53):
 *   top-left (T,D)                               the listed pairs k < min(count[0], cap), fill elsewhere (a pair outside
 *                                                [0,T) x [0,D) is skipped; the listed pairs must be distinct);
 *   rows T + i*D .. T + (i+1)*D, columns < D     detection decision i on the diagonal, fill elsewhere;
 *   columns D + j*T .. D + (j+1)*T, rows < T     tracking decision j on the diagonal, fill elsewhere;
 *   every (i, j) block of the bottom right       the transpose of the top-left block, fill entries included (only when
 *                                                dd > 0 and td > 0).
 * kind PCR_COST_MARGIN: a listed pair holds -logits[k], plus dist_penalty where dist != NULL and dist[t*D + d] > dist_max;
 *   the decision entries are det_dec / trk_dec as given (costs).  With dd == td == 1 the matrix is pcr_assoc_cost_f32's
 *   bit for bit.
 * kind PCR_COST_SOFTMAX (get_cost_mat_softmax, :56-98): logits and decision values are scores.  For track t, p_row is the
 *   softmax over {the logits of its listed pairs} and {trk_dec[j][t]}; for detection d, p_col the softmax over {the logits
 *   of its listed pairs} and {det_dec[i][d]}.  A listed pair holds -max(p_row, p_col), detection decision i of d holds
 *   -p_col of that decision, tracking decision j of t holds -p_row of that decision.  dist must be NULL (the reference
 *   applies no distance prior here) and reduce 0: anything else is PCR_ERR_INVALID.  DIFFERENCE from the reference: a pair
 *   the class gate leaves out takes part in neither softmax and stays at fill (the reference's 10000-filled matrix would put
 *   exp(10000) into the sums).
 *   The arithmetic, written down: the listed logits are scattered into a dense (T,D) score image in ws (unlisted = -inf; a
 *   listed logit of -inf therefore counts as unlisted).  One wave per track and one per detection reduces its set: lane l
 *   takes the set's elements l, l + 64, ... in order (the pairs by ascending partner index, then the decisions by ascending
 *   index); m = the maximum (NaN ignored); s = the sum of exp(x - m) over the lane's elements in that order, then over the
 *   lanes by six butterfly exchanges (s += s of lane ^ 32, then 16, 8, 4, 2, 1), each term and each partial sum in binary64.  An
 *   entry is p = exp(x - m) / s in binary64, rounded to binary32 once, after max(p_row, p_col).  No atomics; the same bits
 *   on every run.  A NaN logit makes its track's and its detection's entries NaN (pcr_lsa_f32 then reports info 1).
 * reduce = 1 (margin only; TrackingAssociatorMax.get_cost_mat_margin, :319-363): each side with at least one decision gets
 *   ONE diagonal block holding the object's cheapest decision, min over the decisions, ties to the lowest decision index
 *   (x < best, strict, starting from decision 0); the chosen index goes to det_choice (D) / trk_choice (T) (a side without
 *   decisions leaves its choice array as it is).  The matrix is (T + [dd>0]*D, D + [td>0]*T); the bottom-right transpose
 *   exists iff both sides have a decision.  Without reduce det_choice / trk_choice may be NULL and are not written.
 * ws: device scratch of pcr_assoc_multi_ws_bytes(T, D, dd, td) bytes (the score image and the 2*(T + D) row / column
 *   maxima and sums in binary64), used by the softmax kind only; may be NULL for margin.
 * count is read on the device.  Nothing to do: R*C == 0.
 *
 * pcr_assoc_decode_i32: cost (R,C) as built above, col4row (R), row4col (C), solver_info (1, NULL = 0) of pcr_lsa_f32 ->
 * track_to_det (T), det_to_track (D) (-1 = none), det_decision (D), track_decision (T), born (D), kill (T), info (4).  One
 * workgroup; every loop is bounded by an integer count.  It restates tracking_association.py:146-245 in fixed shape:
 *   void      an assigned entry (r, c) with cost[r][c] == fill is void: both sides become unassigned; info[1] counts them
 *             (the reference prints and exits);
 *   drop      only when td > 0: pairs with r >= T and c >= D are dropped;
 *   repair    only when td > 0: for every track t ascending without a pair, the column of least cost[t][c] among the
 *             columns no kept pair uses, ties to the lowest index; if there is none or that value == fill the track is
 *             skipped, otherwise (t, c) is a pair and c is used; info[2] counts them.  Then for every detection d ascending
 *             without a pair the same over the unused rows; info[3] counts them.  DIFFERENCE from the reference, which
 *             picks for all forgotten tracks at once (:171-181) and can hand one detection to two tracks: here the picks
 *             are sequential, and equal the reference's whenever its picks are distinct;
 *   classify  det_decision[d]: 0 = matched to a track (det_to_track[d] = it), 1 + i = detection decision i (the row block
 *             of d's pair; under reduce i = det_choice[d]), 1 + dd = unmatched.  track_decision[t] likewise with td, the
 *             column block and trk_choice;
 *   masks     born[d] = det_decision[d] == 1 + born_dec, all 0 when born_dec < 0; kill[t] = track_decision[t] ==
 *             1 + kill_dec, all 0 when kill_dec < 0 (int32 0 / 1, the form pcr_bank_plan_i32 takes);
 *   info[0]   the solver's info; when it is not 0 nothing is assigned: the maps are -1, every decision is "unmatched",
 *             the masks 0, info[1..3] 0.
 * Range as pcr_assoc_multi_ok(T, D, dd, td, 0).  Nothing to do: T + D == 0. */
#define PCR_ASSOC_MAX_DECISIONS 4
#define PCR_COST_MARGIN 0
#define PCR_COST_SOFTMAX 1
typedef struct pcr_assoc_multi {
  int T, D, dd, td, cap;
  int kind, reduce;
  float dist_max, dist_penalty, fill;
  const float *logits;
  const int *pairs, *count;
  const float *det_dec, *trk_dec, *dist;
  void *ws;
  float *cost;
  int *det_choice, *trk_choice;
} pcr_assoc_multi;
typedef struct pcr_assoc_decode {
  int T, D, dd, td;
  int reduce, born_dec, kill_dec;
  float fill;
  const float *cost;
  const int *col4row, *row4col, *solver_info, *det_choice, *trk_choice;
  int *track_to_det, *det_to_track, *det_decision, *track_decision, *born, *kill, *info;
} pcr_assoc_decode;
int pcr_assoc_multi_ok(int T, int D, int dd, int td, int cap);
int pcr_assoc_multi_ws_bytes(int T, int D, int dd, int td);
int pcr_assoc_cost_multi_f32(const pcr_assoc_multi *p, pcr_stream_t stream);
int pcr_assoc_decode_i32(const pcr_assoc_decode *p, pcr_stream_t stream);

/* ------------------------------------------- A4. box overlap and suppression --------- */

/* Overlap between bird's-eye-view boxes and the suppression of duplicates, the two steps of the tracker's frame that the
 * reference leaves the device for: the track NMS (VirtualTracker.non_max_suppression, models/trackers/deprecated/
 * virtual_tracker.py:232-259: torch.where on a data-dependent shape) and the detection NMS of ops/iou3d (iou3d_utils.py:
 * 23-68, src/iou3d.cpp:100-148: the whole mask copied to the host, the sweep in a C++ loop, cudaMalloc / cudaFree in the
 * middle).  Here every step is a fixed-shape launch without a host read, an allocation or an atomic, and writes the same
 * bits on every run.  An entry with nothing to do (N == 0, A == 0 or B == 0) returns PCR_OK, launches nothing and writes
 * nothing.  Thresholds are DEVICE pointers to one float: a replayed graph re-reads them (as seed in pcr_crop_boxes_f32).
 *
 * A BEV box is [x1, y1, x2, y2, angle] (iou3d's xyxyr), float.  Nothing is contracted into fma; divisions are IEEE.
 *
 * pcr_nearest_bev_f32: boxes7 (N,7) [x, y, z, w, l, h, rz] -> out5 (N,5), LiDARInstance3DBoxes.nearest_bev
 * (core/bbox/structures/lidar_box3d.py:96-114 with limit_period, core/bbox/structures/utils.py:6-19):
 *   r = |rz - floorf(rz / pi + 0.5) * pi|, pi rounded to float, every operation in binary32;
 *   (w, l) are swapped where r > pi/4 (rounded to float); out5 = [x - w/2, y - l/2, x + w/2, y + l/2, 0].
 *
 * pcr_bev_frames_f32: boxes5 (N,5) -> frames (N,2) = (cosf(angle), sinf(angle)), through the ONE device function every
 * rotated kernel of this section takes its trigonometry from (the reference's cos(-angle), sin(-angle) in check_in_box2d
 * are c and -s exactly).  With this table a host restatement needs no trigonometry of its own (as pcr_box_frames_f32, A2). */
int pcr_nearest_bev_f32(const float *boxes7, float *out5, int N, pcr_stream_t stream);
int pcr_bev_frames_f32(const float *boxes5, float *frames, int N, pcr_stream_t stream);

/* pcr_iou_bev_f32: a (A,5), b (B,5) -> out (A,B), EVERY element written; 0 <= A, B <= PCR_IOU_MAX_BOXES.
 *   PCR_IOU_AXIS     iou_normal (ops/iou3d/src/iou3d_kernel.cu:335-343): the angle is ignored;
 *                    inter = max(min(ax2,bx2) - max(ax1,bx1), 0) * max(min(ay2,by2) - max(ay1,by1), 0),
 *                    iou = inter / fmaxf((Sa + Sb) - inter, 1e-8f), S = (x2 - x1) * (y2 - y1);
 *   PCR_IOU_OVERLAP  box_overlap (:127-242), the area of the intersection polygon only;
 *   PCR_IOU_ROTATED  iou_bev (:244-251) = overlap / fmaxf((Sa + Sb) - overlap, 1e-8f).
 * The rotated kinds follow the reference's algorithm step by step, in float and in its order of operations:
 *   corners     (x1,y1) (x2,y1) (x2,y2) (x1,y2) rotated about the centre ((x1+x2)/2, (y1+y2)/2):
 *               x' = ((x-cx)*c + (y-cy)*s) + cx, y' = (-(x-cx)*s + (y-cy)*c) + cy (rotate_around_center, :111-119);
 *   crossings   the 16 edge pairs (edge i of a outer, edge j of b inner) through intersection (:79-109): the bounding-
 *               rectangle exclusion check_rect_cross (:45-52), the strict test s1*s2 > 0 && s3*s4 > 0, the point by
 *               (s5*q0 - s1*q1) / (s5 - s1) where fabsf(s5 - s1) > EPS = 1e-8f and by the line equations otherwise;
 *   corners in  for k = 0..3: corner k of b inside a, then corner k of a inside b, check_in_box2d with MARGIN = 1e-5f
 *               (:54-77);
 *   centroid    the running float sum of the points in that order, divided by their number;
 *   order       the reference's bubble sort (:215-224) by atan2f(y - cy, x - cx) about the centroid (swap where the left
 *               angle is greater);
 *   area        the fan sum of cross(p[k] - p[0], p[k+1] - p[0]), k = 0 .. cnt-2, then fabsf(area) / 2.
 * The reference's cross_points[16] can in principle be asked for up to 24 points (16 crossings + 8 corners); here the
 * array has 24 slots.  No point at all (cnt == 0) gives area 0: the reference's NaN centroid is never used.  The points
 * live in LDS (one column per lane), not in a scratch-backed private array. */
#define PCR_IOU_AXIS 0
#define PCR_IOU_ROTATED 1
#define PCR_IOU_OVERLAP 2
#define PCR_IOU_MAX_BOXES 65535
int pcr_iou_bev_f32(const float *a, const float *b, float *out, int A, int B, int kind, pcr_stream_t stream);

/* pcr_nms_f32: greedy NMS entirely on the device (nms_gpu / nms_normal_gpu, iou3d_utils.py:23-68 with iou3d.cpp:96-202).
 * boxes (N,5), scores (N), thresh (device, 1 float) -> order (N), keep (N), count (1), info (1), all int32.
 *   ranking  order holds the indices by descending score; equal scores (float compare, -0 == +0) go lowest index first
 *            (the reference's torch.sort leaves ties unspecified: this rule is ours).  Ranks are counted, never sorted
 *            with atomics: rank_i = #{j : s_j > s_i, or s_j == s_i and j < i}; a NaN score ranks behind every number,
 *            NaNs among themselves by index, so order is always a permutation.  Only the ranks < pre_max take part in
 *            what follows (pre_maxsize; pre_max <= 0 or >= N: all of them); call their number n.
 *   mask     the reference's upper-triangular 64-bit mask over the ranked boxes (nms_kernel, iou3d_kernel.cu:284-333):
 *            bit c of word (r, cb) is set iff column 64*cb + c > r and iou(box of rank r, box of that column) > thresh,
 *            iou = iou_normal for kind PCR_IOU_AXIS (nms_normal_gpu) and iou_bev for PCR_IOU_ROTATED (nms_gpu), row
 *            first.  A wave owns a 64 x 64 tile, lane = column, and one ballot is one word; only column blocks >= the
 *            row block are computed.
 *   sweep    iou3d.cpp:128-143 by one wave: for r = 0 .. n-1, rank r is kept iff its bit of remv is clear, and a kept
 *            row ORs its words into remv.  Row blocks of 64 mask rows pass through two LDS buffers: the global loads of
 *            block b+1 are issued before the 64 decisions of block b, which read LDS and registers only, and are waited
 *            for after them; the kept indices of a block are stored after its decisions.
 *   outputs  keep = the original indices of the kept boxes in rank order, padded with -1 to N; count = their true
 *            number; info = 0.  info = 1 when a score is NaN or a box that takes part holds a NaN or an infinity
 *            (x1..y2; the angle too for PCR_IOU_ROTATED): then keep is all -1 and count 0 (pcr_lsa_f32's convention);
 *            order is written either way.  A NaN score counts at ANY rank, also behind pre_max: where a NaN stands in a
 *            ranking is a convention, so which boxes take part would rest on it; a box is looked at only if it takes part.
 * pcr_nms_ok(N): 0 <= N <= PCR_NMS_MAX (the remv words are one per lane).  ws: pcr_nms_ws_bytes(N) bytes of device
 * memory (0 when N is out of range), 16-byte aligned, the launch's own until it has run: the ranked box table, the
 * flags and the mask.  Every loop is bounded by an integer count. */
#define PCR_NMS_MAX 4096
int pcr_nms_ok(int N);
int pcr_nms_ws_bytes(int N);
int pcr_nms_f32(const float *boxes, const float *scores, const float *thresh, int *order, int *keep, int *count,
                int *info, void *ws, int N, int kind, int pre_max, pcr_stream_t stream);

/* pcr_track_nms_f32: the tracker's rule (virtual_tracker.py:249-255), pairwise and NOT greedy.  boxes5 (N,5) (angle
 * ignored: the tracker compares nearest_bev boxes), classes (N) int32, scores (N), thresh (device, 1 float) ->
 * suppressed (N) int32, every element written, 0 or 1.  For every i < j with classes[i] == classes[j] and
 * iou_normal(box i, box j) > thresh: i is suppressed if scores[i] - scores[j] <= 0, j if that difference is > 0.
 * The reference adds -10000 to the IoU of unlike classes before the compare; an IoU is at most 1, so for every
 * thresh > -9999 that is exactly the class gate used here.  Range: pcr_nms_ok(N). */
int pcr_track_nms_f32(const float *boxes5, const int *classes, const float *scores, const float *thresh,
                      int *suppressed, int N, pcr_stream_t stream);

/* ------------------------------------------------------------ A5. track state --------- */

/* The state the assignments of A3 and the masks of A4 refer to, kept on the device: a bank of C track slots that a frame
 * updates in place by fixed-shape launches.  It stands for what the reference's tracker keeps on the host between frames
 * (models/trackers/deprecated/): PointFeatureSet (tracking_feature_set.py:11-63: a store grown by torch.cat, replaced
 * through a torch.where of data-dependent shape), TrackingUpdater.__call__ (tracking_updater.py:22-98: a walk over
 * decisions[...].cpu().numpy() and lists of Track objects), Track.transform_over_time / EgoVehicle.transform_over_time
 * (track.py:116-183, tracking_manager.py:111-149: numpy on the host) and VirtualTracker.get_track_det_distances
 * (virtual_tracker.py:287-295: the detections go to the host and back).  No host read, no allocation, no atomic; the same
 * bits on every run.  Pointers are checked against NULL only (as everywhere in this header, they are not probed for
 * being device memory).
 *
 * The bank.  Slot s of C holds feats (feat_floats), xyz (xyz_floats), lengths, boxes (W floats: [x, y, z, w, l, h, rz] and,
 * for W == 9, [vx, vy]), scores, labels, ids (the global track id), steps (the reference's len(det_bboxes)) and misses
 * (its unmatchedFrameCount).  A slot is ACTIVE iff ids[s] >= 0; a free slot has ids = labels = -1 and lengths = 0, so the
 * class gate of pcr_assoc_pairs_i32 leaves it out without further code; its other entries are stale.  next_id (1) is the
 * id the next born track gets, info (1) the number of newborns the last plan dropped.
 * pcr_bank_ok: 1 <= C <= PCR_ASSOC_MAX_OBJECTS, 0 <= D <= PCR_ASSOC_MAX_OBJECTS, W == 7 or 9,
 * 0 <= feat_floats, xyz_floats <= PCR_BANK_MAX_ROW.
 *
 * pcr_bank_plan_i32 makes one frame's decisions and updates the small state IN PLACE (everything but feats / xyz).
 * Inputs: track_to_det (C), det_to_track (D) as the assignment gives them (anything outside the range means none),
 * det_labels / det_lengths (D) int32, det_boxes (D,W), det_scores (D); optional masks born (D), kill (C) int32; optional
 * carry (12): a row-major 3 x 4 affine that takes the previous sweep's frame to the current one; frame_limit >= 1 and the
 * flags replace_all, reset_on_match, propagate.  The det_* pointers, det_slot and det_id may be NULL when D == 0.
 * Outputs: src (C): the detection whose features go into the slot, or -1 (pcr_bank_move_f32 reads it); det_slot / det_id
 * (D): the slot and the global id of the track a detection joined (the reference's dets_to_trk_idx), -1 for none.
 * The result is DEFINED by these rules over the state as it was BEFORE the launch (tests/track_ref.py::plan restates
 * them; the kernel equals it bit for bit):
 *   killed   slot s is active and kill != NULL and kill[s] != 0: ids = labels = -1, lengths = 0, whatever else holds;
 *   matched  s is active, not killed, d = track_to_det[s] lies in [0, D), det_labels[d] >= 0 and det_to_track[d] == s
 *            (the two maps must agree: nothing is trusted).  boxes[s], scores[s], labels[s] are the detection's,
 *            steps += 1, misses = 0 if reset_on_match and unchanged otherwise (the reference's reset is commented out,
 *            track.py:78-79).  If replace_all or lengths[s] <= det_lengths[d] (replace_old's rule): lengths[s] =
 *            det_lengths[d] and src[s] = d; otherwise lengths stays and src[s] = -1.  det_slot[d] = s, det_id[d] = ids[s];
 *   missed   s is active, neither killed nor matched: misses += 1; if misses >= frame_limit the slot is freed like a
 *            killed one (tracking_updater.py:133-139).  Otherwise, if propagate (update_track_false_negative; without
 *            it the track only waits, update_track_unmatched): the centre becomes
 *              x' = x + vx / 2, y' = y + vy / 2 for W == 9 (x' = x, y' = y for W == 7), z' = z, and then, unless carry is
 *              NULL, row i of the box centre = ((carry[4i] * x' + carry[4i+1] * y') + carry[4i+2] * z') + carry[4i+3],
 *            each operation rounded to binary32, nothing contracted; size, yaw and velocity stay (track.py:168-181);
 *            scores *= 0.01f and steps += 1 (add_false_negative_timestep, :97-113).  src[s] = -1;
 *   born     detection d has det_labels[d] >= 0, is the detection of no matched slot, and born == NULL or born[d] != 0.
 *            The k-th such detection in index order takes the k-th slot that was free BEFORE the launch, in slot order
 *            (a slot freed by this launch is reused from the next one on): ids = next_id + k, steps = 1, misses = 0,
 *            labels, boxes, scores, lengths from the detection, src = d; det_slot[d] / det_id[d] name them.  Newborns
 *            beyond the free slots are dropped (det_slot = det_id = -1); info[0] = how many, and next_id advances by the
 *            number really born.  A free slot that takes no newborn is left as it is, src = -1.
 * One workgroup: every cross-thread read of the old state (ids, the maps) happens before the first barrier; the two
 * ranks are ballots and popcounts per 64-entry word plus a prefix over the words in LDS, and a slot_of_rank / det_of_rank
 * pair of LDS tables joins the k-th birth to the k-th free slot.  A slot is written by its owner thread only.
 *
 * pcr_bank_move_f32: for every slot s with src[s] in [0, D): feats[s] = det_feats[src[s]], xyz[s] = det_xyz[src[s]]; any
 * other slot keeps its bits.  16-byte accesses where the row size is a multiple of 4 floats and both bases are 16-byte
 * aligned (decided per array), 4-byte accesses otherwise.  Grid (row chunk, slot): the workgroups of an idle slot leave at
 * once.  Nothing to do: D == 0 or feat_floats + xyz_floats == 0.
 *
 * pcr_bank_dist_f32: out (C,D), EVERY element written: 0 for a free slot, otherwise the BEV distance between the stored
 * centre and the detection's centre taken back into the previous frame (get_track_det_distances, in the direct form;
 * the reference's torch.cdist may take the matmul form, which is less exact):
 *   px = ((m[0] * x + m[1] * y) + m[2] * z) + m[3], py with m[4..7], m = carry_inv (12), (px, py) = (x, y) for NULL;
 *   dx = boxes[s][0] - px, dy = boxes[s][1] - py, out = sqrtf(dx * dx + dy * dy), IEEE (correctly rounded) square root.
 * Nothing to do: D == 0.
 *
 * pcr_bank_retire_i32: every active slot with mask[s] != 0 is freed (ids = labels = -1, lengths = 0): the pruning of
 * activeTracks by pcr_track_nms_f32's mask, run after the update as the reference does (tracking_updater.py:96). */
#define PCR_BANK_MAX_ROW 1048576
typedef struct pcr_bank {
  int C, D, W;
  int frame_limit, replace_all, reset_on_match, propagate;
  int *lengths;   /* state (C ...), updated in place */
  float *boxes, *scores;
  int *labels, *ids, *steps, *misses, *next_id, *info;
  const int *track_to_det, *det_to_track, *det_labels, *det_lengths;   /* the frame */
  const float *det_boxes, *det_scores;
  const int *born, *kill;
  const float *carry;
  int *src, *det_slot, *det_id;   /* the decisions */
} pcr_bank;
int pcr_bank_ok(int C, int D, int W, int feat_floats, int xyz_floats);
int pcr_bank_plan_i32(const pcr_bank *p, pcr_stream_t stream);
int pcr_bank_move_f32(const int *src, const float *det_feats, const float *det_xyz, float *feats, float *xyz, int C, int D,
                      int feat_floats, int xyz_floats, pcr_stream_t stream);
int pcr_bank_dist_f32(const float *boxes, const int *ids, const float *det_boxes, const float *carry_inv, float *out,
                      int C, int D, int W, pcr_stream_t stream);
int pcr_bank_retire_i32(const int *mask, int *labels, int *ids, int *lengths, int C, pcr_stream_t stream);

/* ------------------------------------------------------------ A6. crop store ---------- */

/* The loader side of training and evaluation with the crop set resident on the device: what the reference does per item
 * on the host -- one file read per cloud, subsamplePC (datasets/utils.py:606-621) and the training pair rule
 * (ReIDDatasetNuscenesFP.__getitem__, datasets/reidentification_nuscenes.py:37-72, with get_random_other_even_train,
 * get_class_list_density and get_random_frame_even, reidentification_base.py:316-357, object_loader_base.py:201-238) on
 * numpy's global generator -- as two launches over tables that are uploaded once (pcr_amd/store.py builds them).  No host
 * read, no allocation, no synchronisation; the same bits on every run.  tests/store_ref.py restates both.
 *
 * The word.  Every sample is a 32-bit word of a counter-based generator keyed by (seed, stream, key, k), with the mix of
 * section A2:
 *       mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (uint32)
 *       h = mix((uint32)seed ^ 0x9e3779b9); h = mix(h ^ (uint32)(seed >> 32)); h = mix(h ^ stream); h = mix(h ^ key);
 *       W(seed, stream, key, k) = mix(h ^ k)
 *       pick(u, len) = ((uint64)u * len) >> 32
 *   stream 1 is the pair rule, stream 2 the gather.  seed is a DEVICE pointer to one int64 (NULL = 0), read at run time:
 *   a captured launch draws fresh samples once that word changes.  The stream of samples is not numpy's; the
 *   distribution is.
 *
 * info (1) is a word of sticky flags that both launches OR into and never clear (the caller zeroes it when it wants to):
 *   PCR_STORE_INFO_RETRY  an item's PCR_STORE_PAIR_ATTEMPTS candidate picks all hit its own object (see below);
 *   PCR_STORE_INFO_ITEM   an item the tables cannot serve (index out of range, fewer than two observations, a class or
 *                         pool without a bucket of two objects): its rows, labels and ids are -1;
 *   PCR_STORE_INFO_ROW    a row >= R, or a row whose offsets do not lie in order inside [offsets[0], offsets[R]].
 *
 * pcr_store_gather_f32: subsamplePC of B stored crops.  points (total,3) f32; offsets (R+1) int64 ascending: crop r is
 * points[offsets[r] .. offsets[r+1]); rows (B) int32; keys (B) int32 or NULL (key = b); rand (B*n) int32 read as bits, or
 * NULL -> clouds (B,n,3), sizes (B) = the stored length of the row.  With len = sizes[b]:
 *   len <= 2 -> zeros; len == n -> the stored points in order; otherwise slot s takes point pick(u, len) of the crop,
 *   u = rand[b*n + s], or W(seed, 2, keys[b], s).
 *   rows[b] < 0 is padding: zeros, size 0.  A row >= R gives zeros and size 0 too and sets PCR_STORE_INFO_ROW: no address
 *   outside points[offsets[0] .. offsets[R]) is ever read.
 * One wave per cloud, lanes over the cloud's 3n floats: every store of a wave is 64 consecutive words.  The two clouds of
 * a batch of pairs go through ONE launch: rows (2B) = (pair, side), key 2 * key + side.  1 <= n <= PCR_STORE_MAX_SAMPLES.
 *
 * pcr_store_train_pairs_i32: TrainPairs.__getitem__ for B items, one thread each.  items (B): object indices; keys (B);
 * rand (B * PCR_STORE_PAIR_WORDS) int32 or NULL: word k of item b, in the place of W(seed, 1, keys[b], k) (for tests)
 * -> rows (B,2), labels (B,2), ids (B,2).  The tables (int32, on the device), every order the one the host rule indexes:
 *   obj_cls, obj_fp, obj_id (num_objects);
 *   nums_off (num_objects + 1), nums_rows: the rows of an object's usable observations, ascending observation number;
 *   bucket_off (num_objects * PCR_STORE_BUCKETS + 1), bucket_rows: CSR over (object, point-count bucket [2^b, 2^(b+1)))
 *     of the same rows, bucket by bucket;
 *   pool_off (2 * num_classes * PCR_STORE_BUCKETS + 1), pool_objs: CSR over (pool: 0 true objects, 1 false positives;
 *     class; bucket) of the indices of the objects with an observation in the bucket, in table order.
 * With c the item's class, n its number of usable observations, and the item's draws W0, W1, ... counted from 0:
 *   W0 >> 31 == 1: a POSITIVE.  ia = pick(W1, n), j = pick(W2, n - 1), ib = j + (j >= ia); rows = nums[ia], nums[ib];
 *     labels (c, c); both ids the object's.
 *   otherwise a NEGATIVE.  rows[0] = nums[pick(W1, n)].  Density: r = pick(W2, n), d = the bucket that holds the r-th
 *     entry of the object's bucket_rows (a draw from the object's own bucket distribution).  use_tp = W3 >> 31 == 1.
 *     Candidates: from d down to 0, then from 0 up, the first bucket d' of (pool, c) with at least two objects.
 *     Partner: pool_objs entry pick(W(4 + t), len) for attempts t = 0 .. PCR_STORE_PAIR_ATTEMPTS - 1 until it is not the
 *     item's own object; after that many failures the first entry that is not, and PCR_STORE_INFO_RETRY.  Observation:
 *     from d' down to 0, then from 0 up, the partner's first non-empty bucket; rows[1] = its entry pick(W, len), W the
 *     item's next draw.  labels (c, c) from the true pool, (c, c + num_classes) from the false positives;
 *     ids[1] = -1 for a false positive. */
#define PCR_STORE_BUCKETS 20
#define PCR_STORE_PAIR_ATTEMPTS 32
#define PCR_STORE_PAIR_WORDS 40
#define PCR_STORE_MAX_SAMPLES 65536
#define PCR_STORE_INFO_RETRY 1
#define PCR_STORE_INFO_ITEM 2
#define PCR_STORE_INFO_ROW 4
typedef struct pcr_store_tables {
  int num_objects, num_classes;
  const int *obj_cls, *obj_fp, *obj_id;
  const int *nums_off, *nums_rows;
  const int *bucket_off, *bucket_rows;
  const int *pool_off, *pool_objs;
} pcr_store_tables;
int pcr_store_gather_f32(const float *points, const long long *offsets, int R, const int *rows, const int *keys,
                         const int *rand, const long long *seed, float *clouds, int *sizes, int *info, int B, int n,
                         pcr_stream_t stream);
int pcr_store_train_pairs_i32(const pcr_store_tables *tables, const int *items, const int *keys, const int *rand,
                              const long long *seed, int *rows, int *labels, int *ids, int *info, int B,
                              pcr_stream_t stream);

/* ------------------------------------------------------------ A7. ground truth -------- */

/* Scoring the tracker of A3 - A5 against ground-truth tracks, the last host-side half of the reference's
 * VirtualTracker.step (models/trackers/deprecated/): get_iou_idx (virtual_tracker.py:186-229: detections matched to
 * ground-truth boxes by centre distance or IoU plus a +10000 class mask, scipy on a host copy, a threshold through
 * torch.where), TrackingDecisionModifier.__call__ (tracking_decision_modifier.py:62-129 with the four rules at :35-59: the
 * frame's TRUE decisions, np.intersect1d on host copies), get_stats (:132-172) with get_scene_metrics
 * (virtual_tracker.py:1008-1017), update_gt_track_mapping (:297-347) and teacher forcing in mode 'gt' (:620-622,
 * tracking_decision_modifier.py:200-208).  Here: a cost launch, pcr_lsa_f32 of A3 over it as a (1, D, G) problem, one
 * launch before pcr_bank_plan_i32 and one after the update and the track NMS.  Fixed shapes, no host read, no allocation,
 * no float atomic (integer sums and minima in LDS only: their result does not depend on the order); the same bits on
 * every run; every loop is bounded by an integer count.  Pointers are checked against NULL only.
 * pcr_truth_ok: 1 <= C <= PCR_ASSOC_MAX_OBJECTS, 0 <= D, G <= PCR_LSA_MAX, W == 7 or 9, 1 <= gt_cap <= PCR_TRUTH_MAX_IDS.
 *
 * Validity.  A detection d is VALID iff det_labels[d] >= 0; a ground-truth box j iff gt_labels[j] >= 0 and gt_ids[j] lies
 * in [0, gt_cap).  Anything else is PADDING.  (This rule is ours: the reference has no padding, and its class mask gives
 * two entries of equal label -1 a zero.)  Padding takes part in the assignment the way an entry of another class does in
 * the reference: a padding row that has to take a real column pays 10000 plus its distance to it, and which columns are
 * left to such rows is part of the optimum, so it can move real pairs.  Where a frame holds as many valid detections as
 * valid ground-truth boxes and D == G, the padding rows take the padding columns (zero boxes: 10000 flat) and the real
 * boxes are assigned as in the unpadded problem; so are they with an IoU base, which lies in [-1, 0].  With D == G and
 * fewer valid detections than valid ground-truth boxes -- any frame with a missed object -- it does happen: a detection at
 * (10, 0), its object at (9.7, 0) and a missed object at (20, 0) cost 10019.7 with the detection on the missed object
 * and the padding row on its own, against 10020.3 for the true pair.  It is avoidable by the shape: with
 * G >= D + (the most valid ground-truth boxes of a frame) every row has a padding column of its own at 10000 flat and no
 * padding row takes a real column (with the roles swapped where D > G).  What then remains is the reference's own: a valid
 * detection without a partner of its class still pays 10000 plus a distance somewhere.
 *
 * pcr_truth_cost_f32: det_boxes (D,W), det_labels (D), gt_boxes (G,W), gt_labels / gt_ids (G), iou (D,G) or NULL ->
 * cost (D,G), EVERY element written:
 *   base = sqrtf(dx * dx + dy * dy), dx = det_boxes[d][0] - gt_boxes[g][0], dy likewise with [1], for iou == NULL
 *          (Center2DRange, :31-42, in the direct form as pcr_bank_dist_f32: the reference's cdist may take the matmul
 *          form), and base = -iou[d*G + g] otherwise;
 *   cost = base + m, m = 10000.0f where the labels differ or either side is padding, 0.0f otherwise; each operation
 *          rounded to binary32, nothing contracted, IEEE square root.
 * Nothing to do: D == 0 or G == 0.
 *
 * pcr_truth_decide_i32: one launch (one workgroup) over the bank's state as it is BEFORE pcr_bank_plan_i32.  Inputs: ids
 * (C), the book slot_gt / slot_tte (C): the ground-truth track id a slot's track was last seen as (-1: a false positive
 * or none) and its time to end; col4row (D), row4col (G), info (1) of the assignment over cost (D,G); thresh (device, 1
 * float: a replayed graph re-reads it); gt_labels / gt_ids / gt_tte (G); det_labels (D); the tracker's own track_to_det
 * (C), det_to_track (D) and the optional born (D) / kill (C) with pcr_bank_plan_i32's meaning.  The D-sized pointers may
 * be NULL when D == 0, the G-sized ones when G == 0.  The result is DEFINED by these rules (tests/truth_ref.py::decide
 * restates them; the kernel equals it bit for bit):
 *   det_gt (D)       det_gt[d] = j iff info[0] == 0, j = col4row[d] lies in [0, G), row4col[j] == d (nothing is
 *                    trusted), d and j are valid and of one label, and cost[d*G + j] < thresh[0], strictly (get_iou_idx's
 *                    `<`); -1 otherwise.  Such a d is a TRUE POSITIVE and g(d) = gt_ids[det_gt[d]] its track.
 *   true_t2d (C), true_d2t (D)   slot s HOLDS id g iff s is active, slot_gt[s] == g >= 0 and no lower slot does (np.
 *                    intersect1d's first occurrence; the reference cannot hold one id twice, a bank driven by a learned
 *                    head can).  The holder of g(d) and the LOWEST true positive d of that id belong together
 *                    (true_t2d[s] = d, true_d2t[d] = s); everything else is -1.
 *   det_truth (D)    -1 padding; 0 match (true_d2t >= 0); 1 newborn: any other true positive; 2 false positive: a valid
 *                    detection that is no true positive.
 *   track_truth (C)  -1 a free slot; 0 match (true_t2d >= 0); 2 false positive: slot_gt[s] < 0 or slot_tte[s] < 0;
 *                    1 false negative: the rest.  The classes are exclusive, in the order match, false positive, false
 *                    negative (the reference's sets can overlap only for a track whose stored tte contradicts its ground
 *                    truth: matched by id while its tte says the track has ended).
 *   the tracker's own decisions, by pcr_bank_plan_i32's rules: a slot is killed, matched (the two maps agree) or missed;
 *                    a valid detection is matched, else born (born == NULL or born[d] != 0; a birth that the plan later
 *                    drops for want of a slot still counts), else rejected.
 *   stats            for kind k of PCR_TRUTH_DET_MATCH .. PCR_TRUTH_TRACK_FP, with the true set / the tracker's set:
 *                    match (true_d2t >= 0 / matched), newborn (det_truth 1 / born), det false positive (det_truth 2 /
 *                    rejected), track false negative (track_truth 1 / missed), track false positive (track_truth 2 /
 *                    killed): stats[3k] += |true| (gt), stats[3k+1] += |both| (correct; for the match kind the (slot,
 *                    detection) PAIRS in both), stats[3k+2] += |tracker's| (num_pred); PCR_TRUTH_TOTAL_GT / _CORRECT add
 *                    up gt and correct over the kinds (get_stats).  skip_empty != 0 keeps the reference's quirk: a kind
 *                    whose true set is empty in a frame adds nothing that frame, num_pred included (:139-140).
 * Teacher forcing in mode 'gt' needs no entry of its own: true_t2d / true_d2t, det_truth == 1 and track_truth == 2 are
 * pcr_bank_plan_i32's track_to_det / det_to_track, born and kill.  forced != 0 says that these are the decisions the
 * frame applies: the tracker's sets ARE the true sets then (track_to_det, det_to_track, born and kill are not read and
 * may be NULL), so every kind counts gt == correct == num_pred.  (The reference scores the head's own decisions in
 * both modes; forced == 0 does.)
 *
 * pcr_truth_record_i32: one launch (one workgroup) AFTER the update and the track NMS.  ids (C) are read as they are NOW;
 * track_truth tells which slots were active before the frame; det_slot / det_id (D) are the plan's, det_gt decide's (an
 * entry outside [0, G), or whose ground-truth box is padding, counts as -1).
 *   the book   (update_gt_track_mapping) per slot s, in this order: if track_truth[s] >= 0: slot_tte[s] -= 1; if a
 *              detection d has det_slot[d] == s (the lowest such d): (slot_gt, slot_tte)[s] = (g(d), gt_tte[det_gt[d]])
 *              for a true positive and (-1, -1) otherwise; if ids[s] < 0: (-1, -1), so that stale truth cannot reach the
 *              slot's next occupant.
 *   MOT        (an addition: the reference keeps none) stats[PCR_TRUTH_FRAMES] += 1; GT_TOTAL += the valid ground-truth
 *              boxes; TP += the true positives; FP += the valid detections that are none; FN += the valid ground-truth
 *              boxes that are no true positive's; for a true positive d with g = g(d) and i = det_id[d]: if i < 0:
 *              UNTRACKED += 1; and, for the lowest true positive of g only (ids are distinct in a sane frame): if
 *              gt_last[g] >= 0 and gt_last[g] != i: SWITCHES += 1; then gt_last[g] = i.  gt_last (gt_cap) starts at -1. */
#define PCR_TRUTH_MAX_IDS 65536
#define PCR_TRUTH_DET_MATCH 0
#define PCR_TRUTH_DET_NEWBORN 1
#define PCR_TRUTH_DET_FP 2
#define PCR_TRUTH_TRACK_FN 3
#define PCR_TRUTH_TRACK_FP 4
#define PCR_TRUTH_TOTAL_GT 15
#define PCR_TRUTH_TOTAL_CORRECT 16
#define PCR_TRUTH_FRAMES 17
#define PCR_TRUTH_GT_TOTAL 18
#define PCR_TRUTH_TP 19
#define PCR_TRUTH_FP 20
#define PCR_TRUTH_FN 21
#define PCR_TRUTH_SWITCHES 22
#define PCR_TRUTH_UNTRACKED 23
#define PCR_TRUTH_STATS 24
typedef struct pcr_truth {
  int C, D, G, gt_cap, skip_empty, forced;
  const int *ids;                                            /* the bank's (C) */
  int *slot_gt, *slot_tte, *gt_last, *stats;                 /* the book: (C), (C), (gt_cap), (PCR_TRUTH_STATS) */
  const int *col4row, *row4col, *info;                       /* the assignment over cost */
  const float *cost, *thresh;
  const int *gt_labels, *gt_ids, *gt_tte, *det_labels;       /* the frame */
  const int *track_to_det, *det_to_track, *born, *kill;      /* the tracker's own decisions */
  int *det_gt, *true_t2d, *true_d2t, *det_truth, *track_truth;   /* decide writes them, record reads det_gt, track_truth */
  const int *det_slot, *det_id;                              /* record: the plan's */
} pcr_truth;
int pcr_truth_ok(int C, int D, int G, int W, int gt_cap);
int pcr_truth_cost_f32(const float *det_boxes, const int *det_labels, const float *gt_boxes, const int *gt_labels,
                       const int *gt_ids, const float *iou, float *cost, int D, int G, int W, int gt_cap,
                       pcr_stream_t stream);
int pcr_truth_decide_i32(const pcr_truth *p, pcr_stream_t stream);
int pcr_truth_record_i32(const pcr_truth *p, pcr_stream_t stream);

/* ------------------------------------------------------------ A8. ranking a gallery -------- */

/* The other use of a re-identification model: for every query object, which gallery objects is it, and how often does
 * the right one come first.  (The reference asks the question inside its tracker, VirtualTracker.
 * log_reid_matching_score, trackers/deprecated/virtual_tracker.py:350-430; that code does not run.)  Three launches
 * of fixed shape, no host read, no allocation, no atomic; the same bits on every run; every loop is bounded by an integer
 * count.  The result is DEFINED by the rules below (tests/rank_ref.py restates them; the kernels equal it bit for bit).
 * Pointers are checked against NULL only.
 * pcr_rank_ok: 0 <= Q <= PCR_RANK_MAX_QUERIES, 0 <= G <= PCR_RANK_MAX_GALLERY, 1 <= K <= PCR_RANK_MAX_K,
 * 0 <= cap <= Q * G (in 64-bit arithmetic).
 *
 * pcr_rank_scores_f32: logits (cap), pairs (cap,2), count (1, device) -> scores (Q,G), EVERY element written:
 * scores[q][g] = logits[k] for the listed pairs k < min(count[0], cap) (a negative count is 0) with (q, g) = pairs[k]
 * inside [0,Q) x [0,G); -inf ("not a candidate") elsewhere.  A pair outside the range is skipped.  The listed pairs must be
 * distinct (pcr_assoc_pairs_i32's are).  This is the score image of pcr_assoc_cost_multi_f32's softmax kind, restated so
 * that the ranking takes any dense score matrix as well.  Nothing to do: Q * G == 0.
 *
 * pcr_rank_gallery_f32: one wave per query q over its row of scores (Q,G), staged in LDS.  query_ids (Q), gallery_ids (G):
 * a value < 0 is "no identity"; exclude (Q) or NULL.  Every element of every output is written.
 *   candidates  gallery g is a CANDIDATE of q iff scores[q][g] != -inf and g != exclude[q] (NULL, or a value outside
 *               [0,G): nothing is excluded).  +inf is an ordinary score.  If any candidate's score is a NaN, info[q] = 1 and
 *               the query is not ranked: topk_idx -1, topk_score -inf, n_cand = n_true = 0, first_hit = -1, ap = 0.
 *               Otherwise info[q] = 0.  (A NaN at an excluded slot is no candidate's.)
 *   order       descending score; equal scores, lowest gallery index first.  Equality is the float compare: -0 == +0.
 *   rank        rank(g) = #{candidates j : s_j > s_g, or s_j == s_g and j < g}.
 *   top-k       topk_idx[q][r] (Q,K) = the candidate of rank r for r < min(K, n_cand[q]), -1 beyond; topk_score[q][r] its
 *               score as stored (the sign of a zero included), -inf beyond.  n_cand (Q) = the number of candidates.
 *   truth       the TRUE set = {candidates g : query_ids[q] >= 0 and gallery_ids[g] == query_ids[q]}; n_true (Q) its size,
 *               first_hit (Q) its least rank, -1 when it is empty -- exact whatever K is.
 *   ap          with the true candidates' ranks ascending r_0 < r_1 < ...: ap = (sum_i (i+1)/(r_i+1)) / n_true; each
 *               quotient an IEEE binary64 division of two integers converted to binary64, the sum in ascending i in
 *               binary64, the last division in binary64, rounded to binary32 once.  0 when n_true == 0.
 * Cost: one read of the row, then min(K, n_cand) + n_true passes over it in LDS (top-k: rounds of a 64-bit wave maximum
 * over (order-preserving score bits, inverted index); a true candidate's rank: ballot popcounts over the row).
 * Nothing to do: Q == 0.  With G == 0 every query is empty and the outputs are still written.
 *
 * pcr_rank_accumulate: one launch (one wave) adds a chunk's per-query results to a persistent table, so that an
 * evaluation over chunks of queries makes no host read.  valid (1, device) or NULL: only the queries
 * q < clamp(valid[0], 0, Q) count; NULL = all Q.  A query is FLAGGED iff info[q] != 0, SCORED iff info[q] == 0 and
 * n_true[q] > 0 (then first_hit[q] >= 0), UNSCORED otherwise.
 *   counts (3 + nranks)   counts[0] += scored, counts[1] += unscored, counts[2] += flagged,
 *                         counts[3 + i] += #{scored q : first_hit[q] < ranks[i]}; nranks <= PCR_RANK_MAX_RANKS values
 *                         ranks[i] in [1, G].
 *   sums (2, binary64)    for q ascending over the scored queries: sums[0] = sums[0] + (double)ap[q], sums[1] = sums[1] +
 *                         1.0 / (double)(first_hit[q] + 1) -- each a running binary64 sum that starts at the table's value,
 *                         so two chunks added one after the other equal their union added at once.
 * Nothing to do: Q == 0. */
#define PCR_RANK_MAX_QUERIES 65535
#define PCR_RANK_MAX_GALLERY 4096
#define PCR_RANK_MAX_K 64
#define PCR_RANK_MAX_RANKS 8
typedef struct pcr_rank {
  int Q, G, K;
  const float *scores;                                       /* (Q,G) */
  const int *query_ids, *gallery_ids, *exclude;              /* (Q), (G), (Q) or NULL */
  int *topk_idx;                                             /* (Q,K) */
  float *topk_score;                                         /* (Q,K) */
  int *n_cand, *n_true, *first_hit;                          /* (Q) */
  float *ap;                                                 /* (Q) */
  int *info;                                                 /* (Q) */
} pcr_rank;
typedef struct pcr_rank_acc {
  int Q, G, nranks;
  int ranks[8];                                              /* PCR_RANK_MAX_RANKS */
  const int *n_true, *first_hit, *info;                      /* (Q): pcr_rank_gallery_f32's */
  const float *ap;                                           /* (Q) */
  const int *valid;                                          /* (1) device, or NULL */
  int *counts;                                               /* (3 + nranks) */
  double *sums;                                              /* (2) */
} pcr_rank_acc;
int pcr_rank_ok(int Q, int G, int K, int cap);
int pcr_rank_scores_f32(const float *logits, const int *pairs, const int *count, float *scores, int Q, int G, int cap,
                        pcr_stream_t stream);
int pcr_rank_gallery_f32(const pcr_rank *p, pcr_stream_t stream);
int pcr_rank_accumulate(const pcr_rank_acc *p, pcr_stream_t stream);

/* ------------------------------------------------------------ A9. identity preservation -------- */

/* Did an object keep one identity over its whole life?  The MOT counters of A7 count a switch once, however long the wrong
 * identity is then kept; this section keeps what the identity metrics need (IDF1 / IDP / IDR; per trajectory MT / PT / ML,
 * FRAG, TID, LGD; MOTP) in persistent tables on the device: one launch per frame after pcr_truth_record_i32, and at the
 * end of a scene a compaction, pcr_lsa_f32 of A3 as a (1, max_rows, max_cols) problem and a score launch.  (An addition:
 * the reference keeps none of it.)  Fixed shapes, no host read, no allocation, no float atomic (integer sums, minima and
 * maxima only: their result does not depend on the order); the same bits on every run; every loop is bounded by an integer
 * count; every element of every output is written.  Pointers are checked against NULL only.  The result is DEFINED by the
 * rules below (tests/ident_ref.py restates them; the kernels equal it bit for bit, the binary64 sums included).
 * pcr_ident_ok: D and G as in pcr_truth_ok (0 <= D, G <= PCR_LSA_MAX), 1 <= gt_cap <= PCR_TRUTH_MAX_IDS, 1 <= gt_rows,
 * id_cap <= PCR_IDENT_MAX_DIM, gt_rows * id_cap <= PCR_IDENT_MAX_CELLS, 1 <= max_rows, max_cols <= PCR_LSA_MAX.
 *
 * The notions are pcr_truth_record_i32's, unchanged: a detection d is VALID iff det_labels[d] >= 0, a ground-truth box j
 * iff gt_labels[j] >= 0 and gt_ids[j] lies in [0, gt_cap); d is a TRUE POSITIVE iff it is valid, j = det_gt[d] lies in
 * [0, G) and box j is valid; then g = gt_ids[j] is its track and i = det_id[d] the identity the tracker gave it.  Every
 * index is checked against its range before it addresses memory: det_gt[d], gt_ids[j], det_id[d], g and i; a value out of
 * range has the meaning stated here or counts as -1.
 *
 * Scene state.  cooc (gt_rows, id_cap) int32; gt_track (gt_rows, PCR_IDENT_TRACK_COLS) int32 with the columns
 * PCR_IDENT_PRESENT .. PCR_IDENT_LAST; totals (PCR_IDENT_TOTALS) int32; dist_sum (1) binary64.  All start at zero.
 *
 * pcr_ident_record_i32: one launch (one workgroup) per frame, AFTER pcr_truth_record_i32, over its buffers as they stand.
 *   tracks   an id g is PRESENT iff a valid ground-truth box carries it -- once, however many boxes do.  The LOWEST true
 *            positive of g is the least d among the true positives whose track is g (over all boxes that carry g).  g is
 *            TRACKED this frame iff that d exists and det_id[d] >= 0.  For every present g < gt_rows: PRESENT += 1; if
 *            tracked: TRACKED += 1; if EVER and LAST == 0: FRAGS += 1; if not EVER: FIRST_GAP = CUR_GAP; then EVER = 1,
 *            CUR_GAP = 0, LAST = 1; if not tracked: CUR_GAP += 1, LONGEST_GAP = max(LONGEST_GAP, CUR_GAP), LAST = 0.  An
 *            absent g keeps its row.  A present g >= gt_rows has no row: totals[PCR_IDENT_T_DROPPED_GT] += 1 instead.
 *   cooc     for every tracked g < gt_rows with i = det_id[d] of its lowest true positive: i < id_cap: cooc[g][i] += 1;
 *            otherwise totals[PCR_IDENT_T_DROPPED_ID] += 1.  One writer per g: the writes do not race.
 *   totals   FRAMES += 1; GT_TOTAL += the valid ground-truth boxes; PRED_TOTAL += the valid detections with det_id >= 0
 *            (a propagated track without a detection is no prediction here); TP += the true positives;
 *   dist_sum for the true positives in ascending d: dist_sum = dist_sum + (double)cost[d*G + det_gt[d]], a running binary64
 *            sum that starts at the stored value (cost is pcr_truth_cost_f32's: the centre distance, or -iou).
 * The D-sized pointers may be NULL when D == 0, the G-sized ones when G == 0, cost when D * G == 0.
 *
 * pcr_ident_compact_f32: the scene's problem, gathered.  Row g of cooc is ACTIVE iff it holds a non-zero count, column i
 * likewise.  flags (gt_rows + id_cap) int32 is workspace (row then column activity, every element written).
 *   counts (PCR_IDENT_COUNTS)  N_ROWS / N_COLS = the number of active rows / columns, whatever max_rows / max_cols are;
 *            MAX_COUNT = the largest count of cooc (0 for an all-zero matrix); the last is written 0.
 *   row_list (max_rows), col_list (max_cols)  the active rows / columns ascending, as many as fit; -1 beyond.
 *   cost (max_rows, max_cols)  -(float)cooc[row_list[r]][col_list[c]] for r < N_ROWS and c < N_COLS, +0.0f in the padding;
 *            all +0.0f when N_ROWS > max_rows or N_COLS > max_cols (OVERFLOW).  Zeros do not change the optimum total: every
 *            count is >= 0.
 * Launches: a clear, a sweep of the whole matrix (a row's activity by ballot, a column's by the thread that owns it over the
 * rows of its workgroup, the maximum by an integer atomic), the ranks by one workgroup (ballot, lanes below, a prefix over
 * its waves, a running base from chunk to chunk), the gather.
 *
 * pcr_ident_score_i32: one launch (one workgroup) after pcr_lsa_f32 over cost -> col4row (max_rows), info (1).
 *   OVERFLOW iff N_ROWS > max_rows or N_COLS > max_cols; INEXACT iff info[0] != 0 or
 *            (min(max_rows, max_cols) + 1) * MAX_COUNT >= 2^24 in 64-bit arithmetic: below that every solver operation is
 *            exact in binary32 (all values are integers of magnitude < 2^24) and the total is the true optimum, whatever
 *            the ties.
 *   IDTP_scene = sum over r < N_ROWS with c = col4row[r] in [0, N_COLS) of cooc[row_list[r]][col_list[c]]; 0 on OVERFLOW or
 *            info[0] != 0.
 *   id_map (gt_rows)  id_map[row_list[r]] = col_list[c] for those pairs whose count is > 0; -1 everywhere else.
 *   table (PCR_IDENT_TABLE) 64-bit integers, ADDED to, so that scene after scene gives the pooled figures: IDTP, the
 *            four totals of the scene; over the rows g with PRESENT > 0: TRACKS += 1; MT += 1 iff 5 * TRACKED >= 4 *
 *            PRESENT, ML += 1 iff 5 * TRACKED < PRESENT, PT += 1 otherwise; FRAG += FRAGS; TID_SUM += (EVER ? FIRST_GAP :
 *            PRESENT); LGD_SUM += LONGEST_GAP; OVERFLOW / INEXACT += 1 for a scene so flagged; DROPPED_GT / DROPPED_ID +=
 *            the scene's.
 *   dist_total (1) binary64  dist_total = dist_total + dist_sum.
 * The scene state is not changed: zeroing it (the caller's) opens the next scene. */
#define PCR_IDENT_MAX_DIM 65536
#define PCR_IDENT_MAX_CELLS 67108864                         /* 2^26 */
#define PCR_IDENT_TRACK_COLS 8
#define PCR_IDENT_PRESENT 0
#define PCR_IDENT_TRACKED 1
#define PCR_IDENT_FRAGS 2
#define PCR_IDENT_FIRST_GAP 3
#define PCR_IDENT_LONGEST_GAP 4
#define PCR_IDENT_CUR_GAP 5
#define PCR_IDENT_EVER 6
#define PCR_IDENT_LAST 7
#define PCR_IDENT_TOTALS 8
#define PCR_IDENT_T_FRAMES 0
#define PCR_IDENT_T_GT_TOTAL 1
#define PCR_IDENT_T_PRED_TOTAL 2
#define PCR_IDENT_T_TP 3
#define PCR_IDENT_T_DROPPED_GT 4
#define PCR_IDENT_T_DROPPED_ID 5
#define PCR_IDENT_COUNTS 4
#define PCR_IDENT_N_ROWS 0
#define PCR_IDENT_N_COLS 1
#define PCR_IDENT_MAX_COUNT 2
#define PCR_IDENT_TABLE 16
#define PCR_IDENT_IDTP 0
#define PCR_IDENT_FRAMES 1
#define PCR_IDENT_GT_TOTAL 2
#define PCR_IDENT_PRED_TOTAL 3
#define PCR_IDENT_TP 4
#define PCR_IDENT_TRACKS 5
#define PCR_IDENT_MT 6
#define PCR_IDENT_PT 7
#define PCR_IDENT_ML 8
#define PCR_IDENT_FRAG 9
#define PCR_IDENT_TID_SUM 10
#define PCR_IDENT_LGD_SUM 11
#define PCR_IDENT_OVERFLOW 12
#define PCR_IDENT_INEXACT 13
#define PCR_IDENT_DROPPED_GT 14
#define PCR_IDENT_DROPPED_ID 15
typedef struct pcr_ident {
  int D, G, gt_cap, gt_rows, id_cap;
  const int *det_labels, *det_gt, *det_id;                   /* (D): the frame's, pcr_truth_decide_i32's, the plan's */
  const int *gt_labels, *gt_ids;                             /* (G) */
  const float *cost;                                         /* (D,G): pcr_truth_cost_f32's */
  int *cooc, *gt_track, *totals;                             /* the scene: (gt_rows,id_cap), (gt_rows,8), (PCR_IDENT_TOTALS) */
  double *dist_sum;                                          /* (1) */
} pcr_ident;
typedef struct pcr_ident_close {
  int gt_rows, id_cap, max_rows, max_cols;
  const int *cooc, *gt_track, *totals;                       /* the scene */
  const double *dist_sum;
  int *flags, *counts, *row_list, *col_list;                 /* compact: (gt_rows + id_cap), (PCR_IDENT_COUNTS), (max_rows), (max_cols) */
  float *cost;                                               /* (max_rows,max_cols) */
  const int *col4row, *info;                                 /* score: pcr_lsa_f32's over cost, (max_rows), (1) */
  int *id_map;                                               /* (gt_rows) */
  long long *table;                                          /* (PCR_IDENT_TABLE) */
  double *dist_total;                                        /* (1) */
} pcr_ident_close;
int pcr_ident_ok(int D, int G, int gt_cap, int gt_rows, int id_cap, int max_rows, int max_cols);
int pcr_ident_record_i32(const pcr_ident *p, pcr_stream_t stream);
int pcr_ident_compact_f32(const pcr_ident_close *p, pcr_stream_t stream);
int pcr_ident_score_i32(const pcr_ident_close *p, pcr_stream_t stream);

/* ------------------------------------------------------------ A10. pair head over embeddings -------- */

/* The `concat` matching head of a gallery (additive to ABI 17; reid_pts_point-transformer_baseline.py: match_type
 * 'concat', models/ReIDNet.py:455-458): a pair's input is [e_i | e_j], e = pool_channel_max(h) (M, F), and the head is
 * LinearRes(n, n, GroupNorm) + Linear(n, 1) with n = 2F (models/lanegcn_nets.py:228-241).  linear1 has no bias, so its
 * product splits into two per-OBJECT tables, W1 [e_i ; e_j] = W1[:, :F] e_i + W1[:, F:] e_j = u[i] + v[j], which the
 * caller computes once per object (pcr_dense_f32).  Per live pair p = (i, j) the launch computes
 *     z = relu(GN1(u[i] + v[j]));   y = GN2(W2 z) + [e_i | e_j];   logits[p] = w_out . relu(y) + b_out
 * (GroupNorm: biased variance, eps 1e-5).  pairs[p] = (i, j), i the FIRST argument of match_forward_inference: the head is
 * not symmetric.
 *   Arithmetic.  W2 z runs on the matrix core as f32-input MFMA (v_mfma_f32_32x32x2_f32) whatever the precision mode of
 *     the model launches; pcr_last_launch_arith() says PCR_PREC_F32 afterwards.
 *   Shapes.  pcr_pair_head_ok (shape only, never M or P): F in {32, 64, 128} and a GroupNorm group of n / groups = 4, 8, 16
 *     or 32 channels (pcr_dense_gn_f32's rule).  Anything else, n != 2F, a NULL tensor or a table that is not 16-byte
 *     aligned returns PCR_ERR_INVALID before anything is written.
 *   Batch independence.  A pair's bits never depend on the batch it travels in: not on P, not on its position in the
 *     list, not on *count.
 *   Gating (pcr_live, pairs in place of clouds, as pcr_pool_head_live_f32).  A dead pair reads nothing -- its two indices
 *     included -- and gets *dead_value (a HOST float, read when the call is made; NULL: 0.0f).  live == NULL scores all P
 *     pairs.  *count is read by the launch, so a captured graph follows it.
 *   Out-of-range indices.  A live pair with an index outside [0, M) reads nothing of the tables and gets NaN.
 *   Grid.  One launch, one-dimensional and strided over tiles of 32 pairs: P is bounded by memory alone.
 * (The block is a tagged struct followed by its typedef; the layout is the plain C one.) */
struct pcr_pair_head_params {
  int M, F, n, groups;              /* objects; embedding width; n = 2F = head width; GroupNorm groups of LinearRes */
  long P;                           /* pairs in the list */
  const float *emb;                 /* (M, F)  e = pool_channel_max(h) */
  const float *u, *v;               /* (M, n)  u = emb W1[:, :F]^T, v = emb W1[:, F:]^T */
  const int *pairs;                 /* (P, 2) int32 */
  const float *w2p;                 /* linear2 (n, n): pcr_pack_weight_f32 image */
  const float *gn1_g, *gn1_b, *gn2_g, *gn2_b, *w_out, *b_out;   /* (n) x 5, (1) */
  float *logits;                    /* (P) */
};
typedef struct pcr_pair_head_params pcr_pair_head_params;
struct pcr_live;                    /* section B, "Gated launches" */
int pcr_pair_head_ok(int F, int groups);
int pcr_pair_head_f32(const pcr_pair_head_params *p, const struct pcr_live *live, const float *dead_value,
                      pcr_stream_t stream);

/* ------------------------------------------------------------ A11. the updater as configured; the scene log ---- */

/* The reference's TrackingUpdater (models/trackers/deprecated/tracking_updater.py:22-203) applies an `update_config` to
 * every decision of a frame -- `match`, the detection decisions, the tracking decisions, each with output / active / decom
 * flags -- and returns the tracks to output, propagated ones included (virtual_tracker.py:847, 923, 1044-1071).  The two
 * entries below (additive to ABI 17) are that step and the record it feeds, as fixed-shape launches of ONE workgroup
 * without a host read, an allocation or an atomic; they write the same bits on every run.  pcr_bank_plan_i32 (A5) is
 * untouched: it stays the one-flag form.
 *
 * pcr_bank_plan_rules_i32: the bank, the frame inputs, carry, frame_limit, replace_all, reset_on_match, src, det_slot and
 * det_id of pcr_bank_plan_i32 with the same meaning.  born, kill and propagate are replaced by
 *   det_decision (D), track_decision (C)  as pcr_assoc_decode_i32 writes them: 0 = matched, 1 + i = decision i, 1 + dd /
 *                 1 + td = unmatched; any value outside that range reads as unmatched;
 *   dd, td        the decisions per side, 0 .. PCR_ASSOC_MAX_DECISIONS;
 *   match_rule, det_rule[i], trk_rule[j]  rule words of the bits PCR_RULE_OUTPUT, PCR_RULE_ACTIVE, PCR_RULE_DECOM (only
 *                 the first dd / td entries are read).  ACTIVE and DECOM together in a word that is read is
 *                 PCR_ERR_INVALID (the reference raises, update_, :190-191);
 *   trk_kind[j]   PCR_TRK_KEEP (track_false_positive: update_ only) or PCR_TRK_MISS (track_false_negative).
 * The result is DEFINED by these rules over the state as it was BEFORE the launch (tests/update_ref.py::plan_rules restates
 * them; the kernel equals it bit for bit).  "Freed" means ids = labels = -1, lengths = 0.
 *   matched  slot s is active and track_decision[s] == 0, d = track_to_det[s] lies in [0, D), det_labels[d] >= 0,
 *            det_to_track[d] == s and det_decision[d] == 0.  The slot takes A5's matched update word for word (box, score,
 *            label, steps += 1, reset_on_match, the replace_all / lengths rule for src, det_slot / det_id); then match_rule
 *            applies;
 *   keep     s is active, track_decision[s] == 1 + j, j < td, trk_kind[j] == PCR_TRK_KEEP: the state is unchanged, src = -1;
 *            then trk_rule[j] applies;
 *   miss     as keep, but trk_kind[j] == PCR_TRK_MISS: misses += 1; if misses >= frame_limit the slot is freed and not
 *            output (:136-138).  Otherwise the box is propagated by exactly the arithmetic of A5's missed rule with
 *            propagate set (carry included), scores *= 0.01f, steps += 1, src = -1; then trk_rule[j] applies;
 *   wait     every other active slot (decision 1 + td, a matched code whose maps disagree, a code out of range):
 *            misses += 1, freed at frame_limit, otherwise unchanged; never output (update_track_unmatched, :161-186);
 *   a rule   OUTPUT: row s of the output table is valid and holds the slot's id, label, score and box as they are after the
 *            update above.  Not ACTIVE: the slot is freed after its row was taken (src stays as the update left it).
 *            DECOM changes nothing in the bank; it is bit 0 of the row's flags;
 *   new      a detection d with det_labels[d] >= 0 and det_decision[d] == 1 + i, i < dd, is numbered as the reference
 *            numbers it (:36-52): grouped by decision in ascending i, by ascending d within a decision; the k-th of that
 *            order gets id = next_id + k, and next_id advances by their number whether or not they get a slot.  With ACTIVE
 *            in det_rule[i] it takes a slot as A5's born: the k-th ACTIVE one of that same order takes the k-th slot that
 *            was free BEFORE the launch (steps = 1, misses = 0, fields from the detection, src = d, det_slot / det_id
 *            written).  ACTIVE ones beyond the free slots are dropped: det_slot = -1, info[0] counts them, det_id still
 *            names the id.  With OUTPUT a slotted newborn is output in its slot's row, an unslotted one (not ACTIVE, or
 *            dropped) in row C + d from the detection's own fields.  A detection with label < 0, or with any other
 *            decision that is not a match, takes no part: det_slot = det_id = -1, no id is consumed.
 * Output table, C + D rows, EVERY element written: out_valid, out_ids, out_labels (int32), out_scores, out_boxes (C + D, W),
 * out_flags (int32: bit 0 = the rule's DECOM, bit 1 = the row is a propagated track).  An invalid row has ids = labels = -1
 * and zeros elsewhere.  info (2): [0] = dropped newborns, [1] = valid output rows.
 * The kernel follows pcr_bank_plan_i32's: every cross-thread read of the old state happens before the first barrier; the
 * ranks are ballots and popcounts per 64-entry word, one set per detection decision, with a prefix over words and decisions
 * in LDS; a slot and a row are written by their owner thread only.
 * pcr_bank_rules_ok: pcr_bank_ok(C, D, W, 0, 0) and 0 <= dd, td <= PCR_ASSOC_MAX_DECISIONS.  The det_* pointers,
 * det_decision, det_slot and det_id may be NULL when D == 0; carry may be NULL (identity).
 *
 * pcr_scene_log_append_i32: the device-side record a result file is written from.  The log has the columns frame, id,
 * label, flags (int32), score (float), box (W floats) of rows_max rows each, and cursor, dropped, frame_no (1 each, int32).
 * One append takes an R-row table in the form above (R = C + D for a bank): the valid rows (in_valid != 0) are compacted
 * in row order by ballot, popcount and a prefix over the words, and written from row cursor[0] on with frame =
 * frame_no[0].  Rows that do not fit are dropped and added to dropped[0]; cursor advances by the rows written, frame_no by
 * 1 -- a device counter, so a captured frame replays correctly.  A cursor outside [0, rows_max] reads as a full log.  One
 * writer, no atomics.  pcr_scene_log_ok: 1 <= rows_max <= PCR_LOG_MAX_ROWS, 1 <= R <= 2 * PCR_ASSOC_MAX_OBJECTS, W == 7 or 9.
 * (Both blocks are tagged structs followed by their typedefs, as in A10; the layout is the plain C one.) */
#define PCR_RULE_OUTPUT 1
#define PCR_RULE_ACTIVE 2
#define PCR_RULE_DECOM 4
#define PCR_TRK_KEEP 0
#define PCR_TRK_MISS 1
#define PCR_LOG_MAX_ROWS 16777216
struct pcr_bank_rules {
  int C, D, W;
  int frame_limit, replace_all, reset_on_match;
  int dd, td;
  int match_rule;
  int det_rule[4], trk_rule[4], trk_kind[4];                  /* PCR_ASSOC_MAX_DECISIONS each */
  int *lengths;   /* state (C ...), updated in place */
  float *boxes, *scores;
  int *labels, *ids, *steps, *misses, *next_id;
  const int *track_to_det, *det_to_track, *det_labels, *det_lengths;   /* the frame */
  const float *det_boxes, *det_scores;
  const int *det_decision, *track_decision;
  const float *carry;
  int *src, *det_slot, *det_id, *info;   /* the decisions; info (2) */
  int *out_valid, *out_ids, *out_labels;   /* the output table (C + D ...) */
  float *out_scores, *out_boxes;
  int *out_flags;
};
typedef struct pcr_bank_rules pcr_bank_rules;
struct pcr_scene_log {
  int rows_max, R, W;
  const int *in_valid, *in_ids, *in_labels;   /* the table (R ...) */
  const float *in_scores, *in_boxes;
  const int *in_flags;
  int *frame, *id, *label, *flags;   /* the log (rows_max ...) */
  float *score, *box;
  int *cursor, *dropped, *frame_no;   /* (1) each */
};
typedef struct pcr_scene_log pcr_scene_log;
int pcr_bank_rules_ok(int C, int D, int W, int dd, int td);
int pcr_bank_plan_rules_i32(const pcr_bank_rules *p, pcr_stream_t stream);
int pcr_scene_log_ok(int rows_max, int R, int W);
int pcr_scene_log_append_i32(const pcr_scene_log *p, pcr_stream_t stream);

/* ------------------------------------------------------------ A12. ranking a wide gallery -------- */

/* Section A8 beyond PCR_RANK_MAX_GALLERY entries: the score matrix is built from gallery blocks of at most
 * PCR_ASSOC_MAX_OBJECTS entries (one pair list and one scatter per block, into the block's column window), and the ranking
 * reads a query's row from global memory instead of staging it in LDS.  (An addition: a validation set of nuScenes or Waymo
 * detections gives a gallery of tens of thousands of entries.)  Fixed-shape launches, no host read, no allocation, no float
 * atomic and no global atomic (integer LDS adds only: their sum does not depend on the order); the same bits on every run;
 * every loop is bounded by an integer count.  Pointers are checked against NULL only.  Nothing of section A8 changes, and a
 * caller that stays below its limits has no reason to come here.
 * pcr_rank_wide_ok: 0 <= Q <= PCR_RANK_MAX_QUERIES, 0 <= G <= PCR_RANK_WIDE_MAX_GALLERY, 1 <= K <= PCR_RANK_MAX_K.  The
 * products Q * G and Q * width are formed in 64-bit arithmetic everywhere.
 *
 * pcr_rank_fill_f32: every element of scores (Q,G) becomes -inf ("not a candidate").  Nothing to do: Q * G == 0.
 *
 * pcr_rank_scatter_f32: the scatter half of pcr_rank_scores_f32 with a column window [col0, col0 + width): logits (cap),
 * pairs (cap,2), count (1, device); for k < min(max(count[0], 0), cap) with (q, g) = pairs[k], 0 <= q < Q and
 * 0 <= g < width: scores[q * G + col0 + g] = logits[k].  Every other element of scores is left as it is.  A pair outside the
 * range is skipped.  The listed pairs must be distinct.  Invalid without a launch: col0 < 0, width < 0, col0 + width > G,
 * cap < 0, cap > Q * width, or a NULL pointer while there is work to do (cap > 0).  Nothing to do: cap == 0.
 *
 * pcr_rank_wide_f32: pcr_rank_gallery_f32's block, fields and rules -- candidates, the NaN rule, order, rank, top-k, truth,
 * first_hit and ap with its binary64 order of operations are section A8's, word for word, and every element of every output
 * is written -- with one rule added:
 *   true cap    if no candidate's score is a NaN and the true set has more than PCR_RANK_WIDE_MAX_TRUE members, info[q] = 2
 *               and the query is not ranked: topk_idx -1, topk_score -inf, n_cand = n_true = 0, first_hit = -1, ap = 0.  A
 *               NaN among the candidates takes precedence (info[q] = 1).  pcr_rank_accumulate counts info != 0 as flagged,
 *               so such a query never reads as a miss.
 * For G <= PCR_RANK_MAX_GALLERY the true set cannot exceed the cap, and the outputs equal pcr_rank_gallery_f32's bit for bit
 * on every input.
 * Cost: one workgroup (four waves) per query, 57.6 KiB of LDS whatever G is.  The row is read from memory at most twice,
 * whatever K and n_true are, plus one read per top-k entry: sweep 1 counts the candidates, looks for NaNs, collects the true
 * candidates' keys (order-preserving score bits, inverted index) and carries the K best keys from step to step of 1024
 * columns -- only the keys above the carried K-th one are looked at again, by section A8's rounds of a 64-bit wave maximum, in
 * LDS; the true keys are then sorted in LDS; sweep 2 (only when the true set is not empty) has every candidate find by
 * binary search the first true key below its own and add one there, so that a prefix sum gives every true candidate's rank.
 * Nothing to do: Q == 0.  With G == 0 every query is empty and the outputs are still written. */
#define PCR_RANK_WIDE_MAX_GALLERY 4194304
#define PCR_RANK_WIDE_MAX_TRUE 4096
int pcr_rank_wide_ok(int Q, int G, int K);
int pcr_rank_fill_f32(float *scores, int Q, int G, pcr_stream_t stream);
int pcr_rank_scatter_f32(const float *logits, const int *pairs, const int *count, float *scores, int Q, int G, int cap,
                         int col0, int width, pcr_stream_t stream);
int pcr_rank_wide_f32(const pcr_rank *p, pcr_stream_t stream);

/* ------------------------------------------------------------ A13. scoring a validation split -------- */

/* `val_match_acc` and the reference's MatchingEval tables (datasets/reidentification_base.py:87-199, datasets/utils.py:
 * 254-533) kept as ONE table of 64-bit integer counters on the device (additive to ABI 17): a batch of validation pairs is
 * added by one fixed-shape launch without a host read, an allocation or a float accumulate.  Every add is an integer
 * atomic (32-bit in LDS, 64-bit in memory), so the table does not depend on the order of the adds and is the same bits on
 * every run.  The result is DEFINED by the rules below (tests/match_ref.py restates them; the kernels equal it bit for bit).
 * Pointers are checked against NULL only.  pcr_match_ok: 0 <= P, M <= PCR_MATCH_MAX_ROWS, 1 <= C <= PCR_MATCH_MAX_CLASSES.
 *
 * pcr_match_record_i64.  Row i is one pair: logit[i], gt[i] (float), cls[i][2], num_points[i][2], vis[i][2] (int32).
 *   rows      count (1, device) or NULL: only the rows i < clamp(count[0], 0, P) take part; NULL = all P.  A row beyond
 *             the count reads nothing and contributes nothing.
 *   gt        g = 0 for gt == 1, 1 for gt == 0, 2 for gt == -1 (a pair with a false-positive detection).  Any other value,
 *             a NaN included: info |= PCR_MATCH_INFO_GT and the row contributes nothing.
 *   decision  pred = logit > 0 (the float compare).  A NaN logit gives pred = 0 and info |= PCR_MATCH_INFO_NAN.  This is
 *             the rule of the training log (ReIDNet._log_match); `sigmoid(logit) > 0.5` evaluated in binary32, the host
 *             route's, differs from it for logits in about (0, 2e-7], where the sigmoid rounds to 0.5.
 *   cell      c = 2 g + pred, 0 <= c < PCR_MATCH_CELLS; a subset key k owns the counters table[base + k * 6 + c].
 *   ALL       key 0: every row.
 *   CLS0      key cls[i][0] + 1;  CLSMAX  key max(cls[i][0], cls[i][1]) + 1.  Both values must lie in [-1, 62];
 *             otherwise info |= PCR_MATCH_INFO_CLS and the row is left out of both tables.
 *   PTS       key 32 * bin(lo) + bin(hi), lo / hi the smaller / larger of num_points[i]; bin(0) = 0, bin(n) = 1 +
 *             floor(log2 n) for n >= 1 (31 for 2^31 - 1).  A negative value: info |= PCR_MATCH_INFO_PTS, left out.
 *   VIS       key 64 * (lo + 1) + (hi + 1), lo / hi the smaller / larger of vis[i].  Both values must lie in [-1, 62];
 *             otherwise info |= PCR_MATCH_INFO_VIS, left out.  (The reference feeds its distance and its visibility
 *             table from this one column; 5-unit distance buckets are sums over the raw values.)
 * The launch: workgroups of 256 rows-at-a-time threads, strided over the rows; ALL, CLS0, CLSMAX and PTS are counted in an
 * LDS histogram and the non-zero counters added to the table once per workgroup; VIS is added in memory directly.
 * Nothing to do: P == 0.
 *
 * pcr_match_record_objects_i64: the per-object heads.  Object m is counted iff count == NULL or
 * (m % period) < clamp(count[0], 0, period): the M = 2 b objects of b pairs, side 1 then side 2, with period = b follow
 * the pairs' count; period = M is a flat list.  objects (PCR_MATCH_OBJECTS counters, usually table + PCR_MATCH_OBJ):
 *   cls       (cls_logits (M,C) and cls_gt (M) both given) CLS_TOTAL += 1; CLS_CORRECT += 1 iff the argmax of the row --
 *             the LOWEST index of the largest value, a NaN being larger than any number, as torch.argmax -- equals cls_gt[m].
 *             A NaN in the row: info |= PCR_MATCH_INFO_NAN.
 *   fp        (fp_logits (M) and fp_gt (M) both given) FP_TOTAL += 1; FP_CORRECT += 1 iff (fp_logits[m] > 0 ? 1.0f : 0.0f)
 *             == fp_gt[m].  A NaN logit: pred 0 and info |= PCR_MATCH_INFO_NAN.
 * Nothing to do: M == 0, or neither head given.
 * (The block is a tagged struct followed by its typedef, as in A10; the layout is the plain C one.) */
#define PCR_MATCH_MAX_ROWS 1073741824                        /* 2^30 */
#define PCR_MATCH_MAX_CLASSES 4096
#define PCR_MATCH_CELLS 6
#define PCR_MATCH_KEY_BINS 64                                /* cls and vis values -1 .. 62 */
#define PCR_MATCH_PTS_BINS 32
#define PCR_MATCH_ALL 0                                      /* bases, in counters */
#define PCR_MATCH_CLS0 6
#define PCR_MATCH_CLSMAX 390
#define PCR_MATCH_PTS 774
#define PCR_MATCH_VIS 6918
#define PCR_MATCH_OBJ 31494
#define PCR_MATCH_OBJECTS 4
#define PCR_MATCH_CLS_CORRECT 0
#define PCR_MATCH_CLS_TOTAL 1
#define PCR_MATCH_FP_CORRECT 2
#define PCR_MATCH_FP_TOTAL 3
#define PCR_MATCH_TABLE 31498
#define PCR_MATCH_INFO_NAN 1
#define PCR_MATCH_INFO_GT 2
#define PCR_MATCH_INFO_CLS 4
#define PCR_MATCH_INFO_PTS 8
#define PCR_MATCH_INFO_VIS 16
struct pcr_match {
  int P;
  const float *logit, *gt;                                   /* (P) */
  const int *cls, *num_points, *vis;                         /* (P,2) */
  const int *count;                                          /* (1) device, or NULL */
  long long *table;                                          /* (PCR_MATCH_TABLE), added to */
  int *info;                                                 /* (1), or-ed into */
};
typedef struct pcr_match pcr_match;
int pcr_match_ok(int P, int M, int C);
int pcr_match_record_i64(const pcr_match *p, pcr_stream_t stream);
int pcr_match_record_objects_i64(const float *cls_logits, const int *cls_gt, const float *fp_logits, const float *fp_gt,
                                 const int *count, long long *objects, int *info, int M, int C, int period,
                                 pcr_stream_t stream);

/* ------------------------------------------------- B. fused model kernels ------------ */

/* Neighbour search of the "Point-Transformer" set-abstraction layers: centres are the first S
 * points of each cloud (random_point_sample, models/pointnet2_utils.py:139-149) and the K nearest
 * of all N points are selected (knn_point, :205-216).  The reference ranks an expanded-matmul
 * distance with an unstable argsort; this kernel selects by the direct squared distance
 * (dx*dx+dy*dy)+dz*dz with ties to the lower index and writes idx (B,S,K) in (distance, index)
 * order.  The consumer is a max over K, so only the K-SET matters (hard part 1).
 * xyz (B,N,3).  K <= N, K <= 64, N <= 16384. */
int pcr_knn_prefix_f32(const float *xyz, int *idx, int B, int N, int S, int K, pcr_stream_t stream);
/* The same search for TWO set-abstraction levels that query the same cloud (ABI 15; the Point-Transformer's first level
 * keeps all N points, so its second level -- S2 <= S centres, K2 >= K neighbours -- searches the cloud the first one
 * did): the K nearest of a query are the first K of its K2 nearest in (distance, index) order, so the first S2 queries are
 * ranked ONCE for K2 and write both lists.  idx (B,S,K) and idx2 (B,S2,K2) = what pcr_knn_prefix_f32(.., S, K) and
 * pcr_knn_prefix_f32(.., S2, K2) write, entry for entry (pointnet2_utils.py:139-149, 205-216 called by two layers,
 * backbone_net.py:50-81). */
int pcr_knn_prefix2_f32(const float *xyz, int *idx, int *idx2, int B, int N, int S, int K, int S2, int K2,
                        pcr_stream_t stream);

/* Packed weight image of one dense layer out = W x (W is (cout, cin) row-major as in
 * nn.Linear / 1x1 conv).  Returns the number of floats of the packed image for (cout, cin);
 * pcr_pack_weight_f32 writes it on the HOST (plain C, no GPU) so that a model can be packed at
 * load time and uploaded once.  The image is what the MFMA A-operand loads of every fused kernel
 * below read with one 16-byte load per lane. */
long pcr_packed_weight_floats(int cout, int cin);
int pcr_pack_weight_f32(const float *w, int cout, int cin, float *packed);
/* The same matrix as a bf16 image for the bf16 matrix core (v_mfma_f32_32x32x16_bf16): every weight is stored as
 * hi = bf16(w) and lo = bf16(w - hi) (round to nearest), laid out [ceil16(cin)/16][ceil32(cout)/32][hi, lo][64 lanes]
 * [8 bf16] so that a lane's A operand of one 16-channel step is one 16-byte load; element j of lane l (row l % 32, half
 * h = l / 32) of step s is column 16 s + 4 h + j (j < 4) | 16 s + 8 + 4 h + (j - 4): the order in which a 32 x 32
 * accumulator tile holds its rows, so that a layer's output can be stored already converted (csrc/tile_dense.h).  Kernels run in "bf16x3" mode (split
 * bf16: W x ~= W_hi x_hi + W_hi x_lo + W_lo x_hi, f32 accumulate, ~2^-17 relative per term) read both parts, in plain
 * "bf16" mode the hi part only.  Size in floats (4-byte units) / host-side pack. */
long pcr_packed_weight_bf16_floats(int cout, int cin);
int pcr_pack_weight_bf16x2_f32(const float *w, int cout, int cin, float *packed);

/* Grouped set-abstraction MLP: gather + edge/relative features + 3 x (1x1 conv -> per-channel
 * affine (folded eval-mode BatchNorm) -> ReLU) + max over the K neighbours, one pass, nothing but
 * the (B,C3,S) result written.
 *   mode 0 ("edge", PointNetSetAbstractionEdgeSA, models/pointnet2_utils.py:242-288, 333-357):
 *          rows = [xyz[idx]-centre (3), feat[centre] (D), feat[idx]-feat[centre] (D)], centre =
 *          point s (prefix sampling);
 *   mode 1 ("query-and-group", ops/group_points/group_points.py:94-118 with use_xyz=True, as used
 *          by PointSAModule, ops/pointnet_modules/point_sa_module.py:166-216):
 *          rows = [xyz[idx]-centre_xyz (3), feat[idx] (D)], centres given by centre_idx (B,S).
 * xyz (B,N,3); feat (B,D,N) or NULL when D == 0; idx (B,S,K); centre_idx (B,S) or NULL (=> s).
 * wp[l]: packed weights of layer l; scale[l]/shift[l]: (C_l) affine applied after the matmul
 * (conv bias and BatchNorm folded by the host).  out (B,C3,S). */
typedef struct pcr_sa_params {
  int mode, B, N, S, K, D;
  int c1, c2, c3;
  const float *xyz, *feat;
  const int *idx, *centre_idx;
  const float *wp[3], *scale[3], *shift[3];
  /* Optional decomposed first layer (fast path).  Layer 1 is linear in its input row, so
   *   W1 row = Wa dxyz + P[i] + Q[c],  P = Wf f (per point), Q = (Wc - Wf) f (edge mode only),
   * with Wa = W1[:, 0:3]; edge mode: Wc = W1[:, 3:3+D], Wf = W1[:, 3+D:3+2D]; query-and-group:
   * Wf = W1[:, 3:3+D], no Q.  wa is (c1,3) row-major; wpq is the PACKED image of the stacked
   * matrix [Wf ; Wc - Wf] ((2*c1, D), edge) or Wf ((c1, D), query-and-group); pq_ws is a caller
   * workspace of B*N*(2*c1 or c1) floats.  Leave wa NULL to force the generic kernel (wp[0]).
   * wa and wpq must be PRE-SCALED by scale[0] (row o times scale[0][o]); the fast path then
   * evaluates layer 1 as relu(wa dxyz + P[i] + Q[c] + shift[0]) and never reads scale[0].
   * Likewise wps[0], wps[1] are the packed images of diag(scale[1]) W2 and diag(scale[2]) W3, and
   * shift_pad[0], shift_pad[1] are shift[1], shift[2] zero-padded to a multiple of 32 floats: the
   * fast path seeds the MFMA accumulators with the shift and its epilogue is a bare ReLU. */
  const float *wa, *wpq;
  const float *wps[2], *shift_pad[2];
  /* Optional duplicate-free evaluation for ball-query groups (mode 1): cnt (B,S) = number of genuine hits
   * of each row of idx as returned by pcr_ball_query_cnt_f32 (entries [cnt,K) of a row repeat entry 0, and
   * a max over K ignores repeats), tile_ws = caller workspace of pcr_sa_tile_ws_ints(B,S,K,c2,c3) ints.  The kernel then runs the
   * MLP on ceil2(max(cnt,1)) rows per centre; the result is bit-identical to the K-row evaluation. */
  const int *cnt;
  int *tile_ws;
  float *pq_ws;
  int pq_ready; /* nonzero: pq_ws already holds the tables (caller ran pcr_dense_pm_f32 itself) */
  /* Layouts.  feat_point_major: feat is (B,N,D) instead of (B,D,N).  out_point_major: out is (B,S,c3) instead
   * of (B,c3,S): a centre's c3 channels are then one contiguous run (full-line stores; the (B,c3,S) form writes
   * 4-byte pieces S floats apart).  Both are pure layout choices; values are identical. */
  int feat_point_major, out_point_major;
  float *out;
  /* optional: (c1,3) dxyz weights of layer 1 (BatchNorm scale folded in, like wa) as a PACKED image
   * (pcr_pack_weight_f32 of the (c1,3) matrix): lets the persistent kernel run layer 1 on the matrix core too */
  const float *wa_packed;
  /* arithmetic of layers 2 and 3 (layer 1 and the tables stay f32): PCR_PREC_F32 = f32-input MFMA, exact fmaf chains
   * (wps); PCR_PREC_BF16X3 = split bf16, three bf16 MFMAs per product with f32 accumulation; PCR_PREC_BF16 = plain bf16
   * activations and weights, f32 accumulation (BASELINE config 2 as stated).  wps_bf[l]: pcr_pack_weight_bf16x2_f32
   * images of the matrices wps[l] holds.  Shapes the bf16 kernels do not cover run in f32 (pcr_last_launch_arith says
   * so).  Among them, not exhaustively (sa_make_plan is the rule, tests/sa_ref.py restates it): c1 or c2 no multiple of 32; a
   * layer wider than 256; in the K-row kernel K no multiple of 16, and a layer 2 of up to 128 channels (one cout-block
   * round) whose layer 1 cannot share its class on the matrix core (32 / 64 / 64, 64 / 32 / 32, 64 / 128 / 256); layer classes
   * other than equal ones and (64 -> up to 128 channels) -- in particular 64 / 64 / c3 with 129 <= c3 <= 256, whose last
   * layer would need two cout-block rounds behind a two-way layer 2, an instantiation the bf16 units do not hold. */
  int precision;
  const float *wps_bf[2];
  /* optional (ABI 11): pcr_pack_weight_f32 image of the (c1, 4) matrix [wa | shift[0]] -- the cout-split kernel feeds
   * (dx, dy, dz, 1) to the matrix core, so that layer 1's shift arrives with the coordinate term and costs no seed
   * reads.  Without it that kernel is not chosen. */
  const float *wa_shift_packed;
  /* optional (ABI 12): the ball query's row table of THIS launch's groups (pcr_ball_query_rows_f32, same B / S / K),
   * for ball-query layers with hit counts whose shape pcr_sa_uses_row_table accepts: the wave-autonomous ragged kernel
   * then reads a row's {neighbour, point - centre} with one load instead of chasing cnt -> idx -> xyz.  idx may be
   * NULL when it is given (cnt is still read).  Ignored by every other kernel. */
  const float *row_tab;
  /* optional (ABI 16): pcr_sa_claim_ws_ints(..) ints of scratch for the wave-autonomous K-row kernel on clouds of >= 1024
   * points: its waves then CLAIM their work items from counters in it (zeroed by the launch itself, on `stream`) instead
   * of walking a fixed stride, which keeps the waves of an XCD on consecutive items -- one or two clouds' tables live in
   * its L2 instead of three or four.  Same results bit for bit (an item's arithmetic does not depend on who runs it).
   * NULL, or a shape the query answers 0 for: fixed-stride items. */
  int *claim_ws;
  /* optional (ABI 17): nonzero = pq_ws was built by pcr_dense_pm_xyz_f32 (pq_ready must be set): the tables carry the
   * coordinate term of layer 1 and its shift -- P'[i] = P[i] + wa xyz[i], Q'[c] = Q[c] - wa xyz[c] + shift[0] -- so a row of
   * layer 1 is relu(P'[i] + Q'[c]): no coordinate loads, no layer-1 MFMAs, one add per element in the launch.  Only the
   * wave-autonomous K-row kernel reads such tables: set it ONLY when pcr_sa_tables_take_xyz answers 1 for the launch;
   * any other dispatch returns PCR_ERR_INVALID rather than evaluating the wrong formula. */
  int pq_has_xyz;
} pcr_sa_params;
int pcr_sa_mlp_f32(const pcr_sa_params *p, pcr_stream_t stream);
/* ints of pcr_sa_params.claim_ws a launch of this shape would use (0: it would not use any); shape-only */
long pcr_sa_claim_ws_ints(int c1, int c2, int c3, int K, int N, int precision);
/* ints of pcr_sa_params.tile_ws for the duplicate-free evaluation (tile lists + per-tile row tables) */
long pcr_sa_tile_ws_ints(int B, int S, int K, int c2, int c3);
/* 1: a launch of this shape WITHOUT hit counts (cnt NULL: all K rows of every group) also runs on the tile plan and
 * wants tile_ws (the cout-split kernel with register-resident weights, 128 / 128 / 256 in the bf16 modes): ragged and
 * K-row evaluation of such a layer then share one kernel, hence one arithmetic. */
int pcr_sa_krow_uses_tiles(int c1, int c2, int c3, int K, int precision);
/* 1: a ball-query layer of this shape with hit counts reads pcr_sa_params.row_tab when given (shape-only) */
int pcr_sa_uses_row_table(int c1, int c2, int c3, int K, int precision);
/* Which kernel would pcr_sa_mlp_f32 launch for *p?  The dispatcher's own plan (csrc/sa_kernels_impl.h: sa_make_plan) and
 * nothing else; no device is touched, pointers are read against NULL only, nothing is launched and
 * pcr_last_launch_arith is left alone.  Returns what the launch would return before its first kernel (PCR_ERR_INVALID
 * for a block it refuses) and writes PCR_SA_FORM_INTS ints:
 *   form[0]  the arithmetic unit that runs layers 2 and 3 (PCR_PREC_*: a shape the asked bf16 unit does not hold says F32)
 *   form[1]  the kernel family, PCR_SA_*
 *   form[2]  PCR_SA_STREAM_RAG: 0 = index form on 8 waves, 1 = row-table form on 8 waves, 2 = row-table form on 12; else 0
 *   form[3]  n = the number of template arguments that follow
 *   form[4 .. 4 + n)  the kernel's template arguments in the kernel's order, defaults filled in, bools as 0 / 1:
 *     PCR_SA_GENERIC     sa_mlp_kernel            none
 *     PCR_SA_KROW_TILE   sa_fused_kernel          TB, NR, W2, W3, MAXE, NR2, RKB, PREC, IMG
 *     PCR_SA_RAG_TILE    sa_rag_kernel            TB, NR, W2, W3, NR2, W1, PREC
 *     PCR_SA_STREAM      sa_stream_kernel         NCB, NCB3, LO
 *     PCR_SA_STREAM_RAG  sa_stream_rag_kernel     NCB, NCB3, LO, TAB, WAVES
 *     PCR_SA_WSPLIT      sa_wsplit_rag_kernel     NCB, NCB3, LO
 * the rest is zero. */
#define PCR_SA_FORM_INTS 16
#define PCR_SA_GENERIC 0
#define PCR_SA_KROW_TILE 1
#define PCR_SA_RAG_TILE 2
#define PCR_SA_STREAM 3
#define PCR_SA_STREAM_RAG 4
#define PCR_SA_WSPLIT 5
int pcr_sa_launch_form(const pcr_sa_params *p, int *form);

/* Per-point linear map with POINT-major output: x (B,cin,L) channel-major (or (B,L,cin) when x_point_major)
 * -> y (B,L,cout) = W x, wp packed (cout,cin), cout <= 1024 (a multiple of 4 beyond 256).  This is the table builder of the decomposed first
 * SA layer (pcr_sa_mlp_f32 runs it itself unless pq_ready is set). */
int pcr_dense_pm_f32(const float *x, const float *wp, float *y, int B, int cin, int cout, int L,
                     int x_point_major, pcr_stream_t stream);
/* the same map on the bf16 matrix core: wp_bf = pcr_pack_weight_bf16x2_f32 image of W, precision = PCR_PREC_BF16X3 or
 * PCR_PREC_BF16 */
int pcr_dense_pm_prec_f32(const float *x, const float *wp_bf, float *y, int B, int cin, int cout, int L,
                          int x_point_major, int precision, pcr_stream_t stream);
/* (ABI 17) the same tables WITH the coordinate term of the decomposed first layer (reference: the dxyz columns of
 * sample_and_group_edge's new_points, models/pointnet2_utils.py:242-288): y[b][l][o] = (W x)[o] + wxyz[o][3] +
 * wxyz[o][0] xyz[b][l][0] + wxyz[o][1] xyz[b][l][1] + wxyz[o][2] xyz[b][l][2], the coordinate products as f32 fmas on the
 * f32 sum (added z, y, x in that order), whatever `precision` the feature product W x runs in.  xyz (B,L,3), wxyz (cout,4)
 * row-major: the caller puts {+wa, 0} in the P rows and {-wa, shift} in the Q rows.  cout % 4 == 0.
 * q_rows / q_off: tokens l >= q_rows receive the couts [0, q_off) only, the rest of their rows is left unwritten -- the Q
 * half of an SA table is read for CENTRES only, which under prefix sampling (centre_idx == NULL) are the first S points:
 * q_rows = S rounded up to a multiple of 64, q_off = c1.  q_rows = L, q_off = cout: every token, every cout. */
int pcr_dense_pm_xyz_f32(const float *x, const float *wp_bf, const float *xyz, const float *wxyz, float *y, int B, int cin,
                         int cout, int L, int x_point_major, int precision, int q_rows, int q_off, pcr_stream_t stream);
/* shape-only: does the pcr_sa_mlp_f32 launch of this shape run on the wave-autonomous K-row kernel, i.e. may its tables be
 * built with pcr_dense_pm_xyz_f32 (pcr_sa_params.pq_has_xyz)?  Edge mode (0) with features, c1 == c2 == c3 in {32, 64, 128},
 * K a multiple of 16 that divides 32, 64 or 96, a bf16 precision. */
int pcr_sa_tables_take_xyz(int mode, int D, int c1, int c2, int c3, int K, int precision);

/* Linear-attention block shared by Self_Attention (models/pointnet2_utils.py:90-114), FP_SA
 * (:407-437) and corss_attention (models/attention.py:192-219), in two kernels.
 *
 * With h = relu(W0 xyz + b0) the reference's position encoding is pos = W2 h + b2; the HOST folds
 * W2/b2 into the projections (all products formed in fp64, rounded once to fp32):
 *   wq  = packed [Wq | Wq W2] (d, c1+d)  if q_pos  else packed Wq (d, c1);   bq = Wq b2 or 0
 *   wkv = packed [[Wk | kpos Wk W2] ; [Wv | Wv W2]] (2d, c2+d);   bkv = [kpos Wk b2 ; Wv b2]
 * where kpos = 1 for Self_Attention (keys carry the position encoding) and 0 otherwise.
 *
 * pcr_attn_kv_f32: per key-side cloud, K = elu(.)+1, V = (.)/Sk from one fused projection of
 *   [feat_k ; h]; accumulates KV_head = sum_s K V^T and ksum = sum_s K, folds the merge projection
 *   (wmerge (d,d) row-major) into KV and writes, per cloud, the packed (d,d) matrix
 *   M[o][dd] = sum_{v in head(dd)} Wm[o][v] KV[dd][v] followed by ksum (d).
 * pcr_attn_apply_f32: per query token, Q = elu(wq [x ; h] + bq)+1, Q' = Q Sk / (Q.ksum + 1e-6)
 *   per head, msg = LayerNorm(M Q'), feed-forward mlp2(relu(mlp0 [x ; msg])), LayerNorm, optional
 *   residual; cloud b reads the kv image of cloud kv_index[b] (NULL => b), which is how the siamese
 *   matching head pairs clouds without copying (ReIDNet.xcorr_eff, models/ReIDNet.py:231-247).
 *   Optional fused trailing 1x1 conv (Pointnet_Backbone.cov_final, models/backbone_net.py:89,124).
 * d_model in {32,64,96,128,256,512}; c2 % 8 == 0; q_pos requires c1 == c2 == d; residual requires cout == c1. */
typedef struct pcr_attn_params {
  int B, Lq, Sk;             /* clouds, query tokens per cloud, key tokens per cloud */
  int c1, c2, d, cout;       /* query feature dim, key feature dim, d_model, output dim */
  int nhead;
  int q_pos, residual;
  const float *feat_q, *xyz_q; /* (B,c1,Lq), (B,Lq,3) (xyz_q only read when q_pos) */
  const float *feat_k, *xyz_k; /* (B,c2,Sk), (B,Sk,3) */
  const int *kv_index;         /* (B) or NULL: apply: cloud b reads the kv image of cloud kv_index[b] */
  const int *q_index;          /* (B) or NULL: apply: cloud b takes its query tokens from cloud q_index[b]
                                  (gallery matching: B = number of (query, template) combinations) */
  const float *pos0_w, *pos0_b;   /* (d,3) row-major, (d) */
  const float *wq, *bq;           /* packed fused query projection, (d) */
  const float *wkv, *bkv;         /* packed fused key/value projection, (2d) */
  const float *wmerge;            /* (d,d) row-major */
  const float *wmlp0, *wmlp2;     /* packed (2d, c1+d), packed (cout, 2d) */
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  const float *wfinal, *bfinal; int cfinal;       /* optional trailing conv: packed (cfinal,cout); bias zero-padded to a multiple of 32 */
  /* d_model 256 / 512 only (d % 64 == 0, head width a multiple of 64 and <= 256; the mul = 2 / 4 Point-Transformer
   * configs): the kv kernel splits a cloud over d/64 workgroups, band g owning rows [64g, 64g+64) of KV.
   * wkv_wide: d/64 packed images, image g = pcr_pack_weight_f32 of the (64 + dh, c2 + d) matrix made of rows
   * [64g, 64g+64) (K band) and [d + hd dh, d + (hd+1) dh) (V rows of the band's head hd) of the fused projection wkv;
   * bkv_wide: the same rows of bkv, (d/64, 64 + dh); wmerge_packed: packed image of wmerge (d,d).  NULL otherwise. */
  const float *wkv_wide, *bkv_wide, *wmerge_packed;
  float *kv;    /* workspace (B, pcr_attn_kv_floats(d)) */
  float *out;   /* (B, cfinal ? cfinal : cout, Lq) */
  /* precision != PCR_PREC_F32 and d <= 128: the dense phases of the apply kernel (Q, message, feed-forward, cov_final)
   * run as split bf16 (three bf16 MFMAs per product, f32 accumulate) on the pcr_pack_weight_bf16x2_f32 images of the same
   * matrices: wq_bf, wmlp0_bf, wmlp2_bf, wfinal_bf (NULL: f32).  The kv kernel then writes the per-cloud matrix M as a
   * bf16 image, so pcr_attn_kv_f32 and pcr_attn_apply_f32 must be called with the SAME precision. */
  int precision;
  const float *wq_bf, *wmlp0_bf, *wmlp2_bf, *wfinal_bf;
  /* pcr_attn_kv_f32, d <= 128: kv_splits > 1 splits every cloud's key tokens over that many workgroups (raw partial
   * matrices in kv_part, (B, kv_splits, d d + d) floats) and a second launch adds them in order and folds the merge
   * projection -- parallelism for batches of a few clouds; free on a grid that fills the chip.
   * pcr_attn_kv_splits(B, Sk, d) suggests a count from the launch shape alone (1 = the single-launch form; kv_part may
   * then be NULL): results do not depend on the batch size. */
  int kv_splits;
  float *kv_part;
  /* precision != PCR_PREC_F32, d = c2 = 64, Sk % 32 == 0 (the wave-autonomous kv kernel): pcr_pack_weight_bf16x2_f32
   * image of the fused K / V projection wkv -- the projection then runs as split bf16 too.  NULL: f32 projection. */
  const float *wkv_bf;
  /* c1 not a multiple of 16 (the first FP_SA block: c1 = 3): pcr_pack_weight_bf16x2_f32 image of mlp[0]'s weight with the
   * query-feature columns padded to a whole 16-channel step, [W[:, :c1] | 0 | W[:, c1:]] -- the wave-autonomous apply
   * kernel's contraction steps are 16 channels wide.  NULL: the tile kernel. */
  const float *wmlp0_bf_xpad;
  /* ABI 16 (round 6): pooled output.  NULL: the block output goes to `out` as before.  Non-NULL (only where
   * pcr_attn_apply_pool_ok says yes: the wave-autonomous d = c1 = cout = 64 form without q_pos / trailing conv, i.e. the
   * matching stages' corss_attention, models/attention.py:192-219): `out` is NOT written (may be NULL); instead every
   * virtual cloud leaves its per-channel maximum and SUM over its Lq tokens, pool_out (B, 2, 64) = [max | sum] -- what
   * get_pooled_feats 'both' (models/ReIDNet.py:526-534) needs of the block output, 512 bytes instead of 256 Lq. */
  float *pool_out;
} pcr_attn_params;
long pcr_attn_kv_floats(int d);
int pcr_attn_kv_splits(int B, int Sk, int d);
int pcr_attn_kv_f32(const pcr_attn_params *p, pcr_stream_t stream);
int pcr_attn_apply_f32(const pcr_attn_params *p, pcr_stream_t stream);
/* 1 if pcr_attn_apply_f32 honours p->pool_out for these parameters (a function of the launch SHAPE and the arithmetic
 * mode, never of B: a pair's result does not depend on the batch it travels in), else 0 */
int pcr_attn_apply_pool_ok(const pcr_attn_params *p);

/* Gated launches (additive to ABI 17): score only the live pairs of a device-counted list.  A fixed-shape pair list
 * (pcr_assoc_pairs_i32: capacity rows of which *count are real, the rest (0, 0) padding) makes fixed-shape launches, and a
 * captured graph fixes their grids -- so the launches themselves read the count and do no work for the padding.
 * pcr_live says which virtual clouds of a launch are live: with n = clamp(*count - offset, 0, period), cloud b is live
 * iff b % period < n.  For the matching stages (B = 2 period: cloud p < period is pair p's first direction, cloud
 * period + p its second) the live clouds are the two runs [0, n) and [period, period + n).
 *   Dead clouds.  The launch reads NOTHING of a dead cloud -- neither its q_index / kv_index entries nor its features --
 *     and writes nothing for it: its rows of kv / out / pool_out keep what they held.
 *   Live clouds.  A live cloud's output is bit for bit what the un-gated entry point writes for that cloud.  The kernel
 *     choice stays a function of the launch shape and the arithmetic mode; a pair's bits never depend on the batch it
 *     travels in, and *count does not change that.
 *   Capture.  *count is read by the launch (one load per workgroup), not by the host: a captured graph re-reads it on
 *     every replay.  count may exceed period (a list scored in chunks: offset = the pairs of the earlier chunks).
 *   live == NULL is the un-gated call.
 *   Unsupported shapes.  pcr_attn_live_ok (shape and arithmetic only, never B) says yes for d = c1 = c2 = cout = 64
 *     without kv_splits -- the matching stages' corss_attention blocks -- whichever kernel pcr_attn_kv_f32 /
 *     pcr_attn_apply_f32 choose for them (wave-autonomous or tile form, pooled output, q_pos, trailing conv; all three
 *     arithmetic modes).  Where it says no, the _live entry points return PCR_ERR_INVALID; they never score everything
 *     silently. */
typedef struct pcr_live {
  const int *count;          /* device, (1): the caller's pair count (may exceed period) */
  int period;                /* > 0: cloud b is live iff (b % period) < clamp(*count - offset, 0, period) */
  int offset;                /* >= 0: pairs scored by earlier chunks */
} pcr_live;
int pcr_attn_live_ok(const pcr_attn_params *p);
int pcr_attn_kv_live_f32(const pcr_attn_params *p, const pcr_live *live, pcr_stream_t stream);
int pcr_attn_apply_live_f32(const pcr_attn_params *p, const pcr_live *live, pcr_stream_t stream);
/* Which kernel would pcr_attn_kv_f32 (apply == 0) or pcr_attn_apply_f32 (apply != 0) launch for *p -- with live != NULL,
 * their _live forms?  The dispatcher's own plan (csrc/attn_kernels_impl.h: attn_plan_kv / attn_plan_apply behind the
 * entry's checks) and nothing else; no device is touched, pointers are read against NULL only, nothing is launched and
 * pcr_last_launch_arith is left alone.  Returns what the launch would return before its first kernel (PCR_ERR_INVALID for
 * a block it refuses; form is then left untouched); B = 0, where the launch returns PCR_OK without a kernel, reports the
 * plan.  Writes PCR_ATTN_FORM_INTS ints:
 *   form[0]  the arithmetic the launch notes (PCR_PREC_*: what pcr_last_launch_arith() says after it)
 *   form[1]  the kernel family, PCR_ATTN_*
 *   form[2]  1: the gated twin is launched (GATE = true as the kernel's last template argument; attn_kv_kernel_o3_live)
 *   form[3]  n = the number of template arguments that follow
 *   form[4 .. 4 + n)  the kernel's template arguments in the kernel's order, defaults filled in, bools as 0 / 1, GATE
 *            left out (n <= 6):
 *     PCR_ATTN_KV_TILE          attn_kv_kernel               TB, NR, WSEL, NTW
 *     PCR_ATTN_KV_TILE_O3       attn_kv_kernel_o3            TB, NR, WSEL, NTW
 *     PCR_ATTN_KV_TILE_O2       attn_kv_kernel_o2            TB, NR, WSEL, NTW, BFP
 *     PCR_ATTN_KV_STREAM64      attn_kv_stream64_kernel      DIAG, BF, XS, ONEW
 *     PCR_ATTN_KV_STREAM32      attn_kv_stream32_kernel      none
 *     PCR_ATTN_KV_STREAM128     attn_kv_stream128_kernel     NH
 *     PCR_ATTN_KV_WIDE          attn_kv_wide_kernel          NRW
 *     PCR_ATTN_APPLY_TILE       attn_apply_kernel            TB, NR
 *     PCR_ATTN_APPLY_STREAM64   attn_apply_stream64_kernel   QPOS, C1S, CF, NOB, ND, POOL
 *     PCR_ATTN_APPLY_STREAM128  attn_apply_stream128_kernel  NH
 *   form[10] kv: the effective token split (kv_splits cut to the number of tiles; 1 = whole clouds)
 *   form[11] kv: 1 = attn_kv_fold_kernel follows
 *   form[12] kv: waves per cloud of attn_kv_stream128_kernel, else 0
 *   form[13] dynamic LDS bytes of the kernel
 * the rest is zero. */
#define PCR_ATTN_FORM_INTS 16
#define PCR_ATTN_KV_TILE 0
#define PCR_ATTN_KV_TILE_O3 1
#define PCR_ATTN_KV_TILE_O2 2
#define PCR_ATTN_KV_STREAM64 3
#define PCR_ATTN_KV_STREAM32 4
#define PCR_ATTN_KV_STREAM128 5
#define PCR_ATTN_KV_WIDE 6
#define PCR_ATTN_APPLY_TILE 7
#define PCR_ATTN_APPLY_STREAM64 8
#define PCR_ATTN_APPLY_STREAM128 9
int pcr_attn_launch_form(const pcr_attn_params *p, const pcr_live *live, int apply, int *form);

/* Matching head tail: pool 'both' over the point-concatenated pair (get_pooled_feats,
 * models/ReIDNet.py:526-534: [max over 2L points, mean over 2L points]) followed by
 * LinearRes(2C,2C,GroupNorm) + Linear(2C,1) (models/lanegcn_nets.py:228-241, ReIDNet.py:455-457).
 * o (2P, C, L): cloud p and cloud p+P form pair p.  logits (P); pooled (P,2C) optional (may be NULL). */
typedef struct pcr_head_params {
  int P, C, L, groups;
  const float *o;
  const float *w1, *w2;            /* (2C,2C) row-major, NOT packed */
  const float *gn1_g, *gn1_b, *gn2_g, *gn2_b;
  const float *w_out, *b_out;      /* (1,2C), (1) */
  float *pooled, *logits;
  /* optional (ABI 12, appended): the TRANSPOSES of w1 / w2 ((2C,2C) row-major: w1t[i][o] = w1[o][i]).  With them the
   * matrix-vector products read 256 contiguous bytes per wave and step instead of 64 scattered 16-byte pieces (the
   * head of a 32 k-pair gallery launch was bound by exactly those reads); same products, same summation order. */
  const float *w1t, *w2t;
} pcr_head_params;
int pcr_pool_head_f32(const pcr_head_params *p, pcr_stream_t stream);
/* gated (pcr_live above, pairs in place of clouds: pair p is live iff p % period < n): a dead pair's clouds are not read;
 * logits[p] = *dead_value (a HOST float, read when the call is made; NULL: 0.0f) and, if asked for, pooled[p] = zeros.
 * Live pairs: bit for bit pcr_pool_head_f32.  live == NULL is the un-gated call. */
int pcr_pool_head_live_f32(const pcr_head_params *p, const pcr_live *live, const float *dead_value, pcr_stream_t stream);

/* get_pooled_feats with pool_type='both' on its own (models/ReIDNet.py:529-532):
 * x (B,C,L) -> out (B,2C) = [max over L, mean over L]. */
int pcr_pool_both_f32(const float *x, float *out, int B, int C, int L, pcr_stream_t stream);

/* get_pooled_feats with pool_type='max' (models/ReIDNet.py:145,526-528; reid_pts_point-transformer_baseline.py):
 * nn.MaxPool1d(window) on the permuted (B,L,C) tensor = max over windows of `window` consecutive channels of every
 * point, floor mode.  x (B,C,L) -> out (B,L,C/window). */
int pcr_channel_max_f32(const float *x, float *out, int B, int C, int L, int window, pcr_stream_t stream);

/* Generic per-point dense layer y = act(scale * (W x) + shift) on channel-major tensors
 * x (B,cin,L) -> y (B,cout,L): 1x1 Conv1d / Linear (+ folded BatchNorm) of the PointNet encoder
 * (models/pointnet.py:27-45, 67-85, 103-127).  act: 0 none, 1 ReLU, 2 LeakyReLU(0.2) (dgcnn_orig.py:112-114).
 * wp packed. */
int pcr_dense_f32(const float *x, const float *wp, const float *scale, const float *shift, float *y,
                  int B, int cin, int cout, int L, int act, pcr_stream_t stream);
/* the same with x given point-major, (B,L,cin) */
int pcr_dense_xpm_f32(const float *x, const float *wp, const float *scale, const float *shift, float *y,
                      int B, int cin, int cout, int L, int act, pcr_stream_t stream);

/* Linear (no bias) -> GroupNorm [-> + res] [-> ReLU] in one launch: the three steps LinearRes repeats
 * (lanegcn_nets.py:228-241) on channel-major token tensors, y (B,cout,L) = [relu](GN(W x) * gamma + beta [+ res]).
 * GroupNorm is per token over groups of cout/groups consecutive channels (4, 8, 16 or 32 per group; anything else
 * returns PCR_ERR_INVALID and the caller runs pcr_dense_f32 + pcr_groupnorm_f32), biased variance, eps 1e-5;
 * res (optional) is (B,cout,L). */
int pcr_dense_gn_f32(const float *x, const float *wp, const float *gamma, const float *beta, const float *res,
                     float *y, int B, int cin, int cout, int L, int groups, int relu, pcr_stream_t stream);
/* The same two launches on the bf16 matrix core (round 4; ABI 11): wp_bf = pcr_pack_weight_bf16x2_f32 image of W,
 * precision = PCR_PREC_BF16X3 (split bf16, three MFMAs per product, f32 accumulate) or PCR_PREC_BF16.  Covered shapes:
 * pcr_dense_prec_ok(cin, cout, L) != 0 (cin a multiple of 64, cout a multiple of 32, channel-major x, shared weights);
 * anything else returns PCR_ERR_INVALID and belongs to the f32 launches.  Reference: the 1x1 convs / Linear layers of
 * models/pointnet.py:27-127, dgcnn_orig.py:147, lanegcn_nets.py:228-241 (LinearRes). */
int pcr_dense_prec_ok(int cin, int cout, int L);
int pcr_dense_prec_f32(const float *x, const float *wp_bf, const float *scale, const float *shift, float *y, int B, int cin,
                       int cout, int L, int act, int precision, pcr_stream_t stream);
int pcr_dense_gn_prec_f32(const float *x, const float *wp_bf, const float *gamma, const float *beta, const float *res,
                          float *y, int B, int cin, int cout, int L, int groups, int relu, int precision,
                          pcr_stream_t stream);
/* pcr_dense_prec_f32 for a POINT-major input x (B,L,cin) (ABI 12; pcr_dense_xpm_f32's shapes on the bf16 matrix core):
 * cin a multiple of 64, cout <= 128, the weight image within LDS (pcr_dense_xpm_prec_ok).  Reference: the Conv1d after
 * the last set-abstraction layer of models/pointnet2_ssg.py (PointNet2SSG.cov_final). */
int pcr_dense_xpm_prec_ok(int cin, int cout, int L);
int pcr_dense_xpm_prec_f32(const float *x, const float *wp_bf, const float *scale, const float *shift, float *y, int B,
                           int cin, int cout, int L, int act, int precision, pcr_stream_t stream);

/* ---- PointNet encoder pieces (models/pointnet.py:10-127) and LinearRes rows (lanegcn_nets.py:228-241) ---- */

/* (B,C,L) -> out (C,B) with out[c*B + b] = max over L: the global max pool of STN3d/STNkd
 * (pointnet.py:31,71), written channel-major with the clouds as tokens so that the fc layers that
 * follow are plain pcr_dense_f32 calls on a (1,C,B) tensor. */
int pcr_max_over_l_f32(const float *x, float *out, int B, int C, int L, pcr_stream_t stream);

/* pcr_dense_f32 followed by pcr_max_over_l_f32 as ONE launch that never writes the (B,cout,L) tensor (round 5): the conv3 +
 * BN + ReLU + max over the points of STN3d / STNkd (models/pointnet.py:27-33, 67-73).  out (cout,B) as pcr_max_over_l_f32
 * writes it; bit-equal to the two-launch form (a maximum does not depend on the order).  pcr_dense_max_ok: cout a multiple
 * of 256 and cin small enough for a 64-token tile of the whole input extent in 64 KB of LDS (cin <= 232). */
int pcr_dense_max_ok(int cin, int cout, int L);
int pcr_dense_max_f32(const float *x, const float *wp, const float *scale, const float *shift, float *out, int B, int cin,
                      int cout, int L, int act, pcr_stream_t stream);

/* t (1,k*k,B) = the fc3 output of an STN (+identity), entry [c*k + c2][b] = T_b[c][c2] -> per-cloud packed
 * weight images (B, packed(k,k)) of W_b = T_b^T; pcr_dense_bmm_f32(x, images) then equals
 * torch.bmm(x^T, T)^T (pointnet.py:110,118). */
int pcr_pack_bmm_f32(const float *t, float *wp_per_cloud, int B, int k, pcr_stream_t stream);
int pcr_dense_bmm_f32(const float *x, const float *wp_per_cloud, float *y, int B, int cin, int cout, int L,
                      pcr_stream_t stream);

/* GroupNorm over channel groups of every token of x (B,C,L) (nn.GroupNorm on (M,C) rows in the reference's
 * LinearRes, with M = B*L tokens), optional residual add, optional ReLU: y = [relu](GN(x) [+ res]). */
int pcr_groupnorm_f32(const float *x, const float *gamma, const float *beta, const float *res, float *y, int B,
                      int C, int L, int groups, int relu, pcr_stream_t stream);

/* ---- DGCNN EdgeConv (models/dgcnn_orig.py: knn :22-29, get_graph_feature :32-56, DGCNN.forward :127-152) ---- */

/* Feature-space kNN of every point among the points of its own cloud (replaces dgcnn_orig.knn, :22-29):
 * x (B,C,N) channel-major with batch stride x_bstride floats (0 = C*N), xx_ws = caller workspace of B*N floats
 * -> idx (B,N,K) int32, the K largest pd_ij = (2 <x_i,x_j> - |x_i|^2) - |x_j|^2 of row i, largest first, ties by
 * the lower index.  The reference leaves the order of summation of its matmul to the BLAS; this library fixes
 * <.,.> = fmaf chain over channels 0..C-1 and |.|^2 = left-to-right sum of rounded squares
 * (oracle/pcr_oracle.c:pcr_oracle_knn_feat).  K <= 64, K <= N <= 2048, C <= 512 (and the LDS budget: see
 * csrc/edge_kernels.hip). */
int pcr_knn_feat_f32(const float *x, float *xx_ws, int *idx, int B, int C, int N, int K, long x_bstride,
                     pcr_stream_t stream);

/* The gather + max + BatchNorm shift + LeakyReLU tail of one EdgeConv layer (dgcnn_orig.py:129-131 and the
 * like): ta, tb (B,N,Co) point-major tables A = (s.W1) f and Bt = (s.(W2-W1)) f built with pcr_dense_pm_f32
 * (s = folded BatchNorm scale, W = [W1 | W2] the (Co,2C) conv weight), idx (B,N,K) ->
 * out[b][c][i] = leaky_slope(max_j ta[b][idx[b][i][j]][c] + tb[b][i][c] + shift[c]), channel-major with batch
 * stride out_bstride floats (0 = Co*N); out2 (optional, may be NULL) receives the same values with its own
 * batch stride (the x1..x4 slices of the concatenated conv5 input, dgcnn_orig.py:145).  Co <= 256, K <= 64. */
int pcr_edge_max_f32(const float *ta, const float *tb, const int *idx, const float *shift, float slope, float *out,
                     long out_bstride, float *out2, long out2_bstride, int B, int N, int Co, int K,
                     pcr_stream_t stream);

/* The attention step of local_self_attention (models/attention.py:262-289): every point is ONE query token over its
 * K feature-space neighbours.  qkv (B,N,3C) point-major rows [q | k | v] = the three projections of
 * feat + pos_mlp(xyz) (built with pcr_dense_pm_f32), idx (B,N,K) from pcr_knn_feat_f32 ->
 * msg (B,C,N) channel-major, msg_i = sum_j a_ij v_j / (sum_j a_ij + eps), a_ij = <elu(q_i)+1, elu(k_j)+1> per head
 * (identical to the reference's LinearAttention with L = 1, S = K).  C <= 64, C / nhead a power of two. */
int pcr_local_attn_f32(const float *qkv, const int *idx, float *msg, int B, int N, int C, int K, int nhead, float eps,
                       pcr_stream_t stream);

/* ------------------------------------------------- C. training-mode kernels ------------ */
/* Forward with BatchNorm batch statistics and backward of the same path (the reference trains it with autograd over
 * unfused ATen ops: models/ReIDNet.py:586-634,694-738; pointnet2_utils.py:333-360; group_points_cuda.cu:10-31).
 * All tensors are (B, C, L) channel-major fp32; every reduction is two-stage in a fixed order (per-workgroup partials
 * + a reduce / finalize launch): no float atomics, gradients are bit-reproducible.  csrc/train_kernels.hip. */

/* device-side pcr_pack_weight_f32 (weights change every iteration): W (rows x cols, leading dimension ld) -> packed
 * image of W (transpose = 0), of W^T (transpose = 1), or both, W first (transpose = 2); packed holds
 * pcr_packed_weight_floats(cout, cin) floats per image */
int pcr_pack_weight_dev_f32(const float *w, int rows, int cols, int ld, int transpose, float *packed, pcr_stream_t stream);

/* workgroups a train-dense launch uses for (B, L) (a workgroup strides over tiles AND clouds): the partial buffers
 * below have this many entries */
int pcr_train_groups(int B, int L);
/* ... of a pcr_tdense_bwd_f32 launch that accumulates dW (cout x cin; cout = 0: no dW): wide layers on short clouds use
 * fewer workgroups, each accumulating over more clouds */
int pcr_train_groups_bwd(int B, int L, int cout, int cin);
/* ... of THE launch a parameter block describes (ABI 8): the narrow grouped-MLP layers (32 / 64 channels, L a multiple
 * of 32) run through wave-autonomous kernels with their own grid (csrc/train_stream_kernels.hip); every other launch
 * returns what the two functions above return.  Size stats / dstats / dwp / dbp with these. */
struct pcr_tdense_fwd;
struct pcr_tdense_bwd;
int pcr_tdense_fwd_groups(const struct pcr_tdense_fwd *p);
int pcr_tdense_bwd_groups(const struct pcr_tdense_bwd *p);
/* launch policy: train-dense launches with fewer than n 32-token blocks (B * L / 32) stay on the tile kernels
 * (default 8192); returns the previous value, n < 0 only reads it.  Process-wide; tests use it to run small shapes
 * through the wave-autonomous kernels. */
int pcr_set_stream_min_blocks(int n);

/* y = [relu](W f([x ; x2]) + bias [+ res]),  f(x) = [relu](isc x + ish) on the cin1 channels of x (the previous
 * layer's BatchNorm + ReLU, applied while the tile is loaded; isc NULL = identity).  stats (optional): partials
 * [groups][2][ceil32(cout)] of sum y and sum y^2 (before res / relu) for pcr_bn_fwd_finalize_f32.  cout <= 384. */
typedef struct pcr_tdense_fwd {
  int B, cin1, cin2, cout, L;
  const float *x, *x2;
  const float *isc, *ish;
  int in_relu;
  const float *wp, *bias;      /* packed (cout, cin1+cin2); bias zero-padded to ceil32(cout) or NULL */
  const float *res;
  int out_relu;
  float *y;
  float *stats;
  /* optional fused pooling of a grouped MLP's LAST layer (L = S pool_K rows per cloud): the max over the K rows of every
   * centre of relu(BatchNorm(y)) has its winner at the max of the RAW y where pool_gamma[c] >= 0 and at the min where
   * it is negative, so the launch can leave pool_ymax (B,cout,S) = the raw y at the winning row and pool_arg (B,cout,S)
   * = that row -- what pcr_sa_pool_fwd_f32 computes from a second pass over y.  Only the wave-autonomous kernels do
   * this (pool_K >= 32, L a multiple of lcm(32, pool_K)): pcr_tdense_fwd_pooled() says whether THIS launch will;
   * otherwise the fields are ignored and the caller runs pcr_sa_pool_fwd_f32. */
  int pool_K;
  const float *pool_gamma;
  float *pool_ymax;
  int *pool_arg;
} pcr_tdense_fwd;
int pcr_tdense_fwd_f32(const pcr_tdense_fwd *p, pcr_stream_t stream);
int pcr_tdense_fwd_pooled(const pcr_tdense_fwd *p);

/* Backward of that layer.  dy is formed while the tiles are loaded: dy_mode 0: dy = g; 1: dy = ka g + kb y + kc
 * (BatchNorm backward, constants from pcr_bn_bwd_finalize_f32; y = the layer's stored raw output); 2: dy = g [y > 0]
 * (layer stored after its ReLU); 3: as 1 with g = the gradient gp (B,cout,S) of the max-pooled output routed to row
 * argmax (B,cout,S) of every centre where pooled (B,cout,S) > 0 (L = S K; pooled NULL: gp is already zero there).
 * Outputs (each optional): dx / dx2 = W^T dy masked by f(x) > 0 when in_relu (wpT = packed W^T); dstats = partials
 * [groups][2][ceil32(cin1)] of sum dx and sum dx * (raw x) for the next BatchNorm backward (iinv = 1 / isc);
 * dwp = partials [groups][ceil32(cout)][ceil32(cin)] of dy f(x)^T, dbp = partials [groups][ceil32(cout)] of sum dy
 * (reduce with pcr_reduce_parts_f32).  cout <= 384, cin1 + cin2 <= 288, and dy and the forward input of a 64-token tile
 * must fit the LDS together: ((max(ceil32(cout), ceil32(cin)) + ceil32(cin)) * 65 + 3 cout + 3 cin1) * 4 <= 160 KiB with
 * cin = cin1 + cin2 -- (256, 288), (288, 256) and (384, 192) are taken, (320, 288), (352, 256) and (384, 224) are not.  A
 * shape outside returns PCR_ERR_INVALID before anything is launched (pcr_amd.train_ops.dense tiles such layers). */
typedef struct pcr_tdense_bwd {
  int B, cin1, cin2, cout, L;
  const float *g, *y;
  int dy_mode;
  const float *ka, *kb, *kc;
  const int *argmax;
  const float *pooled;
  int K, S;
  const float *x, *x2;
  const float *isc, *ish, *iinv;
  int in_relu;
  const float *wpT;
  float *dx, *dx2, *dstats, *dwp, *dbp;
  long part_stride;   /* floats between consecutive workgroups' dwp / dbp partials; 0 = two dense arrays */
  /* optional (ABI 11): precision = PCR_PREC_BF16X3 with wpT_bf = the bf16 hi / lo image of W^T
   * (pcr_pack_weight_bf16_dev_f32, transpose = 1) runs the 128 x 128 layers' dx and dW as split bf16 on the bf16 matrix
   * core (three MFMAs per product, f32 accumulation); every other shape ignores both fields */
  int precision;
  const float *wpT_bf;
} pcr_tdense_bwd;
int pcr_tdense_bwd_f32(const pcr_tdense_bwd *p, pcr_stream_t stream);
/* device-side pcr_pack_weight_bf16x2_f32: the bf16 hi / lo image of W (rows x cols, leading dimension ld; transpose = 0)
 * or of W^T (transpose = 1); packed holds pcr_packed_weight_bf16_floats(cout, cin) floats */
int pcr_pack_weight_bf16_dev_f32(const float *w, int rows, int cols, int ld, int transpose, float *packed,
                                 pcr_stream_t stream);

/* Training-mode core of local_self_attention (attention.py:262-296): qkv (B,3C,N) channel-major = the fused q | k | v
 * projection of feat + pos(xyz) per POINT, idx (B,N,K) feature-space neighbours (pcr_knn_feat_f32).
 * fwd: msg (B,C,N), msg_i = sum_j a_ij v_j / (sum_j a_ij + eps), a_ij = <elu(q_i)+1, elu(k_j)+1> per head.
 * bwd: g (B,C,N) -> dq (C rows of N per cloud, clouds dq_bstride floats apart: a slice of the (B,3C,N) gradient) and
 * the per-edge gradients edge (B,2C,N,K) = [d k_j | d v_j contributions]; pcr_group_bwd_f32(edge, idx, .) folds them
 * onto the points (no float atomics).  C <= 64, C / nhead a power of two. */
int pcr_local_attn_train_fwd_f32(const float *qkv, const int *idx, float *msg, int B, int N, int C, int K, int nhead,
                                 float eps, pcr_stream_t stream);
int pcr_local_attn_train_bwd_f32(const float *qkv, const int *idx, const float *g, float *dq, long dq_bstride, float *edge,
                                 int B, int N, int C, int K, int nhead, float eps, pcr_stream_t stream);

/* out[r][c] = sum over p < nparts (increasing p) of part[p * stride + r * ld + c] */
int pcr_reduce_parts_f32(const float *part, int nparts, long stride, int rows, int cols, int ld, float *out,
                         pcr_stream_t stream);

/* n reductions of that kind in ONE launch (round 5): out (rows x cols, contiguous) = sum over p < nparts (increasing p) of
 * part[p stride + r ld + c].  `jobs` is a HOST array (passed by value in the kernel arguments, 64 per launch): the
 * regions of a backward launch's partial record are summed into compact per-parameter tensors (pcr_amd/train_ops.py:
 * reduce_regions). */
typedef struct pcr_reduce_job {
  const float *part;
  float *out;
  long stride;
  int nparts, rows, cols, ld;
} pcr_reduce_job;
int pcr_reduce_multi_f32(const pcr_reduce_job *jobs, int n, pcr_stream_t stream);

/* BatchNorm (training) from the statistics partials [nparts][2][ceil32(C)] over R rows: mean, biased variance ->
 * scale = gamma invstd, shift = beta - mean scale, inv_scale = 1 / scale; running statistics updated in place
 * (momentum, unbiased variance) when given.  nn.BatchNorm2d semantics (pointnet2_utils.py:353-355). */
typedef struct pcr_bn_fwd_fin {
  const float *part;
  int nparts, C;
  double R;
  const float *gamma, *beta;
  float eps, momentum;
  float *running_mean, *running_var;
  float *scale, *shift, *inv_scale, *mean, *invstd;
  /* optional: the partials are sums of (y - shift0[c * shift0_stride]) and of its square (a per-channel offset close
   * to the mean removes the cancellation of E[y^2] - mean^2); NULL = plain sums */
  const float *shift0;
  int shift0_stride;
} pcr_bn_fwd_fin;
int pcr_bn_fwd_finalize_f32(const pcr_bn_fwd_fin *p, pcr_stream_t stream);

/* BatchNorm backward constants from partials [nparts][2][ceil32(C)] of S1 = sum dyhat, S2 = sum dyhat * y:
 * dbeta = S1, dgamma = invstd (S2 - mean S1), and ka, kb, kc with dy = ka dyhat + kb y + kc */
typedef struct pcr_bn_bwd_fin {
  const float *part;
  int nparts, C;
  double R;
  const float *gamma, *mean, *invstd;
  float *ka, *kb, *kc, *dgamma, *dbeta;
  const float *centre;   /* optional (C): S2 was taken of dyhat * (y - centre[c]) (centre = mean: no cancellation); NULL = 0 */
} pcr_bn_bwd_fin;
int pcr_bn_bwd_finalize_f32(const pcr_bn_bwd_fin *p, pcr_stream_t stream);

/* First layer of the grouped edge MLP from per-point tables (training; csrc/train_sa_kernels.hip):
 * y[b][c][s K + k] = wa[c] . (xyz[idx] - xyz[s]) + bias[c] + tab[b][c][idx] + tab[b][c1 + c][s]   (tab NULL: no
 * point features), stats = partials [B][2][ceil32(c1)] of sum y, sum y^2.  Centres are the first S points. */
int pcr_sa_l1_fwd_f32(const float *xyz, const int *idx, const float *tab, const float *wa, const float *bias,
                      float *y, float *stats, int B, int N, int S, int K, int c1, pcr_stream_t stream);
/* its backward: dy = ka g + kb y + kc; dtab (B,2 c1,N) = [sum of dy over the rows that gathered each point ; sum over
 * the K rows of each centre (zero beyond S)], dwa = partials [B][c1][4] of (d wa, d bias).  No atomics: every
 * accumulator has one owner that adds in row order. */
int pcr_sa_l1_bwd_f32(const float *xyz, const int *idx, const float *g, const float *y, const float *ka,
                      const float *kb, const float *kc, float *dtab, float *dwa, int B, int N, int S, int K, int c1,
                      pcr_stream_t stream);
/* The same pair for a ball-query group (QueryAndGroup with use_xyz: rows [dxyz, f_i]) whose centres are sampled points:
 * centre (B,S) int32 holds every centre's point index, tab (B,c1,N) or NULL is P alone (no centre half), bias may be
 * NULL:  y[b][c][s K + k] = wa[c] . (xyz[idx] - xyz[centre[b][s]]) + tab[b][c][idx] (+ bias[c]);  stats as above.
 * Backward: dtab (B,c1,N) = sum of dy over the rows that gathered each point (a row repeated in idx counts once per
 * copy), dwa as above.  Same kernels, same ownership rule: no atomics, bit-reproducible.  PCR_ERR_INVALID, before any
 * launch, for a NULL centre, N > 8192 (one channel's table row must fit the 32 KiB LDS slice) or K, S < 1; S may
 * exceed N.  The VALUES of idx and centre are the caller's to guarantee, as for pcr_sa_l1_*: every one must lie in
 * [0, N) -- the kernels index the cloud and the table slice in LDS with them unchecked. */
int pcr_sa_l1c_fwd_f32(const float *xyz, const int *idx, const int *centre, const float *tab, const float *wa,
                       const float *bias, float *y, float *stats, int B, int N, int S, int K, int c1, pcr_stream_t stream);
int pcr_sa_l1c_bwd_f32(const float *xyz, const int *idx, const int *centre, const float *g, const float *y,
                       const float *ka, const float *kb, const float *kc, float *dtab, float *dwa, int B, int N, int S,
                       int K, int c1, pcr_stream_t stream);
/* pooled[b][c][s] = max_k relu(scale[c] y[b][c][s K + k] + shift[c]), argmax = the first k attaining it, ymax (optional)
 * = the raw y at that row (what the backward's BatchNorm sums need) */
int pcr_sa_pool_fwd_f32(const float *y, const float *scale, const float *shift, float *pooled, int *argmax, float *ymax,
                        int B, int C, int S, int K, pcr_stream_t stream);
/* partials [B][2][ceil32(C)] of S1 = sum gp [pooled > 0], S2 = sum gp [pooled > 0] ymax for pcr_bn_bwd_finalize_f32;
 * gz (optional, (B,C,S)) = gp [pooled > 0], the routed gradient: pass it as g with pooled = NULL to dy_mode 3 */
int pcr_sa_pool_bwd_stats_f32(const float *gp, const float *pooled, const float *ymax, float *part, float *gz, int B, int C,
                              int S, pcr_stream_t stream);

/* LayerNorm / GroupNorm over the channels of every token of x (B,C,L) (G groups of C/G consecutive channels; LayerNorm:
 * G = 1), y = [relu]((x - mean) rstd gamma + beta [+ res]); mean / rstd (B,G,L) are kept for the backward.  Backward: dx and
 * partials [ceil(B L / 64)][2][C] (one row per 64-token wave) of (d gamma, d beta) for pcr_reduce_parts_f32.  csrc/train_attn_kernels.hip. */
int pcr_tnorm_fwd_f32(const float *x, const float *gamma, const float *beta, const float *res, float *y, float *mean,
                      float *rstd, int B, int C, int L, int G, float eps, int relu, pcr_stream_t stream);
/* y_relu: the forward output when relu was set (the gradient is masked by y > 0 first), else NULL; dres (optional): the
 * masked gradient = gradient of the residual input */
int pcr_tnorm_bwd_f32(const float *g, const float *x, const float *gamma, const float *mean, const float *rstd,
                      const float *y_relu, float *dx, float *dres, float *part, int B, int C, int L, int G,
                      pcr_stream_t stream);

/* Linear-attention core (LinearAttention.forward, models/pointnet2_utils.py:26-47), forward and backward, one workgroup
 * per (cloud, head): Q' = elu(q)+1, K' = elu(k)+1, V' = v/Sk, A = sum_s K'_s V'_s^T, ks = sum_s K'_s,
 * out_l = (Q'_l^T A) Sk / (Q'_l . ks + eps).  q / k / v (and dq / dk / dv) are (d, L) channel-major blocks per cloud
 * addressed with a batch stride, so slices of a fused (B,3d,L) projection need no copies.  d / H in {16, 32, 64, 128}.
 * A (B,H,dh,dh) and ks (B,H,dh) are written by the forward and read by the backward. */
typedef struct pcr_linattn {
  int B, Lq, Sk, d, H;
  float eps;
  const float *q, *k, *v;
  long q_bs, k_bs, v_bs;
  float *out, *A, *ks;
  const float *dout;
  float *dq, *dk, *dv;
  long dq_bs, dk_bs, dv_bs;
  int kv_roll;                /* (ABI 13, appended) query cloud b reads the keys / values of cloud (b + kv_roll) % B and writes
                               * their gradients there: the matching stage's "halves swapped" without a rolled copy */
} pcr_linattn;
int pcr_linattn_fwd_f32(const pcr_linattn *p, pcr_stream_t stream);
int pcr_linattn_bwd_f32(const pcr_linattn *p, pcr_stream_t stream);

/* Fused per-token chain: the TAIL of an attention block in training mode (round 5, csrc/train_chain_kernels.hip) --
 * Self_Attention (models/pointnet2_utils.py:105-114), FP_SA (:428-437), corss_attention (models/attention.py:210-219):
 *   out = LN2(W2 relu(W0 [res ; LN1(Wm msg)])) [+ res]        msg (B,d,L) = the attention core's output, res (B,c1,L)
 * as ONE forward and ONE backward launch (the unfused graph: merge, norm, two dense layers, norm = 5 + 7 launches and
 * five partial-sum reductions).  A 64-token tile walks the chain inside LDS; the backward recomputes the chain for its
 * tile (bit-identically: same code) and keeps nothing but msg and res.  wm / w0 / w2 are pcr_pack_weight images of merge
 * (d,d), mlp[0] (hid, c1+d), mlp[2] (out,hid); w*T of their transposes; g1 b1 (d), g2 b2 (out) the LayerNorm affines;
 * residual needs out == c1.  Backward outputs: dmsg (B,d,L), dres (B,c1,L) and per-workgroup partial records
 * [pcr_attn_tail_groups][part_stride >= pcr_attn_tail_part_floats] =
 *   dWm [d][d] | dW0 [hid][ceil32(c1+d)] | dW2 [out][hid] | dgamma1 [d] | dbeta1 [d] | dgamma2 [out] | dbeta2 [out]
 * to be summed by pcr_reduce_parts_f32 (fixed order: gradients are bit-identical from run to run).
 * pcr_attn_tail_ok: is (d, c1, hid, out) one of the instantiated shapes (the reference's mul = 1 blocks with d <= 64)? */
typedef struct pcr_attn_tail {
  int B, L, d, c1, hid, out, residual;
  float eps;
  const float *msg, *res;
  const float *wm, *w0, *w2, *wmT, *w0T, *w2T;
  const float *g1, *b1, *g2, *b2;
  float *outp;                /* forward */
  const float *dout;          /* backward */
  float *dmsg, *dres, *parts;
  long part_stride;
  int precision;              /* (ABI 14, appended) arithmetic of the BACKWARD's matrix phases (dx, dW): PCR_PREC_F32 =
                               * f32-input MFMAs, wmT / w0T / w2T pcr_pack_weight images; PCR_PREC_BF16X3 = split bf16 on the
                               * bf16 matrix core, wmT / w0T / w2T pcr_pack_weight_bf16x2_f32 images (pcr_pack_weights_multi_f32
                               * kind 1), the f32 tile in LDS converted where it is consumed.  The forward chain and its
                               * recomputation keep the unfused launches' f32 fmaf chains: same ReLU masks, same values */
  int fwd_precision;          /* (ABI 14) PCR_PREC_BF16X3: the forward chain (and the recomputation, and then the backward
                               * whatever `precision` says) as split bf16 too, wm / w0 / w2 bf16 images -- an opt-in: a
                               * ReLU whose argument is within ~1e-5 of zero may open where the f32 graph keeps it shut */
} pcr_attn_tail;
int pcr_attn_tail_ok(int d, int c1, int hid, int out, int residual);
int pcr_attn_tail_part_floats(int d, int c1, int hid, int out);
int pcr_attn_tail_groups(const pcr_attn_tail *p);
int pcr_attn_tail_fwd_f32(const pcr_attn_tail *p, pcr_stream_t stream);
int pcr_attn_tail_bwd_f32(const pcr_attn_tail *p, pcr_stream_t stream);

/* Fused per-token chain: the HEAD of an attention block in training mode (csrc/train_chain_kernels.hip) -- position MLP,
 * residual add and the projections that read the result (models/pointnet2_utils.py:92-100 Self_Attention, :410-421 FP_SA;
 * models/attention.py:195-205 corss_attention):
 *   fp = x + P2 relu(P1 xyz + c1) + c2          x (B,c,L), xyz (B,3,L) channel-major, P1 (hd,3), P2 (c,hd)
 *   out (B, np d, L) = [W_0 s_0 ; ... ; W_{np-1} s_{np-1}],  s_j = fp if bit j of src is set, else x;  W_j (d,c)
 * (self block: q | k | v of fp, src = 7; cross / FP block: k of x | v of fp, src = 2) as one launch each way; the backward
 * recomputes the chain for its tile.  p1 / p2 / w[j] are pcr_pack_weight images, p2T / wT[j] of the transposes, c1 / c2
 * zero-padded to a multiple of 32 floats.  Backward outputs: dx (B,c,L) and per-workgroup partial records
 * [pcr_attn_head_groups][part_stride >= pcr_attn_head_part_floats] =
 *   dP1 [hd][32] | dP2 [c][hd] | dW_0 [d][c] | .. | dc1 [hd] | dc2 [c]        for pcr_reduce_parts_f32. */
typedef struct pcr_attn_head {
  int B, L, c, hd, d, np, src;
  const float *x, *xyz;
  const float *p1, *p2, *c1, *c2, *p2T;
  const float *w[3], *wT[3];
  float *outp;                /* forward */
  const float *dout;          /* backward */
  float *dx, *parts;
  long part_stride;
  int precision;              /* (ABI 14, appended) as pcr_attn_tail.precision: p2T, wT[] bf16 hi / lo images when
                               * PCR_PREC_BF16X3 */
  int fwd_precision;          /* as pcr_attn_tail.fwd_precision: p2, w[] bf16 images; p1 (three input channels) stays an f32
                               * image either way */
} pcr_attn_head;
int pcr_attn_head_ok(int c, int hd, int d, int np, int src);
int pcr_attn_head_part_floats(int c, int hd, int d, int np, int src);
int pcr_attn_head_groups(const pcr_attn_head *p);
int pcr_attn_head_fwd_f32(const pcr_attn_head *p, pcr_stream_t stream);
int pcr_attn_head_bwd_f32(const pcr_attn_head *p, pcr_stream_t stream);

/* Match-head pooling in training (get_pooled_feats 'both' over the point-concatenated pair, models/ReIDNet.py:529-532):
 * o (2P,C,L) -> pooled (P,2C) = [max, mean] over the 2L points of pair p (clouds p, p+P), arg (P,C) = position of the
 * maximum; backward: dout (2P,C,L) from g (P,2C). */
int pcr_pool_pair_fwd_f32(const float *o, float *pooled, int *arg, int P, int C, int L, pcr_stream_t stream);
int pcr_pool_pair_bwd_f32(const float *g, const int *arg, float *dout, int P, int C, int L, pcr_stream_t stream);
/* The same pooling for ONE tensor (match types that pool a single branch: `xcorr-baseline`, models/ReIDNet.py:258-264
 * with get_pooled_feats 'both' :529-532): o (P,C,L) -> pooled (P,2C) = [max over L, mean over L], arg (P,C); and its
 * backward dout (P,C,L). */
int pcr_pool_both_fwd_f32(const float *o, float *pooled, int *arg, int P, int C, int L, pcr_stream_t stream);
int pcr_pool_both_bwd_f32(const float *g, const int *arg, float *dout, int P, int C, int L, pcr_stream_t stream);
/* get_pooled_feats 'max' (models/ReIDNet.py:145, 526-528: nn.MaxPool1d(W) on the permuted (B,L,C) tensor) with the
 * winning channel kept for the backward: x (B,C,L) -> y (B,C/W,L), arg (B,C/W,L); backward dx (B,C,L). */
int pcr_channel_max_fwd_f32(const float *x, float *y, int *arg, int B, int C, int L, int W, pcr_stream_t stream);
int pcr_channel_max_bwd_f32(const float *g, const int *arg, float *dx, int B, int C, int L, int W, pcr_stream_t stream);

/* BatchNorm in batch-statistics mode as a stand-alone layer on (B,C,L) channel-major tensors (PointNet's BatchNorm1d
 * layers, models/pointnet.py:27-45, 103-127; csrc/train_bn_kernels.hip).
 * pcr_bn_sums_f32: partials [nparts][2][ceil32(C)] for pcr_bn_fwd_finalize_f32 (g NULL: sum y', sum y'^2) or
 *   pcr_bn_bwd_finalize_f32 (g given: sum g', sum g' y' with g' = g [scale y + shift > 0] when relu, else g), where
 *   y' = y - centre[c] (centre given), y - y[0][c][0] (centre NULL, centre_first != 0) or y.
 * pcr_bn_affine_f32: g NULL: out = [relu](a0 y + a1) (a0 = scale, a1 = shift); g given: out = a0 g' + a1 (y - centre[c])
 *   + a2, the gradient with respect to y: (ka, kb, kc) with centre NULL, or its centred form (ka, kb, -ka dbeta / R) with
 *   centre = the batch mean. */
int pcr_bn_sums_f32(const float *y, const float *g, const float *scale, const float *shift, int relu, float slope,
                    const float *centre, int centre_first, float *part, int nparts, int B, int C, int L,
                    pcr_stream_t stream);
int pcr_bn_affine_f32(const float *y, const float *g, const float *a0, const float *a1, const float *a2,
                      const float *scale, const float *shift, const float *centre, int relu, float slope, float *out,
                      int B, int C, int L, pcr_stream_t stream);
/* (relu != 0: the activation after the norm is z > 0 ? z : slope z -- ReLU with slope 0, LeakyReLU(0.2) with 0.2.)
 * EdgeConv tail in training mode (models/dgcnn_orig.py:127-143) on the materialised pre-activation y (B,C,N K):
 * pooled (B,C,N) = act(max_k (scale y + shift)), arg = the first k attaining it, yraw = y there; and the pooled gradient
 * routed back to its edge: g (B,C,N K) = gp act'(pooled) at k == arg, 0 elsewhere. */
int pcr_edge_pool_fwd_f32(const float *y, const float *scale, const float *shift, float slope, float *pooled, int *arg,
                          float *yraw, int B, int C, int N, int K, pcr_stream_t stream);
int pcr_edge_pool_route_f32(const float *gp, const float *pooled, const int *arg, float slope, float *g, int B, int C,
                            int N, int K, pcr_stream_t stream);
/* Per-cloud transforms (torch.bmm(x^T, T)^T, models/pointnet.py:109-111, 117-119): x (B,k,N), T (B,k,k) ->
 * y[b][j][n] = sum_i T[b][i][j] x[b][i][n]; transposed = 1 applies T^T instead (the backward's dx from dy);
 * pcr_bmm_dt_f32: dT[b][i][j] = sum_n x[b][i][n] dy[b][j][n].  1 <= k <= 128 for both (the apply keeps T[b] in
 * k (k + 1) floats of LDS: 66 048 bytes at k = 128, launched with the large-LDS opt-in); B = 0 is a no-op. */
int pcr_bmm_apply_f32(const float *x, const float *T, float *y, int B, int k, int N, int transposed, pcr_stream_t stream);
int pcr_bmm_dt_f32(const float *x, const float *dy, float *dT, int B, int k, int N, pcr_stream_t stream);

/* The packed images of MANY weights in one launch (a training step re-packs every weight after the update: ~76 small
 * launches otherwise).  descs (device): per tensor the contiguous row-major (rows x cols) matrix w and out, which
 * receives the image of W (pcr_packed... ceil8(cols) * ceil32(rows) floats) followed by the image of W^T
 * (ceil8(rows) * ceil32(cols) floats), as pcr_pack_weight_dev_f32(transpose = 2) lays them out.
 * cols == 0 marks a BIAS entry: w holds `rows` floats that are copied to the head of out, the caller's zero-padded
 * ceil32(rows) image (what the train-dense launches seed their accumulators from). */
typedef struct pcr_pack_desc {
  const float *w;
  float *out;
  int rows, cols;
  int kind;                   /* (ABI 14) 0: the f32 images above (or a bias); 1: the bf16 hi / lo images instead --
                               * pcr_pack_weight_bf16_dev_f32's image of W (pcr_packed_weight_bf16_floats(rows, cols)
                               * floats) followed by that of W^T (pcr_packed_weight_bf16_floats(cols, rows) floats) */
  int reserved;
} pcr_pack_desc;
int pcr_pack_weights_multi_f32(const pcr_pack_desc *descs_dev, int n, pcr_stream_t stream);

/* Parameter update of one iteration over EVERY parameter tensor in two launches: the global gradient norm of mmcv's
 * OptimizerHook(grad_clip=dict(max_norm, norm_type=2)) = torch.nn.utils.clip_grad_norm_, then torch.optim.AdamW's
 * step (configs_reid/_base_/schedules/cyclic_200e_lr3e-4.py:7-9; the cyclic lr / beta1 of lines 10-21 arrive as
 * per-tensor constants).  `tab` (device) lists the tensors; the launch is cut into chunks of pcr_opt_chunk() elements,
 * chunk i = elements [chunk_first[i], +chunk) of tensor chunk_tensor[i] (both device arrays).  A tensor whose g is
 * NULL is skipped (no gradient this iteration).  Per element, with g' = g * coef:
 *   p <- p * decay;  m <- m + one_m_beta1 (g' - m);  v <- beta2 v + one_m_beta2 g'^2;
 *   p <- p - step_size * m / (sqrt(v) / bc2_sqrt + eps)
 * where the host sets (in double, then rounds) decay = 1 - lr * weight_decay, step_size = lr / (1 - beta1^step),
 * bc2_sqrt = sqrt(1 - beta2^step), one_m_beta = 1 - beta.
 * pcr_grad_sumsq_f32 writes one sum of squares per chunk into part (n_chunks doubles); pcr_adamw_step_f32 with
 * part != NULL adds them in a fixed order, writes the norm to *grad_norm (optional) and, when max_norm > 0, uses
 * coef = min(1, max_norm / (norm + 1e-6)) and stores g' back into g; with part == NULL coef = 1.  No atomics: the
 * update is reproducible bit for bit. */
typedef struct pcr_opt_tensor {
  float *p, *g, *m, *v;
  long n;
  float step_size, bc2_sqrt, decay, one_m_beta1, beta2, one_m_beta2, eps, pad_;
} pcr_opt_tensor;
int pcr_opt_chunk(void);
int pcr_grad_sumsq_f32(const pcr_opt_tensor *tab, const int *chunk_tensor, const int *chunk_first, int n_chunks,
                       double *part, pcr_stream_t stream);
int pcr_adamw_step_f32(const pcr_opt_tensor *tab, const int *chunk_tensor, const int *chunk_first, int n_chunks,
                       const double *part, float max_norm, float *grad_norm, pcr_stream_t stream);

/* ------------------------------------------------- C2. auxiliary training losses ------------ */

/* The two auxiliary losses of ReIDNet.forward_train with a hot path: get_kl_loss (ReIDNet.py:467-482) and
 * get_triplet_loss (:538-582).  (cls and fp are two small heads composed from the launches of section C.)  Common rules:
 * no host read, no allocation; every sum has one order fixed by the launch shape (per-thread strides in index order, a
 * shuffle tree, the waves left to right) and the only atomics are integer ones, so every output is reproducible bit for
 * bit; every launch can be captured.  No entry point takes a float or long scalar: margin and alpha travel in
 * hyper (2) f32 ON THE DEVICE = (margin, alpha), like the upstream gradient gout (1) and the seed.
 * info (1) is a word of sticky flags that the launches OR into and never clear:
 *   PCR_AUX_INFO_KL_EMPTY      the batch holds no match or only matches: the empty group's mean counts as 0;
 *   PCR_AUX_INFO_TRIPLET_NONE  no triplet was formed (no matching pair with a pool): the loss is 0;
 *   PCR_AUX_INFO_TRIPLET_POOL  a matching pair found no row with another id: its row of neg is -1 (inactive).
 * The reference gives NaN in the first two cases and raises in the third; that is the one deviation.
 *
 * kl.  h (2B, D) f32: row i is h1[i].flat, row B + i is h2[i].flat (the two halves of the contiguous (2B, C, N) tensor,
 * D = C N); match (B) int32, nonzero = a match.  With x = log_softmax(h1[i]), t = log_softmax(h2[i]), p2 = exp(t):
 *   kl[i] = (1/D) sum_j p2_j (t_j - x_j) = (1/D) [cross[i] - (lse[B + i] - lse[i])],  cross[i] = sum_j p2_j (h2_j - h1_j)
 *   loss  = mean over non-matches of -kl[i]  +  mean over matches of kl[i]            (unscaled: alpha is the caller's)
 * pcr_kl_pairs_fwd_f32 -> lse (2B), cross (B), kl (B), loss (1), counts (2) int32 = (non-matches, matches).  One workgroup
 * per pair makes ONE pass over the two rows with an online maximum and sum (any D >= 1); one finalising workgroup counts
 * the groups and adds the pairs in index order in binary64.
 * pcr_kl_pairs_bwd_f32: with w_i = +-gout[0] / (counts[group of i] * D) (minus for a non-match), in closed form
 *   dh[i][k]     = w_i (p1_k - p2_k)
 *   dh[B + i][k] = w_i p2_k [(h2_k - h1_k) - cross[i]]
 * every element of dh (2B, D) is written. */
#define PCR_AUX_INFO_KL_EMPTY 1
#define PCR_AUX_INFO_TRIPLET_NONE 2
#define PCR_AUX_INFO_TRIPLET_POOL 4
int pcr_kl_pairs_fwd_f32(const float *h, const int *match, float *lse, float *cross, float *kl, float *loss, int *counts,
                         int *info, int B, int D, pcr_stream_t stream);
int pcr_kl_pairs_bwd_f32(const float *h, const int *match, const float *lse, const float *cross, const int *counts,
                         const float *gout, float *dh, int B, int D, pcr_stream_t stream);

/* triplet.  For every matching pair i the anchor is row i of h (2B, D), the positive row B + i, and T negatives are
 * rows whose id differs from ids[i]; the loss is TripletMarginLoss(margin, p = 2) over all triplets,
 * d(x, y) = || (x - y) + PCR_PAIR_DIST_EPS ||_2.  pcr_triplet_ok(B, T): 2B <= PCR_TRIPLET_MAX_ROWS (the pool and the
 * counters of a pair live in LDS) and B T < 2^31.
 *
 * pcr_triplet_draw_i32: ids (2B) int32, match (B) int32 -> neg (B, T) int32, one wave per pair.  The row of a
 * non-matching pair is -1.  For a matching pair the pool is the list of rows r in [0, 2B) with ids[r] != ids[i], in index
 * order, P entries; with W_t = rand[i T + t] (rand (B T) int32 read as bits, for tests) or W(seed, 3, i, t) of section A6
 * and pick(u, len) = ((uint64)u * len) >> 32:
 *   P == 0: the row is -1 and PCR_AUX_INFO_TRIPLET_POOL is set;
 *   P <  T: neg[i][t] = pool[pick(W_t, P)]                                     (with replacement)
 *   P >= T: for t = 0 .. T - 1: j = t + pick(W_t, P - t); swap(pool[t], pool[j]); neg[i][t] = pool[t]
 *           (T steps of a Fisher-Yates shuffle: without replacement) -- torch.multinomial's replacement= rule of the
 *           reference (:554).  seed is a DEVICE pointer to one int64 (NULL = 0) that the caller advances after the draw,
 *           so a replayed graph draws afresh.  The stream of samples is not torch's; the distribution is.
 *
 * pcr_pair_dist_f32: a (B, D), h (R, D) -> dist (B, R) = || (a_i - h_r) + eps ||_2 by direct differences: a 32 x 32 tile per
 * workgroup, D in chunks of 32 through LDS, one f32 accumulator per entry that walks d = 0 .. D - 1.  (Not the Gram form:
 * |a|^2 + |h|^2 - 2 a.h cancels where anchor and positive converge.)  Any D >= 1.  The positive's distance is column B + i.
 *
 * pcr_triplet_select_f32: dist (B, 2B), neg (B, T), match (B), hyper -> E (B, 2B), pair_loss (B), loss (1), count (1)
 * int32.  A row takes part when match[i] != 0 and neg[i][0] >= 0; its triplet t is ACTIVE when
 * v = dist[i][B + i] - dist[i][neg[i][t]] + margin > 0 (an entry of neg outside [0, 2B) is skipped).
 *   pair_loss[i] = sum of the active v;  count = T * (rows taking part);  loss = alpha * sum_i pair_loss[i] / count
 *   E[i][r]      = #{t active, neg[i][t] = r} / dist[i][r];   E[i][B + i] -= k_i / dist[i][B + i], k_i = #{t active}
 *   a coefficient whose distance is exactly 0 is 0.  count == 0: loss 0, PCR_AUX_INFO_TRIPLET_NONE.
 *
 * pcr_pair_dist_bwd_f32: with g = gout[0] * alpha / count (0 when count == 0), all read on the device,
 *   da[i] = -g sum_r E[i][r] ((a_i - h_r) + eps)          dh[r] = +g sum_i E[i][r] ((a_i - h_r) + eps)
 * by direct differences; an output row belongs to one workgroup per 1024 columns, which adds the other side's rows in
 * index order (coefficients through LDS, zero ones skipped).  The anchors are rows of h: the caller adds da into dh[:B]. */
#define PCR_PAIR_DIST_EPS 1e-6f
#define PCR_TRIPLET_MAX_ROWS 8192
int pcr_triplet_ok(int B, int T);
int pcr_triplet_draw_i32(const int *ids, const int *match, const int *rand, const long long *seed, int *neg, int *info,
                         int B, int T, pcr_stream_t stream);
int pcr_pair_dist_f32(const float *a, const float *h, float *dist, int B, int R, int D, pcr_stream_t stream);
int pcr_triplet_select_f32(const float *dist, const int *neg, const int *match, const float *hyper, float *E,
                           float *pair_loss, float *loss, int *count, int *info, int B, int T, pcr_stream_t stream);
int pcr_pair_dist_bwd_f32(const float *a, const float *h, const float *E, const float *gout, const float *hyper,
                          const int *count, float *da, float *dh, int B, int R, int D, pcr_stream_t stream);

/* ------------------------------------------------- C3. training on a pair list -------------- */

/* The training twin of match_gallery: every object of a step is encoded ONCE and a list of (i, j) slots is matched,
 * differentiably (pcr_amd/train_graph.py match_logits_list, ReIDNet.match_gallery_train).  Rules:
 *   objects  h (M, C, N), xyz (M, N, 3): the encoded objects of the current step, with their autograd history.
 *   list     pairs (cap, 2) int32 on the device; count (1) int32 on the device, or NULL = cap.  Only
 *            pairs[:min(count, cap)] are live.  Slots from count on must hold valid indices (compare_pairs writes (0, 0));
 *            a slot with an index outside [0, M) is dead.  Dead slots contribute exactly zero to every gradient and to
 *            the loss.
 *   logits   slot p scores as the training graph scores the one pair (h[i], xyz[i]) against (h[j], xyz[j]), i first.
 *            xcorr_eff is symmetric; xcorr-baseline, xcorr and concat are one-way, as in match_gallery.
 *   loss     sum_{p < count} bce(logit_p, match_p) / max(count, 1), formed on the device over a mask arange(cap) < count.
 *   cartesian rule (the reference's sampling == 'cartesian', models/ReIDNet.py:339-344): the list is
 *            cartesian_prod(arange(b), arange(b)) in that order; slot (i, j) is object i of side 1 against object j of
 *            side 2, rows i and b + j of cat(h1, h2); match = (id_1[i] == id_2[j]); the loss is the BCE-with-logits mean
 *            over the b^2 slots times alpha['match'].
 *
 * pcr_index_sum_f32 is the one scatter primitive: src (P, R), idx (P) int32, count as above, dst (M, R):
 *   dst[m][r] = sum over p < min(count, P) with idx[p] == m of src[p][r]
 * in f32, added in increasing p, starting from +0; a row no live slot names is written as 0.  An index outside [0, M)
 * names no row.  Every (m, chunk of R) accumulator has one owning workgroup, which compacts the slots that name m into
 * LDS in list order and then adds their rows: no float atomics, the same bits on every run.  It is the backward of
 * out[p] = x[idx[p]].  R <= 65535 * 1024. */
int pcr_index_sum_f32(const float *src, const int *idx, const int *count, float *dst, int P, int M, int R,
                      pcr_stream_t stream);

/* The linear-attention core of pcr_linattn split in two and addressed by index lists (csrc/train_pair_kernels.hip).  The
 * fused core keeps A | ks per (cloud, head) and writes dk / dv of the cloud it read, which needs the query -> key mapping
 * to be a permutation (kv_roll).  A pair list is many-to-one, so the state and its gradient are per OBJECT:
 *   state_fwd  per (object m, head): A_m = sum_s K'_s V'_s^T, ks_m = sum_s K'_s from the object's own k, v.
 *   apply_fwd  per (slot r, head):   out_r = (Q'_{qi[r]}^T A_{si[r]}) L / (Q'_{qi[r]} . ks_{si[r]} + eps)      (R, d, L)
 *   apply_bwd  per (slot r, head):   dqs_r (R, d, L), the slot's query gradient, and its record
 *                                    rec_r = [dA_r (dh x dh) | dks_r (dh)]                          (R, H, dh (dh + 1))
 *   state_bwd  per (object m, head): dk, dv of the object from drec_m = the sum of the records of the slots with
 *                                    si[r] == m (pcr_index_sum_f32) and its own k, v.
 * The per-object query gradient is pcr_index_sum_f32 of dqs over qi.  Launch order: state_fwd, apply_fwd; apply_bwd, the
 * two index sums, state_bwd.  For a list of cap pairs R = 2 cap, qi = [i.. ; j..], si = [j.. ; i..]: direction 1 of every
 * pair, then direction 2, so slots p and p + cap are pair p -- the layout pcr_pool_pair and kv_roll = cap of the next
 * stage expect.  A slot with qi or si outside [0, M) is dead: apply_fwd writes zeros for it, apply_bwd writes nothing.
 * Its dqs and rec rows keep whatever the buffers held, so the caller of pcr_index_sum_f32 must pass lists in which a dead
 * slot is dead in BOTH: -1 in qi and in si wherever either was outside [0, M) (train_ops.LinAttnPairs forms them).
 * eps >= 0, 0 included: the padding tokens of a partial 64-token chunk (Q' = 0, so 1 / (Q'.ks + eps) = 1 / eps) are inert
 * in both apply launches -- their reciprocal is taken as 0 -- and a live token has Q'.ks > 0.
 * q / k / v / dk / dv are (d, L) channel-major blocks per object addressed with a batch stride in floats (q_bs; kv_bs for
 * k and v; dkv_bs for dk and dv: slices of a fused (M, 3d, L) projection); Lq = Sk = L.  A (M,H,dh,dh) and ks (M,H,dh)
 * are written by state_fwd.  eps is a DEVICE pointer to one f32: as in section C2 no entry point takes a float scalar.
 * Same arithmetic as pcr_linattn's matrix-core form, tile for tile: f32,
 * v_mfma_f32_32x32x2_f32.  pcr_linattn_pairs_ok(d, H): d / H in {32, 64} (every point-cat matching stage: d = 64,
 * H = 2); other shapes take the gathered route (pcr_linattn on gathered per-slot tensors). */
int pcr_linattn_pairs_ok(int d, int H);
int pcr_linattn_state_fwd_f32(const float *k, const float *v, int kv_bs, float *A, float *ks, int M, int L, int d, int H,
                              pcr_stream_t stream);
int pcr_linattn_apply_fwd_f32(const float *q, int q_bs, const float *A, const float *ks, const int *qi, const int *si,
                              const float *eps, float *out, int M, int R, int L, int d, int H, pcr_stream_t stream);
int pcr_linattn_apply_bwd_f32(const float *q, int q_bs, const float *A, const float *ks, const int *qi, const int *si,
                              const float *eps, const float *dout, float *dqs, float *rec, int M, int R, int L, int d, int H,
                              pcr_stream_t stream);
int pcr_linattn_state_bwd_f32(const float *k, const float *v, int kv_bs, const float *drec, float *dk, float *dv,
                              int dkv_bs, int M, int L, int d, int H, pcr_stream_t stream);

/* ---- measurement aid (bench.py; not on the hot path) ---- */

/* Sustained f32-MFMA probe: n_wg workgroups (one per CU: pass the CU count) each run iters * 16
 * v_mfma_f32_32x32x2_f32 per wave (= iters * 1024 matrix-pipe cycles) and write ticks[2 wg] = shader-clock ticks,
 * ticks[2 wg + 1] = constant-rate wall-clock ticks (pcr_wall_clock_khz) spent on them.  The clock the matrix core
 * ran at is iters * 1024 / (wall ticks / rate): what `roofline.clock_ghz` in the bench line reports. */
int pcr_wall_clock_khz(void);
/* PCR_PREC_* the matrix phases of the calling thread's LAST pcr_sa_mlp / pcr_dense_pm / pcr_attn_kv / pcr_attn_apply
 * launch really ran in (-1: none yet).  A requested precision is a request: shapes a bf16 unit does not instantiate run
 * f32, the tile kv kernel projects in f32 in every mode.  bench.py prices a launch against the peak of THIS arithmetic. */
int pcr_last_launch_arith(void);
int pcr_clock_probe(unsigned long long *ticks, int n_wg, int iters, pcr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCR_H_ */
