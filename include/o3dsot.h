/*
 * o3dsot.h -- C-ABI of libo3dsot_hip.so, the MI355X (gfx950) native replacement for the
 * `pointnet2_ops._ext` operator set that Open3DSOT's hot path calls.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer (HIP), row-major contiguous, fp32 / int32;
 *   - the call only ENQUEUES work on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream): no allocation, no host synchronisation, caller owns every buffer;
 *   - return value: O3D_OK (0) or a negative O3D_E* code; nothing is thrown;
 *   - stateless and thread-safe.
 *
 * Each declaration cites the reference interface it replaces (paths relative to the
 * Open3DSOT tree).  The reference binds these through the pybind module
 * `pointnet2_ops._ext` (pointnet2/utils/pointnet2_utils.py:17); INTEGRATION.md shows the
 * ctypes stub that re-creates that module on top of this header.
 */
#ifndef O3DSOT_H_
#define O3DSOT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define O3D_OK 0
#define O3D_EINVAL (-1)   /* bad shape / null pointer / unsupported size */
#define O3D_ELAUNCH (-2)  /* the HIP runtime refused a launch or memset     */

/* Library identification: returns a static string "o3dsot-hip <ver> gfx950". */
const char* o3d_version(void);

/* ---- furthest point sampling -------------------------------------------------------
 * replaces _ext.furthest_point_sampling(xyz, npoint)      pointnet2_utils.py:56
 * xyz (B,N,3) f32 -> idx (B,npoint) i32.  Iterative FPS from index 0; points with
 * |p|^2 <= 1e-3 are never selected; tie order identical to the upstream thread-block
 * reduction (block = opt_n_threads(N)).  `temp` is a (B,N) f32 scratch that is only
 * touched when N > 8192 (may be NULL otherwise). */
int o3d_furthest_point_sampling(const float* xyz, int B, int N, int npoint, float* temp,
                                int32_t* idx, void* stream);

/* Test hook: the same sampling with the wave arg-max through ds_bpermute shuffles instead of DPP (the two
 * reductions must agree bit for bit, tests/test_index_ops_gpu.py). */
int o3d_furthest_point_sampling_shfl(const float* xyz, int B, int N, int npoint, float* temp, int32_t* idx,
                                     void* stream);

/* Two independent sets of B clouds in ONE launch (the template and the search cloud of a tracker step,
 * models/bat.py:89-90: 2 x B one-wave workgroups side by side instead of back to back).  Each set's indices are
 * bit-identical to o3d_furthest_point_sampling on it.  max(N0,N1) <= 2048, else O3D_EINVAL (make two calls). */
int o3d_furthest_point_sampling_pair(const float* xyz0, int N0, int npoint0, int32_t* idx0, const float* xyz1,
                                     int N1, int npoint1, int32_t* idx1, int B, void* stream);

/* ---- gather ---------------------------------------------------------------------------
 * replaces _ext.gather_points(features, idx)              pointnet2_utils.py:92
 * feats (B,C,N), idx (B,npoint) -> out (B,C,npoint).  B <= 65535.  N == 0 with anything to gather (B, C, npoint > 0) is
 * O3D_EINVAL: no index could be in range. */
int o3d_gather_points(const float* feats, const int32_t* idx, int B, int C, int N, int npoint,
                      float* out, void* stream);
/* replaces _ext.gather_points_grad(grad_out, idx, N)      pointnet2_utils.py:98
 * grad_out (B,C,npoint) -> grad_feats (B,C,N); grad_feats is zero-filled by the call (a refused call writes nothing). */
int o3d_gather_points_grad(const float* grad_out, const int32_t* idx, int B, int C, int N,
                           int npoint, float* grad_feats, void* stream);

/* rows of a point-major tensor: src (B,N,D), idx (B,npoint) -> out (B,npoint,D), out[b,j,:] = src[b,idx[b,j],:].
 * The ball centres of a set abstraction, new_xyz = gather_operation(xyz^T, fps_idx)^T (pointnet2_modules.py:52-62),
 * without the two transposed copies. */
int o3d_gather_rows(const float* src, const int32_t* idx, int B, int N, int D, int npoint, float* out, void* stream);

/* o3d_gather_rows for one or two point-major tensors (a (B,N,Da), b (B,N,Db) | NULL with Db = 0) through the same index, whose
 * rows may be a prefix of a longer index (idx[b * ld_idx + j], ld_idx >= npoint): the seed labels / BoxCloud rows of the
 * trackers (models/bat.py:96-97,132-133: `.long()` + expand + torch.gather per tensor). */
int o3d_gather_rows2(const float* a, int Da, const float* b, int Db, const int32_t* idx, long ld_idx, int B, int N, int npoint,
                     float* outa, float* outb, void* stream);

/* ---- ball query -----------------------------------------------------------------------
 * replaces _ext.ball_query(new_xyz, xyz, radius, nsample) pointnet2_utils.py:268
 * new_xyz (B,npoint,3), xyz (B,N,3) -> idx (B,npoint,nsample) i32: first `nsample`
 * indices k (ascending) with d^2 < radius^2, padded with the first hit, zeros if none. */
int o3d_ball_query(const float* new_xyz, const float* xyz, int B, int N, int npoint, float radius,
                   int nsample, int32_t* idx, void* stream);

/* Sampling gather + ball query of one or two sets of clouds in one launch: centres = xyz[b, sidx[b, j]] (sidx (B, npoint)
 * int32, or NULL: the first npoint points, pointnet2_modules.py:56) written to `centers` ((B*npoint0 + B*npoint1 + 1, 3):
 * set 0's, set 1's, then an origin row), idx_s (B, npoint_s, nsample) = ball_query around them (bit-identical to
 * o3d_ball_query on the gathered centres).  npoint1 = 0: one set.  Replaces gather_operation + ball_query of
 * pointnet2_modules.py:52-64 / pointnet2_utils.py:92,268 for both clouds of a backbone level. */
int o3d_sample_query(const float* xyz0, const int32_t* sidx0, int N0, int npoint0, int32_t* idx0, const float* xyz1,
                     const int32_t* sidx1, int N1, int npoint1, int32_t* idx1, int B, float radius, int nsample,
                     float* centers, void* stream);

/* ---- grouping -------------------------------------------------------------------------
 * replaces _ext.group_points(features, idx)               pointnet2_utils.py:217
 * feats (B,C,N), idx (B,npoint,nsample) -> out (B,C,npoint,nsample).  B <= 65535.  N == 0 with anything to group
 * (B, C, npoint * nsample > 0) is O3D_EINVAL: no index could be in range. */
int o3d_group_points(const float* feats, const int32_t* idx, int B, int C, int N, int npoint,
                     int nsample, float* out, void* stream);
/* replaces _ext.group_points_grad(grad_out, idx, N)       pointnet2_utils.py:237
 * grad_out (B,C,npoint,nsample) -> grad_feats (B,C,N); zero-filled by the call (a refused call writes nothing). */
int o3d_group_points_grad(const float* grad_out, const int32_t* idx, int B, int C, int N,
                          int npoint, int nsample, float* grad_feats, void* stream);

/* ---- 3-NN + inverse-distance interpolation ------------------------------------------
 * replaces _ext.three_nn(unknown, known)                  pointnet2_utils.py:125
 * unknown (B,n,3), known (B,m,3) -> dist2 (B,n,3) f32 SQUARED distances, idx (B,n,3) */
int o3d_three_nn(const float* unknown, const float* known, int B, int n, int m, float* dist2,
                 int32_t* idx, void* stream);
/* replaces _ext.three_interpolate(features, idx, weight)  pointnet2_utils.py:162
 * feats (B,c,m), idx (B,n,3), weight (B,n,3) -> out (B,c,n).  m == 0 with anything to interpolate (B, c, n > 0) is
 * O3D_EINVAL: feats has no column to read (o3d_three_nn with m == 0 returns idx 0 and dist2 inf, which must not come here). */
int o3d_three_interpolate(const float* feats, const int32_t* idx, const float* weight, int B,
                          int c, int m, int n, float* out, void* stream);
/* replaces _ext.three_interpolate_grad(grad_out, idx, weight, m)  pointnet2_utils.py:184
 * grad_out (B,c,n) -> grad_feats (B,c,m); zero-filled by the call (a refused call writes nothing). */
int o3d_three_interpolate_grad(const float* grad_out, const int32_t* idx, const float* weight,
                               int B, int c, int n, int m, float* grad_feats, void* stream);

/* ---- stable k-nearest selection -----------------------------------------------------
 * replaces torch.cdist + torch.argsort(...)[:k]   models/head/xcorr.py:81,87 and
 *                                                 pointnet2_utils.py:399-400 (knn_point)
 * query (B,Q,D), ref (B,R,D) -> idx (B,Q,k) i32, ascending squared distance, ties ->
 * lowest ref index (argsort leaves tie order unspecified; this pins it).  1 <= k <= 32. */
int o3d_knn(const float* query, const float* ref, int B, int Q, int R, int D, int k,
            int32_t* idx, void* stream);


/* ======================================================================================
 * Fused grouped-MLP layers (fp32-MFMA GEMMs, open3dsot_amd/csrc/mlp.hip).
 * Replace, per SharedMLP layer, Conv2d(1x1,bias=False) + BatchNorm2d + ReLU
 *                                   pointnet2/utils/pytorch_utils.py:12-37,68-121
 * the QueryAndGroup gather feeding layer 0          pointnet2_utils.py:299-339
 * the max-pool over nsample                          pointnet2_modules.py:69-73
 * BoxAwareXCorr's group + mlp + max                  models/head/xcorr.py:89-100
 * and the autograd backward of that chain.  P = npoint*nsample positions per batch item,
 * P % 128 == 0 and nsample % 4 == 0.  "Raw" tensors Y are conv outputs BEFORE BatchNorm;
 * consumers apply BN+ReLU on load via per-channel (scale, shift).
 * ====================================================================================== */

/* Y[b,co,p] = sum_ci W[co,ci] * f(X[b,ci,p]);  f = identity when in_scale == NULL, else
 * f(x) = max(x*in_scale[ci] + in_shift[ci], 0).  X (B,Cin,P), W (Cout,Cin), Y (B,Cout,P).
 * part != NULL: receives per-tile partial statistics [B*P/128][2][Cout] = {sum y,
 * sum (y - stat_c[co])^2} (stat_c == NULL means 0).  in_scale and in_shift are both given or both NULL: exactly one of them
 * NULL is refused with O3D_EINVAL. */
int o3d_mlp_conv_fwd(const float* X, const float* W, const float* in_scale, const float* in_shift,
                     int B, int Cin, int Cout, int P, float* Y, float* part, const float* stat_c,
                     void* stream);

/* BatchNorm statistics from the partials, forward and backward.  One job per BatchNorm layer; njobs = 1 or 2 (two
 * independent layers, e.g. of two conv stacks advancing side by side, share ONE launch).  jobs: HOST array.
 * The partial list of a job: part [nparts (+ nparts1)][2][C] rows of per-tile sums.
 *   meta == NULL: every row is live and tile is ignored.  Otherwise (compact layout) only the first
 *     ceil(meta[0] / tile) rows are live; tile = columns per partial row (> 0).
 *   nparts1 == 0: one segment.  Otherwise two segments in one launch (template + search cloud through a shared module,
 *     models/bat.py:89-90): segment 1's rows follow segment 0's nparts, its count is count1, its live columns meta[4],
 *     and stat_c / mean / invstd / scale / shift / A1..A3 are laid out (2,C).  Same numbers as one job per segment,
 *     segment 0 first; the running statistics see segment 0's update first.
 *   meta != NULL and tile == 128: the rows of a direct GEMM launch -- the extra rows of its remainder tiles (see
 *     o3d_direct_tail_slots below, with C = the launch's output rows) follow the nparts + nparts1 regular ones.
 * Forward, training mode: mean, invstd = 1/sqrt(var_biased+eps), scale = gamma*invstd, shift = beta - mean*scale (C
 * each) from partials {sum y, sum (y - stat_c)^2} over `count` positions (stat_c == NULL means 0); when running_mean !=
 * NULL and momentum >= 0 the running statistics are updated like torch.nn.BatchNorm (unbiased var). */
typedef struct {
    const float* part; int nparts, C; double count; const float* stat_c; const float* gamma; const float* beta;
    float* running_mean; float* running_var; float momentum, eps; float* mean; float* invstd; float* scale; float* shift;
    const int32_t* meta; int tile, nparts1; double count1;
} o3d_bn_fin_args;
int o3d_bn_finalize(const o3d_bn_fin_args* jobs, int njobs, void* stream);

/* out[b,c,j] = max_k relu(Y[b,c,j*ns+k]*scale[c] + shift[c]); optional arg (k of the max) and
 * yarg (raw Y at that k) for the backward pass. */
int o3d_bn_relu_maxpool_fwd(const float* Y, const float* scale, const float* shift, int B, int C,
                            int npoint, int ns, float* out, int32_t* arg, float* yarg, void* stream);

/* The same for ONE cloud of npoint balls in the flat (C, npoint) layout (the P2B fusion: npoint = B*N), the balls of
 * a channel split over nsplit workgroups: part [nsplit][2][C]. */
int o3d_pool_bwd_partials_split(const float* dOut, const float* out, const float* yarg, const float* mean, int C,
                                int npoint, int nsplit, float* part, const int32_t* arg, float* pk, void* stream);

/* Backward, from partials {sum dN, sum dN*(Y-mean)}: dgamma, dbeta (C each, summed over the segments) and the
 * per-channel coefficients of dY = A1*dN + A2*Y + A3. */
typedef struct {
    const float* part; int nparts, C; double count; const float* gamma; const float* mean; const float* invstd;
    float* dgamma; float* dbeta; float* A1; float* A2; float* A3;
    const int32_t* meta; int tile, nparts1; double count1;
} o3d_bn_bwd_fin_args;
int o3d_bn_bwd_finalize(const o3d_bn_bwd_fin_args* jobs, int njobs, void* stream);

/* Data gradient of an inner layer.  dY comes from dN (dense, (B,Cout,P)) or, when dN == NULL,
 * from the pooled triple (dOut, out, arg) of o3d_bn_relu_maxpool_fwd.  Writes
 * dNprev (B,Cin,P) = (W^T dY) masked by the producer's ReLU (Yprev*scale_p+shift_p > 0) and the
 * producer's BN-backward partials [B*P/128][2][Cin]. */
int o3d_mlp_conv_dgrad(const float* dN, const float* dOut, const float* out, const int32_t* arg,
                       int ns, const float* Y, const float* A1, const float* A2, const float* A3,
                       const float* W, int B, int Cin, int Cout, int P, const float* Yprev,
                       const float* scale_p, const float* shift_p, const float* mean_p,
                       float* dNprev, float* part, void* stream);

/* o3d_mlp_conv_dgrad with the transposed weights Wt (Cin,Cout) supplied as well: aligned shapes
 * (Cin % 64 == 0, Cout % 16 == 0) run the LDS-free kernel, which reads its A operand along Cout
 * and, for the pooled source, the packed pk of o3d_pool_bwd_partials_split instead of (dOut,out,arg). */
int o3d_mlp_conv_dgrad_wt(const float* dN, const float* dOut, const float* out, const int32_t* arg,
                          int ns, const float* Y, const float* A1, const float* A2, const float* A3,
                          const float* W, const float* Wt, const float* pk, int B, int Cin, int Cout, int P,
                          const float* Yprev, const float* scale_p, const float* shift_p,
                          const float* mean_p, float* dNprev, float* part, void* stream);

/* dX (B,Cin,P) = W^T (A1*dN + A2*Y + A3): gradient w.r.t. an operand that is not a BN+ReLU output
 * (the per-point operand [xyz;feats] of layer 0).  No mask, no statistics.  dN (dense, (B,Cout,P)), Y and A1..A3 are all
 * required -- there is no pooled source and no "dY = dN" shortcut here: any of them NULL is refused with O3D_EINVAL, as is
 * P % 128 != 0. */
int o3d_mlp_conv_dgrad_plain(const float* dN, const float* Y, const float* A1, const float* A2,
                             const float* A3, const float* W, int B, int Cin, int Cout, int P,
                             float* dX, void* stream);

/* Weight gradient dW (Cout,Cin) = sum_{b,p} dY[b,co,p] * X[b,ci,p]; X = f(X raw) as in
 * o3d_mlp_conv_fwd.  part: scratch of (nslices+16)*Cout*Cin floats (split over positions, reduced in a fixed
 * order).  X must not be NULL; in_scale and in_shift are both given or both NULL (exactly one of them NULL is refused with
 * O3D_EINVAL).  P % 32 == 0.  A slice that receives no 32-position chunk (nslices above B*P/32) writes zeros. */
int o3d_mlp_conv_wgrad(const float* dN, const float* dOut, const float* out, const int32_t* arg, int ns,
                       const float* Y, const float* A1, const float* A2, const float* A3,
                       const float* X, const float* in_scale, const float* in_shift, int B, int Cin, int Cout,
                       int P, int nslices, float* part, float* dW, void* stream);

/* Which kernel a batched entry above launches for a shape, computed by the entries' own rules (no launch):
 *   entry 0: o3d_mlp_conv_fwd, M = Cout, K = Cin, part = 1 when statistics partials are requested, else 0
 *   entry 1: o3d_mlp_conv_dgrad_wt with Wt given, M = Cin, K = Cout (part ignored)
 *   entry 2: o3d_mlp_conv_dgrad, o3d_mlp_conv_dgrad_plain, o3d_mlp_conv_dgrad_wt with Wt == NULL, M = Cin, K = Cout
 * -> 64 / 128 / 256: the LDS-staged generic kernel with that many rows per workgroup; 1000 * class + tile: the direct kernel
 * of csrc/mlp_direct.hip (class as o3d_direct_class, at this B; tile = columns per wave tile): 2064, 4064 or 3128;
 * -1: a shape the entry refuses.  tests/test_batched_gemm_kernels_gpu.py asserts it for every case. */
int o3d_mlp_conv_class(int entry, int B, int M, int K, int P, int part);

/* ---- compact (distinct-neighbour) layout, csrc/compact.hip ------------------------------------------
 * ball_query pads a ball with copies of its first hit (pointnet2_utils.py:268); copies have identical
 * values at every layer, so each ball keeps its cnt distinct entries as columns of flat (C, ldp)
 * matrices (ldp = worst-case column count) and the first hit carries the weight 1+nsample-cnt.
 * meta: 4 device ints per SEGMENT = {live columns rounded up to 256, live columns, balls, 0}; kernels
 * skip tiles beyond the live range -- no host synchronisation.
 * Segments: one fused call can carry two independent sets of clouds through the SAME weights with
 * SEPARATE BatchNorm statistics (template and search branch of the backbone, models/bat.py:89-90).
 * Segment 1's columns start at `start1` (a multiple of 256, = worst-case size of segment 0; 0 means one
 * segment), its point columns after segment 0's, its balls after segment 0's, and every per-channel
 * constant array holds segment 1's values right after segment 0's. */

/* One segment: idx (B,npoint,ns) -> ball_cnt (B*npoint), ball_off (B*npoint+1, absolute columns), per
 * column gp = pt_base + b*ld + point, cball = ball_base + ball (dummy_ball for padding columns), cw;
 * written at [col_base, col_base+live).  ns a power of two <= 64, B*npoint <= 65536. */
int o3d_compact_build(const int32_t* idx, int B, int npoint, int ns, int ld, int col_base, int pt_base,
                      int ball_base, int dummy_ball, int32_t* ball_cnt, int32_t* ball_off, int32_t* gp,
                      int32_t* cball, float* cw, int32_t* meta, void* stream);

/* Weight gradient of an xyz-only layer 0 whose input gradient is not needed (set abstraction level 0 of the backbone:
 * features None, models/backbone/pointnet.py:30-38), straight from the columns of the compact layout:
 * dW0[c,k] = sum_q (A1*dN + w*(A2*Y0 + A3))[c,q] * (X[k, gp[q]] - centers[cball[q], k]), k < 3.  Replaces the list-sum
 * reduction (o3d_group_reduce_gather), the K = 3 GEMM and the centre term.  part: (ldp/256)*C0*3 floats of scratch. */
int o3d_group_dw0_xyz(const float* dN, const float* Y0, long ldp, const float* A1, const float* A2, const float* A3,
                      const int32_t* gp, const int32_t* cball, const float* cw, const float* X, long ldz,
                      const float* centers, const int32_t* meta, long start1, int C0, float* part, float* dW, void* stream);

/* o3d_compact_build for the two segments of a paired call (template + search cloud through one shared module,
 * models/bat.py:89-90) in three launches instead of six: segment 0 at column / point / ball base 0, segment 1 at
 * col_base1 / pt_base1 / ball base B*npoint0; ball_cnt, ball_off: B*(npoint0+npoint1) (+1) entries, meta: 8 ints. */
int o3d_compact_build2(const int32_t* idx0, int npoint0, int ld0, const int32_t* idx1, int npoint1, int ld1, int B,
                       int ns, int col_base1, int pt_base1, int dummy_ball, int32_t* ball_cnt, int32_t* ball_off,
                       int32_t* gp, int32_t* cball, float* cw, int32_t* meta, void* stream);

/* Y0[c,q] = Z[c,gp[q]] - W0[c,0:3].centers[cball[q]] (QueryAndGroup + layer 0 after the per-point GEMM
 * Z = W0.[xyz;feats], pointnet2_utils.py:299-339); centers (balls+1, 3) or NULL; weighted statistics
 * partials part [ldp/256][2][C0] or NULL (stat_c: C0 floats per segment). */
int o3d_group_expand_c(const float* Z, long ldz, const int32_t* gp, const int32_t* cball, const float* cw,
                       const float* centers, const float* W0, int ldw, int C0, const int32_t* meta, long start1,
                       long ldp, float* Y0, float* part, const float* stat_c, void* stream);

/* o3d_group_expand_c for an xyz-only layer 0 (set abstraction level 0: features None) without the per-point GEMM:
 * Y0[c,q] = W0[c,0:3] . (X3[:, gp[q]] - centers[cball[q]]) -- the relative coordinate first, as pointnet2_utils.py:319-320
 * computes it; X3 = the packed coordinate operand (3 rows, ldz columns). */
int o3d_group_expand_c3(const float* X3, long ldz, const int32_t* gp, const int32_t* cball, const float* cw,
                        const float* centers, const float* W0, int ldw, int C0, const int32_t* meta, long start1, long ldp,
                        float* Y0, float* part, const float* stat_c, void* stream);

/* Inner layers on the compact layout: forward (BN+ReLU of the producer on load, weighted statistics),
 * data gradient (dY = A1*dN + w*(A2*Y + A3), ReLU mask, statistics; Wt = W^T), weight gradient.
 * tile = columns per wave tile = columns per statistics partial row: o3d_direct_tile(ldp, M, 1). */
int o3d_direct_tile(long P, int M, int compact);
/* Round 5: a 128-column direct GEMM launch over the compact layout (o3d_mlp_conv_fwd_c / o3d_mlp_conv_dgrad_c with tile = 128)
 * cuts the remainder tiles of its last resident round (T mod S live tiles, S = o3d_direct_tail_slots(output rows) resident
 * column-tile slots) into 2 or 4 column blocks that run as workgroups of the same launch, decided on the device from the live
 * count.  Their statistics go to EXTRA rows behind the regular ones: `part` must hold ldp/128 + nseg * S rows; the
 * o3d_bn_finalize / o3d_bn_bwd_finalize jobs with meta and tile = 128 follow the same plan (C = the launch's output rows). */
int o3d_direct_tail_slots(int M);
/* test hook: -1 automatic (default), 0 no remainder split, S > 0 pretend S slots for every shape */
int o3d_direct_tail_override(int slots);
/* The kernel class o3d_mlp_conv_fwd_c (M = Cout, K = Cin) / o3d_mlp_conv_dgrad_c (M = Cin, K = Cout) launch for ldp columns and
 * the caller's tile, computed by the launcher's own rules (no launch): 2 = 64 x 64 wave tiles, 3 = 64 x 128, 4 = the split-K
 * tile, -1 = a shape the entries refuse.  A class-3 launch splits its remainder tiles when o3d_direct_tail_slots(M) > 0.
 * tests/test_compact_gemm_kernels_gpu.py asserts it for every case. */
int o3d_direct_class(long ldp, int M, int K, int tile);
/* Columns: every entry below works on the columns [0, meta[0]) of segment 0 and [start1, start1 + meta[4]) of segment 1
 * (meta[4*s] = the live columns rounded up to 256) and neither reads nor writes any other column of an operand.  The padding
 * columns [live, live rounded up) carry w = 0 and are computed like live ones: the forward stores Y there and its statistics
 * weigh them by w = 0 (so X must be finite there).  The backward entries ASSUME dN == 0 AND finite Y, X / Yprev on the padding
 * columns: dY = A1*dN + w*(A2*Y + A3) is then 0 there, so padding adds nothing to dW, dNprev is written as 0 there, and the
 * data gradient's statistics -- which carry no w -- see only live columns.  (o3d_pool_bwd_c / o3d_pool_bwd_dense write such a
 * dN, and each data gradient hands the next one zeros.)  A non-zero dN on a padding column is counted like a live column. */
int o3d_mlp_conv_fwd_c(const float* X, const float* W, const float* in_scale, const float* in_shift, int Cin,
                       int Cout, long ldp, const float* w, const int32_t* meta, long start1, int tile, float* Y,
                       float* part, const float* stat_c, void* stream);
int o3d_mlp_conv_dgrad_c(const float* dN, const float* Y, const float* A1, const float* A2, const float* A3,
                         const float* Wt, int Cin, int Cout, long ldp, const float* w, const int32_t* meta,
                         long start1, int tile, const float* Yprev, const float* scale_p, const float* shift_p,
                         const float* mean_p, float* dNprev, float* part, void* stream);
int o3d_mlp_conv_wgrad2_c(const float* dN, const float* Y, const float* A1, const float* A2, const float* A3,
                          const float* X, const float* in_scale, const float* in_shift, int Cin, int Cout,
                          long ldp, const float* w, const int32_t* meta, long start1, float* scratch, float* dW,
                          void* stream);

/* out[b,c,j] = max over the ball's columns of relu(Y*scale+shift) (max_pool2d over nsample,
 * pointnet2_modules.py:69-73); argq = column of the maximum, yarg = raw Y there.  Pooled tensors hold
 * one (B,C,npoint_s) block per segment, segment 1's after segment 0's (npoint1 = 0: one segment). */
int o3d_pool_fwd_c(const float* Y, long ldp, const float* scale, const float* shift, const int32_t* ball_off,
                   const int32_t* ball_cnt, int B, int C, int npoint0, int npoint1, float* out, int32_t* argq,
                   float* yarg, void* stream);

/* o3d_pool_fwd_c with the tile transposed through LDS (lane = channel, a wave walks one ball's columns: no idle lanes for
 * the small balls the distinct-neighbour layout produces).  cball (ldp) = ball of every column, meta = the live counts of
 * o3d_compact_build; C % 32 == 0, nsample <= 32 (else O3D_EINVAL: use o3d_pool_fwd_c).  Same results. */
int o3d_pool_fwd_ct(const float* Y, long ldp, const float* scale, const float* shift, const int32_t* ball_off,
                    const int32_t* ball_cnt, const int32_t* cball, const int32_t* meta, long start1, int B, int C,
                    int npoint0, int npoint1, int nsample, float* out, int32_t* argq, float* yarg, void* stream);

/* Backward of the pool: D (C,ldp) = dense class-sum gradient (zero on live columns, D[c,argq] = dOut where
 * out > 0) and the BatchNorm-backward partials of the pooled layer, O3D_POOL_BWD_SPLIT rows per segment:
 * part [nseg][O3D_POOL_BWD_SPLIT][2][C]. */
#define O3D_POOL_BWD_SPLIT 8
int o3d_pool_bwd_c(const float* dOut, const float* out, const int32_t* argq, const float* yarg,
                   const float* mean, int B, int C, int npoint0, int npoint1, const int32_t* meta, long start1,
                   long ldp, float* D, float* part, void* stream);

/* o3d_pool_bwd_c in ONE pass (round 5): D's live columns are written once, column by column (gradient at the ball's arg-max
 * column, zero elsewhere), no zero fill.  cball / ball_off / meta from o3d_compact_build; C % 8 == 0, ldp % 512 == 0,
 * start1 % 512 == 0, else O3D_EINVAL (use o3d_pool_bwd_c).  part [ldp/512][2][C]: one partial row per 512-column chunk
 * (segment 1's rows after segment 0's Pmax0/512), only the live ones written: finalize with meta and tile = 512.
 * dOut0 / dOut1: the pooled-output gradient of segment 0 / 1 as (B, C, npoint_s) with batch / channel strides sb / sc in
 * floats, innermost stride 1; NULL = no gradient (zeros).
 * Replaces max_pool2d's backward of pointnet2_modules.py:70-73 together with o3d_pool_bwd_c. */
int o3d_pool_bwd_dense(const float* dOut0, long sb0, long sc0, const float* dOut1, long sb1, long sc1, const float* out,
                       const int32_t* argq, const float* yarg, const float* mean,
                       const int32_t* cball, const int32_t* ball_off, const int32_t* meta, long start1, long ldp, int B,
                       int C, int npoint0, int npoint1, float* D, float* part, void* stream);

/* The same sums as o3d_group_reduce_c without float atomics: the cloud's columns are sorted by (column chunk,
 * point) once per call (perm: ldp ints; poff: o3d_group_reduce_gather_scratch(...) ints, -1 = shape not covered,
 * use o3d_group_reduce_c) and the sums are gathers from an LDS-staged chunk.  The ball sums T add up in a fixed order;
 * the point sums S do not: the order inside a point's list comes from the LDS atomics of the sort, and a thread flushes
 * each run of equal points with one LDS float atomic, so two runs of the same call may differ in the last bits of S.
 * spanmax = npoint*nsample of the largest segment. */
long o3d_group_reduce_gather_scratch(int B, int nseg, int npoint0, int ld0, int npoint1, int ld1, int spanmax);
int o3d_group_reduce_gather(const float* dN, const float* Y0, long ldp, const float* A1, const float* A2,
                            const float* A3, const int32_t* gp, const float* cw, const int32_t* ball_off,
                            const int32_t* ball_cnt, int B, int nseg, int npoint0, int ld0, int npoint1, int ld1, int C0,
                            int spanmax, int32_t* perm, int32_t* poff, float* S, float* T, void* stream);

/* o3d_group_reduce_gather in a FIXED order (deterministic mode): same arguments, same poff, no float atomic; S and T are
 * one fp32 expression of (gp, ball_off, ball_cnt, sizes; dN, Y0, cw, A1..A3) -- independent of timing, of C0 and the
 * channel slabs, and of whether T is NULL.  o3d_group_reduce_gather_ordered_scratch: ints of poff, -1 = the shape does
 * not fit the ordered kernels' LDS budget (3 KiB / 8 KiB tighter than the default pair's; there is no ordered fallback).
 *
 * The order, per cloud (b of segment s; its point columns start at pbase, its balls at bbase):
 *   q0 = ball_off[bbase], q1 = ball_off[last ball] + ball_cnt[last ball], q0a = q0 & ~3, CH = 2048.
 *   Chunk k = the columns q of [q0, q1) with (q - q0a) / CH == k, i.e. [max(q0, q0a + k*CH), min(q1, q0a + (k+1)*CH)).
 *   dY[c, q] = fmaf(A1[c], dN[c, q], cw[q] * fmaf(A2[c], Y0[c, q], A3[c]))   (segment 1: A at +C0)
 *   perm: per chunk, the entries (n << 16) | (q - q0a - k*CH), n = gp[q] - pbase, sorted by ascending entry value (by point,
 *   then column); chunk k's entries are perm[q0 + poff[k*ld] .. q0 + poff[(k+1)*ld]), poff[k*ld + n] = start of point
 *   n's list, relative to q0, the cloud's total at poff[nchunk*ld].
 *   S[c, pbase + n] = acc, where acc = 0 and, for k = 0, 1, .. ascending with a non-empty list of n in chunk k:
 *       cnt = entries of chunk k, per = ceil(cnt / 256); the list occupies positions [a, b) of the chunk's entries;
 *       it is cut into pieces at the multiples of per inside (a, b); piece = (((0 + dY[e0]) + dY[e1]) + ..) over its
 *       entries in position order; total = ((piece0 + piece1) + piece2) ..; acc = acc + total.
 *   T[c, bbase + j] = acc, where acc = 0 and, for k ascending where ball j has columns in chunk k:
 *       t = (((0 + dY[s0]) + dY[s0+1]) + ..) over the ball's columns inside the chunk, ascending; acc = acc + t.
 * All additions are fp32 round-to-nearest, nothing is fused.  tests/ordered_reduce_oracle.py restates this in numpy. */
long o3d_group_reduce_gather_ordered_scratch(int B, int nseg, int npoint0, int ld0, int npoint1, int ld1, int spanmax);
int o3d_group_reduce_gather_ordered(const float* dN, const float* Y0, long ldp, const float* A1, const float* A2,
                                    const float* A3, const int32_t* gp, const float* cw, const int32_t* ball_off,
                                    const int32_t* ball_cnt, int B, int nseg, int npoint0, int ld0, int npoint1, int ld1,
                                    int C0, int spanmax, int32_t* perm, int32_t* poff, float* S, float* T, void* stream);

/* Per-point operand of layer 0 (QueryAndGroup's inputs before the gather, pointnet2_utils.py:318-333):
 * X0 (rows, ldz), ldz = B*(ld0 + ld1): rows [0,nxyz) = xyz^T * inv_radius, rows [nxyz, nxyz+C) = feats, further
 * rows zero; cloud b of segment s occupies columns [base_s + b*ld_s, +N_s), padded to ld_s by zeros.
 * xyz_s (B,N_s,3), feats_s (B,C,N_s); N1 = 0: one segment. */
int o3d_pack_points(const float* xyz0, const float* feats0, int N0, int ld0, const float* xyz1, const float* feats1,
                    int N1, int ld1, int B, int nxyz, int C, float inv_radius, int rows, float* X0, void* stream);

/* Centre term of the layer-0 weight gradient (grouped_xyz = xyz[idx] - new_xyz, pointnet2_utils.py:322-324):
 * dW (C0,ldw) columns 0..2 -= T (C0,nballs) . centers (nballs,3) */
int o3d_center_term(const float* T, const float* centers, int C0, int nballs, int ldw, float* dW, void* stream);
/* the same into a compact gradient: out (C0, ncols) = dW[:, :ncols], columns 0..2 minus the centre term (dW untouched) */
int o3d_center_term_out(const float* T, const float* centers, int C0, int nballs, int ldw, const float* dW, int ncols,
                        float* out, void* stream);

/* Gradient of the ball centres: out (3, nballs)[k, ball] = scale * sum_c W0[c, k] * T[c, ball] (grouped_xyz = xyz[idx] -
 * new_xyz, pointnet2_utils.py:319-320; live where the centres carry a gradient: the vote aggregation, rpn.py:55-60). */
int o3d_center_grad(const float* T, const float* W0, int ldw, int C0, int nballs, float scale, float* out, void* stream);

/* Layer-0 backward sums of dY = A1*dN + w*(A2*Y0 + A3): S (C0, point columns) per source point
 * (= group_points_grad, pointnet2_utils.py:237), T (C0, balls) per ball (may be NULL). */
int o3d_group_reduce_c(const float* dN, const float* Y0, long ldp, const float* A1, const float* A2,
                       const float* A3, const int32_t* gp, const int32_t* cball, const float* cw,
                       const int32_t* ball_off, const int32_t* ball_cnt, int B, int nseg, int npoint0, int ld0,
                       int npoint1, int ld1, int C0, float* S, float* T, void* stream);

/* ---- ends of a per-point MLP chain on the flat (C, P = B*N) layout (csrc/pointwise.hip): the M2-Track
 * stacks (models/backbone/pointnet.py:91-204) run on the GEMM kernels above; these finish a chain. */
/* out = relu(Y*scale+shift) */
int o3d_bn_relu_apply(const float* Y, const float* scale, const float* shift, int C, long P, float* out,
                      void* stream);
/* dN = g masked by the activation, part [P/128][2][C] = {sum dN, sum dN*(Y-mean)} */
int o3d_act_bwd_partials(const float* g, const float* Y, const float* scale, const float* shift,
                         const float* mean, int C, long P, float* dN, float* part, void* stream);
/* AdaptiveMaxPool1d(1) of relu(bn(Y)) per cloud: out (B,C), argq (B,C) column of the first maximum,
 * yarg raw Y there (backward: o3d_pool_bwd_c with one ball per cloud) */
int o3d_gmax_fwd(const float* Y, const float* scale, const float* shift, int B, int C, int N, float* out,
                 int32_t* argq, float* yarg, void* stream);

/* Weight gradient of an aligned inner layer (Cin, Cout, P multiples of 64), workgroup
 * tile matched to the layer: dW (Cout,Cin) = sum dY * f(X), dY = A1*dN + A2*Y + A3 from dN (dense) or,
 * when dN == NULL, from the packed pooled source pk of o3d_pool_bwd_partials_split; f(x) =
 * max(x*in_scale+in_shift, 0), or x when in_scale == in_shift == NULL.  scratch:
 * o3d_mlp_conv_wgrad2_scratch(...) floats. */
long o3d_mlp_conv_wgrad2_scratch(int B, int Cin, int Cout, int P);
int o3d_mlp_conv_wgrad2(const float* dN, const float* pk, int ns, const float* Y, const float* A1,
                        const float* A2, const float* A3, const float* X, const float* in_scale,
                        const float* in_shift, int B, int Cin, int Cout, int P, float* scratch, float* dW,
                        void* stream);

/* ---- 1-D conv stacks of the heads on the flat (C, P = B*N) layout -------------------------------------
 * Replaces pt_utils.Seq / Conv1d (+BatchNorm1d +ReLU) stacks, pointnet2/utils/pytorch_utils.py:124-155,300-457, as
 * used by models/head/rpn.py:16-39 (FC_layer_cla, vote_layer, FC_proposal), models/head/xcorr.py:14-17 (fea_layer)
 * and models/bat.py:22-26 (conv_final, mlp_bc): hidden layers conv -> BatchNorm -> ReLU (BatchNorm + ReLU applied
 * by the consumer on load, statistics partials from the producer), last layer conv + bias.
 * P % 64 == 0; contraction sizes % 16 == 0 and output rows % 64 == 0 (callers zero-pad, see o3d_pack_rows /
 * o3d_prep_weights).  Statistics partial rows are per o3d_pw_tile(P, output rows) columns. */
typedef struct { const float* p; long sb, sc, sn; int C; } o3d_rows_src;

/* X (rows, B*N) <- up to 4 sources of shape (B, C_i, N) with arbitrary strides (in floats) stacked along the rows
 * (torch.cat(dim=1) of e.g. [xyz^T ; features]: rpn.py:50, bat.py:94); rows beyond sum C_i are zero.
 * srcs: HOST array. */
int o3d_pack_rows(const o3d_rows_src* srcs, int nsrc, int B, int N, int rows, float* X, void* stream);
/* the same into a column block of a wider operand (X = the block's first column, ld = the operand's row stride): two sets
 * of clouds of different sizes as the columns of ONE GEMM -- conv_final on the template and on the search feature,
 * models/bat.py:91-92 */
int o3d_pack_rows_ld(const o3d_rows_src* srcs, int nsrc, int B, int N, int rows, float* X, long ld, void* stream);

/* The element-wise glue of the vote head, models/head/rpn.py:47-56 (round 5; strides in floats, sources (B, C, N) views):
 * score (B,N) = sigmoid(cla), vote_xyz (B,N,3) = vote[:, :3]^T, vote_feature (B,1+f,N) = cat(score, vote[:, 3:]) in one
 * launch (were sigmoid + a transposing copy + torch.cat); and its backward: dvote (3+f, B*N) = [d vote_xyz^T ; d vote_feature
 * [:, 1:]] in the flat layout of the conv stacks, dcla (B,N) = d vote_feature[:, 0] * s (1 - s); a NULL gradient is zeros. */
int o3d_rpn_votes_fwd(const float* cla, long cla_sb, long cla_sn, const float* vote, long v_sb, long v_sc, long v_sn, int B, int N,
                      int f, float* score, float* vote_xyz, float* vote_feature, void* stream);
int o3d_rpn_votes_bwd(const float* score, const float* dvf, long f_sb, long f_sc, long f_sn, const float* dvx, long x_sb, long x_sc,
                      long x_sn, int B, int N, int f, float* dcla, float* dvote, void* stream);
/* boxes (B,P,5) = transpose(cat(offsets[:, :3] + centers^T, offsets[:, 3:])) of models/head/rpn.py:62-66 (offsets (B,5,P) with
 * any strides, centers (B,P,3) contiguous): one launch (were add + cat + a transposing copy; the backward is two views). */
int o3d_box_assemble(const float* offsets, long o_sb, long o_sc, long o_sn, const float* centers, int B, int P, float* boxes,
                     void* stream);

/* Every padded / transposed weight copy of a step in one launch.  jobs: DEVICE array of njobs x 6 longs
 * {src ptr, dst ptr, rows, cols, dst_ld, transpose}: src (rows, cols) row-major -> dst[r*ld + c], or
 * dst[c*ld + r] when transpose != 0; the padding of dst is not written. */
int o3d_prep_weights(const long* jobs, int njobs, void* stream);

/* out (C) = row sums of G (C, P): bias gradient of a plain Conv1d layer. */
int o3d_row_sum(const float* G, int C, long P, float* out, void* stream);

int o3d_pw_tile(long P, int M);
/* The kernel class o3d_pw_fwd (M = Cout, K = Cin) / o3d_pw_dgrad (M = Cin, K = Cout) launch for a shape, computed by the
 * launcher's own rules (no launch): 2 = 64 x 64 wave tiles, 3 = 64 x 128, 4 = the split-K tile, 5 = the 32-row narrow
 * tile, -1 = a shape the entries refuse.  tests/test_gemm_kernels_gpu.py asserts it for every case. */
int o3d_pw_class(long P, int M, int K);

/* Data gradient + weight gradient of one aligned inner layer in ONE launch (csrc/mlp_wgrad.hip::fused_bwd_kernel):
 * replaces the pair o3d_mlp_conv_wgrad2_c + o3d_mlp_conv_dgrad_c for Cin == 64, Cout in {64, 128} and a dense dN --
 * dY and relu(bn(Yprev)) are staged once for both MFMA chains.  A1..A3 (nseg,Cout); in_scale / in_shift / in_mean
 * (nseg,Cin): BatchNorm of the producer layer; Wt (Cin,Cout) = W^T; w / meta / start1: compact layout (or NULL, NULL, 0).
 * scratch: o3d_mlp_conv_bwd_fused_scratch(...) floats.  part_s [2][rows][2][Cin], rows = o3d_mlp_conv_bwd_fused_rows(...)
 * (-1: shape not supported): BatchNorm-backward partials {sum g, sum g*(yprev-mean)} of dNprev, segment 1's block after
 * segment 0's -- finalize with an o3d_bn_bwd_finalize job over part_s: nparts = rows, nparts1 = rows for two segments,
 * meta = NULL. */
int o3d_mlp_conv_bwd_fused_rows(int Cin, int Cout, long P);
long o3d_mlp_conv_bwd_fused_scratch(int Cin, int Cout, long P);
int o3d_mlp_conv_bwd_fused_c(const float* dN, const float* Y, const float* A1, const float* A2, const float* A3,
                             const float* X, const float* in_scale, const float* in_shift, const float* in_mean,
                             const float* Wt, int Cin, int Cout, long ldp, const float* w, const int32_t* meta,
                             long start1, float* scratch, float* dW, float* part_s, float* dNprev, void* stream);

/* Two independent 1-D conv launches over the same number of columns as ONE launch (blockIdx.z selects): the stacks of
 * the RPN that read the same seeds -- FC_layer_cla and vote_layer, models/head/rpn.py:16-28,44-54 -- advance layer by layer
 * side by side.  Fields = the arguments of o3d_pw_fwd / o3d_pw_dgrad.  When the two problems do not take the same kernel
 * instantiation the entry issues the two single launches instead; the numbers are the same either way. */
typedef struct {
    const float* X; const float* W; const float* in_scale; const float* in_shift; const float* bias; const float* resid;
    int Cin, Cout; long P;
    float* Y; float* part; const float* stat_c;
} o3d_pw_fwd_args;
typedef struct {
    const float* dN; const float* Y; const float* A1; const float* A2; const float* A3; const float* Wt;
    int Cin, Cout; long P;
    const float* Yprev; const float* scale_p; const float* shift_p; const float* mean_p; const float* resid;
    float* dNprev; float* part;
} o3d_pw_dgrad_args;
int o3d_pw_fwd_pair(const o3d_pw_fwd_args* a, const o3d_pw_fwd_args* b, void* stream);
int o3d_pw_dgrad_pair(const o3d_pw_dgrad_args* a, const o3d_pw_dgrad_args* b, void* stream);

/* Several independent weight gradients of the flat (C, P) layout in one launch (+ one reduction launch): the 1-D conv
 * stacks of the heads (models/head/rpn.py:16-39, models/head/xcorr.py:14-17, models/bat.py:22-26).  Job i computes what
 * o3d_mlp_conv_wgrad2(dN, NULL, 4, Y, A1, A2, A3, X, in_scale, in_shift, 1, Cin, Cout, P, scratch, dW, stream) computes
 * (same tile plan and summation order); njobs <= 8; scratch: o3d_mlp_conv_wgrad2_scratch(1, Cin, Cout, P) floats each.
 * A job with X == NULL and Y == NULL is a ROW-SUM job (the bias gradient of a stack's last layer, o3d_row_sum):
 * dW (Cout) = row sums of dN (Cout, P). */
typedef struct {
    const float* dN; const float* Y; const float* A1; const float* A2; const float* A3;
    const float* X; const float* in_scale; const float* in_shift;
    int Cin, Cout; long P;
    float* scratch; float* dW;
    int out_rows, out_cols;      /* 0, 0: dW is (Cout, Cin); else dW is the COMPACT (out_rows, out_cols) top-left block of it
                                  * (the parameter's own shape when Cout / Cin are its zero-padded sizes) */
} o3d_wgrad_job;
int o3d_mlp_conv_wgrad2_group(const o3d_wgrad_job* jobs, int njobs, void* stream);

/* torch.optim.Adam's update (models/base_model.py:32-33) for all parameters in one launch: parameters and moments in
 * flat buffers, gradients found through a DEVICE job table of njobs x 3 longs {gradient ptr, offset, n};
 * bc1 = 1 - beta1^t, bc2 = 1 - beta2^t.  p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps), g += weight_decay*p first. */
int o3d_adam_step(const long* jobs, int njobs, float* params, float* exp_avg, float* exp_avg_sq, double lr,
                  double beta1, double beta2, double eps, double weight_decay, double bc1, double bc2, void* stream);

/* The rest of the flat-buffer optimizer family (csrc/optim.hip), on o3d_adam_step's job table; gradients may sit on any
 * 4-byte boundary.
 *
 * o3d_grad_norm: the total 2-norm of all gradients of the table and torch.nn.utils.clip_grad_norm_'s coefficient
 * (main.py:85 `gradient_clip_val`, norm clipping), in two plain launches: (njobs, O3D_NORM_SLICES) blocks store
 * partials[job * O3D_NORM_SLICES + slice] = the sum of (double)g * (double)g over the slice (0 for an empty one; every
 * entry is written, nothing needs clearing), one block adds them in a fixed order to S and writes
 *   out[0] = (float)sqrt(S),   out[1] = (float)min(1, max_norm / (sqrt(S) + 1e-6))      (double, rounded once).
 * partials: njobs * O3D_NORM_SLICES doubles, out: 2 floats, both DEVICE.  max_norm <= 0 (or NaN) is O3D_EINVAL: "no
 * clipping" means not calling.  Non-finite gradients follow the arithmetic (out[0] shows them; a NaN stays a NaN).
 *
 * o3d_adam_step_scaled: o3d_adam_step with g * *grad_scale in place of g (before the weight decay); grad_scale is a
 * DEVICE float, typically out + 1 above.  The same bits as o3d_adam_step on gradients scaled beforehand.
 *
 * o3d_sgd_step: torch.optim.SGD with momentum, dampening 0, no Nesterov (models/base_model.py:29-31), per element in
 * this order, each line one float rounding:
 *   g' = g * *grad_scale (grad_scale != NULL);  g' = fma(weight_decay, p, g') (weight_decay != 0);
 *   buf = fma(momentum, buf, g');  p = fma(-lr, buf, p).
 * A zero momentum buffer gives buf = g' exactly: torch's first-step rule without a flag. */
#define O3D_NORM_SLICES 32
int o3d_grad_norm(const long* jobs, int njobs, double max_norm, double* partials, float* out, void* stream);
int o3d_adam_step_scaled(const long* jobs, int njobs, float* params, float* exp_avg, float* exp_avg_sq, double lr,
                         double beta1, double beta2, double eps, double weight_decay, double bc1, double bc2,
                         const float* grad_scale, void* stream);
int o3d_sgd_step(const long* jobs, int njobs, float* params, float* momentum_buf, double lr, double momentum,
                 double weight_decay, const float* grad_scale, void* stream);

/* Best proposal of a tracked frame: replaces the host-side selection of MatchingBaseModel.evaluate_one_sample
 * (models/base_model.py:44-57: `estimation_box.cpu().numpy()`, `[:, 4].argmax()`, `[best, 0:4]`) -- SURVEY.md section
 * 8f-4 lists that device->host copy as part of the per-frame latency path.  boxes (B, P, 5) contiguous;
 * out (B, 4) = boxes[b, argmax_p boxes[b, p, 4], 0:4] with numpy's tie rule (first maximum); out_idx (B) int32 or NULL. */
int o3d_best_proposal(const float* boxes, int B, int P, float* out, int32_t* out_idx, void* stream);

/* A per-point stack whose input is [X ; a per-cloud CONSTANT block] (SegPointNet: the pooled feature broadcast to every
 * point and concatenated, models/backbone/pointnet.py:188-190): the constant block contributes W_b . pooled[b] to every
 * column of cloud b -- a per-cloud bias cbias (Cout, B), not 1024 more GEMM rows.
 * o3d_pw_fwd_cloud: Y (Cout, B*N) = W_a (Cout, Cin) . X + cbias[:, cloud], statistics partials [P/128][2][Cout] of it.
 * o3d_cloud_sum_dy: out (C, B) = per-cloud sums of dY = A1*dN + A2*Y + A3, the gradient of cbias. */
int o3d_pw_fwd_cloud(const float* X, const float* W, const float* cbias, int B, int N, int Cin, int Cout, float* Y,
                     float* part, const float* stat_c, void* stream);
int o3d_cloud_sum_dy(const float* dN, const float* Y, const float* A1, const float* A2, const float* A3, int C, int B,
                     int N, float* out, void* stream);

/* Eval-mode BatchNorm constants in one launch: vec (4, nrep, C) = {mean, invstd, scale, shift} with
 * invstd = 1/sqrt(running_var + eps), scale = gamma*invstd, shift = beta - mean*scale (pytorch_utils.py:56-59 in
 * eval mode); conv_bias (C) or NULL is a bias of the convolution in front, folded into the mean. */
int o3d_bn_eval_consts(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                       const float* conv_bias, float eps, int C, int nrep, float* vec, void* stream);

/* Y (Cout, P) = W (Cout, Cin) . f(X),  f = relu(x*in_scale + in_shift) per input row, or identity (both NULL).
 * part != NULL: BatchNorm statistics partials [P/tile][2][Cout] = {sum y, sum (y - stat_c)^2};
 * part == NULL: Y += bias[row] + resid (Cout, P), either may be NULL (last layer of a stack; the residual is the
 * `seeds + vote_layer(seeds)` of rpn.py:53). */
int o3d_pw_fwd(const float* X, const float* W, const float* in_scale, const float* in_shift, const float* bias,
               const float* resid, int Cin, int Cout, long P, float* Y, float* part, const float* stat_c,
               void* stream);

/* dNprev (Cin, P) = Wt (Cin, Cout) . dY,  dY = dN (Y == NULL) or A1*dN + A2*Y + A3.
 * Yprev != NULL: masked by relu(Yprev*scale_p + shift_p) > 0, BatchNorm-backward partials of the producer
 * [P/tile][2][Cin] = {sum g, sum g*(Yprev - mean_p)} in `part`;
 * Yprev == NULL: plain store (+ resid (Cin, P)): the gradient of the stack's input. */
int o3d_pw_dgrad(const float* dN, const float* Y, const float* A1, const float* A2, const float* A3,
                 const float* Wt, int Cin, int Cout, long P, const float* Yprev, const float* scale_p,
                 const float* shift_p, const float* mean_p, const float* resid, float* dNprev, float* part,
                 void* stream);

/* ---- P2B template<->search fusion, layer 0 (models/head/xcorr.py:25-53) ---------------------------------
 * The reference materialises x_ij = [cos_sim(t_i, s_j) ; xyz_i ; feat_i] for all M*N (template, search) pairs and
 * runs SharedMLP + max over the template axis.  Only channel 0 depends on j, so with Z = W0[:,1:].[xyz;feat]
 * (a GEMM over the M template points):   Y0[c, q] = Z[c, b*M + i] + W0[c*ldw] * sim[q],   q = (b*N + j)*M + i.
 * M a power of two in [4, 64], (M*N) % 1024 == 0, C0 % 16 == 0.  part [P/256][2][C0] = {sum y, sum (y-stat_c)^2}. */
int o3d_xcorr_expand(const float* Z, long ldz, const float* sim, const float* W0, int ldw, int B, int M, int N, int C0,
                     float* Y0, float* part, const float* stat_c, void* stream);

/* Backward of the above with dY0 = A1*dN + A2*Y0 + A3:  S (C0, lds) = sum over j (-> dW0[:,1:], d[xyz;feat] through
 * the per-point GEMMs), dsim_part (o3d_xcorr_reduce_groups(C0), P) = per-channel-group partial sums of
 * W0[c,0]*dY0 (the caller adds the rows), dw_part (B, C0) = per-cloud partial sums of dY0*sim (-> dW0[:,0]). */
long o3d_xcorr_reduce_groups(int C0);
int o3d_xcorr_reduce(const float* dN, const float* Y0, const float* A1, const float* A2, const float* A3,
                     const float* sim, const float* W0, int ldw, int B, int M, int N, int C0, float* S, long lds,
                     float* dsim_part, float* dw_part, void* stream);

/* ---- tracking inference: one set abstraction in ONE kernel ---------------------
 * Eval mode (models/base_model.py:59-86 tracks frame by frame, batch 1, BatchNorm on running statistics): gather +
 * centre subtraction + three 1x1 convolutions with BatchNorm + ReLU + max over nsample, activations in LDS.
 * out (B, C2, np) from Z (C0, ldz) = W0 . [xyz ; feats] per point (o3d_pack_points + o3d_mlp_conv_fwd),
 * idx (B, np, ns), centers (B*np, 3) or NULL, v_l (4, C_l) = o3d_bn_eval_consts of layer l.
 * C0 % 8 == 0, C1 % 32 == 0, C2 % 32 == 0, ns a power of two <= 32, (B*np*ns) % 32 == 0; ld = point columns per
 * cloud in Z, pt_base = first column of this set of clouds.  v1, v2 are read as float4: 16-byte aligned, else O3D_EINVAL
 * (W1, W2 may sit on any 4-byte boundary: views of a flat parameter buffer). */
int o3d_sa_eval_fused(const float* Z, long ldz, const int32_t* idx, const float* centers, const float* W0, int ldw,
                      const float* v0, const float* W1, const float* v1, const float* W2, const float* v2, int C0, int C1,
                      int C2, int B, int np, int ns, int ld, long pt_base, float* out, void* stream);

/* ---- P2B_XCorr's cosine similarity map (models/head/xcorr.py:37-38, nn.CosineSimilarity(dim=1, eps=1e-8)) ----------
 * sim (B,N,M)[b,j,i] = <t[b,:,i], s[b,:,j]> / (max(|t_i|, eps) * max(|s_j|, eps));  t (B,f,M), s (B,f,N) with ELEMENT
 * strides (batch, channel, point) -- the features are views of a flat conv output; tn (B,M), sn (B,N) = the clamped
 * norms (kept for the backward).  f % 32 == 0, M <= 64, M % 4 == 0, N <= 128.
 * Backward: dt (B,f,M), ds (B,f,N) contiguous from dsim (B,N,M). */
int o3d_cosine_sim_fwd(const float* t, long tsb, long tsc, long tsn, const float* s, long ssb, long ssc, long ssn, int B, int f,
                       int M, int N, float* sim, float* tn, float* sn, void* stream);
int o3d_cosine_sim_bwd(const float* dsim, const float* sim, const float* tn, const float* sn, const float* t, long tsb, long tsc,
                       long tsn, const float* s, long ssb, long ssc, long ssn, int B, int f, int M, int N, float* dt, float* ds,
                       void* stream);

/* ---- Linear (+ BatchNorm1d over the rows) (+ ReLU) on R <= 64 rows: the heads of M2-Track (models/m2track.py:43-71) and
 * the hidden rows of MiniPointNet (models/backbone/pointnet.py:118-126), one launch per layer each way (csrc/rowmlp.hip).
 * Forward: Y (R, Cout) = act(bn(X (R, Cin; row stride ldx) . W^T (Cout, Cin) + bias)); gamma == NULL: no BatchNorm;
 * training: batch statistics over the rows (biased variance), running statistics updated with `momentum` (unbiased
 * variance), else the running statistics.  Z (R, Cout) = the pre-BatchNorm output, mean / invstd (Cout) = the constants the
 * normalisation used: kept for the backward (any may be NULL).
 * Backward of one layer: gradient of the layer's OUTPUT = dY (R, C; row stride lddy) or, dY == NULL, dZup (R, Cup) . Wup
 * (Cup, C) (the layer above, computed on the spot); -> dZ (R, C) gradient of the pre-BatchNorm output, dW (C, Cin), db (C),
 * dgamma / dbeta (C).  input_mode != 0: only the product, stored to dX (R, C; row stride lddx): the stack's input gradient. */
int o3d_row_mlp_fwd(const float* X, int ldx, const float* W, const float* bias, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps, int training, int relu, int R, int Cin,
                    int Cout, float* Z, float* Y, float* mean, float* invstd, void* stream);
int o3d_row_mlp_bwd(const float* dY, int lddy, const float* dZup, const float* Wup, int Cup, int input_mode, float* dX, int lddx,
                    const float* Z, const float* gamma, const float* beta, const float* mean, const float* invstd, int training,
                    int relu, const float* X, int ldx, int R, int Cin, int C, float* dZ, float* dW, float* db, float* dgamma,
                    float* dbeta, void* stream);

/* Several independent layers in one launch (njobs <= 4; the heads of M2-Track that read the same feature, models/m2track.py:
 * 60-71): job j is what o3d_row_mlp_fwd / o3d_row_mlp_bwd do with the same arguments (input_mode must be 0).
 * o3d_row_mlp_input_grad: dX (R, C) = sum over the jobs of dZup_j (R, Cup_j) . Wup_j (Cup_j, C), fixed order; R, C, dX, lddx
 * are taken from jobs[0], the other fields are ignored. */
typedef struct {
    const float* X; int ldx; const float* W; const float* bias; const float* gamma; const float* beta;
    float* running_mean; float* running_var; float momentum, eps; int training, relu; int R, Cin, Cout;
    float* Z; float* Y; float* mean; float* invstd;
} o3d_row_fwd_args;
typedef struct {
    const float* dY; int lddy; const float* dZup; const float* Wup; int Cup; int input_mode; float* dX; int lddx;
    const float* Z; const float* gamma; const float* beta; const float* mean; const float* invstd; int training, relu;
    const float* X; int ldx; int R, Cin, C; float* dZ; float* dW; float* db; float* dgamma; float* dbeta;
} o3d_row_bwd_args;
int o3d_row_mlp_fwd_group(const o3d_row_fwd_args* jobs, int njobs, void* stream);
int o3d_row_mlp_bwd_group(const o3d_row_bwd_args* jobs, int njobs, void* stream);
int o3d_row_mlp_input_grad(const o3d_row_bwd_args* jobs, int njobs, void* stream);

/* ---- tracker losses (next row of SURVEY.md section 8f: the loss as one launch) ----------------------
 * MatchingBaseModel.compute_loss (models/base_model.py:122-164) + the BoxCloud term (models/bat.py:57-65)
 * + the weighted total (models/bat.py:131-137, models/p2b.py:69-74) and the gradients of the total.
 * losses[6] = {total, objective, box, seg, vote, bc}.  bc_pred == NULL: no BoxCloud term (P2B).
 * g_* == NULL: losses only.  scratch: 512 floats. */
int o3d_track_loss(const float* cla, const float* seg, const float* vote, const float* box_label,
                   const float* centers, const float* boxes, const float* bc_pred, const float* bc_label, int B,
                   int N, int P, int K, float w_obj, float w_box, float w_seg, float w_vote, float w_bc,
                   float* scratch, float* losses, float* g_cla, float* g_vote, float* g_boxes, float* g_bc, void* stream);

/* M2-Track between its two stages (models/m2track.py:120-137 over datasets/points_utils.py:390-452): aux = the previous box
 * `prev` (B,4 = x, y, z, yaw; NULL: zeros) moved by `motion` (B,4) [get_offset_box_tensor]; the first N/2 points carried along
 * that motion [get_offset_points_tensor], then all N points expressed in the frame of aux [remove_transform_points_tensor].
 * pts: channel c of point n of cloud b at pts[b*bstride + c*cstride + n] (channels 0..2 = xyz).  merged (B,3,N), aux (B,4).
 * _bwd: g_merged (B,3,N), g_aux (B,4) | NULL -> g_prev (B,4) | NULL, g_motion (B,4); no gradient to the points. */
int o3d_motion_merge_fwd(const float* pts, long bstride, long cstride, const float* prev, const float* motion, int B, int N,
                         float* merged, float* aux, void* stream);
int o3d_motion_merge_bwd(const float* pts, long bstride, long cstride, const float* prev, const float* motion, int B, int N,
                         const float* g_merged, const float* g_aux, float* g_prev, float* g_motion, void* stream);

/* Backward of o3d_gmax_fwd without the dense gradient: pk (C, B) float2 = {dOut where out > 0 else 0, bits(column of the
 * maximum relative to its cloud)} -- the pooled operand of o3d_mlp_conv_dgrad_wt / o3d_mlp_conv_wgrad2 with one ball of
 * ns = N columns per cloud -- and the BatchNorm-backward sums part[0][0][c] = sum g, part[0][1][c] = sum g * (yarg - mean). */
int o3d_gmax_bwd_pk(const float* dOut, const float* out, const int32_t* argq, const float* yarg, const float* mean, int B, int C,
                    int N, float* pk, float* part, void* stream);

/* Backward of a thin first layer of a per-point stack (models/backbone/pointnet.py:91-204 with 12-14 input channels) on the
 * flat (C, P) layout, Cout == 64, Cin <= 16, P % 64 == 0: dY = A1*dN + A2*Y + A3 (per-row constants, the BatchNorm backward
 * folded); dW (64, Cin) = dY . X^T; dX (Cin, P) = W^T . dY when dX != NULL.  One pass over dN and Y.
 * scratch: o3d_thin_bwd_scratch() floats. */
long o3d_thin_bwd_scratch(void);
int o3d_thin_bwd(const float* dN, const float* Y, const float* A1, const float* A2, const float* A3, const float* X,
                 const float* W, int Cin, int Cout, long P, float* scratch, float* dW, float* dX, void* stream);

/* get_offset_box_tensor (datasets/points_utils.py:420-436): box = `ref` (B,4) moved by `off` (B,4) given in ref's frame.
 * g_box == NULL: forward, writes box; else backward: g_ref / g_off (either may be NULL) from g_box. */
int o3d_offset_box(const float* ref, const float* off, int B, float* box, const float* g_box, float* g_ref, float* g_off,
                   void* stream);

/* M2-Track's loss (models/m2track.py:153-231) and the gradients of its weighted total: segmentation cross entropy with class
 * weights (cw0, cw1) = (0.5, 2.0), motion-state cross entropy, (centre, angle) smooth-L1 pairs of the refined / previous /
 * first-stage box and of the motion (the latter over the moving samples when `state` is given), BoxCloud smooth-L1 against
 * the concatenation of bc_a and bc_b (B, N/2, K each).  NULL predictions switch their terms off: bc_pred (box_aware), motion_cls +
 * state (use_motion_cls), est (use_second_stage), prev (use_prev_refinement).  losses[12] = {total, motion_cls, center, angle,
 * center_prev, angle_prev, seg, center_aux, center_motion, angle_aux, angle_motion, bc}.  g_seg == NULL: losses only.
 * scratch: 1024 floats. */
int o3d_m2track_loss(const float* seg_logits, const int64_t* seg_label, const float* bc_pred, const float* bc_a, const float* bc_b,
                     const float* motion_cls, const int64_t* state, const float* motion, const float* motion_lab, const float* aux,
                     const float* est, const float* prev, const float* box_lab, const float* prev_lab, int B, int N, int K,
                     float w_center, float w_angle, float w_seg, float w_bc, float w_mcls, float cw0, float cw1, float* scratch,
                     float* losses, float* g_seg, float* g_bc, float* g_mcls, float* g_motion, float* g_aux, float* g_est,
                     float* g_prev, void* stream);

/* ---- BoxCloud (next row of SURVEY.md section 8f-2) -------------------------------------------------
 * get_point_to_box_distance (datasets/points_utils.py:127-143) with Box.corners (datasets/data_classes.py:
 * 226-250): out (B,N,9) = distance of every point to the box centre (channel 0) and to the 8 corners
 * (channels 1..8, the corner order of Box.corners).  wlh = (width, length, height); rot (B,3,3) row-major
 * rotation matrix of the box orientation.  B <= 65535 (one grid row per box), else O3D_EINVAL. */
int o3d_boxcloud(const float* points, const float* center, const float* wlh, const float* rot, float wlh_factor,
                 int B, int N, float* out, void* stream);

/* ---- the tracking front end (csrc/track.hip): crop, resample and box update of a tracked sequence on the device --------
 * A box is 15 floats: centre (3), wlh = width, length, height (3), row-major rotation matrix (9).
 *
 * o3d_track_crop: up to O3D_CROP_MAX_JOBS box crops with order-preserving compaction in two launches.  Job: the n points
 * (n,3) kept by `box` (scale, offset) are written, expressed in the frame of the box and in their original order, to out
 * (capacity,3); count[0] = the number kept (survivors beyond `capacity` are counted, not written).  mode O3D_CROP_SUBWINDOW:
 * generate_subwindow(oriented=True) (datasets/points_utils.py:218-250); O3D_CROP_MODEL: cropAndCenterPC (:103-124).  The
 * fp32 operation order is fixed and written down at the head of csrc/track.hip.  `jobs` is a HOST table; scratch: at least
 * o3d_track_crop_scratch(jobs, n_jobs) int32 on the device (one per workgroup of 256 points; -1: bad table). */
#define O3D_CROP_MAX_JOBS 4
#define O3D_CROP_SUBWINDOW 0
#define O3D_CROP_MODEL 1
typedef struct {
    const float* points; int n; const float* box; float scale, offset; int mode; float* out; int capacity; int32_t* count;
} o3d_crop_job;
long o3d_track_crop_scratch(const o3d_crop_job* jobs, int n_jobs);
int o3d_track_crop(const o3d_crop_job* jobs, int n_jobs, int32_t* scratch, int scratch_len, void* stream);

/* dst (n,3)[i] = src (n_src,3)[idx[i]] for 1 or 2 HOST jobs in one launch (the gather of regularize_pc,
 * datasets/points_utils.py:24-40, straight into the network's input buffers); zero != 0: dst = 0 (its `num_points <= 2`
 * case; src / idx unused).  A row whose index lies outside [0, n_src) is written as zeros. */
typedef struct {
    const float* src; int n_src; const int32_t* idx; float* dst; int n; int zero;
} o3d_resample_job;
int o3d_track_resample(const o3d_resample_job* jobs, int n_jobs, void* stream);

/* getOffsetBB (datasets/points_utils.py:43-85): the box `ref` (15) moved by offset (4) = x, y, z, theta given in ref's frame
 * (a row of o3d_best_proposal's output): centre' = c + R (x, y, use_z ? z : 0), R' = R Rz(theta).  The new box goes to out
 * (15) | NULL and, with results (T,15) and frame (1) int32, to results[frame[0]] (when frame[0] < T); frame[0] += 1.
 * yaw_state (10) | NULL = {R0 (9), yaw}: the orientation is kept as R0 Rz(yaw) and only yaw accumulates (rebase != 0:
 * restart from ref's rotation).  limit_box: :70-76 literally; its random replacement is a counter-based hash of
 * (seed, frame[0], component) in [-1, 1). */
int o3d_track_offset_box(const float* ref, const float* offset, float* yaw_state, int rebase, int degrees, int use_z,
                         int limit_box, int seed, float* out, float* results, int T, int32_t* frame, void* stream);

/* The network input of the motion tracker (M2-Track) in one launch: MotionBaseModel.build_input_dict (models/base_model.py:
 * 263-302) behind its two generate_subwindow crops.  prev (n_prev,3) / cur (n_this,3): the crops of the previous and the
 * current frame (two O3D_CROP_SUBWINDOW jobs by the same box); idx (2N): row i < N of the output gathers prev[idx[i]], row
 * i >= N gathers cur[idx[i]] (an index outside its source leaves a zero row); zero_prev / zero_this != 0: that half is
 * zero-filled (regularize_pc's `num_points <= 2` case) and needs neither its crop nor idx.  wlh (3, on the device): the
 * canonical box = centre 0, identity rotation.  points (2N,5) = xyz, time stamp (0 | 0.1), prior targetness (previous half:
 * points_in_box of the row against the box scaled by 1.25, inclusive, written 1 / 0 when first_frame else 0.8 / 0.2; current
 * half 0.5); candidate_bc (2N,9) | NULL: the previous half's distances to the box centre and its eight corners
 * (get_point_to_box_distance), the current half zeros.  The fp32 operation order is written at the head of csrc/track.hip. */
int o3d_track_motion_input(const float* prev, int n_prev, const float* cur, int n_this, const int32_t* idx, int N,
                           int zero_prev, int zero_this, const float* wlh, int first_frame, float* points,
                           float* candidate_bc, void* stream);

/* ---- the same three steps for K targets of one scene per launch (tracking.MultiTargetTracker) ------------------------------
 * o3d_track_crop_multi: ONE cloud against K boxes.  `groups` is a HOST table of 1 or 2 groups (a frame of the tracker: frame t
 * against the K reference boxes, frame t-1 against the K result boxes); a group's `targets` is a DEVICE table of n_targets
 * (1..O3D_CROP_MULTI_MAX_TARGETS) targets.  Every point is loaded once and tested against all targets of its group
 * (O3D_CROP_MULTI_CHUNK of them staged in LDS at a time); per target, the rows written to out (capacity,3) and count[0] are
 * bit-identical to an o3d_track_crop job with the same box, scale, offset, mode and capacity.  Three launches (count, scan,
 * scatter), no waiting: csrc/track.hip.  scratch: at least o3d_track_crop_multi_scratch(groups, n_groups) int32 on the device
 * (n_targets per workgroup of 256 points; -1: bad table). */
#define O3D_CROP_MULTI_MAX_TARGETS 1024
#define O3D_CROP_MULTI_CHUNK 32
typedef struct { const float* box; float scale, offset; int mode; float* out; int capacity; int32_t* count; } o3d_crop_target;
typedef struct { const float* points; int n; const o3d_crop_target* targets; int n_targets; } o3d_crop_group;
long o3d_track_crop_multi_scratch(const o3d_crop_group* groups, int n_groups);
int o3d_track_crop_multi(const o3d_crop_group* groups, int n_groups, int32_t* scratch, long scratch_len, void* stream);

/* o3d_track_resample for a DEVICE table of n_jobs jobs in one launch (2K per frame: straight into rows of the batched static
 * inputs (K,M,3) and (K,N,3)); per job the semantics of o3d_track_resample (zero-fill job; an index outside the source
 * writes a zero row). */
int o3d_track_resample_multi(const o3d_resample_job* jobs, int n_jobs, void* stream);

/* o3d_track_offset_box for K targets in one launch, one thread per target: ref (K,15), offset (K,4) = o3d_best_proposal's
 * output, yaw_state (K,10) | NULL, rebase (K) int32 | NULL, active (K) int32 | NULL, out (K,15) | NULL, results (T,K,15) | NULL
 * with ONE shared frame counter.  Target k's box is bit-identical to o3d_track_offset_box called with seed + k; an inactive
 * target writes its ref unchanged to out and to its results row and leaves its yaw_state alone. */
int o3d_track_offset_box_multi(const float* ref, const float* offset, float* yaw_state, const int32_t* rebase,
                               const int32_t* active, int K, int degrees, int use_z, int limit_box, int seed, float* out,
                               float* results, int T, int32_t* frame, void* stream);

/* o3d_track_motion_input for K targets of one scene in one launch (tracking.MultiMotionTracker), grid (ceil(2N / 256), K).
 * `jobs` is a DEVICE table of K (1..O3D_CROP_MULTI_MAX_TARGETS) records holding what changes per frame: the target's two
 * crops (prev (n_prev,3), cur (n_this,3)), its 2N indices (rows < N gather from prev, rows >= N from cur) and the zero-fill
 * flags of the two halves.  wlh (K,3): the canonical boxes; points (K,2N,5) and candidate_bc (K,2N,9) | NULL: row k is what
 * o3d_track_motion_input writes for job k with wlh + 3 k, bit for bit (one definition of the row arithmetic serves both).
 * N is 1..2^20.  The host cannot read the table: a half whose crop or whose idx is NULL is zero-filled. */
typedef struct { const float* prev; int n_prev; const float* cur; int n_this; const int32_t* idx; int zero_prev, zero_this; } o3d_motion_job;
int o3d_track_motion_input_multi(const o3d_motion_job* jobs, int K, int N, const float* wlh, int first_frame, float* points,
                                 float* candidate_bc, void* stream);

/* ---- the free-running tracking loop (tracking.SequenceTracker / MotionSequenceTracker with sampling="device"): the crop counts
 * stay on the device and the resampling indices are drawn there, so that a frame is enqueued without a host synchronisation.
 * The draw is the keyed draw of the training batches, sample_index(key, i, n, S) (csrc/train_batch.hip writes it down; n <= 2
 * zero-fills, n == S is the identity, S > n draws with replacement, S < n without); a key travels as an int carrying the bits
 * of the uint32.  Indices therefore differ from regularize_pc's numpy draw by construction.
 *
 * o3d_track_resample_drawn: n_jobs (1 or 2; job 1's arguments are ignored with 1) gathers in one launch.  Per job: src (cap,3),
 * n_dev (1) int32 on the device, n = min(n_dev[0], cap); row i of dst (S,3) is zero when n <= 2, else src[sample_index(key, i,
 * n, S)]; used (S) int32 | NULL receives the index (-1 for a zero row).  cap 1..2^29, S 1..2^20. */
int o3d_track_resample_drawn(const float* src0, const int32_t* n_dev0, int cap0, int key0, float* dst0, int S0, int32_t* used0,
                             const float* src1, const int32_t* n_dev1, int cap1, int key1, float* dst1, int S1, int32_t* used1,
                             int n_jobs, void* stream);

/* o3d_track_bank_update: the template bank's book-keeping as device state.  state = {fixed, total} int32, read from state_in and
 * written to state_out (two different slots).  crop (crop_cap,3) with count (1) int32: the frame's staged model crop, nm =
 * min(count[0], crop_cap); bank (bank_cap,3).  rule = the shape_aggregation; first != 0: the first tracked frame.  slot = 0 for
 * FIRST and PREVIOUS, for FIRSTANDPREVIOUS 0 when first else fixed, for ALL total; rows [slot, slot + nm) of the bank become
 * the crop, FIRSTANDPREVIOUS at first also writes rows [nm, 2 nm) (getModel of the same crop twice); total' = slot + nm (2 nm
 * there), fixed' = first ? nm : fixed.  Rows at or beyond bank_cap are dropped and total' is clipped to bank_cap.  has_crop == 0
 * (FIRST after the first frame): the state is copied through and nothing else is written. */
#define O3D_BANK_FIRST 0
#define O3D_BANK_PREVIOUS 1
#define O3D_BANK_FIRSTANDPREVIOUS 2
#define O3D_BANK_ALL 3
int o3d_track_bank_update(const float* crop, const int32_t* count, int crop_cap, float* bank, int bank_cap, int rule, int first,
                          int has_crop, const int32_t* state_in, int32_t* state_out, void* stream);

/* o3d_track_motion_input with the two counts read from the device and the indices drawn there: prev / cur (capacity,3), counts
 * (2) int32 on the device = (previous, current); per half n = min(count, capacity), zero-filled when n <= 2, else row i gathers
 * sample_index(key of the half, i - half N, n, N).  used (2N) int32 | NULL: the indices (-1 for a zero row).  With the same
 * indices the outputs are bit-identical to o3d_track_motion_input's (one definition of the row arithmetic). */
int o3d_track_motion_input_drawn(const float* prev, const float* cur, const int32_t* counts, int capacity, int key_prev,
                                 int key_this, int N, const float* wlh, int first_frame, float* points, float* candidate_bc,
                                 int32_t* used, void* stream);

/* ---- the free-running loop L lanes wide (tracking.LaneTracker / MotionLaneTracker: the test epoch, one tracklet per lane) -------
 * Every buffer is regular and a lane is its leading axis; L is 1..O3D_CROP_MULTI_MAX_TARGETS.  What changes per step and lane
 * travels in `lanes` (L, O3D_LANE_COLS) int32 on the device, row l = {active, first, has_crop, t, row, ref_row, rebase}: whether
 * the lane tracks at all, whether this is its tracklet's first tracked frame, whether a model crop was made, the frame index
 * (>= 1), the lane's row of the result pool, the row of the ground-truth pool that is its reference box (-1: its own current
 * box) and whether the yaw state restarts from that reference.  Each entry calls the device function of its single form on
 * lane l's operands: lane l's output is that entry's, bit for bit.
 *
 * o3d_track_bank_update_lanes: o3d_track_bank_update per lane.  crop (L,crop_cap,3), lane l's count = counts[l * count_stride],
 * bank (L,bank_cap,3), state_in / state_out (L,2).  An inactive lane, or one without a crop, copies its state through and
 * writes nothing else. */
#define O3D_LANE_ACTIVE 0
#define O3D_LANE_FIRST 1
#define O3D_LANE_HAS_CROP 2
#define O3D_LANE_T 3
#define O3D_LANE_ROW 4
#define O3D_LANE_REF_ROW 5
#define O3D_LANE_REBASE 6
#define O3D_LANE_COLS 7
int o3d_track_bank_update_lanes(const float* crop, const int32_t* counts, int count_stride, int crop_cap, float* bank, int bank_cap,
                                int rule, const int32_t* lanes, int L, const int32_t* state_in, int32_t* state_out, void* stream);

/* o3d_track_resample_drawn for two clouds times L lanes in one launch.  Per cloud: src (L,cap,3), lane l's count =
 * n_dev[l * stride], the key, dst (L,S,3), used (L,S) | NULL.  Row l is what o3d_track_resample_drawn writes for that job. */
int o3d_track_resample_drawn_lanes(const float* src0, const int32_t* n_dev0, int stride0, int cap0, int key0, float* dst0, int S0,
                                   int32_t* used0, const float* src1, const int32_t* n_dev1, int stride1, int cap1, int key1,
                                   float* dst1, int S1, int32_t* used1, int L, void* stream);

/* o3d_track_motion_input_drawn per lane: prev / cur (L,capacity,3), counts (L,2), wlh (L,3), first_frame = the lane's `first`;
 * points (L,2N,5), candidate_bc (L,2N,9) | NULL, used (L,2N) | NULL. */
int o3d_track_motion_input_drawn_lanes(const float* prev, const float* cur, const int32_t* counts, int capacity, int key_prev,
                                       int key_this, int N, const float* wlh, const int32_t* lanes, int L, float* points,
                                       float* candidate_bc, int32_t* used, void* stream);

/* ---- the tabled forms (tracking.py, sampling="table"): the four drawn entries above with a device table of indices where they
 * take a key, so that the free-running loop resamples with the reference's own draw.  table (cap + 1, S) int32, row-major: row n
 * holds the S indices for a cloud of n rows (tracking.draw_table fills it with regularize_pc's numpy draw); that it has cap + 1
 * rows of S entries is the CALLER's guarantee.  With n = min(count, cap), output row i reads
 *     index = (n > 2) ? table[(long)n * S + i] : -1
 * and is zero for -1.  An entry outside [0, n) leaves its row zero, as an index outside the source does in o3d_track_resample;
 * used receives the entry as read (-1 for a zero row).  Everything else -- operands, ranges (cap 1..2^29, S and N 1..2^20),
 * n_jobs, strides, lanes -- is the drawn twin's; a NULL table returns O3D_EINVAL before any launch.  With the same indices the
 * outputs are o3d_track_resample's / o3d_track_motion_input's bit for bit, and row l of a lane form is the single form's.
 * o3d_track_motion_input_tabled[_lanes] reads ONE table (capacity + 1, N) for both halves. */
int o3d_track_resample_tabled(const float* src0, const int32_t* n_dev0, int cap0, const int32_t* table0, float* dst0, int S0,
                              int32_t* used0, const float* src1, const int32_t* n_dev1, int cap1, const int32_t* table1, float* dst1,
                              int S1, int32_t* used1, int n_jobs, void* stream);
int o3d_track_motion_input_tabled(const float* prev, const float* cur, const int32_t* counts, int capacity, const int32_t* table, int N,
                                  const float* wlh, int first_frame, float* points, float* candidate_bc, int32_t* used, void* stream);
int o3d_track_resample_tabled_lanes(const float* src0, const int32_t* n_dev0, int stride0, int cap0, const int32_t* table0, float* dst0,
                                    int S0, int32_t* used0, const float* src1, const int32_t* n_dev1, int stride1, int cap1,
                                    const int32_t* table1, float* dst1, int S1, int32_t* used1, int L, void* stream);
int o3d_track_motion_input_tabled_lanes(const float* prev, const float* cur, const int32_t* counts, int capacity, const int32_t* table,
                                        int N, const float* wlh, const int32_t* lanes, int L, float* points, float* candidate_bc,
                                        int32_t* used, void* stream);

/* o3d_track_offset_box per lane, one thread each.  ref = row ref_row[l] of gt (R,15), or cur[l] of cur (L,15) when ref_row[l] is
 * -1; offset (L,4), yaw_state (L,10).  The new box goes to out[l] (out (L,15) may be cur) and to results[row[l]] of the pool
 * results (R,15); limit_box's draw hashes (seed, t[l], component), so lane l's box is o3d_track_offset_box's with that seed and
 * frame[0] = t[l].  counts_log (R,2) | NULL with counts (L,2): row row[l] receives the lane's two crop counts (-1 for the second
 * without a crop).  An inactive lane writes nothing; neither does one whose ref_row lies outside [-1, R). */
int o3d_track_offset_box_lanes(const float* cur, const float* gt, int R, const float* offset, float* yaw_state, const int32_t* lanes,
                               int L, int degrees, int use_z, int limit_box, int seed, float* out, float* results,
                               const int32_t* counts, int32_t* counts_log, void* stream);

/* A lane's start: every lane that is active and first takes row row[l] - t[l] of gt (R,15) -- its tracklet's first box -- as
 * cur[l], restarts yaw_state[l] = {that rotation, 0}, takes its wlh as the canonical box wlh[l] (L,3) and, with state (L,2) int32
 * | NULL (the template banks' {fixed, total} that the step's o3d_track_bank_update_lanes reads), sets state[l] = {0, 0}: what
 * the single trackers' init() sets, in the same bits. */
int o3d_track_lane_start(const float* gt, int R, const int32_t* lanes, int L, float* cur, float* yaw_state, float* wlh,
                         int32_t* state, void* stream);

/* ---- training batches built on the device (csrc/train_batch.hip): the device form of PointTrackingSampler +
 * siamese_processing (datasets/sampler.py:16-79) for BAT and P2B.  Frames and ground-truth boxes resident in HBM go in, the
 * training dict comes out; no host synchronisation.  The formulas are written at the head of csrc/train_batch.hip.
 *
 * o3d_track_crop_groups: o3d_track_crop_multi for G (1..O3D_CROP_MAX_GROUPS) groups.  A group is one cloud and a DEVICE table
 * of n_targets (1..O3D_CROP_MULTI_MAX_TARGETS) o3d_crop_target records, with the semantics of o3d_track_crop_multi; per
 * (group, target), rows and count[0] are bit-identical to o3d_track_crop_multi on that group alone.  The host knows every n:
 * o3d_track_crop_groups_scratch (host only, no HIP call) fills wg_start / row_start / sbase of the HOST table `groups`,
 * writes grid[0] = the workgroups of the count and scatter launches, grid[1] = those of the scan launch, and returns the
 * scratch length in int32 (-1: bad table).  The caller uploads the planned records; o3d_track_crop_groups takes the planned
 * host table (validated again, before any HIP call) and its device copy `dev_groups`, which the three launches read. */
#define O3D_CROP_MAX_GROUPS 4096
typedef struct {
    const float* points; int n; const o3d_crop_target* targets; int n_targets;
    int wg_start;             /* planned: the group's first workgroup in the count / scatter grids */
    int row_start;            /* planned: its first (group, target) row = its first workgroup in the scan grid */
    long sbase;               /* planned: its first word in scratch (n_targets rows of ceil(n / 256) int32 follow) */
} o3d_crop_plan;
long o3d_track_crop_groups_scratch(o3d_crop_plan* groups, int n_groups, int* grid);
int o3d_track_crop_groups(const o3d_crop_plan* groups, const o3d_crop_plan* dev_groups, int n_groups, int32_t* scratch,
                          long scratch_len, void* stream);

/* Which candidates fill the batch (one workgroup).  counts (J,3) int32 = the counts of the first-frame, template-frame and
 * search crops of candidate j, before any truncation; 1 <= B <= J <= O3D_TRAIN_MAX_CANDIDATES.  Candidate j is valid iff
 * counts[j][0] + counts[j][1] > 20 and counts[j][2] > 20 (datasets/sampler.py:46,59).  sel (B): sel[r] = the (r mod n_valid)-th
 * valid candidate, -1 when none is valid; n_valid (1); overflow (1) = the number of crops, over the B chosen rows, whose count
 * exceeds its capacity cap[c]. */
#define O3D_TRAIN_MAX_CANDIDATES 1024
int o3d_train_select(const int32_t* counts, int J, int B, int cap_first, int cap_template, int cap_search, int32_t* sel,
                     int32_t* n_valid, int32_t* overflow, void* stream);

/* Per candidate, one thread each, double precision inside and rounded once: gt_search, sample_bb, template_bb (J,15) and
 * offset (J,4) = the search jitter (x, y, 0, theta) -> search_box (J,15) = transform_box(gt_search, sample_bb)
 * (datasets/points_utils.py:253-258: centre R_sb^T (c - c_sb), rotation R_sb^T R), box_label (J,4) = (its centre,
 * -theta), bbox_size (J,3) = its wlh, model_box (J,15) = centre 0, the wlh of template_bb, identity. */
int o3d_train_labels(const float* gt_search, const float* sample_bb, const float* template_bb, const float* offset, int J,
                     float* search_box, float* box_label, float* bbox_size, float* model_box, void* stream);

/* Sample and gather, grid (rows, B, 2).  Output row r takes candidate j = sel[r].  Template cloud: the virtual concatenation
 * of crop_first[j] (min(counts[j][0], cap_first) rows) and crop_template[j] (min(counts[j][1], cap_template) rows), resampled
 * to M rows; search cloud: crop_search[j] (min(counts[j][2], cap_search) rows) resampled to N rows (regularize_pc,
 * datasets/points_utils.py:24-40).  The crops are pools (J,cap,3).  idx_t (J,M) / idx_s (J,N) int32 | NULL: the indices of
 * candidate j (both or neither); NULL: the device draw keyed by (seed, counter, j, cloud, row), integers only
 * (csrc/train_batch.hip).  A cloud of n <= 2 rows, sel[r] < 0 or an index outside [0, n) gives a zero row with seg_label 0.
 * seg_label (B,N) = crop_test of the row against search_box[j] (scale 1, offset 0: get_in_box_mask).  Row r of box_label (B,4),
 * bbox_size (B,3) and of the BoxCloud boxes bc_boxes [2][centre (B,3) | wlh (B,3) | rotation (B,9)] ([0] = model_box, [1] =
 * search_box; | NULL) is candidate j's (zeros when sel[r] < 0).  used_t (B,M) / used_s (B,N) int32 | NULL: the indices used
 * (-1: zero row). */
typedef struct {
    const int32_t* sel; const int32_t* counts;
    const float* crop_first; const float* crop_template; const float* crop_search;
    int cap_first, cap_template, cap_search, J, B, M, N;
    const int32_t* idx_t; const int32_t* idx_s;
    unsigned seed, counter;
    const float* search_box; const float* model_box; const float* cand_box_label; const float* cand_bbox_size;
    float* template_points; float* search_points; float* seg_label; float* box_label; float* bbox_size; float* bc_boxes;
    int32_t* used_t; int32_t* used_s;
} o3d_train_sample_args;
int o3d_train_sample(const o3d_train_sample_args* args, void* stream);

/* ---- M2-Track training batches (csrc/train_batch.hip): the device form of MotionTrackingSampler + motion_processing
 * (datasets/sampler.py:82-180,262-288) with apply_augmentation (datasets/points_utils.py:299-361).  Boxes are assumed
 * yaw-only (rotations about z), as every box of the reference's datasets is: the angle of a box is atan2(R[1][0], R[0][0]).
 *
 * An augmentation record: a point p with inside_box(p, box, 1.25) -- the inclusive test of points_in_box: d = p - c, q = R^T d,
 * |qx| <= (l*1.25)*0.5 and |qy| <= (w*1.25)*0.5 and |qz| <= (h*1.25)*0.5 -- is replaced by A d + c; every other point, and
 * every point when enabled == 0, is unchanged. */
typedef struct { int enabled; float box[15]; float A[9]; float c[3]; } o3d_crop_aug;

/* apply_transform for the boxes, one thread per record slot.  gt (K,15), draw (K,6) = (tx, ty, tz, rot in degrees, flip_x,
 * flip_y; a flip is set when its value is not 0).  Box k, double inside and rounded once:  c' = c + R t,  R' = R Rz(rot)
 * (flip_x ? Rz(180 deg) : I),  wlh unchanged  -> out_box (K,15).  Its record: enabled = 1, box = gt[k],
 * A = R Rz(rot) diag(flip_x ? -1 : 1, flip_y ? -1 : 1, 1) R^T,  c = c'.  slot_src (n_slots) int32 | NULL: slot i of `aug`
 * takes record slot_src[i], or a disabled record (all zero) when slot_src[i] < 0, so that the records land in the order of
 * the crop's target tables; NULL: n_slots == K and slot i takes record i.  out_box[k] is written by the slot that takes
 * record k.  1 <= K, n_slots <= 3 * O3D_TRAIN_MAX_CANDIDATES. */
int o3d_train_augment(const float* gt, const float* draw, const int32_t* slot_src, int K, int n_slots, float* out_box,
                      o3d_crop_aug* aug, void* stream);

/* o3d_track_crop_groups with an optional augmentation record per target.  dev_aug: a DEVICE array of n_groups pointers |
 * NULL (= every entry NULL); entry g points at the n_targets records of group g, or is NULL.  The point is loaded once; a
 * target whose record is enabled tests and writes the replaced point.  Same three launches, same planner
 * (o3d_track_crop_groups_scratch), same validation before any HIP call.  With every record NULL or disabled, rows and counts
 * are bit-identical to o3d_track_crop_groups. */
int o3d_track_crop_groups_aug(const o3d_crop_plan* groups, const o3d_crop_plan* dev_groups, const o3d_crop_aug* const* dev_aug,
                              int n_groups, int32_t* scratch, long scratch_len, void* stream);

/* inside_box for n points against ONE box: mask (n) int32 = 1 | 0.  The device function the augmentation mask and the motion
 * seg_label use, as an entry of its own (points_utils.points_in_box; tests). */
int o3d_train_inside_box(const float* points, int n, const float* box, float factor, int32_t* mask, void* stream);

/* The per-candidate labels of motion_processing (datasets/sampler.py:122-158), one thread per candidate, double inside and
 * rounded once.  prev_gt, this_gt (J,15): the two frames' boxes (augmented or not); ref_box (J,15) = getOffsetBB(prev_gt).
 * this_box (J,15) = transform_box(this_gt, ref_box), prev_box (J,15) = transform_box(prev_gt, ref_box), canon_box (J,15) =
 * centre 0, the wlh of prev_gt, identity; with motion_box = transform_box(this_box, prev_box): box_label (J,4) = (centre of
 * this_box, theta), box_label_prev, motion_label likewise; theta = atan2(R[1][0], R[0][0]), times 180/pi when `degrees` (the
 * reference's orientation.radians * orientation.axis[-1] for a yaw-only box away from +-pi); motion_state (J) int32 =
 * |c_this - c_prev| > motion_threshold; bbox_size (J,3) = the wlh of this_gt. */
int o3d_train_motion_labels(const float* prev_gt, const float* this_gt, const float* ref_box, int J, int degrees,
                            float motion_threshold, float* this_box, float* prev_box, float* canon_box, float* box_label,
                            float* box_label_prev, float* motion_label, int32_t* motion_state, float* bbox_size, void* stream);

/* o3d_train_select for motion batches.  counts (J,3) = (points of the un-augmented previous frame inside the un-augmented
 * previous box, previous crop, current crop), before truncation; candidate j is valid iff counts[j][0] > 10 and counts[j][2] >
 * 20 (datasets/sampler.py:99,120); overflow = the truncated previous and current crops among the chosen rows.
 * DEVIATION: the in-box count comes from the crop (a count-only target: scale 1, offset 0), whose test is strict where
 * points_in_box is inclusive; the two differ only for a point exactly on a face. */
int o3d_train_select_motion(const int32_t* counts, int J, int B, int cap_prev, int cap_this, int32_t* sel, int32_t* n_valid,
                            int32_t* overflow, void* stream);

/* Sample, gather and label, grid (ceil(2N / 256), B).  Output row r takes candidate j = sel[r].  Rows i < N gather from
 * crop_prev[j] (min(counts[j][1], cap_prev) rows), rows i >= N from crop_this[j] (min(counts[j][2], cap_this) rows); idx_prev /
 * idx_this (J,N) int32 | NULL (both or neither): the indices, NULL: o3d_train_sample's draw keyed by (seed, counter, j, cloud,
 * row), cloud 0 = previous, 1 = current.  A half of n <= 2 rows, or an index outside [0, n), gives a zero xyz.  points (B,2N,5)
 * and candidate_bc (B,2N,9) | NULL are o3d_track_motion_input's row for the gathered xyz, the wlh of canon_box[j] and
 * first_frame = (candidate_id[j] == 0); seg_label (B,2N) int64 = inside_box(xyz, prev_box[j], 1.25) on the previous half,
 * inside_box(xyz, this_box[j], 1.25) on the current half.  Row r of box_label, box_label_prev, motion_label (B,4),
 * motion_state_label (B) int64, bbox_size (B,3) is candidate j's.  With bc_boxes ([2][centre (B,3) | wlh (B,3) | rotation
 * (B,9)], [0] = prev_box, [1] = this_box; | NULL), xyz_halves (2,B,N,3) receives the xyz of the two halves, the operands of
 * the two o3d_boxcloud calls that follow.  sel[r] < 0: every output of row r is zero.  used_prev / used_this (B,N) int32 |
 * NULL: the indices used (-1: zero xyz). */
typedef struct {
    const int32_t* sel; const int32_t* counts;
    const float* crop_prev; const float* crop_this;
    int cap_prev, cap_this, J, B, N;
    const int32_t* idx_prev; const int32_t* idx_this; const int32_t* candidate_id;
    unsigned seed, counter;
    const float* prev_box; const float* this_box; const float* canon_box;
    const float* cand_box_label; const float* cand_box_label_prev; const float* cand_motion_label;
    const int32_t* cand_motion_state; const float* cand_bbox_size;
    float* points; float* candidate_bc; int64_t* seg_label;
    float* box_label; float* box_label_prev; float* motion_label; int64_t* motion_state_label; float* bbox_size;
    float* bc_boxes; float* xyz_halves;
    int32_t* used_prev; int32_t* used_this;
} o3d_train_motion_sample_args;
int o3d_train_motion_sample(const o3d_train_motion_sample_args* args, void* stream);

/* ---- the planned training epoch (csrc/train_batch.hip; sampler.py's build_planned is the caller): what the host wrote into
 * the per-batch upload -- the candidates' ground-truth boxes and their random draws -- made on the device instead.  One
 * launch per batch, one thread per candidate, no LDS, no atomics.  gt (R,15): the box pool of all tracklets, resident.
 * rows: the pool rows of candidate j's frames, (J,3) int32 = first / template / search (O3D_TRAIN_DRAW_SIAMESE) or (J,2) =
 * previous / current (the motion modes); cand (J) int32: the candidate ids.  A row outside [0, R) is never read and gives a
 * zero box.  seed, counter: the uint32 of the index draw, carried in the bits of an int.
 *   O3D_TRAIN_DRAW_SIAMESE     refs (2J,15) = [template boxes | search boxes], first (J,15), offs (2J,4) = [template jitter |
 *                              search offset] as (x, y, 0, theta); aug is not used
 *   O3D_TRAIN_DRAW_MOTION      refs (2J,15) = [previous | current], offs (J,4) the jitter; first and aug are not used
 *   O3D_TRAIN_DRAW_MOTION_AUG  and aug (2J,6) = [previous | current] rows of (tx, ty, tz, rotation in degrees, flip_x, flip_y)
 * The draw is keyed by (seed, counter, j, tag, component) and written down at the head of csrc/train_batch.hip
 * (tests/epoch_plan_oracle.py restates it): uniform +-0.3 jitter with the angle x5 (`degrees`) or x deg2rad(5), standard
 * normal x sqrt((1, 1, 5 | deg2rad(5))) for the search offset, translation +-0.3 / rotation +-10 degrees / two fair bits for
 * the augmentation.  Candidate id 0: a zero jitter; a zero search offset when num_candidates > 1.
 * O3D_EINVAL, before any HIP call: a NULL operand that the mode uses, J outside 1..O3D_TRAIN_MAX_CANDIDATES, R < 1,
 * num_candidates < 1, an unknown mode. */
#define O3D_TRAIN_DRAW_SIAMESE 0
#define O3D_TRAIN_DRAW_MOTION 1
#define O3D_TRAIN_DRAW_MOTION_AUG 2
int o3d_train_draw(const float* gt, int R, const int32_t* rows, const int32_t* cand, int J, int seed, int counter, int degrees,
                   int num_candidates, int mode, float* refs, float* first, float* offs, float* aug, void* stream);

/* estimateOverlap / estimateAccuracy (utils/metrics.py:27-72) for n box pairs in one launch: a (n,15) the annotation boxes,
 * b (n,15) the result boxes, e.g. the flattened (T,K) rows of a tracker's results buffer.  valid (n) int32 | NULL: a row with
 * valid == 0 is skipped entirely (its outputs are not written, nothing is counted).  dim = 2 (BEV) | 3; up = 1 | 2, the index
 * of the non-zero component of up_axis ((0,-1,0) and (0,0,1), the two the reference supports).  overlaps, distances (n) | NULL.
 * The arithmetic runs in double in the order stated at the head of csrc/metrics.hip and is rounded once to fp32: the
 * footprint is the projection of four box corners under the FULL rotation matrix, the intersection a Sutherland-Hodgman clip,
 * the dim-3 height rule the reference's own (from the centre down by h); the dim-2 distance is |difference of the up
 * component|, as the reference's mask selects.
 * DEGENERATE INPUT: a non-finite box or a union that is not > 0 gives overlap 0 (the reference raises or returns NaN).
 * Counters (each | NULL): cnt_s (ns) int64 += #{overlap >= thr_s[i]}, cnt_p (np) int64 += #{distance <= thr_p[i]}, total (1)
 * int64 += #valid rows; the fp32-rounded results are compared with the fp32 thresholds thr_s (ns), thr_p (np), 1..64 each.
 * Integer atomics: the counts do not depend on the order of execution.
 * O3D_EINVAL (before any HIP call): a or b NULL, n < 0, dim not 2 | 3, up not 1 | 2, a counter without its thresholds, more
 * than 64 thresholds.  n == 0: returns 0 without a launch. */
int o3d_track_score(const float* a, const float* b, const int32_t* valid, int n, int dim, int up, float* overlaps,
                    float* distances, const float* thr_s, int ns, const float* thr_p, int np, int64_t* cnt_s, int64_t* cnt_p,
                    int64_t* total, void* stream);

/* ---- the lifecycle of a scene tracker's K slots as device work (tracking.ManagedSceneTracker / ManagedMotionSceneTracker;
 * DESIGN.md section 12j): per frame, associate a set of detections with the K tracks, retire the lost tracks, enroll the
 * unmatched detections into free slots.  D is 0..O3D_SCENE_MAX_DETECTIONS, K 1..O3D_CROP_MULTI_MAX_TARGETS.
 *
 * o3d_scene_pair_scores (csrc/metrics.hip): tracks (K,15), active (K) int32, dets (D,15), n_det (1) int32 on the device, clamped
 * to [0, D] -> overlaps, distances (K,D) float32.  For an active k and d < n_det the pair (a = tracks[k], b = dets[d]) is
 * scored by the device function o3d_track_score calls, so the two numbers carry o3d_track_score's bits for that pair; rows of
 * inactive slots and columns d >= n_det are written overlap -1, distance +inf.  One thread per pair.  D == 0: no launch.
 *
 * o3d_scene_manage (csrc/scene.hip), ONE launch of one workgroup, after frame t's o3d_track_offset_box_multi; t = frame[0] - 1
 * is read on the device.  State: cur (K,15), yaw_state (K,10), canon_wlh (K,3), results (T,K,15), active (K) int32, slot
 * (K, O3D_SCENE_SLOT_COLS) int32 = {id, misses, starved, start} with id -1 for a free slot (active == (id >= 0)), next_id (1)
 * int32.  counts: the frame's crop counts, slot k's at counts[2 k + count_col] (count_col 0 | 1).  In this order:
 *   admissible   active[k] && d < n_det && overlaps[k,d] >= min_iou && distances[k,d] <= max_dist, as fp32 compares (a NaN is
 *                never admissible)
 *   match        the admissible pairs ordered by (overlap descending, distance ascending, k ascending, d ascending) are walked
 *                and a pair is taken when its track and its detection are both still unmatched -> match[k], det_match[d], an
 *                index or -1: a pure function of the inputs (LDS keeps every free track's first free pair of its row and every
 *                free detection's first free pair of its column; per round every pair that is both is taken, and only the rows
 *                and columns whose kept partner was taken are scanned again; no atomics)
 *   counters     of every slot active on entry: with has_dets != 0 a matched slot's misses = 0, an unmatched slot's += 1; with
 *                min_points > 0, starved = (count < min_points) ? starved + 1 : 0 (on every frame, whatever has_dets)
 *   retire       misses > max_misses || (min_points > 0 && starved > max_starved): active = 0, id = -1; the box stays
 *   enroll       (enroll != 0) the unmatched detections d < n_det whose 15 numbers are finite, in ascending d, take the free
 *                slots (those retired just now included) in ascending k: cur[k] = dets[d], yaw_state[k] = {R, 0}, canon_wlh[k]
 *                = wlh, results[t][k] = dets[d] (0 <= t < T), bank_state_next[k] = {0, 0} (NULL: the motion tracker has no
 *                bank), active[k] = 1, slot[k] = {next_id++, 0, 0, t}; those left over are counted: dropped
 *   lanes        (K, O3D_LANE_COLS), the NEXT frame's lane table: row k = {1, first, has_crop, 0, -1, -1, 0} with first = slot k
 *                was enrolled in this call and has_crop = first || rule != O3D_BANK_FIRST (rule -1, the motion tracker: 1)
 *   logs         row t (0 <= t < T) of ids_log (T,K) = the new id of a slot enrolled in this call, else its id on entry;
 *                match_log (T,K) = match; dropped_log (T) = dropped
 * All stores are ordinary vector stores.  has_dets == 0 (the caller passed no detection set for this frame): n_det counts as 0
 * and the misses stay as they are; the call is still made on every frame, because it is what clears `first`.
 * Both entries return O3D_EINVAL before any HIP call for a NULL operand (bank_state_next excepted; overlaps, distances, dets
 * and n_det may be NULL when D == 0), K or D outside the ranges above, dim not 2 | 3, up not 1 | 2, T < 1, count_col not 0 | 1,
 * rule outside -1..3. */
#define O3D_SCENE_MAX_DETECTIONS 1024
#define O3D_SCENE_SLOT_COLS 4
int o3d_scene_pair_scores(const float* tracks, const int32_t* active, int K, const float* dets, const int32_t* n_det, int D,
                          int dim, int up, float* overlaps, float* distances, void* stream);
int o3d_scene_manage(const float* overlaps, const float* distances, const float* dets, const int32_t* n_det, int K, int D,
                     float* cur, float* yaw_state, float* canon_wlh, float* results, int T, const int32_t* frame,
                     int32_t* active, int32_t* slot, int32_t* next_id, const int32_t* counts, int count_col,
                     int32_t* bank_state_next, int32_t* lanes, int rule, int32_t* ids_log, int32_t* match_log,
                     int32_t* dropped_log, float min_iou, float max_dist, int max_misses, int min_points, int max_starved,
                     int enroll, int has_dets, void* stream);

/* ---- scoring a managed scene on the device: the CLEAR-MOT bookkeeping (metrics.ClearMOT) -------------
 * Ground truth gt (F,G,15) with gt_valid (F,G) int32 (0: object g has no annotation in frame f) against the tracked run's
 * hyp (F,K,15) boxes and hyp_ids (F,K) int32 (the track id slot k carried in frame f, < 0: none), all on the device.  G and K
 * are 1..O3D_CROP_MULTI_MAX_TARGETS.
 *
 * o3d_scene_pair_scores_frames (csrc/metrics.hip) -> overlaps, distances (F,G,K) float32.  Pair (f,g,k) with gt_valid[f,g] != 0
 * && hyp_ids[f,k] >= 0 is scored by the device function of o3d_track_score and o3d_scene_pair_scores (a = gt[f,g], b =
 * hyp[f,k]) and carries their bits for that pair; every other pair is written overlap -1, distance +inf.  One thread per pair
 * on a 64-bit index.  F >= 0; F == 0 returns 0 without a launch.
 *
 * o3d_scene_mot_walk (csrc/scene.hip): ONE launch of one workgroup of 1024 threads walks frames 0..F-1 in order (the loop over
 * the frames is inside the kernel), F in 0..O3D_SCENE_MOT_MAX_FRAMES; F == 0 returns 0 without a launch.  State carried in
 * device memory, read on entry and written on exit, so that a sequence may be walked in several calls: last_id (G) int32, the id
 * g was last matched to (-1: none); tracked_prev (G) int32, whether g was matched at its most recent valid frame; ever (G)
 * int32, whether g was ever matched.  Per frame f, in this order (ov, di = overlaps[f], distances[f]):
 *   admissible   gt_valid[f,g] != 0 && hyp_ids[f,k] >= 0 && ov[g,k] >= min_iou && di[g,k] <= max_dist, as fp32 compares (a NaN
 *                is never admissible)
 *   carry        for g ascending, g valid and last_id[g] >= 0: k = the column with hyp_ids[f,k] == last_id[g].  PRECONDITION:
 *                the non-negative ids of a frame are distinct; where they are not, the lowest such k counts.  When k exists,
 *                (g,k) is admissible and no smaller g took column k: match[g] = k.  A kept identity wins over a better-scoring
 *                new pairing; of two objects that remember the same id the lower g gets it.
 *   rest         the walk of o3d_scene_manage, by the same device function, over the admissible pairs whose two ends are both
 *                still free: ordered by (overlap descending, distance ascending, g ascending, k ascending), a pair is taken
 *                when its object and its column are both still unmatched
 *   count        per valid g, matched: tp += 1; idsw += 1 when last_id[g] >= 0 && last_id[g] != hyp_ids[f,match[g]]; frag += 1
 *                when ever[g] && !tracked_prev[g]; then last_id[g] = that id, ever[g] = 1, tracked_prev[g] = 1.  Unmatched:
 *                fn += 1, tracked_prev[g] = 0.  An invalid g leaves its state untouched.  fp = the columns with an id >= 0 left
 *                unmatched.
 *   rows         match_slot (F,G) int32 = k | -1; match_id (F,G) int32 = hyp_ids[f,k] | -1; match_ov, match_di (F,G) float32 =
 *                ov[g,k], di[g,k] copied (-1 / +inf when g is invalid or unmatched); per_frame (F,8) int32 = {gt, hyp, tp, fp,
 *                fn, idsw, frag, 0} with gt = the valid objects and hyp = the columns with an id
 * The leftover assignment of this entry is the library's greedy rule (o3d_scene_mot_walk_assign below takes the optimal one),
 * and the identity memory is the last known match, kept through gaps.  No atomics and no flag that a thread waits on: barriers and the stream order are the only
 * dependences, and all stores are ordinary vector stores, so the result is a function of the inputs.
 * Both entries return O3D_EINVAL before any HIP call for a NULL operand, F, G or K outside the ranges above, dim not 2 | 3, up
 * not 1 | 2, and (o3d_scene_pair_scores_frames) more than 2^31 - 1 workgroups of 256 pairs. */
#define O3D_SCENE_MOT_MAX_FRAMES 4096
int o3d_scene_pair_scores_frames(const float* gt, const int32_t* gt_valid, const float* hyp, const int32_t* hyp_ids, int F, int G,
                                 int K, int dim, int up, float* overlaps, float* distances, void* stream);
int o3d_scene_mot_walk(const float* overlaps, const float* distances, const int32_t* gt_valid, const int32_t* hyp_ids, int F, int G,
                       int K, float min_iou, float max_dist, int32_t* last_id, int32_t* tracked_prev, int32_t* ever,
                       int32_t* match_slot, int32_t* match_id, float* match_ov, float* match_di, int32_t* per_frame, void* stream);

/* ---- optimal assignment for the scene trackers and CLEAR-MOT (csrc/scene.hip) ------------------------
 * `assignment` selects who belongs to whom on the admissible pairs of an (rows, cols) overlap / distance matrix pair:
 *   O3D_ASSIGN_GREEDY    the walk of o3d_scene_manage above (overlap descending, distance ascending, row, column ascending)
 *   O3D_ASSIGN_OPTIMAL   of the one-to-one sets of admissible pairs on the free rows and columns: the MOST pairs, and among
 *                        those the smallest sum of the integer cost q (maximum-cardinality, minimum-cost; the Hungarian optimum)
 * `cost` is q of an admissible pair, int32 in [0, 2^20], each product one rounded fp32 multiply:
 *   O3D_COST_DISTANCE    (int) rintf(fminf(fmaxf(distance, 0), 1024) * 1024)           unit 1/1024 m; >= 1024 m ties at 2^20
 *   O3D_COST_OVERLAP     (int) rintf((1 - fminf(fmaxf(overlap, 0), 1)) * 1048576)
 * admissible(r,c) is the entry's own test (fp32 compares, a NaN is never admissible).  The optimum is the minimum-sum assignment
 * of the matrix with q on the admissible pairs, one private "stay unmatched" column per row at 2^32 and the inadmissible pairs
 * excluded, in int64: nothing is rounded and at 1024 rows nothing overflows.  WHICH optimum of several: the free rows in play
 * are inserted in ascending order, each by one shortest augmenting path on the reduced costs; the next column of a path is the
 * unused one of smallest tentative length, of equal lengths the lowest column index, real columns before the rows' private
 * ones; a tentative length is replaced only by a strictly smaller one (csrc/scene.hip states the order in full,
 * tests/assign_oracle.py restates it).  One workgroup, no atomics, every loop bounded by the sizes: a pure function of the
 * inputs.  `cost` is ignored by the greedy walk itself.
 *
 * o3d_scene_assign: ONE launch of one workgroup, the match alone.  overlaps, distances (K,D) float32; row_active (K) int32 |
 * NULL: every row is in play; n_col (1) int32 on the device, clamped to [0, D] | NULL: D; K 1..O3D_CROP_MULTI_MAX_TARGETS, D
 * 1..O3D_SCENE_MAX_DETECTIONS.  admissible(r,c) = row r in play && c < n_col && overlaps[r,c] >= min_iou && distances[r,c] <=
 * max_dist.  -> match (K) int32 = c | -1, col_match (D) int32 = r | -1, summary (2) int64 = {pairs, the sum of q over the pairs}
 * (with O3D_ASSIGN_GREEDY too: the greedy pairs summed under `cost`).
 * o3d_scene_manage_assign / o3d_scene_mot_walk_assign: o3d_scene_manage / o3d_scene_mot_walk with the match (the walk's `rest`
 * step; its carry is unchanged) made by `assignment` under `cost`; everything else, and with O3D_ASSIGN_GREEDY every bit, is
 * theirs -- the two older entries forward here.
 * All three return O3D_EINVAL before any HIP call for an unknown assignment or cost, and for what their namesakes refuse
 * (o3d_scene_assign: overlaps, distances, match, col_match or summary NULL, K or D outside the ranges above). */
#define O3D_ASSIGN_GREEDY 0
#define O3D_ASSIGN_OPTIMAL 1
#define O3D_COST_DISTANCE 0
#define O3D_COST_OVERLAP 1
int o3d_scene_assign(const float* overlaps, const float* distances, const int32_t* row_active, const int32_t* n_col, int K, int D,
                     float min_iou, float max_dist, int assignment, int cost, int32_t* match, int32_t* col_match,
                     int64_t* summary, void* stream);
int o3d_scene_manage_assign(const float* overlaps, const float* distances, const float* dets, const int32_t* n_det, int K, int D,
                            float* cur, float* yaw_state, float* canon_wlh, float* results, int T, const int32_t* frame,
                            int32_t* active, int32_t* slot, int32_t* next_id, const int32_t* counts, int count_col,
                            int32_t* bank_state_next, int32_t* lanes, int rule, int32_t* ids_log, int32_t* match_log,
                            int32_t* dropped_log, float min_iou, float max_dist, int max_misses, int min_points, int max_starved,
                            int enroll, int has_dets, int assignment, int cost, void* stream);
int o3d_scene_mot_walk_assign(const float* overlaps, const float* distances, const int32_t* gt_valid, const int32_t* hyp_ids, int F,
                              int G, int K, float min_iou, float max_dist, int32_t* last_id, int32_t* tracked_prev, int32_t* ever,
                              int32_t* match_slot, int32_t* match_id, float* match_ov, float* match_di, int32_t* per_frame,
                              int assignment, int cost, void* stream);

/* ---- the preload crop of a dataset reader (csrc/preload.hip; open3dsot_amd/datasets.py is the caller) ----------------------
 * What kittiDataset._get_frame_from_anno does per annotated object per frame -- PointCloud.transform in camera mode, then
 * crop_pc_axis_aligned(pc, box, offset=preload_offset) -- for a chunk of raw frames in HBM: three launches and one read-back.
 * raw (raw_rows,4) float32 on the device, 16-byte aligned: x y z intensity as in the .bin files (the intensity is ignored).
 * frames (F,6) int32: first raw row, n, first box, number of boxes, workgroup start, scratch base.  The boxes of record f are
 * [first box, first box + number): the records partition [0, B) in order; two records may name the same raw rows.  `frames` is
 * the planned HOST table (checked again in every call, its plan included), frames_dev its copy on the device, which the
 * launches read.  bounds (B,6) float32 on the device: lo x y z, hi x y z, the fp64 bounds of the reference rounded
 * directionally (lo down, hi up), which makes the fp32 compares lo < p < hi exactly the reference's float32-against-double
 * compares; -inf / +inf keep every finite point.  transform: 12 doubles on the HOST, the upper 3x4 of velo_to_cam row-major,
 * passed by value | NULL (velodyne mode): p' = float(((T_i0*x + T_i1*y) + T_i2*z) + T_i3) is tested and written.
 * o3d_preload_scratch (host only, no HIP call): the caller sets columns 0, 1 and 3 of `frames`; columns 2, 4 and 5 are filled
 * in place; grid[0] = the workgroups of the count / scatter launches, grid[1] = B (grid may be NULL).  -> the scratch length in
 * int32, -1 for a bad table.
 * o3d_preload_count: the count and the scan launch -> counts (B) int32 on the device, the survivors of every box.
 * o3d_preload_scatter must follow o3d_preload_count on the same scratch with the same tables: survivor number pos of box b, in
 * the order of the frame, goes to pool (pool_rows,3) row out_row[b] + pos (out_row (B) int64 on the device); a row < 0 or >=
 * pool_rows is not written.
 * O3D_EINVAL, before any HIP call: F outside 0..O3D_PRELOAD_MAX_FRAMES, raw_rows outside 0..O3D_PRELOAD_MAX_ROWS, a record with
 * a negative field, rows past raw_rows, more than O3D_PRELOAD_MAX_BOXES boxes or a plan other than o3d_preload_scratch's, boxes
 * that do not sum to B, a scratch beyond 2^31 - 1 words or shorter than planned, a NULL or misaligned operand that a launch
 * would read or write.  F = 0, B = 0, a frame of n = 0 and a record without boxes succeed; the first two launch nothing.
 *
 * o3d_preload_posed_count / o3d_preload_posed_scatter: the same launches with one transform PER FRAME RECORD -- what
 * WaymoDataset._get_frame_from_anno does, whose frames carry a vehicle-to-global pose each.  poses (F,12) float64 on the
 * DEVICE, 8-byte aligned: row f is the upper 3x4 of record f's transform, row-major; two records over the same raw rows carry
 * the same pose twice.  The rule is the one above, p' = float(((T_i0*x + T_i1*y) + T_i2*z) + T_i3) with T = poses[f], fp64 on
 * the float32 input and rounded once.  row_floats = 3 | 4: raw row r is floats [r*row_floats, r*row_floats + 3) of raw, which
 * is 4-byte aligned, 16-byte when row_floats is 4.  Tables, planning (o3d_preload_scratch), compares, counting and limits are
 * the pair's above.  O3D_EINVAL, before any HIP call: everything that pair refuses, row_floats outside {3,4}, poses NULL with
 * F > 0, poses not 8-byte aligned.  F = 0 and B = 0 succeed without a launch.
 *
 * o3d_preload_steps_count / o3d_preload_steps_scatter: the same launches with a CHAIN OF ROUNDED RIGID STEPS per frame record
 * -- what NuScenesDataset._get_frame_from_anno_data does, whose sweeps go sensor -> ego -> global by rotate / translate pairs on
 * a float32 array.  steps (F,n_steps,12) float64 on the DEVICE, 8-byte aligned: step s of record f is a row-major 3x4 [R | t];
 * n_steps in 1..O3D_PRELOAD_MAX_STEPS; two records over the same raw rows carry the same steps twice.  A step, on the float32
 * input (x, y, z): r_i = float((M_i0*x + M_i1*y) + M_i2*z), fp64 in this order, rounded; then translate32 = 0: p_i =
 * float(double(r_i) + M_i3) (numpy >= 2 adds an np.float64 scalar to a float32 array in fp64 and rounds on assignment), or
 * translate32 = 1: p_i = r_i + float(M_i3), an fp32 add (numpy < 2 demotes the scalar).  p is the next step's input; the last p
 * is tested and written: two steps round a point four times.  row_floats = 3 | 4 | 5: raw row r is floats [r*row_floats,
 * r*row_floats + 3) of raw -- the .pcd.bin rows x y z intensity ring of 20 bytes are uploaded as they lie -- which is 4-byte
 * aligned, 16-byte when row_floats is 4.  Tables, planning, compares, counting and limits are the first pair's.  O3D_EINVAL,
 * before any HIP call: everything that pair refuses, row_floats outside 3..5, n_steps outside 1..O3D_PRELOAD_MAX_STEPS,
 * translate32 outside {0,1}, steps NULL with F > 0, steps not 8-byte aligned.  F = 0 and B = 0 succeed without a launch. */
#define O3D_PRELOAD_MAX_FRAMES 4096
#define O3D_PRELOAD_MAX_BOXES 1024
#define O3D_PRELOAD_MAX_ROWS 536870911
#define O3D_PRELOAD_MAX_STEPS 4
long o3d_preload_scratch(int32_t* frames, int F, long raw_rows, int* grid);
int o3d_preload_count(const float* raw, long raw_rows, const int32_t* frames, const int32_t* frames_dev, int F,
                      const float* bounds, int B, const double* transform, int32_t* scratch, long scratch_len, int32_t* counts,
                      void* stream);
int o3d_preload_scatter(const float* raw, long raw_rows, const int32_t* frames, const int32_t* frames_dev, int F,
                        const float* bounds, int B, const double* transform, int32_t* scratch, long scratch_len,
                        const long* out_row, float* pool, long pool_rows, void* stream);
int o3d_preload_posed_count(const float* raw, long raw_rows, int row_floats, const int32_t* frames, const int32_t* frames_dev,
                            int F, const float* bounds, int B, const double* poses, int32_t* scratch, long scratch_len,
                            int32_t* counts, void* stream);
int o3d_preload_posed_scatter(const float* raw, long raw_rows, int row_floats, const int32_t* frames, const int32_t* frames_dev,
                              int F, const float* bounds, int B, const double* poses, int32_t* scratch, long scratch_len,
                              const long* out_row, float* pool, long pool_rows, void* stream);
int o3d_preload_steps_count(const float* raw, long raw_rows, int row_floats, const int32_t* frames, const int32_t* frames_dev,
                            int F, const float* bounds, int B, const double* steps, int n_steps, int translate32,
                            int32_t* scratch, long scratch_len, int32_t* counts, void* stream);
int o3d_preload_steps_scatter(const float* raw, long raw_rows, int row_floats, const int32_t* frames, const int32_t* frames_dev,
                              int F, const float* bounds, int B, const double* steps, int n_steps, int translate32,
                              int32_t* scratch, long scratch_len, const long* out_row, float* pool, long pool_rows,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* O3DSOT_H_ */
