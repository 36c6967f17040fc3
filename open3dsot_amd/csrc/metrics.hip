// Scoring tracked boxes on the device: estimateOverlap / estimateAccuracy (utils/metrics.py:27-72) for n box pairs in one
// launch, with optional accumulation of the Success / Precision threshold counts (TorchSuccess / TorchPrecision, :75-125).
//
//   o3d_track_score       a (n,15) annotation boxes, b (n,15) result boxes -> overlaps (n), distances (n), counters
//   o3d_scene_pair_scores tracks (K,15) x detections (D,15) -> overlaps (K,D), distances (K,D): the same score_pair for every
//                         pair of a scene tracker's frame (csrc/scene.hip reads the two matrices)
//   o3d_scene_pair_scores_frames  gt (F,G,15) x hyp (F,K,15) -> overlaps (F,G,K), distances (F,G,K): the same score_pair for
//                         every pair of every frame of a tracked run (o3d_scene_mot_walk reads them)
//
// A box is 15 floats: centre c (3), wlh = width, length, height (3), row-major rotation R (9).
//
// ---- the operation order (compiled with -ffp-contract=off; every operation is one IEEE fp64 operation on the fp32 inputs
// widened to double, in the order of the parentheses; tests/metrics_oracle.py restates it in numpy) ---------------------------
// Footprint of a box, `up` = the index of the non-zero component of up_axis (1: camera frame, (0,-1,0); 2: (0,0,1)):
//   hl = l*0.5, hw = w*0.5, hh = h*0.5;  v = the other ground axis: v = 1 for up = 2 (the xy plane), v = 2 for up = 1 (xz)
//   up = 2: corners [2,3,7,6] of Box.corners (bottom_corners): (sx,sy,sz) = (+,-,-) (+,+,-) (-,+,-) (-,-,-)
//   up = 1: corners [0,1,5,4] of Box.corners:                  (sx,sy,sz) = (+,+,+) (+,-,+) (-,-,+) (-,+,+)
//   X_k = c_0 + ((R00*(sx*hl) + R01*(sy*hw)) + R02*(sz*hh)),   Y_k = c_v + ((Rv0*(sx*hl) + Rv1*(sy*hw)) + Rv2*(sz*hh))
// The full rotation is used, not a yaw angle: a pitched or rolled box projects to the parallelogram its matrix gives.
//   twice the signed area of a polygon of m vertices   S = sum over j = 0..m-1, in that order, of (X_j*Y_j' - Y_j*X_j'),
//                                                      j' = j+1, and 0 after the last;  area = 0.5*|S|
// Intersection: quadrilateral A (the annotation) is clipped against the four edges of B in B's vertex order 0-1, 1-2, 2-3,
// 3-0, after B's vertices 1 and 3 are exchanged when S_B < 0 (B then runs counter-clockwise).  One stage, edge P -> Q:
//   E = Q - P;   d_j = (Ex*(Y_j - Py) - Ey*(X_j - Px));   vertex j is inside iff d_j >= 0
//   for j = 0..m-1, k = its successor: emit vertex j when inside; when exactly one of j, k is inside emit
//   t = d_j/(d_j - d_k),  (X_j + t*(X_k - X_j),  Y_j + t*(Y_k - Y_j))
// A stage adds at most one vertex: 4 -> <= 5 -> <= 6 -> <= 7 -> <= 8.  inter = the area of what is left (0 below 3 vertices).
//   dim 2   union = ((areaA + areaB) - inter);   overlap = inter/union
//   dim 3   the reference's height rule as it stands (from the centre DOWN by h, P2B's camera-frame convention):
//           top = min(ca_up, cb_up);  bottom = max(ca_up - ha, cb_up - hb);  iv = inter*max(0, top - bottom)
//           va = ((wa*la)*ha), vb likewise;  union = ((va + vb) - iv);  overlap = iv/union
//   distance  dim 3: sqrt(((dx*dx + dy*dy) + dz*dz)) of the centre difference;  dim 2: |d_up|, the norm over the components
//           where up_axis != 0, which is the ONE up component -- what the reference's mask literally selects
// Both results are rounded once to fp32.
// DEGENERATE INPUT: a box with a non-finite number, or a union that is not > 0 (or an overlap that is not finite), gives
// overlap 0, where the reference raises or returns NaN.  The distance is whatever the arithmetic above gives.
//
// ---- launch ------------------------------------------------------------------------------------------------------------------
// One thread per pair, 256 per workgroup.  The polygon lives in 2 x 8 fp64 registers per coordinate: every array index below
// is a compile-time constant after unrolling (a dynamic append position is a chain of selects over the slots), so nothing goes
// to scratch.  Counters: per threshold a wave64 ballot + popcount of the fp32-rounded result against the fp32 threshold; lane i
// keeps the count of threshold i and adds it with one 64-bit integer atomicAdd -- one atomic per wave and threshold, integer,
// so the sums do not depend on the order of the waves.
#include "o3d_common.hpp"

namespace {

constexpr int SCORE_WG = 256;
constexpr int SCORE_MAX_THR = 64;

struct ScoreArgs {
    const float* a; const float* b; const int32_t* valid;
    int n, dim, up;
    float* overlaps; float* distances;
    const float* thr_s; const float* thr_p;
    int ns, np;
    unsigned long long* cnt_s; unsigned long long* cnt_p; unsigned long long* total;
};

__device__ __forceinline__ void footprint(const float* __restrict__ box, int up, double (&X)[8], double (&Y)[8]) {
    const int v = up == 2 ? 1 : 2;
    const double hl = (double)box[4] * 0.5, hw = (double)box[3] * 0.5, hh = (double)box[5] * 0.5;
    const double c0 = box[0], cv = box[v];
    const double r00 = box[6], r01 = box[7], r02 = box[8];
    const double rv0 = box[6 + 3 * v], rv1 = box[7 + 3 * v], rv2 = box[8 + 3 * v];
    const double flip = up == 2 ? 1.0 : -1.0;          // sy and sz of up = 1 are those of up = 2 negated
    const double z = -flip * hh;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double x = (k < 2 ? 1.0 : -1.0) * hl;
        const double y = ((k == 1 || k == 2) ? flip : -flip) * hw;
        X[k] = c0 + ((r00 * x + r01 * y) + r02 * z);
        Y[k] = cv + ((rv0 * x + rv1 * y) + rv2 * z);
    }
}

// S of the first m (<= M) vertices
template <int M>
__device__ __forceinline__ double signed_area2(const double (&X)[8], const double (&Y)[8], int m) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int jn = j + 1 < M ? j + 1 : 0;
        const bool last = j + 1 >= m;
        const double xn = last ? X[0] : X[jn], yn = last ? Y[0] : Y[jn];
        const double term = X[j] * yn - Y[j] * xn;
        s = j < m ? s + term : s;
    }
    return s;
}

// one Sutherland-Hodgman stage on at most NIN vertices -> the number of vertices written to (OX, OY), at most NIN + 1
template <int NIN>
__device__ __forceinline__ int clip_stage(const double (&IX)[8], const double (&IY)[8], int m, double px, double py, double qx,
                                          double qy, double (&OX)[8], double (&OY)[8]) {
    const double ex = qx - px, ey = qy - py;
    double d[NIN];
#pragma unroll
    for (int j = 0; j < NIN; ++j) d[j] = ex * (IY[j] - py) - ey * (IX[j] - px);
    int out = 0;
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
        const int jn = j + 1 < NIN ? j + 1 : 0;
        const bool live = j < m, last = j + 1 >= m;
        const double dk = last ? d[0] : d[jn], kx = last ? IX[0] : IX[jn], ky = last ? IY[0] : IY[jn];
        const bool in_j = d[j] >= 0.0, in_k = dk >= 0.0;
        const bool keep = live && in_j, cross = live && (in_j != in_k);
#pragma unroll
        for (int s = 0; s <= NIN; ++s) {
            const bool here = keep && s == out;
            OX[s] = here ? IX[j] : OX[s];
            OY[s] = here ? IY[j] : OY[s];
        }
        out += keep ? 1 : 0;
        const double t = d[j] / (d[j] - dk);
        const double cx = IX[j] + t * (kx - IX[j]), cy = IY[j] + t * (ky - IY[j]);
#pragma unroll
        for (int s = 0; s <= NIN; ++s) {
            const bool here = cross && s == out;
            OX[s] = here ? cx : OX[s];
            OY[s] = here ? cy : OY[s];
        }
        out += cross ? 1 : 0;
    }
    return out;
}

__device__ __forceinline__ bool box_finite(const float* __restrict__ box) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 15; ++k) ok = ok && isfinite(box[k]);
    return ok;
}

__device__ __forceinline__ void score_pair(const float* __restrict__ A, const float* __restrict__ B, int dim, int up, float& overlap,
                                           float& distance) {
    double AX[8], AY[8], BX[8], BY[8], TX[8], TY[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) AX[k] = AY[k] = BX[k] = BY[k] = TX[k] = TY[k] = 0.0;
    footprint(A, up, AX, AY);
    footprint(B, up, BX, BY);
    const double sa = signed_area2<4>(AX, AY, 4), sb = signed_area2<4>(BX, BY, 4);
    const double area_a = 0.5 * fabs(sa), area_b = 0.5 * fabs(sb);
    if (sb < 0.0) {                                    // B counter-clockwise: 0,3,2,1
        const double x = BX[1], y = BY[1];
        BX[1] = BX[3]; BY[1] = BY[3];
        BX[3] = x; BY[3] = y;
    }
    int m = clip_stage<4>(AX, AY, 4, BX[0], BY[0], BX[1], BY[1], TX, TY);
    m = clip_stage<5>(TX, TY, m, BX[1], BY[1], BX[2], BY[2], AX, AY);
    m = clip_stage<6>(AX, AY, m, BX[2], BY[2], BX[3], BY[3], TX, TY);
    m = clip_stage<7>(TX, TY, m, BX[3], BY[3], BX[0], BY[0], AX, AY);
    const double inter = m < 3 ? 0.0 : 0.5 * fabs(signed_area2<8>(AX, AY, m));
    const double dx = (double)A[0] - (double)B[0], dy = (double)A[1] - (double)B[1], dz = (double)A[2] - (double)B[2];
    double num, den, dist;
    if (dim == 2) {
        num = inter;
        den = (area_a + area_b) - inter;
        dist = fabs(up == 2 ? dz : dy);
    } else {
        const double ua = A[up], ub = B[up], ha = A[5], hb = B[5];
        const double top = fmin(ua, ub), bottom = fmax(ua - ha, ub - hb);
        num = inter * fmax(0.0, top - bottom);
        const double va = ((double)A[3] * (double)A[4]) * ha, vb = ((double)B[3] * (double)B[4]) * hb;
        den = (va + vb) - num;
        dist = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    double ov = num / den;
    if (!(den > 0.0) || !isfinite(ov) || !box_finite(A) || !box_finite(B)) ov = 0.0;
    overlap = (float)ov;
    distance = (float)dist;
}

__global__ __launch_bounds__(SCORE_WG) void score_kernel(ScoreArgs g) {
    const long i = (long)blockIdx.x * SCORE_WG + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool on = i < g.n && (!g.valid || g.valid[i] != 0);
    float ov = 0.f, di = 0.f;
    if (on) {
        score_pair(g.a + 15 * i, g.b + 15 * i, g.dim, g.up, ov, di);
        if (g.overlaps) g.overlaps[i] = ov;
        if (g.distances) g.distances[i] = di;
    }
    if (g.cnt_s) {
        unsigned long long mine = 0;
        for (int k = 0; k < g.ns; ++k) {
            const unsigned long long hits = __ballot(on && ov >= g.thr_s[k]);
            if (lane == k) mine = __popcll(hits);
        }
        if (mine) atomicAdd(g.cnt_s + lane, mine);
    }
    if (g.cnt_p) {
        unsigned long long mine = 0;
        for (int k = 0; k < g.np; ++k) {
            const unsigned long long hits = __ballot(on && di <= g.thr_p[k]);
            if (lane == k) mine = __popcll(hits);
        }
        if (mine) atomicAdd(g.cnt_p + lane, mine);
    }
    if (g.total) {
        const unsigned long long live = __popcll(__ballot(on));
        if (lane == 0 && live) atomicAdd(g.total, live);
    }
}

// o3d_scene_pair_scores: score_pair for every (track k, detection d) of a scene tracker's frame, one thread per pair; the
// pairs of an inactive slot or of a column at or beyond n_det[0] (clamped to [0, D]) are written -1 / +inf
__global__ __launch_bounds__(SCORE_WG) void pair_score_kernel(const float* __restrict__ tracks, const int32_t* __restrict__ active, int K,
                                                              const float* __restrict__ dets, const int32_t* __restrict__ n_det, int D,
                                                              int dim, int up, float* __restrict__ overlaps,
                                                              float* __restrict__ distances) {
    const long i = (long)blockIdx.x * SCORE_WG + threadIdx.x;
    if (i >= (long)K * D) return;
    const int k = (int)(i / D), d = (int)(i % D);
    const int n = min(max(n_det[0], 0), D);
    float ov = -1.f, di = __int_as_float(0x7f800000);
    if (active[k] != 0 && d < n) score_pair(tracks + 15 * (long)k, dets + 15 * (long)d, dim, up, ov, di);
    overlaps[i] = ov;
    distances[i] = di;
}

// o3d_scene_pair_scores_frames: score_pair for every (frame f, ground-truth object g, hypothesis k) of a tracked run, one thread
// per pair on a 64-bit index; the pairs of an object without annotation (gt_valid == 0) or of an empty column (hyp_ids < 0) are
// written -1 / +inf
__global__ __launch_bounds__(SCORE_WG) void pair_score_frames_kernel(const float* __restrict__ gt, const int32_t* __restrict__ gt_valid,
                                                                     const float* __restrict__ hyp, const int32_t* __restrict__ hyp_ids,
                                                                     long pairs, int G, int K, int dim, int up,
                                                                     float* __restrict__ overlaps, float* __restrict__ distances) {
    const long i = (long)blockIdx.x * SCORE_WG + threadIdx.x;
    if (i >= pairs) return;
    const long fg = i / K, f = fg / G;
    const long fk = f * K + (i - fg * K);
    float ov = -1.f, di = __int_as_float(0x7f800000);
    if (gt_valid[fg] != 0 && hyp_ids[fk] >= 0) score_pair(gt + 15 * fg, hyp + 15 * fk, dim, up, ov, di);
    overlaps[i] = ov;
    distances[i] = di;
}

}  // namespace

extern "C" int o3d_scene_pair_scores_frames(const float* gt, const int32_t* gt_valid, const float* hyp, const int32_t* hyp_ids, int F,
                                            int G, int K, int dim, int up, float* overlaps, float* distances, void* stream) {
    if (F < 0 || G < 1 || G > O3D_CROP_MULTI_MAX_TARGETS || K < 1 || K > O3D_CROP_MULTI_MAX_TARGETS || (dim != 2 && dim != 3) ||
        (up != 1 && up != 2) || !gt || !gt_valid || !hyp || !hyp_ids || !overlaps || !distances)
        return O3D_EINVAL;
    const long pairs = (long)F * G * K;
    if ((pairs + SCORE_WG - 1) / SCORE_WG > 0x7fffffffL) return O3D_EINVAL;       // more workgroups than one launch takes
    if (F == 0) return O3D_OK;
    hipLaunchKernelGGL(pair_score_frames_kernel, dim3(o3d_cdiv(pairs, SCORE_WG)), dim3(SCORE_WG), 0, o3d_stream(stream), gt, gt_valid,
                       hyp, hyp_ids, pairs, G, K, dim, up, overlaps, distances);
    return o3d_launch_status();
}

extern "C" int o3d_scene_pair_scores(const float* tracks, const int32_t* active, int K, const float* dets, const int32_t* n_det, int D,
                                     int dim, int up, float* overlaps, float* distances, void* stream) {
    if (K < 1 || K > O3D_CROP_MULTI_MAX_TARGETS || D < 0 || D > O3D_SCENE_MAX_DETECTIONS || (dim != 2 && dim != 3) ||
        (up != 1 && up != 2) || !tracks || !active)
        return O3D_EINVAL;
    if (D == 0) return O3D_OK;
    if (!dets || !n_det || !overlaps || !distances) return O3D_EINVAL;
    hipLaunchKernelGGL(pair_score_kernel, dim3(o3d_cdiv((long)K * D, SCORE_WG)), dim3(SCORE_WG), 0, o3d_stream(stream), tracks, active,
                       K, dets, n_det, D, dim, up, overlaps, distances);
    return o3d_launch_status();
}

extern "C" int o3d_track_score(const float* a, const float* b, const int32_t* valid, int n, int dim, int up, float* overlaps,
                               float* distances, const float* thr_s, int ns, const float* thr_p, int np, int64_t* cnt_s,
                               int64_t* cnt_p, int64_t* total, void* stream) {
    if (!a || !b || n < 0 || (dim != 2 && dim != 3) || (up != 1 && up != 2)) return O3D_EINVAL;
    if (ns < 0 || np < 0 || ns > SCORE_MAX_THR || np > SCORE_MAX_THR) return O3D_EINVAL;
    if ((cnt_s && (!thr_s || ns < 1)) || (cnt_p && (!thr_p || np < 1))) return O3D_EINVAL;
    if (n == 0) return O3D_OK;
    ScoreArgs g{a, b, valid, n, dim, up, overlaps, distances, thr_s, thr_p, ns, np,
                reinterpret_cast<unsigned long long*>(cnt_s), reinterpret_cast<unsigned long long*>(cnt_p),
                reinterpret_cast<unsigned long long*>(total)};
    hipLaunchKernelGGL(score_kernel, dim3(o3d_cdiv(n, SCORE_WG)), dim3(SCORE_WG), 0, o3d_stream(stream), g);
    return o3d_launch_status();
}
