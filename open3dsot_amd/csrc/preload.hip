// The preload crop of a dataset reader, on the device: what the reference's kittiDataset does on the host once per annotated
// object per frame (datasets/kitti.py:139-189 _get_frame_from_anno: PointCloud.transform in camera mode, then
// datasets/points_utils.py:146-171 crop_pc_axis_aligned with offset = preload_offset), for a chunk of raw velodyne frames that
// one copy has put into HBM.  open3dsot_amd/datasets.py is the caller.
//
//   o3d_preload_scratch   host only: plans the frame table (first box, workgroup start and scratch base of every frame)
//   o3d_preload_count     launch 1 (count) and launch 2 (scan): the survivors of every box -> counts (B)
//   o3d_preload_scatter   launch 3: the survivors of every box, in their original order, as xyz rows of the pool
//   o3d_preload_posed_count / o3d_preload_posed_scatter   the same launches with ONE TRANSFORM PER FRAME RECORD, read from the
//                         device, over raw rows of 3 or 4 floats: the reference's WaymoDataset (datasets/waymo_data.py:118-167
//                         _get_frame_from_anno), whose frames carry a vehicle-to-global pose each
//   o3d_preload_steps_count / o3d_preload_steps_scatter   the same launches with A CHAIN OF ROUNDED RIGID STEPS per frame record
//                         over raw rows of 3, 4 or 5 floats: the reference's NuScenesDataset (datasets/nuscenes_data.py:154-173
//                         _get_frame_from_anno_data), whose sweeps go sensor -> ego -> global by rotate / translate pairs
// The host reads `counts` between the two calls (the only synchronisation of a chunk), sizes the pool and uploads the first
// pool row of every box.
//
// ---- the tables -------------------------------------------------------------------------------------------------------------------------
// raw (raw_rows,4) float32: the frames of the chunk as they lie in the .bin files, x y z intensity; a row is one aligned 16-byte
// load and the intensity is never looked at.  frames (F,6) int32: first raw row, n, first box, number of boxes, workgroup
// start, scratch base.  Two records may name the same raw rows (a frame with more than O3D_PRELOAD_MAX_BOXES boxes is two
// records).  The boxes of record f are [first box, first box + number): the records partition [0, B) in order.  bounds (B,6)
// float32: lo x y z, hi x y z.
//
// ---- the test, and why fp32 compares are exact ------------------------------------------------------------------------------------------
// The reference keeps a point when mini < p < maxi per axis: the float32 coordinate against the fp64 bound.  For a float32 x
// and a double m, x < m <=> x < up(m) with up(m) the smallest float32 >= m, and x > m <=> x > down(m) with down(m) the largest
// float32 <= m (no float32 lies strictly between m and its directed rounding).  The host rounds the fp64 bounds directionally
// -- hi up, lo down -- and the kernel compares in fp32:
//   keep = (x > lo_x && x < hi_x) && (y > lo_y && y < hi_y) && (z > lo_z && z < hi_z)
// A NaN coordinate fails every compare, as on the host.  Bounds of -inf / +inf keep every point with finite coordinates
// (preload_offset <= 0: the reference does not crop).
//
// ---- camera mode --------------------------------------------------------------------------------------------------------------------------
// transform = the 3x4 upper rows of velo_to_cam, fp64, row-major, passed by value.  The point is transformed before the test and
// the transformed point is what is written, computed in fp64 on the float32 input and rounded once:
//   x'_i = float(((T_i0*x + T_i1*y) + T_i2*z) + T_i3)
// which is PointCloud.transform stored back into its float32 array.  This file is compiled with -ffp-contract=off.
//
// ---- a pose per record --------------------------------------------------------------------------------------------------------------------
// poses (F,12) fp64 on the device: the 3x4 upper rows of record f's global_from_car, row-major; two records over the same raw
// rows carry the same pose twice.  The rule is the camera-mode rule above, word for word (preload_apply is the one statement of
// it), and it is WaymoDataset's `pointcloud[:3,:] = global_from_car.dot(vstack(points, ones))[:3,:]`: fp64 on the float32
// input, stored back into the float32 array, so rounded once.  With translations of kilometres that single rounding decides
// bits, which is why the sum is ordered.  Raw row r is floats [r*row_floats, r*row_floats + 3): Waymo's points_xyz lie as
// (n,3) rows, which are three 4-byte loads; rows of four floats stay one aligned 16-byte load.  The record, and with it the
// pose, is uniform over a workgroup: the twelve doubles are scalar loads.
//
// ---- a chain of steps per record --------------------------------------------------------------------------------------------------------
// steps (F,n_steps,12) fp64 on the device: step s of record f is a row-major 3x4 [R | t], n_steps in 1..O3D_PRELOAD_MAX_STEPS.
// NuScenesDataset does pc.rotate(R); pc.translate(t) twice on a float32 array (datasets/data_classes.py:79-94): every rotate and
// every translate stores back into float32, so a point is rounded FOUR times, and with ego translations of hundreds of metres
// every rounding decides bits.  preload_step is the one statement of a step, on the float32 input (x, y, z):
//   r_i = float((M_i0*x + M_i1*y) + M_i2*z)                 fp64, this order, rounded to float32 (np.dot(R, points[:3]) stored back)
//   translate32 == 0:  p_i = float(double(r_i) + M_i3)      points[i] + np.float64 under numpy >= 2: an fp64 sum, rounded on assignment
//   translate32 == 1:  p_i = r_i + float(M_i3)              the same line under numpy < 2: the scalar is demoted, an fp32 add
// p is the next step's input; the last p is tested and written.  Raw row r is floats [r*row_floats, r*row_floats + 3): the
// .pcd.bin rows of NuScenes are x y z intensity ring, 20 bytes, uploaded as they lie; the device reads 12 of every 20 bytes.
// The record, and with it the chain, is uniform over a workgroup.
//
// ---- three launches, no workgroup ever waits for another ----------------------------------------------------------------------------------
// The host knows every n and plans the table, as o3d_track_crop_groups_scratch does: record f owns workgroups [wg_start, wg_start
// + W) of the count and scatter launches (W = ceil(n / 256), 1 for an empty frame, 0 for a record without boxes) and its boxes'
// rows of W int32 of scratch from sbase on (box-major).  A workgroup finds its record by a binary search with blockIdx.x as the
// only input.  Every point is loaded once per launch and tested against all boxes of its frame, O3D_CROP_MULTI_CHUNK boxes
// staged in LDS at a time with one keep bit each.
//   launch 1 (count)    writes scratch[f][k][w], its own word per box.
//   launch 2 (scan)     crop_scan_row (track_common.hpp): one workgroup per box rewrites its OWN row by its exclusive prefix
//                       sums and writes counts[b].
//   launch 3 (scatter)  reads scratch[f][k][w] and out_row[b]; survivor number pos of box b goes to pool row out_row[b] + pos,
//                       when that row is >= 0 and < pool_rows.
// No flag, no atomic, no loop that waits on memory; the order between the launches is the stream's.
#include "track_common.hpp"

namespace {

constexpr int PRELOAD_COLS = 6;                            // raw row, n, first box, boxes, wg_start, sbase

struct preload_xf {                                          // one transform for the whole call, by value
    double m[12];
    int on;
};

struct preload_poses {                                       // one transform per frame record, on the device
    const double* poses;
    int row_floats;
};

struct preload_steps {                                       // a chain of rounded rigid steps per frame record, on the device
    const double* steps;
    int row_floats, n_steps, translate32;
};

// the record of workgroup (COL 4) or box (COL 2) `x`: the last f with frames[f][COL] <= x.  Records that own nothing share
// their start with the record after them, so the last of equals is the owner
template <int COL>
__device__ __forceinline__ int preload_frame_of(const int32_t* __restrict__ frames, int F, int x) {
    int lo = 0, hi = F - 1;
    while (lo < hi) {                                      // at most 12 steps: register state only, every read is of the table
        const int mid = (lo + hi + 1) >> 1;
        if (frames[PRELOAD_COLS * mid + COL] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the one statement of the transform: fp64 on the float32 input, this order of operations, rounded once
__device__ __forceinline__ void preload_apply(const double* __restrict__ m, float fx, float fy, float fz, float& px, float& py,
                                              float& pz) {
    const double x = fx, y = fy, z = fz;
    px = (float)(((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
    py = (float)(((m[4] * x + m[5] * y) + m[6] * z) + m[7]);
    pz = (float)(((m[8] * x + m[9] * y) + m[10] * z) + m[11]);
}

// point `row` of the raw table as record f sees it.  preload_xf: one transform for the call, by value, rows of four floats
__device__ __forceinline__ void preload_point(const float* __restrict__ raw, const preload_xf T, int f, long row, float& px, float& py,
                                              float& pz) {
    const float4 v = reinterpret_cast<const float4*>(raw)[row];
    if (T.on) {
        preload_apply(T.m, v.x, v.y, v.z, px, py, pz);
    } else {
        px = v.x; py = v.y; pz = v.z;
    }
}

// preload_poses: the transform of record f from the device table, rows of 3 or 4 floats
__device__ __forceinline__ void preload_point(const float* __restrict__ raw, const preload_poses P, int f, long row, float& px,
                                              float& py, float& pz) {
    float x, y, z;
    if (P.row_floats == 4) {
        const float4 v = reinterpret_cast<const float4*>(raw)[row];
        x = v.x; y = v.y; z = v.z;
    } else {
        const float* r = raw + 3 * row;
        x = r[0]; y = r[1]; z = r[2];
    }
    preload_apply(P.poses + 12 * (long)f, x, y, z, px, py, pz);
}

// the one statement of a rounded rigid step: rotate in fp64 in this order and round, then translate in fp64 and round
// (translate32 == 0) or in fp32 (translate32 == 1).  In place: p is the next step's input
__device__ __forceinline__ void preload_step(const double* __restrict__ m, int translate32, float& px, float& py, float& pz) {
    const double x = px, y = py, z = pz;
    const float rx = (float)((m[0] * x + m[1] * y) + m[2] * z);
    const float ry = (float)((m[4] * x + m[5] * y) + m[6] * z);
    const float rz = (float)((m[8] * x + m[9] * y) + m[10] * z);
    if (translate32) {
        px = rx + (float)m[3]; py = ry + (float)m[7]; pz = rz + (float)m[11];
    } else {
        px = (float)((double)rx + m[3]); py = (float)((double)ry + m[7]); pz = (float)((double)rz + m[11]);
    }
}

// preload_steps: the chain of record f from the device table, rows of 3, 4 or 5 floats
__device__ __forceinline__ void preload_point(const float* __restrict__ raw, const preload_steps C, int f, long row, float& px,
                                              float& py, float& pz) {
    if (C.row_floats == 4) {
        const float4 v = reinterpret_cast<const float4*>(raw)[row];
        px = v.x; py = v.y; pz = v.z;
    } else {
        const float* r = raw + C.row_floats * row;
        px = r[0]; py = r[1]; pz = r[2];
    }
    const double* m = C.steps + 12 * ((long)C.n_steps * f);
    for (int s = 0; s < C.n_steps; ++s) preload_step(m + 12 * s, C.translate32, px, py, pz);
}

template <bool SCATTER, class XF>
__global__ __launch_bounds__(CROP_WG) void preload_kernel(const float* __restrict__ raw, const int32_t* __restrict__ frames, int F,
                                                          const float* __restrict__ bounds, XF T, int32_t* __restrict__ scratch,
                                                          const long* __restrict__ out_row, float* __restrict__ pool, long pool_rows) {
    __shared__ float bnd[CROP_MULTI_CHUNK][6];
    __shared__ int wave_cnt[CROP_MULTI_CHUNK][CROP_WG / 64];
    const int f = preload_frame_of<4>(frames, F, (int)blockIdx.x);
    const int32_t* rec = frames + PRELOAD_COLS * f;
    const int row0 = rec[0], n = rec[1], b0 = rec[2], nb = rec[3], w = (int)blockIdx.x - rec[4];
    const int W = n > 0 ? (n + CROP_WG - 1) / CROP_WG : 1;
    if (nb <= 0 || w < 0 || w >= W) return;               // a device table that disagrees with the planned grid: nothing is touched
    int32_t* S = scratch + rec[5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = w * CROP_WG + tid;
    const bool in = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (in) preload_point(raw, T, f, (long)row0 + i, px, py, pz);
    for (int k0 = 0; k0 < nb; k0 += CROP_MULTI_CHUNK) {
        const int nc = nb - k0 < CROP_MULTI_CHUNK ? nb - k0 : CROP_MULTI_CHUNK;
        __syncthreads();                                   // the previous chunk's readers are done with bnd / wave_cnt
        for (int e = tid; e < nc * 6; e += CROP_WG) (&bnd[0][0])[e] = bounds[6 * (long)(b0 + k0) + e];
        __syncthreads();
        unsigned bits = 0u;                                // bit k: this thread's point survives box b0 + k0 + k
        for (int k = 0; k < nc; ++k) {
            const bool keep = in && (px > bnd[k][0] && px < bnd[k][3]) && (py > bnd[k][1] && py < bnd[k][4]) &&
                              (pz > bnd[k][2] && pz < bnd[k][5]);
            const unsigned long long mask = __ballot(keep);
            if (lane == 0) wave_cnt[k][wave] = __popcll(mask);
            if (keep) bits |= 1u << k;
        }
        __syncthreads();
        if (!SCATTER) {
            if (tid < nc) S[(long)(k0 + tid) * W + w] = (wave_cnt[tid][0] + wave_cnt[tid][1]) + (wave_cnt[tid][2] + wave_cnt[tid][3]);
            continue;
        }
        for (int k = 0; k < nc; ++k) {
            const bool keep = (bits >> k) & 1u;
            const unsigned long long mask = __ballot(keep);
            if (!keep) continue;
            long pos = S[(long)(k0 + k) * W + w];          // the survivors of the workgroups before this one (launch 2)
            for (int v = 0; v < wave; ++v) pos += wave_cnt[k][v];
            pos += __popcll(mask & ((1ull << lane) - 1ull));
            const long first = out_row[b0 + k0 + k];
            const long row = first + pos;
            if (first >= 0 && row < pool_rows) {
                float* o = pool + 3 * row;
                o[0] = px; o[1] = py; o[2] = pz;
            }
        }
    }
}

__global__ __launch_bounds__(CROP_WG) void preload_scan_kernel(const int32_t* __restrict__ frames, int F, int32_t* __restrict__ scratch,
                                                               int32_t* __restrict__ counts) {
    const int b = (int)blockIdx.x;
    const int32_t* rec = frames + PRELOAD_COLS * preload_frame_of<2>(frames, F, b);
    const int W = rec[1] > 0 ? (rec[1] + CROP_WG - 1) / CROP_WG : 1, k = b - rec[2];
    if (k < 0 || k >= rec[3]) return;
    crop_scan_row(scratch + rec[5] + (long)k * W, W, counts + b);
}

// the plan of the HOST table: checks every record, fills (fill) or compares (check_plan) first box / wg_start / sbase
static bool preload_plan(const int32_t* frames, int F, long raw_rows, bool check_plan, int32_t* fill, long& wgs, long& boxes, long& need,
                         bool& any_points) {
    wgs = boxes = need = 0;
    any_points = false;
    if (F < 0 || F > O3D_PRELOAD_MAX_FRAMES || (F > 0 && !frames) || raw_rows < 0 || raw_rows > O3D_PRELOAD_MAX_ROWS) return false;
    for (int f = 0; f < F; ++f) {
        const int32_t* r = frames + PRELOAD_COLS * f;
        const long row0 = r[0], n = r[1], nb = r[3];
        if (row0 < 0 || n < 0 || row0 + n > raw_rows || nb < 0 || nb > O3D_PRELOAD_MAX_BOXES) return false;
        if (check_plan && (r[2] != boxes || r[4] != wgs || r[5] != need)) return false;
        if (fill) {
            int32_t* o = fill + PRELOAD_COLS * f;
            o[2] = (int32_t)boxes; o[4] = (int32_t)wgs; o[5] = (int32_t)need;
        }
        const long W = nb > 0 ? crop_wgs((int)n) : 0;
        wgs += W;
        boxes += nb;
        need += W * nb;
        if (need > 0x7fffffffL) return false;
        if (nb > 0 && n > 0) any_points = true;
    }
    return true;
}

static bool preload_args_ok(const float* raw, long raw_rows, const int32_t* frames, const int32_t* frames_dev, int F, const float* bounds,
                            int B, const int32_t* scratch, long scratch_len, long& wgs, unsigned raw_align = 16u) {
    long boxes, need;
    bool any_points;
    if (B < 0 || !preload_plan(frames, F, raw_rows, true, nullptr, wgs, boxes, need, any_points) || boxes != B) return false;
    if (wgs == 0) return true;                             // nothing to launch: no pointer is needed
    if (!frames_dev || !bounds || !scratch || scratch_len < need) return false;
    if (any_points && (!raw || (reinterpret_cast<uintptr_t>(raw) & (raw_align - 1u)))) return false;
    return true;
}

static preload_xf preload_transform(const double* transform) {
    preload_xf T;
    for (int i = 0; i < 12; ++i) T.m[i] = transform ? transform[i] : 0.0;
    T.on = transform ? 1 : 0;
    return T;
}

// what the posed pair refuses beyond preload_args_ok
static bool preload_posed_ok(int row_floats, int F, const double* poses) {
    if (row_floats != 3 && row_floats != 4) return false;
    return F <= 0 || (poses && !(reinterpret_cast<uintptr_t>(poses) & 7u));
}

// what the steps pair refuses beyond preload_args_ok
static bool preload_steps_ok(int row_floats, int F, const double* steps, int n_steps, int translate32) {
    if (row_floats < 3 || row_floats > 5 || n_steps < 1 || n_steps > O3D_PRELOAD_MAX_STEPS || (translate32 != 0 && translate32 != 1))
        return false;
    return F <= 0 || (steps && !(reinterpret_cast<uintptr_t>(steps) & 7u));
}

}  // namespace

// Host only (no HIP call).  frames (F,6): the caller sets columns 0 (first raw row), 1 (n) and 3 (number of boxes); this fills
// 2 (first box), 4 (workgroup start) and 5 (scratch base) in place and writes grid[0] = the workgroups of the count / scatter
// launches, grid[1] = B, the boxes (grid may be NULL).  -> the scratch length in int32, -1 for a bad table.
extern "C" long o3d_preload_scratch(int32_t* frames, int F, long raw_rows, int* grid) {
    long wgs, boxes, need;
    bool any_points;
    if (!preload_plan(frames, F, raw_rows, false, frames, wgs, boxes, need, any_points)) return -1;
    if (grid) { grid[0] = (int)wgs; grid[1] = (int)boxes; }
    return need;
}

extern "C" int o3d_preload_count(const float* raw, long raw_rows, const int32_t* frames, const int32_t* frames_dev, int F,
                                 const float* bounds, int B, const double* transform, int32_t* scratch, long scratch_len,
                                 int32_t* counts, void* stream) {
    long wgs;
    if (!preload_args_ok(raw, raw_rows, frames, frames_dev, F, bounds, B, scratch, scratch_len, wgs) || (B > 0 && !counts))
        return O3D_EINVAL;
    if (B == 0) return O3D_OK;                             // wgs == 0 as well: every workgroup belongs to a box
    hipLaunchKernelGGL((preload_kernel<false, preload_xf>), dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), raw, frames_dev, F, bounds,
                       preload_transform(transform), scratch, (const long*)nullptr, (float*)nullptr, 0L);
    hipLaunchKernelGGL(preload_scan_kernel, dim3(B), dim3(CROP_WG), 0, o3d_stream(stream), frames_dev, F, scratch, counts);
    return o3d_launch_status();
}

extern "C" int o3d_preload_scatter(const float* raw, long raw_rows, const int32_t* frames, const int32_t* frames_dev, int F,
                                   const float* bounds, int B, const double* transform, int32_t* scratch, long scratch_len,
                                   const long* out_row, float* pool, long pool_rows, void* stream) {
    long wgs;
    if (!preload_args_ok(raw, raw_rows, frames, frames_dev, F, bounds, B, scratch, scratch_len, wgs) || pool_rows < 0 ||
        (B > 0 && !out_row) || (pool_rows > 0 && !pool))
        return O3D_EINVAL;
    if (B == 0 || pool_rows == 0) return O3D_OK;
    hipLaunchKernelGGL((preload_kernel<true, preload_xf>), dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), raw, frames_dev, F, bounds,
                       preload_transform(transform), scratch, out_row, pool, pool_rows);
    return o3d_launch_status();
}

// The same launches with a pose per frame record (poses (F,12) fp64 on the device) over raw rows of row_floats = 3 | 4 floats
extern "C" int o3d_preload_posed_count(const float* raw, long raw_rows, int row_floats, const int32_t* frames, const int32_t* frames_dev,
                                       int F, const float* bounds, int B, const double* poses, int32_t* scratch, long scratch_len,
                                       int32_t* counts, void* stream) {
    long wgs;
    if (!preload_posed_ok(row_floats, F, poses) ||
        !preload_args_ok(raw, raw_rows, frames, frames_dev, F, bounds, B, scratch, scratch_len, wgs, row_floats == 4 ? 16u : 4u) ||
        (B > 0 && !counts))
        return O3D_EINVAL;
    if (B == 0) return O3D_OK;
    hipLaunchKernelGGL((preload_kernel<false, preload_poses>), dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), raw, frames_dev, F,
                       bounds, preload_poses{poses, row_floats}, scratch, (const long*)nullptr, (float*)nullptr, 0L);
    hipLaunchKernelGGL(preload_scan_kernel, dim3(B), dim3(CROP_WG), 0, o3d_stream(stream), frames_dev, F, scratch, counts);
    return o3d_launch_status();
}

extern "C" int o3d_preload_posed_scatter(const float* raw, long raw_rows, int row_floats, const int32_t* frames,
                                         const int32_t* frames_dev, int F, const float* bounds, int B, const double* poses,
                                         int32_t* scratch, long scratch_len, const long* out_row, float* pool, long pool_rows,
                                         void* stream) {
    long wgs;
    if (!preload_posed_ok(row_floats, F, poses) ||
        !preload_args_ok(raw, raw_rows, frames, frames_dev, F, bounds, B, scratch, scratch_len, wgs, row_floats == 4 ? 16u : 4u) ||
        pool_rows < 0 || (B > 0 && !out_row) || (pool_rows > 0 && !pool))
        return O3D_EINVAL;
    if (B == 0 || pool_rows == 0) return O3D_OK;
    hipLaunchKernelGGL((preload_kernel<true, preload_poses>), dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), raw, frames_dev, F,
                       bounds, preload_poses{poses, row_floats}, scratch, out_row, pool, pool_rows);
    return o3d_launch_status();
}

// The same launches with a chain of n_steps rounded rigid steps per frame record (steps (F,n_steps,12) fp64 on the device) over
// raw rows of row_floats = 3 | 4 | 5 floats
extern "C" int o3d_preload_steps_count(const float* raw, long raw_rows, int row_floats, const int32_t* frames, const int32_t* frames_dev,
                                       int F, const float* bounds, int B, const double* steps, int n_steps, int translate32,
                                       int32_t* scratch, long scratch_len, int32_t* counts, void* stream) {
    long wgs;
    if (!preload_steps_ok(row_floats, F, steps, n_steps, translate32) ||
        !preload_args_ok(raw, raw_rows, frames, frames_dev, F, bounds, B, scratch, scratch_len, wgs, row_floats == 4 ? 16u : 4u) ||
        (B > 0 && !counts))
        return O3D_EINVAL;
    if (B == 0) return O3D_OK;
    hipLaunchKernelGGL((preload_kernel<false, preload_steps>), dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), raw, frames_dev, F,
                       bounds, preload_steps{steps, row_floats, n_steps, translate32}, scratch, (const long*)nullptr, (float*)nullptr, 0L);
    hipLaunchKernelGGL(preload_scan_kernel, dim3(B), dim3(CROP_WG), 0, o3d_stream(stream), frames_dev, F, scratch, counts);
    return o3d_launch_status();
}

extern "C" int o3d_preload_steps_scatter(const float* raw, long raw_rows, int row_floats, const int32_t* frames,
                                         const int32_t* frames_dev, int F, const float* bounds, int B, const double* steps, int n_steps,
                                         int translate32, int32_t* scratch, long scratch_len, const long* out_row, float* pool,
                                         long pool_rows, void* stream) {
    long wgs;
    if (!preload_steps_ok(row_floats, F, steps, n_steps, translate32) ||
        !preload_args_ok(raw, raw_rows, frames, frames_dev, F, bounds, B, scratch, scratch_len, wgs, row_floats == 4 ? 16u : 4u) ||
        pool_rows < 0 || (B > 0 && !out_row) || (pool_rows > 0 && !pool))
        return O3D_EINVAL;
    if (B == 0 || pool_rows == 0) return O3D_OK;
    hipLaunchKernelGGL((preload_kernel<true, preload_steps>), dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), raw, frames_dev, F,
                       bounds, preload_steps{steps, row_floats, n_steps, translate32}, scratch, out_row, pool, pool_rows);
    return o3d_launch_status();
}
