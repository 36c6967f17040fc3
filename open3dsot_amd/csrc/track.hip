// The tracking front end: what the reference does on the host between "a LiDAR frame arrives" and "the network runs", and
// between "the network answers" and "the next frame's search region is known" (models/base_model.py:59-86,166-247).
//
//   o3d_track_crop        generate_subwindow(oriented=True) / cropAndCenterPC  (datasets/points_utils.py:103-124,146-250)
//   o3d_track_resample    the row gather of regularize_pc (:24-40) straight into the network's input buffers
//   o3d_track_offset_box  getOffsetBB (:43-85) with the box sequence kept on the device
//   o3d_track_motion_input  the network input of the motion tracker: MotionBaseModel.build_input_dict behind its two crops
//                         (models/base_model.py:263-302)
//   o3d_track_crop_multi / o3d_track_resample_multi / o3d_track_offset_box_multi / o3d_track_motion_input_multi
//                         the same steps for K targets of one scene per launch (tracking.MultiTargetTracker,
//                         tracking.MultiMotionTracker); every target's result is bit-identical to the single-target entry
//                         point's
//   o3d_track_resample_drawn / o3d_track_bank_update / o3d_track_motion_input_drawn
//                         the free-running loop (tracking.py, sampling="device"): the counts are read where the crop left
//                         them, the indices are the keyed draw of track_common.hpp, the template bank's {fixed, total} is
//                         device state -- nothing of a frame crosses to the host.  Each _drawn entry point, here and on lanes,
//                         has a _tabled twin (sampling="table"): the same launcher, kernel body and row function with the other
//                         index source, a device table of the reference's draw
//   o3d_track_bank_update_lanes / o3d_track_resample_drawn_lanes / o3d_track_motion_input_drawn_lanes /
//   o3d_track_offset_box_lanes / o3d_track_lane_start
//                         the free-running loop L tracklets wide (tracking.LaneTracker, tracking.MotionLaneTracker): a lane is a
//                         leading axis, its row of the (L, O3D_LANE_COLS) int32 lane table says what it does at this step, and
//                         every kernel calls the device function of the single form
//
// A box is 15 floats: centre c (3), wlh = width, length, height (3), row-major rotation R (9).
//
// ---- the crop's fp32 operation order (compiled with -ffp-contract=off: the crop kernels hold no fused multiply-add) ---------------
// Every operation below is one IEEE fp32 operation, in the order of the parentheses; tests/tracking_oracle.py restates it in
// numpy and the two agree bit for bit.
//   d  = p - c                                    dx = px - cx, dy = py - cy, dz = pz - cz
//   q  = R^T d                                    qx = ((R00*dx + R10*dy) + R20*dz)
//                                                 qy = ((R01*dx + R11*dy) + R21*dz)
//                                                 qz = ((R02*dx + R12*dy) + R22*dz)
//   box-frame half extents (x pairs with l,       hx = ((l*scale)*0.5 + offset),  hy = ((w*scale)*0.5 + offset),
//   y with w: Box.corners)                        hz = ((h*scale)*0.5 + offset)
//   box-frame test                                |qx| < hx  and  |qy| < hy  and  |qz| < hz          (six strict inequalities)
//   mode MODEL only, first (crop_pc_axis_aligned on the world-frame cloud, box scaled by 4*scale, padded by 2*offset):
//     s4 = 4*scale,  L = (l*s4)*0.5,  W = (w*s4)*0.5,  H = (h*s4)*0.5,  o2 = 2*offset
//     e_i = (((|Ri0|*L + |Ri1|*W) + |Ri2|*H) + o2)       the extent of the scaled box's corners along world axis i
//     world test                                  |dx| < e_0  and  |dy| < e_1  and  |dz| < e_2
// A point is kept iff it passes the box-frame test (and, in mode MODEL, the world test); the output row is q.
//
// ---- the motion input's fp32 operation order (motion_row, of o3d_track_motion_input[_multi]; tests/motion_oracle.py restates it) ---------------------
// Row i of `points` (2N,5) is (x, y, z, time stamp, prior targetness); (x, y, z) is the gathered row (zeros when the half is
// zero-filled or the index lies outside the source), copied, not computed.  Previous half (i < N), box = centre 0, identity
// rotation, the given wlh (x pairs with l, y with w):
//   half extents of the box scaled by 1.25        hx = ((l*1.25)*0.5),  hy = ((w*1.25)*0.5),  hz = ((h*1.25)*0.5)
//   inside (inclusive: points_in_box)             |x| <= hx  and  |y| <= hy  and  |z| <= hz
//   channel 3 = 0,  channel 4 = inside ? 1 : 0 when first_frame, else inside ? float32(0.8) : float32(0.2)
//   BoxCloud, landmark 0 the centre, 1..8 the corners of Box.corners (wlh_factor 1):
//     a = l*0.5, b = w*0.5, c = h*0.5;  corner k = (sx_k*a, sy_k*b, sz_k*c),  sx = +,+,+,+,-,-,-,-  sy = +,-,-,+,+,-,-,+
//     sz = +,+,-,-,+,+,-,-;   dx = x - X, dy = y - Y, dz = z - Z;   distance = sqrt(((dx*dx + dy*dy) + dz*dz))
// Current half (i >= N): channel 3 = float32(0.1), channel 4 = 0.5, BoxCloud row = 0.
//
// ---- compaction: two launches, no workgroup ever waits for another ------------------------------------------------------------
// Launch 1: every workgroup of 256 points counts its survivors (wave64 ballot + popcount, four waves summed through LDS) into
// scratch[workgroup].  Launch 2: every workgroup sums the counts of the workgroups before it in its job (<= 469 integers for a
// 120 000-point frame, out of L2), evaluates the predicate again and scatters its survivors behind that base, in their original
// order.  Survivors beyond `capacity` are counted, not written.  Up to O3D_CROP_MAX_JOBS jobs share the two launches.
//
// ---- o3d_track_crop_multi: one cloud against K boxes, three launches, no workgroup ever waits for another --------------------
// A group is one cloud of n points and a DEVICE table of K targets (box, scale, offset, mode, out, capacity, count); a call
// takes 1 or 2 groups.  scratch holds, per group, K rows of W = ceil(n / 256) int32 (target-major).
//   launch 1 (count)    workgroup w of a group loads its 256 points ONCE and tests them against all K targets, whose
//                       parameters are staged in LDS CROP_MULTI_CHUNK at a time; per target a wave64 ballot + popcount, the
//                       four waves summed through LDS -> scratch[k][w].  Reads: points, the table, the boxes.
//   launch 2 (scan)     one workgroup per (group, target) replaces its OWN row scratch[k][0..W) by its exclusive prefix sums
//                       and writes count[0] = the row's total.  It reads what launch 1 wrote, nothing of its own launch.
//   launch 3 (scatter)  as launch 1, then every survivor goes to row scratch[k][w] + (survivors before it in the workgroup)
//                       of the target's `out`, when that row is below `capacity`.  It reads what launch 2 wrote and writes
//                       `out` only.
// Within a launch no workgroup reads a word that another workgroup of that launch writes; the order between the launches is
// the stream's.  There is no flag, no atomic and no loop that waits.  Every (point, target) decision is made by crop_test, the
// one function that o3d_track_crop calls too, with no early rejection: rows and counts equal o3d_track_crop's.
// crop_test, gather_row, offset_box_one, inside_box, the keyed index draw and the workgroup bodies of the three launches
// (crop_multi_wg, crop_scan_row) live in track_common.hpp: csrc/train_batch.hip (o3d_track_crop_groups[_aug], o3d_train_sample)
// calls the same definitions.  motion_row is defined here, and so are its other callers, o3d_track_motion_input_drawn and
// o3d_train_motion_sample.
#include "track_common.hpp"

namespace {

struct CropTable {
    o3d_crop_job job[O3D_CROP_MAX_JOBS];
    int wg_start[O3D_CROP_MAX_JOBS + 1];       // first workgroup of job j; [n_jobs] = the grid
    int n_jobs;
};

// crop_test for point i of a job; `box` is J.box, which nothing writes during the launch
__device__ __forceinline__ bool crop_point(const o3d_crop_job& J, const float* __restrict__ box, int i, float& qx, float& qy, float& qz) {
    const float* p = J.points + 3 * (long)i;
    return crop_test(p[0], p[1], p[2], box, J.scale, J.offset, J.mode, qx, qy, qz);
}

__device__ __forceinline__ int crop_job_of(const CropTable& t, int wg) {
    int j = 0;
#pragma unroll
    for (int k = 1; k < O3D_CROP_MAX_JOBS; ++k)
        if (k < t.n_jobs && wg >= t.wg_start[k]) j = k;
    return j;
}

template <bool SCATTER>
__global__ __launch_bounds__(CROP_WG) void crop_kernel(CropTable t, int32_t* __restrict__ scratch) {
    __shared__ int wave_cnt[CROP_WG / 64];
    __shared__ int red[CROP_WG / 64];
    const int wg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = crop_job_of(t, wg);
    const o3d_crop_job& J = t.job[j];
    const int first = t.wg_start[j];
    const int i = (wg - first) * CROP_WG + tid;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    const bool keep = i < J.n && crop_point(J, J.box, i, qx, qy, qz);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    if (!SCATTER) {
        __syncthreads();
        if (tid == 0) scratch[wg] = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
        return;
    }
    // the survivors of the workgroups before this one in the job
    int part = 0;
    for (int k = first + tid; k < wg; k += CROP_WG) part += scratch[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off, 64);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    int base = (red[0] + red[1]) + (red[2] + red[3]);
    int total = base;
#pragma unroll
    for (int k = 0; k < CROP_WG / 64; ++k) {
        if (k < wave) base += wave_cnt[k];
        total += wave_cnt[k];
    }
    if (keep) {
        const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (pos < J.capacity) {
            float* o = J.out + 3 * (long)pos;
            o[0] = qx; o[1] = qy; o[2] = qz;
        }
    }
    if (tid == 0 && wg == t.wg_start[j + 1] - 1) J.count[0] = total;     // the job's last workgroup knows the count
}

__global__ __launch_bounds__(256) void resample_kernel(o3d_resample_job a, o3d_resample_job b) {
    const o3d_resample_job& J = blockIdx.y == 0 ? a : b;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= J.n) return;
    float x, y, z;
    gather_row(J.src, J.n_src, J.idx, i, J.zero, x, y, z);
    float* o = J.dst + 3 * (long)i;
    o[0] = x; o[1] = y; o[2] = z;
}

struct MotionInputArgs {
    const float* src[2]; int n_src[2]; int zero[2];      // [0] the previous crop, [1] the current crop
    const int32_t* idx; const float* wlh; int N, first_frame;
    float* points; float* bc;
};

// Row i of the motion input behind its gather, in the operation order of the header comment: (x, y, z) -> o (5) and bc (9) |
// NULL.  THE row arithmetic of both o3d_track_motion_input and o3d_track_motion_input_multi; wlh (3): the target's canonical box
__device__ __forceinline__ void motion_row(float x, float y, float z, int half, const float* wlh, int first_frame, float* o, float* bc) {
    o[0] = x; o[1] = y; o[2] = z;
    if (half) {
        o[3] = 0.1f; o[4] = 0.5f;
        if (bc) {
#pragma unroll
            for (int k = 0; k < 9; ++k) bc[k] = 0.f;
        }
        return;
    }
    const float w = wlh[0], l = wlh[1], h = wlh[2];
    const float hx = (l * 1.25f) * 0.5f, hy = (w * 1.25f) * 0.5f, hz = (h * 1.25f) * 0.5f;
    const bool inside = fabsf(x) <= hx && fabsf(y) <= hy && fabsf(z) <= hz;
    o[3] = 0.f;
    o[4] = first_frame ? (inside ? 1.f : 0.f) : (inside ? 0.8f : 0.2f);
    if (!bc) return;
    const float ca = l * 0.5f, cb = w * 0.5f, cc = h * 0.5f;
    bc[0] = sqrtf((x * x + y * y) + z * z);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float X = k < 4 ? ca : -ca;
        const float Y = ((k & 3) == 0 || (k & 3) == 3) ? cb : -cb;
        const float Z = (k & 2) ? -cc : cc;
        const float dx = x - X, dy = y - Y, dz = z - Z;
        bc[1 + k] = sqrtf((dx * dx + dy * dy) + dz * dz);
    }
}

__global__ __launch_bounds__(256) void motion_input_kernel(MotionInputArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * a.N) return;
    const int half = i >= a.N ? 1 : 0;
    float x, y, z;
    gather_row(a.src[half], a.n_src[half], a.idx, i, a.zero[half], x, y, z);
    motion_row(x, y, z, half, a.wlh, a.first_frame, a.points + 5 * (long)i, a.bc ? a.bc + 9 * (long)i : nullptr);
}

// ---- the free-running loop (tracking.py, sampling="device"): counts stay on the device, the indices are drawn here ---------------
// The two index sources of the free-running loop: draw_index(source, i, n, S) -> the row of a cloud of n rows that output row i of
// S reads, -1 (zero-fill) for n <= 2.  A key (unsigned): sample_index, always inside [0, n).  A table (sampling="table"): entry i
// of row n of a device table of cap + 1 rows of S int32 (tracking.draw_table: the reference's own draw for every count),
// whatever it holds.  The structs and row functions below are templates over the source's type
__device__ __forceinline__ int draw_index(unsigned key, int i, int n, int S) { return n > 2 ? sample_index(key, i, n, S) : -1; }
__device__ __forceinline__ int draw_index(const int32_t* table, int i, int n, int S) { return n > 2 ? table[(long)n * S + i] : -1; }
static bool draw_ok(unsigned) { return true; }                                        // host: a key is always a source,
static bool draw_ok(const int32_t* table) { return table != nullptr; }                // a table must be there

// One job of o3d_track_resample_drawn / _tabled: dst (S,3) resampled from the first min(n_dev[0], cap) rows of src by `draw`
template <class Draw>
struct DrawnJobT {
    const float* src; const int32_t* n_dev; int cap; Draw draw; float* dst; int S; int32_t* used;
};
using DrawnJob = DrawnJobT<unsigned>;
using TabledJob = DrawnJobT<const int32_t*>;

// resample_kernel with the count read from the device and the index drawn in place: reads n_dev and src, writes dst and used
// THE row of o3d_track_resample_drawn[_lanes] and o3d_track_resample_tabled[_lanes].  An index outside [0, n) (a table's entry
// only) leaves the row zero, as o3d_track_resample does; used receives it as read
template <class Draw>
__device__ __forceinline__ void resample_drawn_row(const DrawnJobT<Draw>& J, int i) {
    if (i >= J.S) return;
    const int n = min(J.n_dev[0], J.cap);
    const int s = draw_index(J.draw, i, n, J.S);
    float x, y, z;
    gather_row(J.src, n, &s, 0, s < 0, x, y, z);
    float* o = J.dst + 3 * (long)i;
    o[0] = x; o[1] = y; o[2] = z;
    if (J.used) J.used[i] = s;
}

__global__ __launch_bounds__(256) void resample_drawn_kernel(DrawnJob a, DrawnJob b) {
    resample_drawn_row(blockIdx.y == 0 ? a : b, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void resample_tabled_kernel(TabledJob a, TabledJob b) {
    resample_drawn_row(blockIdx.y == 0 ? a : b, blockIdx.x * 256 + threadIdx.x);
}

struct BankArgs {
    const float* crop; const int32_t* count; int crop_cap; float* bank; int bank_cap;
    const int32_t* state_in; int32_t* state_out; int rule, first, has_crop;
};

// The template bank's book-keeping as device state {fixed, total}: every thread reads state_in and count, thread 0 of
// workgroup 0 writes state_out (another two words: the tracker alternates two slots), so no workgroup reads a word that
// another one of the launch writes.  Thread i carries row i of the staged crop to row slot + i of the bank.  THE body of both
// o3d_track_bank_update and o3d_track_bank_update_lanes
__device__ __forceinline__ void bank_update_rows(const BankArgs& a, int i) {
    const int fixed = a.state_in[0], total = a.state_in[1];
    if (!a.has_crop) {                                     // rule `first` after frame 1: the template does not change
        if (i == 0) { a.state_out[0] = fixed; a.state_out[1] = total; }
        return;
    }
    const int nm = max(0, min(a.count[0], a.crop_cap));
    const bool twice = a.rule == O3D_BANK_FIRSTANDPREVIOUS && a.first;      // getModel([first, previous]) at t = 1
    const int slot = a.rule == O3D_BANK_ALL ? total : (a.rule == O3D_BANK_FIRSTANDPREVIOUS && !a.first) ? fixed : 0;
    if (i == 0) {
        a.state_out[0] = a.first ? nm : fixed;
        a.state_out[1] = min(twice ? 2 * nm : slot + nm, a.bank_cap);
    }
    if (i >= nm) return;
    const float* p = a.crop + 3 * (long)i;
    const float x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int copy = 0; copy < 2; ++copy) {
        const long r = (long)slot + i + (copy ? nm : 0);
        if ((copy == 0 || twice) && r >= 0 && r < a.bank_cap) {
            float* o = a.bank + 3 * r;
            o[0] = x; o[1] = y; o[2] = z;
        }
    }
}

__global__ __launch_bounds__(256) void bank_update_kernel(BankArgs a) { bank_update_rows(a, blockIdx.x * 256 + threadIdx.x); }

template <class Draw>
struct MotionDrawnArgsT {
    const float* src[2]; const int32_t* counts; int cap; Draw draw[2];      // [0] the previous crop, [1] the current crop
    const float* wlh; int N, first_frame;
    float* points; float* bc; int32_t* used;
};
using MotionDrawnArgs = MotionDrawnArgsT<unsigned>;
using MotionTabledArgs = MotionDrawnArgsT<const int32_t*>;

// motion_input_kernel with the two counts read from the device and the indices drawn in place: THE row of
// o3d_track_motion_input_drawn[_lanes] and o3d_track_motion_input_tabled[_lanes]
template <class Draw>
__device__ __forceinline__ void motion_drawn_row(const MotionDrawnArgsT<Draw>& a, int i) {
    if (i >= 2 * a.N) return;
    const int half = i >= a.N ? 1 : 0;
    const int n = min(a.counts[half], a.cap);
    const int s = draw_index(a.draw[half], i - half * a.N, n, a.N);
    float px, py, pz;
    gather_row(a.src[half], n, &s, 0, s < 0, px, py, pz);
    motion_row(px, py, pz, half, a.wlh, a.first_frame, a.points + 5 * (long)i, a.bc ? a.bc + 9 * (long)i : nullptr);
    if (a.used) a.used[i] = s;
}

__global__ __launch_bounds__(256) void motion_input_drawn_kernel(MotionDrawnArgs a) { motion_drawn_row(a, blockIdx.x * 256 + threadIdx.x); }

__global__ __launch_bounds__(256) void motion_input_tabled_kernel(MotionTabledArgs a) { motion_drawn_row(a, blockIdx.x * 256 + threadIdx.x); }

struct OffsetArgs {
    const float* ref; const float* offset; float* yaw_state; float* out; float* results; int32_t* frame;
    int T, degrees, use_z, limit_box, rebase, seed;
};

// one thread of the launch's 64 works
__global__ void offset_box_kernel(OffsetArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int k = a.frame ? a.frame[0] : 0;
    float box[15];
    offset_box_one(a.ref, a.offset, a.yaw_state, a.rebase, a.degrees, a.use_z, a.limit_box, (unsigned)a.seed, (unsigned)k, box);
    for (int i = 0; i < 15; ++i) {
        if (a.out) a.out[i] = box[i];
        if (a.results && k >= 0 && k < a.T) a.results[15 * (long)k + i] = box[i];
    }
    if (a.frame) a.frame[0] = k + 1;
}

// ---- L lanes per launch (tracking.LaneTracker / MotionLaneTracker: the test epoch, one tracklet per lane) ---------------------------
// A lane is a leading axis of every buffer; what changes per step and lane is row l of `lanes` (L, O3D_LANE_COLS) int32:
// {active, first, has_crop, t, row, ref_row, rebase}.  Every kernel below hands lane l's operands to the device function of
// the single form, so lane l's rows are that entry point's, bit for bit.
struct BankLanesArgs {
    const float* crop; const int32_t* counts; int count_stride, crop_cap; float* bank; int bank_cap, rule;
    const int32_t* lanes; const int32_t* state_in; int32_t* state_out;
};

// blockIdx.y = the lane; an inactive lane and a lane without a crop take bank_update_rows' copy-through path
__global__ __launch_bounds__(256) void bank_update_lanes_kernel(BankLanesArgs a) {
    const long l = blockIdx.y;
    const int32_t* f = a.lanes + O3D_LANE_COLS * l;
    const BankArgs b{a.crop + 3 * l * a.crop_cap, a.counts + l * a.count_stride, a.crop_cap, a.bank + 3 * l * a.bank_cap, a.bank_cap,
                     a.state_in + 2 * l, a.state_out + 2 * l, a.rule, f[O3D_LANE_FIRST] != 0,
                     f[O3D_LANE_ACTIVE] != 0 && f[O3D_LANE_HAS_CROP] != 0};
    bank_update_rows(b, blockIdx.x * 256 + threadIdx.x);
}

// one cloud of o3d_track_resample_drawn_lanes / o3d_track_resample_tabled_lanes: lane l reads src + 3 l cap and n_dev[l stride],
// writes dst + 3 l S and used + l S; the index source is the same for every lane
template <class Draw>
struct DrawnLanesT {
    const float* src; const int32_t* n_dev; int stride, cap; Draw draw; float* dst; int S; int32_t* used;
};
using DrawnLanes = DrawnLanesT<unsigned>;
using TabledLanes = DrawnLanesT<const int32_t*>;

// blockIdx.y = the cloud, blockIdx.z = the lane.  (The two lane kernels of a form hold the same statements: written out in each
// kernel, the cloud is chosen by the ADDRESS of its kernel argument; behind a shared function the compiler loads both clouds.)
__global__ __launch_bounds__(256) void resample_drawn_lanes_kernel(DrawnLanes a, DrawnLanes b) {
    const DrawnLanes& C = blockIdx.y == 0 ? a : b;
    const long l = blockIdx.z;
    const DrawnJob J{C.src + 3 * l * C.cap, C.n_dev + l * C.stride, C.cap, C.draw, C.dst + 3 * l * C.S, C.S, C.used ? C.used + l * C.S : nullptr};
    resample_drawn_row(J, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void resample_tabled_lanes_kernel(TabledLanes a, TabledLanes b) {
    const TabledLanes& C = blockIdx.y == 0 ? a : b;
    const long l = blockIdx.z;
    const TabledJob J{C.src + 3 * l * C.cap, C.n_dev + l * C.stride, C.cap, C.draw, C.dst + 3 * l * C.S, C.S, C.used ? C.used + l * C.S : nullptr};
    resample_drawn_row(J, blockIdx.x * 256 + threadIdx.x);
}

// blockIdx.y = the lane: a.src / counts / wlh / points / bc / used are the (L, ...) buffers, lane l's arguments are cut out here
__global__ __launch_bounds__(256) void motion_input_drawn_lanes_kernel(MotionDrawnArgs a, const int32_t* __restrict__ lanes) {
    const long l = blockIdx.y, rows = 2 * (long)a.N;
    const MotionDrawnArgs m{{a.src[0] + 3 * l * a.cap, a.src[1] + 3 * l * a.cap}, a.counts + 2 * l, a.cap, {a.draw[0], a.draw[1]}, a.wlh + 3 * l,
                            a.N, lanes[O3D_LANE_COLS * l + O3D_LANE_FIRST] != 0, a.points + 5 * l * rows, a.bc ? a.bc + 9 * l * rows : nullptr,
                            a.used ? a.used + l * rows : nullptr};
    motion_drawn_row(m, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void motion_input_tabled_lanes_kernel(MotionTabledArgs a, const int32_t* __restrict__ lanes) {
    const long l = blockIdx.y, rows = 2 * (long)a.N;
    const MotionTabledArgs m{{a.src[0] + 3 * l * a.cap, a.src[1] + 3 * l * a.cap}, a.counts + 2 * l, a.cap, {a.draw[0], a.draw[1]}, a.wlh + 3 * l,
                             a.N, lanes[O3D_LANE_COLS * l + O3D_LANE_FIRST] != 0, a.points + 5 * l * rows, a.bc ? a.bc + 9 * l * rows : nullptr,
                             a.used ? a.used + l * rows : nullptr};
    motion_drawn_row(m, blockIdx.x * 256 + threadIdx.x);
}

struct OffsetLanesArgs {
    const float* cur; const float* gt; const float* offset; float* yaw_state; const int32_t* lanes; float* out; float* results;
    const int32_t* counts; int32_t* counts_log;
    int L, R, degrees, use_z, limit_box, seed;
};

// One thread per lane.  Thread l reads cur[l] (or a row of gt, which nothing writes), offset[l], yaw_state[l], counts[l] and
// writes out[l] (which may be cur[l]: its own row), yaw_state[l] and row[l] of results / counts_log (a row belongs to one
// tracklet, a tracklet to one lane): no thread reads what another one writes.
__global__ __launch_bounds__(256) void offset_box_lanes_kernel(OffsetLanesArgs a) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= a.L) return;
    const int32_t* f = a.lanes + O3D_LANE_COLS * (long)l;
    const int ref_row = f[O3D_LANE_REF_ROW], row = f[O3D_LANE_ROW];
    if (!f[O3D_LANE_ACTIVE] || ref_row < -1 || ref_row >= a.R) return;
    const float* ref = ref_row >= 0 ? a.gt + 15 * (long)ref_row : a.cur + 15 * (long)l;
    float box[15];
    offset_box_one(ref, a.offset + 4 * (long)l, a.yaw_state + 10 * (long)l, f[O3D_LANE_REBASE] != 0, a.degrees, a.use_z, a.limit_box,
                   (unsigned)a.seed, (unsigned)f[O3D_LANE_T], box);
    const bool logged = row >= 0 && row < a.R;
    for (int i = 0; i < 15; ++i) {
        a.out[15 * (long)l + i] = box[i];
        if (logged) a.results[15 * (long)row + i] = box[i];
    }
    if (logged && a.counts_log) {                          // the frame's record: what the crops counted, -1 where none was made
        a.counts_log[2 * (long)row] = a.counts[2 * (long)l];
        a.counts_log[2 * (long)row + 1] = f[O3D_LANE_HAS_CROP] ? a.counts[2 * (long)l + 1] : -1;
    }
}

// One thread per lane: a lane that starts a tracklet (active and first) takes the tracklet's first ground-truth box, row
// row[l] - t[l] of gt, as its current box, restarts its yaw state from that rotation, takes its wlh as the canonical box and
// empties its template bank (state (L,2) | NULL = {fixed, total}, the slot that the step's bank update reads)
__global__ __launch_bounds__(256) void lane_start_kernel(const float* __restrict__ gt, int R, const int32_t* __restrict__ lanes, int L,
                                                         float* __restrict__ cur, float* __restrict__ yaw_state, float* __restrict__ wlh,
                                                         int32_t* __restrict__ state) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const int32_t* f = lanes + O3D_LANE_COLS * (long)l;
    const long row0 = (long)f[O3D_LANE_ROW] - f[O3D_LANE_T];
    if (!f[O3D_LANE_ACTIVE] || !f[O3D_LANE_FIRST] || row0 < 0 || row0 >= R) return;
    const float* b = gt + 15 * row0;
    for (int i = 0; i < 15; ++i) cur[15 * (long)l + i] = b[i];
    for (int i = 0; i < 9; ++i) yaw_state[10 * (long)l + i] = b[6 + i];
    yaw_state[10 * (long)l + 9] = 0.f;
    for (int i = 0; i < 3; ++i) wlh[3 * (long)l + i] = b[3 + i];
    if (state) { state[2 * (long)l] = 0; state[2 * (long)l + 1] = 0; }
}

// ---- K targets per launch ------------------------------------------------------------------------------------------------------

struct CropMultiTable {
    const float* points[2]; const o3d_crop_target* targets[2];
    int n[2], K[2], wgs[2];                    // wgs: workgroups of 256 points of the group (1 for an empty cloud)
    long sbase[2];                             // the group's first word in scratch
    int n_groups;
};

template <bool SCATTER>
__global__ __launch_bounds__(CROP_WG) void crop_multi_kernel(CropMultiTable t, int32_t* __restrict__ scratch) {
    const int g = (t.n_groups > 1 && (int)blockIdx.x >= t.wgs[0]) ? 1 : 0;
    const int w = (int)blockIdx.x - (g ? t.wgs[0] : 0);
    crop_multi_wg<SCATTER>(t.points[g], t.n[g], t.targets[g], t.K[g], t.wgs[g], scratch + t.sbase[g], w);
}

// one workgroup per (group, target): its row of W counts -> exclusive prefix sums in place, count[0] = the total
__global__ __launch_bounds__(CROP_WG) void crop_multi_scan_kernel(CropMultiTable t, int32_t* __restrict__ scratch) {
    const int g = (t.n_groups > 1 && (int)blockIdx.x >= t.K[0]) ? 1 : 0;
    const int k = (int)blockIdx.x - (g ? t.K[0] : 0);
    crop_scan_row(scratch + t.sbase[g] + (long)k * t.wgs[g], t.wgs[g], t.targets[g][k].count);
}

// resample_kernel's rows for a DEVICE table of jobs: blockIdx.x = the job, its rows strided over blockIdx.y and the threads
__global__ __launch_bounds__(256) void resample_multi_kernel(const o3d_resample_job* __restrict__ jobs) {
    const o3d_resample_job J = jobs[blockIdx.x];
    for (int i = blockIdx.y * 256 + threadIdx.x; i < J.n; i += gridDim.y * 256) {
        float x, y, z;
        gather_row(J.src, J.n_src, J.idx, i, J.zero || !J.src || !J.idx, x, y, z);      // the host cannot check a device table
        float* o = J.dst + 3 * (long)i;
        o[0] = x; o[1] = y; o[2] = z;
    }
}

struct OffsetMultiArgs {
    const float* ref; const float* offset; float* yaw_state; const int32_t* rebase; const int32_t* active;
    float* out; float* results; int32_t* frame;
    int K, T, degrees, use_z, limit_box, seed;
};

// ONE workgroup: every thread reads the shared frame counter before thread 0 advances it
__global__ __launch_bounds__(256) void offset_box_multi_kernel(OffsetMultiArgs a) {
    const int k = a.frame ? a.frame[0] : 0;
    __syncthreads();
    for (int j = threadIdx.x; j < a.K; j += 256) {
        const float* ref = a.ref + 15 * (long)j;
        float box[15];
        if (a.active && !a.active[j]) {
            for (int i = 0; i < 15; ++i) box[i] = ref[i];
        } else {
            offset_box_one(ref, a.offset + 4 * (long)j, a.yaw_state ? a.yaw_state + 10 * (long)j : nullptr,
                           a.rebase ? a.rebase[j] != 0 : 0, a.degrees, a.use_z, a.limit_box, (unsigned)a.seed + (unsigned)j,
                           (unsigned)k, box);
        }
        for (int i = 0; i < 15; ++i) {
            if (a.out) a.out[15 * (long)j + i] = box[i];
            if (a.results && k >= 0 && k < a.T) a.results[15 * ((long)k * a.K + j) + i] = box[i];
        }
    }
    if (a.frame && threadIdx.x == 0) a.frame[0] = k + 1;
}

// motion_input_kernel for a DEVICE table of K jobs: blockIdx.y = the target, whose rows are rows [k * 2N, (k + 1) * 2N) of
// points / bc and whose canonical box is wlh + 3 k
static_assert(sizeof(o3d_motion_job) == 48, "o3d_motion_job: points_utils.MOTION_JOB mirrors this layout");
__global__ __launch_bounds__(256) void motion_input_multi_kernel(const o3d_motion_job* __restrict__ jobs, int N, const float* __restrict__ wlh,
                                                                 int first_frame, float* __restrict__ points, float* __restrict__ bc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * N) return;
    const int k = blockIdx.y;
    const o3d_motion_job J = jobs[k];
    const int half = i >= N ? 1 : 0;
    const float* src = half ? J.cur : J.prev;
    float x, y, z;
    gather_row(src, half ? J.n_this : J.n_prev, J.idx, i, (half ? J.zero_this : J.zero_prev) || !src || !J.idx, x, y, z);      // the host cannot check a device table
    const long row = (long)k * (2 * (long)N) + i;
    motion_row(x, y, z, half, wlh + 3 * (long)k, first_frame, points + 5 * row, bc ? bc + 9 * row : nullptr);
}

static_assert(sizeof(o3d_train_motion_sample_args) == 248, "o3d_train_motion_sample_args: points_utils._TrainMotionSampleArgs mirrors this layout");
// ---- o3d_train_motion_sample (the training-batch form of the motion input, sampler.MotionBatchBuilder: it lives here, beside
// motion_row, so that the row arithmetic keeps its one definition; the draw and inside_box are track_common.hpp's) -----------------
__global__ __launch_bounds__(256) void train_motion_sample_kernel(o3d_train_motion_sample_args a) {
    const int r = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int N = a.N, B = a.B;
    const int j = a.sel[r];
    const bool live = j >= 0 && j < a.J;
    if (blockIdx.x == 0) {                                 // the rows of the per-candidate labels that the batch takes
        for (int e = threadIdx.x; e < 46; e += 256) {
            if (e < 4) a.box_label[4 * (long)r + e] = live ? a.cand_box_label[4 * (long)j + e] : 0.f;
            else if (e < 8) a.box_label_prev[4 * (long)r + (e - 4)] = live ? a.cand_box_label_prev[4 * (long)j + (e - 4)] : 0.f;
            else if (e < 12) a.motion_label[4 * (long)r + (e - 8)] = live ? a.cand_motion_label[4 * (long)j + (e - 8)] : 0.f;
            else if (e < 15) a.bbox_size[3 * (long)r + (e - 12)] = live ? a.cand_bbox_size[3 * (long)j + (e - 12)] : 0.f;
            else if (e == 15) a.motion_state_label[r] = live ? (int64_t)a.cand_motion_state[j] : 0;
            else if (a.bc_boxes) {
                const int which = e < 31 ? 0 : 1, f = e - (which ? 31 : 16);      // f: the field of the (15) box
                const float v = live ? (which ? a.this_box : a.prev_box)[15 * (long)j + f] : 0.f;
                float* o = a.bc_boxes + (long)which * 15 * B;
                if (f < 3) o[3 * (long)r + f] = v;
                else if (f < 6) o[3 * (long)B + 3 * (long)r + (f - 3)] = v;
                else o[6 * (long)B + 9 * (long)r + (f - 6)] = v;
            }
        }
    }
    if (i >= 2 * N) return;
    const int half = i >= N ? 1 : 0, ih = i - half * N;
    const long row = (long)r * (2 * (long)N) + i;
    float* o = a.points + 5 * row;
    float* bc = a.candidate_bc ? a.candidate_bc + 9 * row : nullptr;
    float* xyz = a.xyz_halves ? a.xyz_halves + 3 * (((long)half * B + r) * N + ih) : nullptr;
    int32_t* used = half ? a.used_this : a.used_prev;
    if (!live) {
        for (int e = 0; e < 5; ++e) o[e] = 0.f;
        if (bc) for (int e = 0; e < 9; ++e) bc[e] = 0.f;
        if (xyz) { xyz[0] = 0.f; xyz[1] = 0.f; xyz[2] = 0.f; }
        a.seg_label[row] = 0;
        if (used) used[(long)r * N + ih] = -1;
        return;
    }
    const int cap = half ? a.cap_this : a.cap_prev;
    const int n = min(a.counts[3 * (long)j + 1 + half], cap);
    int s = -1;
    if (n > 2) {
        const int32_t* given = half ? a.idx_this : a.idx_prev;
        if (given) {
            s = given[(long)j * N + ih];
        } else {
            const unsigned key = mix32((a.seed * 0x9E3779B1u) ^
                                       (a.counter * 0x85EBCA77u + (unsigned)j * 0xC2B2AE3Du + (unsigned)half * 0x27D4EB2Fu + 0x165667B1u));
            s = sample_index(key, ih, n, N);
        }
        if ((unsigned)s >= (unsigned)n) s = -1;
    }
    const float* src = (half ? a.crop_this : a.crop_prev) + 3 * (long)j * cap;
    float px, py, pz;
    gather_row(src, n, &s, 0, s < 0, px, py, pz);
    motion_row(px, py, pz, half, a.canon_box + 15 * (long)j + 3, a.candidate_id[j] == 0, o, bc);
    if (xyz) { xyz[0] = px; xyz[1] = py; xyz[2] = pz; }
    float dx, dy, dz;
    a.seg_label[row] = inside_box(px, py, pz, (half ? a.this_box : a.prev_box) + 15 * (long)j, 1.25f, dx, dy, dz) ? 1 : 0;
    if (used) used[(long)r * N + ih] = s;
}

}  // namespace

extern "C" long o3d_track_crop_scratch(const o3d_crop_job* jobs, int n_jobs) {
    if (!jobs || n_jobs < 1 || n_jobs > O3D_CROP_MAX_JOBS) return -1;
    long wgs = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (jobs[j].n < 0) return -1;
        wgs += crop_wgs(jobs[j].n);
    }
    return wgs;
}

// jobs: a HOST table of n_jobs (1..O3D_CROP_MAX_JOBS) jobs; scratch: scratch_len >= o3d_track_crop_scratch(jobs, n_jobs) int32
// on the device.  A job with n == 0 writes count = 0.
extern "C" int o3d_track_crop(const o3d_crop_job* jobs, int n_jobs, int32_t* scratch, int scratch_len, void* stream) {
    if (!jobs || n_jobs < 1 || n_jobs > O3D_CROP_MAX_JOBS || !scratch) return O3D_EINVAL;
    CropTable t;
    t.n_jobs = n_jobs;
    long wgs = 0;
    for (int j = 0; j < O3D_CROP_MAX_JOBS; ++j) {
        t.wg_start[j] = (int)wgs;
        if (j >= n_jobs) { t.job[j] = o3d_crop_job{}; continue; }
        const o3d_crop_job& J = jobs[j];
        if (J.n < 0 || J.n > (1 << 30) || J.capacity < 0 || !J.box || !J.count || (J.n > 0 && !J.points) || (J.capacity > 0 && !J.out) ||
            (J.mode != O3D_CROP_SUBWINDOW && J.mode != O3D_CROP_MODEL) || !(J.scale >= 0.f) || !(J.offset >= 0.f))
            return O3D_EINVAL;
        t.job[j] = J;
        wgs += crop_wgs(J.n);
    }
    t.wg_start[O3D_CROP_MAX_JOBS] = (int)wgs;
    for (int j = n_jobs; j < O3D_CROP_MAX_JOBS; ++j) t.wg_start[j] = (int)wgs;
    if (wgs > scratch_len) return O3D_EINVAL;
    hipLaunchKernelGGL(crop_kernel<false>, dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), t, scratch);
    hipLaunchKernelGGL(crop_kernel<true>, dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), t, scratch);
    return o3d_launch_status();
}

// dst[i] = src[idx[i]] (rows of 3 floats) for n_jobs (1 or 2) HOST jobs in one launch; a job with `zero` set fills dst with
// zeros instead (regularize_pc's `num_points <= 2` case) and needs neither src nor idx
extern "C" int o3d_track_resample(const o3d_resample_job* jobs, int n_jobs, void* stream) {
    if (!jobs || n_jobs < 1 || n_jobs > 2) return O3D_EINVAL;
    int nmax = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const o3d_resample_job& J = jobs[j];
        if (J.n < 0 || J.n_src < 0 || (J.n > 0 && !J.dst) || (J.n > 0 && !J.zero && (!J.src || !J.idx || J.n_src < 1))) return O3D_EINVAL;
        nmax = J.n > nmax ? J.n : nmax;
    }
    if (nmax == 0) return O3D_OK;
    hipLaunchKernelGGL(resample_kernel, dim3(o3d_cdiv(nmax, 256), n_jobs), dim3(256), 0, o3d_stream(stream), jobs[0], jobs[n_jobs - 1]);
    return o3d_launch_status();
}

// getOffsetBB on the device.  ref (15): the reference box; offset (4) = x, y, z, theta in ref's frame (o3d_best_proposal's
// output row); out (15) | NULL: the new box; results (T,15) | NULL with frame (1) int32 | NULL: the new box is also written to
// row frame[0] (when < T) and frame[0] is incremented -- the host never reads the box.
//   centre' = c + R (ox, oy, use_z ? oz : 0),   R' = R Rz(theta),   wlh unchanged
// yaw_state (10) | NULL = R0 (9) and the yaw accumulated since: with it (and rebase == 0) the orientation of `ref` is taken as
// R0 Rz(yaw) and the new one is R0 Rz(yaw + theta), one product from an orthonormal R0 however long the chain; rebase != 0
// restarts the state from ref (R0 = ref's rotation, yaw = theta).  limit_box mirrors datasets/points_utils.py:70-76 literally:
// `offset[0] > w`, `offset[1] > min(l, 2)` replace the component by a draw from U[-1, 1), `use_z and offset[2] > h` sets it
// to 0 (no abs).  The reference's draw is the unseeded global numpy generator, so there is nothing to reproduce: the draw here
// is a counter-based hash of (seed, frame[0], component), the same for the same three numbers.
extern "C" int o3d_track_offset_box(const float* ref, const float* offset, float* yaw_state, int rebase, int degrees, int use_z,
                                    int limit_box, int seed, float* out, float* results, int T, int32_t* frame, void* stream) {
    if (!ref || !offset || (!out && !results) || T < 0 || (results && (!frame || T < 1))) return O3D_EINVAL;
    OffsetArgs a{ref, offset, yaw_state, out, results, frame, T, degrees, use_z, limit_box, rebase, seed};
    hipLaunchKernelGGL(offset_box_kernel, dim3(1), dim3(64), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

// The network input of the motion tracker in one launch (MotionBaseModel.build_input_dict behind its two crops).  prev
// (n_prev,3) / cur (n_this,3): the crops of the previous and the current frame in the frame of the reference box; idx (2N):
// row i < N gathers prev[idx[i]], row i >= N gathers cur[idx[i]]; zero_prev / zero_this: that half is zero-filled instead
// (regularize_pc with <= 2 points) and needs neither its crop nor idx; wlh (3, device): the canonical box.  points (2N,5) and
// candidate_bc (2N,9) | NULL (box_aware=False) are written as the header of this file states.
extern "C" int o3d_track_motion_input(const float* prev, int n_prev, const float* cur, int n_this, const int32_t* idx, int N,
                                      int zero_prev, int zero_this, const float* wlh, int first_frame, float* points,
                                      float* candidate_bc, void* stream) {
    if (N < 0 || N > (1 << 29) || n_prev < 0 || n_this < 0 || !wlh || !points) return O3D_EINVAL;
    if (!zero_prev && (!prev || n_prev < 1 || !idx)) return O3D_EINVAL;
    if (!zero_this && (!cur || n_this < 1 || !idx)) return O3D_EINVAL;
    if (N == 0) return O3D_OK;
    MotionInputArgs a{{prev, cur}, {n_prev, n_this}, {zero_prev != 0, zero_this != 0}, idx, wlh, N, first_frame != 0, points, candidate_bc};
    hipLaunchKernelGGL(motion_input_kernel, dim3(o3d_cdiv(2 * N, 256)), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

// ---- the free-running loop: no count and no index ever crosses to the host (include/o3dsot.h states the contracts) ---------------
// One host launcher per launch form, a template over the index source like the kernels: (unsigned)key for the _drawn entry point of
// a form, a table (cap + 1, S) int32 for its _tabled one (tracking.py, sampling="table").  Job: DrawnJobT or DrawnLanesT
template <class Job>
static bool drawn_job_ok(const Job& j) {
    return j.src && j.n_dev && draw_ok(j.draw) && j.dst && j.cap >= 1 && j.cap <= (1 << 29) && j.S >= 1 && j.S <= (1 << 20);
}

template <class Draw, class Job = DrawnJobT<Draw>>      // job1 is read when n_jobs == 2 only
static int launch_resample_drawn(void (*kernel)(Job, Job), const Job& a, const Job& job1, int n_jobs, void* stream) {
    if (n_jobs < 1 || n_jobs > 2 || !drawn_job_ok(a) || (n_jobs == 2 && !drawn_job_ok(job1))) return O3D_EINVAL;
    const Job& b = n_jobs == 2 ? job1 : a;
    hipLaunchKernelGGL(kernel, dim3(o3d_cdiv(a.S > b.S ? a.S : b.S, 256), n_jobs), dim3(256), 0, o3d_stream(stream), a, b);
    return o3d_launch_status();
}

template <class Args>      // MotionDrawnArgsT, either source
static bool motion_drawn_ok(const Args& a) {
    return a.src[0] && a.src[1] && a.counts && draw_ok(a.draw[0]) && draw_ok(a.draw[1]) && a.wlh && a.points && a.cap >= 1 &&
           a.cap <= (1 << 29) && a.N >= 1 && a.N <= (1 << 20);
}

template <class Draw, class Args = MotionDrawnArgsT<Draw>>
static int launch_motion_drawn(void (*kernel)(Args), const Args& a, void* stream) {
    if (!motion_drawn_ok(a)) return O3D_EINVAL;
    hipLaunchKernelGGL(kernel, dim3(o3d_cdiv(2 * a.N, 256)), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_track_resample_drawn(const float* src0, const int32_t* n_dev0, int cap0, int key0, float* dst0, int S0, int32_t* used0,
                                        const float* src1, const int32_t* n_dev1, int cap1, int key1, float* dst1, int S1, int32_t* used1,
                                        int n_jobs, void* stream) {
    return launch_resample_drawn<unsigned>(resample_drawn_kernel, {src0, n_dev0, cap0, (unsigned)key0, dst0, S0, used0},
                                           {src1, n_dev1, cap1, (unsigned)key1, dst1, S1, used1}, n_jobs, stream);
}

extern "C" int o3d_track_resample_tabled(const float* src0, const int32_t* n_dev0, int cap0, const int32_t* table0, float* dst0, int S0,
                                         int32_t* used0, const float* src1, const int32_t* n_dev1, int cap1, const int32_t* table1,
                                         float* dst1, int S1, int32_t* used1, int n_jobs, void* stream) {
    return launch_resample_drawn<const int32_t*>(resample_tabled_kernel, {src0, n_dev0, cap0, table0, dst0, S0, used0},
                                                 {src1, n_dev1, cap1, table1, dst1, S1, used1}, n_jobs, stream);
}

extern "C" int o3d_track_bank_update(const float* crop, const int32_t* count, int crop_cap, float* bank, int bank_cap, int rule, int first,
                                     int has_crop, const int32_t* state_in, int32_t* state_out, void* stream) {
    if (!crop || !count || !bank || !state_in || !state_out || state_in == state_out || crop_cap < 1 || crop_cap > (1 << 29) ||
        bank_cap < 1 || bank_cap > (1 << 29) || rule < O3D_BANK_FIRST || rule > O3D_BANK_ALL)
        return O3D_EINVAL;
    const BankArgs a{crop, count, crop_cap, bank, bank_cap, state_in, state_out, rule, first != 0, has_crop != 0};
    hipLaunchKernelGGL(bank_update_kernel, dim3(has_crop ? o3d_cdiv(crop_cap, 256) : 1), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_track_motion_input_drawn(const float* prev, const float* cur, const int32_t* counts, int capacity, int key_prev,
                                            int key_this, int N, const float* wlh, int first_frame, float* points, float* candidate_bc,
                                            int32_t* used, void* stream) {
    return launch_motion_drawn<unsigned>(motion_input_drawn_kernel, {{prev, cur}, counts, capacity, {(unsigned)key_prev, (unsigned)key_this},
                                         wlh, N, first_frame != 0, points, candidate_bc, used}, stream);
}

extern "C" int o3d_track_motion_input_tabled(const float* prev, const float* cur, const int32_t* counts, int capacity, const int32_t* table,
                                             int N, const float* wlh, int first_frame, float* points, float* candidate_bc, int32_t* used,
                                             void* stream) {      // one table for both halves
    return launch_motion_drawn<const int32_t*>(motion_input_tabled_kernel, {{prev, cur}, counts, capacity, {table, table}, wlh, N,
                                               first_frame != 0, points, candidate_bc, used}, stream);
}

// ---- L lanes per launch: validation first, the contracts are include/o3dsot.h's ------------------------------------------------------
static bool lanes_ok(const int32_t* lanes, int L) { return lanes && L >= 1 && L <= O3D_CROP_MULTI_MAX_TARGETS; }

extern "C" int o3d_track_bank_update_lanes(const float* crop, const int32_t* counts, int count_stride, int crop_cap, float* bank, int bank_cap,
                                           int rule, const int32_t* lanes, int L, const int32_t* state_in, int32_t* state_out, void* stream) {
    if (!crop || !counts || !bank || !state_in || !state_out || state_in == state_out || !lanes_ok(lanes, L) || count_stride < 1 ||
        crop_cap < 1 || crop_cap > (1 << 29) || bank_cap < 1 || bank_cap > (1 << 29) || rule < O3D_BANK_FIRST || rule > O3D_BANK_ALL)
        return O3D_EINVAL;
    const BankLanesArgs a{crop, counts, count_stride, crop_cap, bank, bank_cap, rule, lanes, state_in, state_out};
    hipLaunchKernelGGL(bank_update_lanes_kernel, dim3(o3d_cdiv(crop_cap, 256), L), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

template <class Draw, class Job = DrawnLanesT<Draw>>
static int launch_resample_drawn_lanes(void (*kernel)(Job, Job), const Job& a, const Job& b, int L, void* stream) {
    if (L < 1 || L > O3D_CROP_MULTI_MAX_TARGETS || a.stride < 1 || b.stride < 1 || !drawn_job_ok(a) || !drawn_job_ok(b)) return O3D_EINVAL;
    hipLaunchKernelGGL(kernel, dim3(o3d_cdiv(a.S > b.S ? a.S : b.S, 256), 2, L), dim3(256), 0, o3d_stream(stream), a, b);
    return o3d_launch_status();
}

template <class Draw, class Args = MotionDrawnArgsT<Draw>>
static int launch_motion_drawn_lanes(void (*kernel)(Args, const int32_t*), const Args& a, const int32_t* lanes, int L, void* stream) {
    if (!motion_drawn_ok(a) || !lanes_ok(lanes, L)) return O3D_EINVAL;
    hipLaunchKernelGGL(kernel, dim3(o3d_cdiv(2 * a.N, 256), L), dim3(256), 0, o3d_stream(stream), a, lanes);
    return o3d_launch_status();
}

extern "C" int o3d_track_resample_drawn_lanes(const float* src0, const int32_t* n_dev0, int stride0, int cap0, int key0, float* dst0, int S0,
                                              int32_t* used0, const float* src1, const int32_t* n_dev1, int stride1, int cap1, int key1,
                                              float* dst1, int S1, int32_t* used1, int L, void* stream) {
    return launch_resample_drawn_lanes<unsigned>(resample_drawn_lanes_kernel, {src0, n_dev0, stride0, cap0, (unsigned)key0, dst0, S0, used0},
                                                 {src1, n_dev1, stride1, cap1, (unsigned)key1, dst1, S1, used1}, L, stream);
}

extern "C" int o3d_track_resample_tabled_lanes(const float* src0, const int32_t* n_dev0, int stride0, int cap0, const int32_t* table0,
                                               float* dst0, int S0, int32_t* used0, const float* src1, const int32_t* n_dev1, int stride1,
                                               int cap1, const int32_t* table1, float* dst1, int S1, int32_t* used1, int L, void* stream) {
    return launch_resample_drawn_lanes<const int32_t*>(resample_tabled_lanes_kernel, {src0, n_dev0, stride0, cap0, table0, dst0, S0, used0},
                                                       {src1, n_dev1, stride1, cap1, table1, dst1, S1, used1}, L, stream);
}

extern "C" int o3d_track_motion_input_drawn_lanes(const float* prev, const float* cur, const int32_t* counts, int capacity, int key_prev,
                                                  int key_this, int N, const float* wlh, const int32_t* lanes, int L, float* points,
                                                  float* candidate_bc, int32_t* used, void* stream) {      // first_frame is the lane's
    return launch_motion_drawn_lanes<unsigned>(motion_input_drawn_lanes_kernel, {{prev, cur}, counts, capacity,
                                               {(unsigned)key_prev, (unsigned)key_this}, wlh, N, 0, points, candidate_bc, used}, lanes, L, stream);
}

extern "C" int o3d_track_motion_input_tabled_lanes(const float* prev, const float* cur, const int32_t* counts, int capacity,
                                                   const int32_t* table, int N, const float* wlh, const int32_t* lanes, int L, float* points,
                                                   float* candidate_bc, int32_t* used, void* stream) {
    return launch_motion_drawn_lanes<const int32_t*>(motion_input_tabled_lanes_kernel, {{prev, cur}, counts, capacity, {table, table}, wlh, N,
                                                     0, points, candidate_bc, used}, lanes, L, stream);
}

extern "C" int o3d_track_offset_box_lanes(const float* cur, const float* gt, int R, const float* offset, float* yaw_state, const int32_t* lanes,
                                          int L, int degrees, int use_z, int limit_box, int seed, float* out, float* results,
                                          const int32_t* counts, int32_t* counts_log, void* stream) {
    if (!cur || !gt || !offset || !yaw_state || !out || !results || !lanes_ok(lanes, L) || R < 1 || R > (1 << 26) || seed < 0 ||
        (counts_log && !counts))
        return O3D_EINVAL;
    const OffsetLanesArgs a{cur, gt, offset, yaw_state, lanes, out, results, counts, counts_log, L, R, degrees, use_z, limit_box, seed};
    hipLaunchKernelGGL(offset_box_lanes_kernel, dim3(o3d_cdiv(L, 256)), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_track_lane_start(const float* gt, int R, const int32_t* lanes, int L, float* cur, float* yaw_state, float* wlh,
                                    int32_t* state, void* stream) {
    if (!gt || !cur || !yaw_state || !wlh || !lanes_ok(lanes, L) || R < 1 || R > (1 << 26)) return O3D_EINVAL;
    hipLaunchKernelGGL(lane_start_kernel, dim3(o3d_cdiv(L, 256)), dim3(256), 0, o3d_stream(stream), gt, R, lanes, L, cur, yaw_state, wlh, state);
    return o3d_launch_status();
}

// ---- K targets per launch ------------------------------------------------------------------------------------------------------
static bool crop_multi_table(const o3d_crop_group* groups, int n_groups, CropMultiTable& t, long& need) {
    if (!groups || n_groups < 1 || n_groups > 2) return false;
    t = CropMultiTable{};
    t.n_groups = n_groups;
    need = 0;
    for (int g = 0; g < n_groups; ++g) {
        const o3d_crop_group& G = groups[g];
        if (G.n < 0 || G.n > (1 << 30) || (G.n > 0 && !G.points) || !G.targets || G.n_targets < 1 ||
            G.n_targets > O3D_CROP_MULTI_MAX_TARGETS)
            return false;
        t.points[g] = G.points; t.targets[g] = G.targets; t.n[g] = G.n; t.K[g] = G.n_targets;
        t.wgs[g] = crop_wgs(G.n);
        t.sbase[g] = need;
        need += (long)t.wgs[g] * G.n_targets;
    }
    return true;
}

extern "C" long o3d_track_crop_multi_scratch(const o3d_crop_group* groups, int n_groups) {
    CropMultiTable t;
    long need;
    return crop_multi_table(groups, n_groups, t, need) ? need : -1;
}

// groups: a HOST table of 1 or 2 groups; a group's `targets` is a DEVICE table of n_targets (1..O3D_CROP_MULTI_MAX_TARGETS)
// targets whose boxes, out buffers and counts live on the device.  The host cannot read that table: a target whose capacity
// is <= 0 is counted only; a mode other than O3D_CROP_MODEL crops as O3D_CROP_SUBWINDOW.  scratch: scratch_len >=
// o3d_track_crop_multi_scratch(groups, n_groups) int32 on the device.  An empty cloud writes count = 0 for its targets.
extern "C" int o3d_track_crop_multi(const o3d_crop_group* groups, int n_groups, int32_t* scratch, long scratch_len, void* stream) {
    CropMultiTable t;
    long need;
    if (!crop_multi_table(groups, n_groups, t, need) || !scratch || scratch_len < need) return O3D_EINVAL;
    const int wgs = t.wgs[0] + t.wgs[1], rows = t.K[0] + t.K[1];
    hipLaunchKernelGGL(crop_multi_kernel<false>, dim3(wgs), dim3(CROP_WG), 0, o3d_stream(stream), t, scratch);
    hipLaunchKernelGGL(crop_multi_scan_kernel, dim3(rows), dim3(CROP_WG), 0, o3d_stream(stream), t, scratch);
    hipLaunchKernelGGL(crop_multi_kernel<true>, dim3(wgs), dim3(CROP_WG), 0, o3d_stream(stream), t, scratch);
    return o3d_launch_status();
}

// o3d_track_resample for a DEVICE table of n_jobs jobs in one launch (the 2K gathers of a frame of K targets); the host
// cannot read the table: a job with n <= 0 writes nothing, a job without src or idx is zero-filled
extern "C" int o3d_track_resample_multi(const o3d_resample_job* jobs, int n_jobs, void* stream) {
    if (n_jobs < 0 || n_jobs > (1 << 20) || (n_jobs > 0 && !jobs)) return O3D_EINVAL;
    if (n_jobs == 0) return O3D_OK;
    hipLaunchKernelGGL(resample_multi_kernel, dim3(n_jobs, 4), dim3(256), 0, o3d_stream(stream), jobs);
    return o3d_launch_status();
}

// o3d_track_offset_box for K targets in one launch: ref (K,15), offset (K,4), yaw_state (K,10) | NULL, rebase (K) int32 | NULL
// (per target; NULL = none), active (K) int32 | NULL (NULL = all), out (K,15) | NULL (may be ref), results (T,K,15) | NULL with
// the ONE frame counter: every target's box goes to results[frame[0]][k], then frame[0] += 1.  Target k is updated as
// o3d_track_offset_box updates it with seed + k (seed + K < 2^31); an inactive target's ref goes to out and results unchanged
// and its yaw_state is not touched.
extern "C" int o3d_track_offset_box_multi(const float* ref, const float* offset, float* yaw_state, const int32_t* rebase,
                                          const int32_t* active, int K, int degrees, int use_z, int limit_box, int seed, float* out,
                                          float* results, int T, int32_t* frame, void* stream) {
    if (!ref || !offset || K < 1 || K > (1 << 20) || (!out && !results) || T < 0 || (results && (!frame || T < 1)) || seed < 0 ||
        seed > 0x7fffffff - K)
        return O3D_EINVAL;
    OffsetMultiArgs a{ref, offset, yaw_state, rebase, active, out, results, frame, K, T, degrees, use_z, limit_box, seed};
    hipLaunchKernelGGL(offset_box_multi_kernel, dim3(1), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

// o3d_track_motion_input for K targets in one launch (tracking.MultiMotionTracker): jobs is a DEVICE table of K records that
// hold what changes per frame (the two crops, their counts, the 2N indices, the zero-fill flags); wlh (K,3), points (K,2N,5),
// candidate_bc (K,2N,9) | NULL.  Row k is what o3d_track_motion_input writes for job k and wlh + 3 k, bit for bit.  The host
// cannot read the table: a half without its crop or without idx is zero-filled.
extern "C" int o3d_track_motion_input_multi(const o3d_motion_job* jobs, int K, int N, const float* wlh, int first_frame, float* points,
                                            float* candidate_bc, void* stream) {
    if (!jobs || !wlh || !points || K < 1 || K > O3D_CROP_MULTI_MAX_TARGETS || N < 1 || N > (1 << 20)) return O3D_EINVAL;
    hipLaunchKernelGGL(motion_input_multi_kernel, dim3(o3d_cdiv(2 * N, 256), K), dim3(256), 0, o3d_stream(stream), jobs, N, wlh,
                       first_frame != 0, points, candidate_bc);
    return o3d_launch_status();
}

// Sample, gather and label for M2-Track training batches (include/o3dsot.h states the contract; the other kernels of a batch are
// csrc/train_batch.hip's)
extern "C" int o3d_train_motion_sample(const o3d_train_motion_sample_args* args, void* stream) {
    if (!args) return O3D_EINVAL;
    const o3d_train_motion_sample_args& a = *args;
    if (!a.sel || !a.counts || !a.crop_prev || !a.crop_this || a.cap_prev < 0 || a.cap_this < 0 || a.cap_prev > (1 << 29) ||
        a.cap_this > (1 << 29) || a.J < 1 || a.J > O3D_TRAIN_MAX_CANDIDATES || a.B < 1 || a.B > a.J || a.N < 1 || a.N > (1 << 20) ||
        (a.idx_prev == nullptr) != (a.idx_this == nullptr) || !a.candidate_id || !a.prev_box || !a.this_box || !a.canon_box ||
        !a.cand_box_label || !a.cand_box_label_prev || !a.cand_motion_label || !a.cand_motion_state || !a.cand_bbox_size || !a.points ||
        !a.seg_label || !a.box_label || !a.box_label_prev || !a.motion_label || !a.motion_state_label || !a.bbox_size ||
        (a.bc_boxes != nullptr) != (a.xyz_halves != nullptr))
        return O3D_EINVAL;
    hipLaunchKernelGGL(train_motion_sample_kernel, dim3(o3d_cdiv(2 * a.N, 256), a.B), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}
