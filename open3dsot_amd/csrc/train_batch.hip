// Training batches built on the device: what the reference does on the host, one pair at a time in DataLoader workers,
// between "frames and annotated boxes" and "the training dict" (datasets/sampler.py:16-79 siamese_processing over
// datasets/points_utils.py), for BAT and P2B.
//
//   o3d_track_offset_box_multi (track.hip)  the two jittered boxes of every candidate (getOffsetBB with a 3-vector), K = 2J
//   o3d_train_labels        transform_box, box_label, bbox_size and the canonical model box of every candidate
//   o3d_track_crop_groups   the three crops of every candidate: o3d_track_crop_multi over G clouds, every frame read once
//   o3d_train_select        which candidates fill the batch (the reference's two assertions, sampler.py:46,59)
//   o3d_train_sample        regularize_pc of both clouds, the template as the virtual concatenation of its two crops
//                           (getModel), seg_label, and the rows of the per-candidate labels that the batch takes
//   o3d_boxcloud (boxcloud.hip)             points2cc_dist_t / _s (BAT)
//
// and for M2-Track (datasets/sampler.py:82-180 motion_processing with apply_augmentation, datasets/points_utils.py:299-361):
//   o3d_train_augment           apply_transform for the boxes of both frames of every candidate, and the records by which the
//                               crop moves the points (K = 2J)
//   o3d_track_offset_box_multi  the jittered reference box of every candidate (K = J)
//   o3d_train_motion_labels     the three transform_box, the three labels, motion_state_label, bbox_size
//   o3d_track_crop_groups_aug   both crops of every candidate and the in-box count of its previous frame; a target with an
//                               enabled record sees the augmented point
//   o3d_train_select_motion     which candidates fill the batch (sampler.py:99,120)
//   o3d_train_motion_sample     (track.hip, beside motion_row) regularize_pc of both halves, the row's channels, seg_label, the label rows
//   o3d_boxcloud (2)            prev_bc, this_bc
// and in front of either list on the planned route (sampler.py's build_planned), in place of the per-batch upload:
//   o3d_train_draw              the candidates' boxes gathered from the resident pool, and the draws of the batch
//
// Every keep decision (the crops and seg_label) is crop_test or inside_box, every row gather gather_row: the definitions of
// track_common.hpp, which track.hip uses.  This file is compiled with -ffp-contract=off like track.hip.
//
// ---- the augmented point's fp32 operation order (aug_point, track_common.hpp; tests/motion_sampler_oracle.py restates it) -----------
// A record holds enabled, the un-augmented box (c, wlh, R), A (3x3 row-major) and c'.  For the point p and an enabled record:
//   d  = p - c                                    dx = px - cx, dy = py - cy, dz = pz - cz
//   q  = R^T d                                    qx = ((R00*dx + R10*dy) + R20*dz), qy, qz as in the crop (track.hip)
//   inside (inclusive: points_in_box, 1.25)       |qx| <= ((l*1.25)*0.5)  and  |qy| <= ((w*1.25)*0.5)  and  |qz| <= ((h*1.25)*0.5)
//   inside:  p'_i = (((A_i0*dx + A_i1*dy) + A_i2*dz) + c'_i)          otherwise p' = p
// The crop of that target is crop_test(p') with the operation order of track.hip.  A and c' are computed once per record in
// double and rounded once (o3d_train_augment): A = R Rz(rot) diag(fx, fy, 1) R^T, c' = c + R t.
// seg_label of a motion batch is inside_box(row, box, 1.25) in the same order, with the row's xyz as p.
//
// ---- o3d_track_crop_groups: G clouds, three launches, no workgroup ever waits for another -------------------------------------------
// The host knows every n and plans the table (o3d_track_crop_groups_scratch): group g owns workgroups [wg_start, wg_start +
// W) of the count and scatter launches (W = ceil(n / 256), 1 for an empty cloud), workgroups [row_start, row_start + K) of the
// scan launch, and K rows of W int32 of scratch from sbase on (target-major).  A workgroup finds its group by a binary search
// over the planned starts in the device table; blockIdx.x is the only input of the search, so the index is the same for
// all its threads.
//   launch 1 (count)    crop_multi_wg<false>: reads points, the tables, the boxes; writes scratch[g][k][w], its own word per k.
//   launch 2 (scan)     crop_scan_row: one workgroup per (group, target) rewrites its OWN row by its exclusive prefix sums and
//                       writes count[0].  It reads what launch 1 wrote.
//   launch 3 (scatter)  crop_multi_wg<true>: reads scratch[g][k][w] (launch 2) and writes `out` only.
// Within a launch no workgroup reads a word that another workgroup of that launch writes; the order between the launches is
// the stream's.  There is no flag, no atomic and no loop that waits on memory.  The boxes of the targets may be the output
// of an earlier launch of the same stream (the jittered boxes); nothing in these three launches writes them.
//
// ---- o3d_train_sample: the index draw (integers only; tests/sampler_oracle.py restates it and the two agree exactly) -----------------
// All arithmetic is uint32 and wraps.
//   mix32(x):  x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16     (the MurmurHash3 finaliser)
//   key = mix32( (seed * 0x9E3779B1) ^ (counter * 0x85EBCA77 + j * 0xC2B2AE3D + cloud * 0x27D4EB2F + 0x165667B1) )
//         j = the candidate, cloud = 0 (template) | 1 (search)
// A cloud of n rows resampled to S rows, row i:
//   n <= 2            no index: a zero row                                   (regularize_pc's `num_points <= 2`)
//   n == S            idx = i                                                (np.arange)
//   S > n             idx = mulhi( mix32(key ^ (i * 0x9E3779B1 + 0x85EBCA77)), n )            with replacement
//   S < n             idx = P(i), a keyed bijection of [0, n):               without replacement
//       b = bits(n - 1) (>= 2),  h = ceil(b / 2),  mask = 2^h - 1;  the domain [0, 2^(2h)) holds fewer than 4 n values
//       E(x):  L = x >> h, R = x & mask;  for round = 0..3:  (L, R) = (R, L ^ (mix32(key ^ (R * 0x9E3779B1 + round *
//              0x85EBCA77 + 0xC2B2AE3D)) & mask));  E = (L << h) | R            a balanced Feistel network: a bijection
//       P(i):  x = E(i);  while x >= n: x = E(x)                                cycle walking
//   The walk stays on the cycle of E through i, which comes back to i < n: it ends after at most 2^(2h) - n + 1 < 4 n
//   applications, 2^(2h) / n < 4 in the mean.  It is a register-only loop that reads no memory.
//
// ---- o3d_train_draw: the boxes and the random numbers of a planned batch (tests/epoch_plan_oracle.py restates it) ------------------------
// One thread per candidate j gathers its frames' boxes from the resident pool and draws what the host drew from a numpy
// Generator on the per-batch route.  The key is the index draw's with tags beyond its clouds 0 / 1, one tag per drawn vector:
//   key(tag) = mix32( (seed * 0x9E3779B1) ^ (counter * 0x85EBCA77 + j * 0xC2B2AE3D + tag * 0x27D4EB2F + 0x165667B1) )
//         tag = 2 the (template) jitter | 3 the search offset | 4 the previous frame's augmentation | 5 the current frame's
//   h(c) = mix32( key(tag) ^ (c * 0x9E3779B1 + 0x85EBCA77) )                       component c of the vector, a uint32
// In double, rounded to fp32 once at the end:
//   u(h)            = ((h >> 8) + 0.5) * 2^-24                                      in (0, 1)
//   uniform(lo, hi) = lo + (hi - lo) * u(h)
//   normal(ha, hb)  = sqrt(-2 log u(ha)) * cos((2 pi) * ((hb >> 8) * 2^-24))        Box-Muller
//   ang             = 5 with `degrees`, 5 * (pi / 180) otherwise
//   jitter (tag 2)          (x, y) = uniform(-0.3, 0.3) of h(0), h(1);  theta = uniform(-0.3, 0.3) of h(2), times ang
//   search offset (tag 3)   (x, y) = normal(h(0), h(1)), normal(h(2), h(3));  theta = normal(h(4), h(5)) * sqrt(ang)
//   augmentation (tag 4, 5) (tx, ty, tz) = uniform(-0.3, 0.3) of h(0..2);  rot = uniform(-10, 10) of h(3);
//                           flip_x = h(4) >> 31, flip_y = h(5) >> 31                (1.0 | 0.0)
// Zero rows (the reference's): candidate id 0 has a zero jitter, and with num_candidates > 1 a zero search offset; the
// augmentation is drawn for every candidate.  offs rows are (x, y, 0, theta).  A pool row outside [0, R) is not read: its box
// is 15 zeros, whose crops (scale 1 or model mode, offset 0) count nothing, so the candidate is invalid.
//
// ---- fixed capacities -----------------------------------------------------------------------------------------------------------------
// A crop is written into a buffer of `capacity` rows; a longer one is truncated to its first `capacity` survivors (the crop's
// own rule) and the draw uses the truncated length min(count, capacity).  Validity (o3d_train_select) is decided on the counts
// before truncation, as the reference's assertions are; `overflow` reports the truncated crops among the chosen rows.
#include "track_common.hpp"

static_assert(sizeof(o3d_crop_target) == 48, "o3d_crop_target: points_utils.CROP_TARGET mirrors this layout");
static_assert(sizeof(o3d_crop_plan) == 48, "o3d_crop_plan: points_utils.CROP_PLAN mirrors this layout");
static_assert(sizeof(o3d_train_sample_args) == 192, "o3d_train_sample_args: points_utils._TrainSampleArgs mirrors this layout");
static_assert(sizeof(o3d_crop_aug) == 112, "o3d_crop_aug: points_utils.CROP_AUG mirrors this layout");

namespace {

// the group of workgroup `wg`: the last g with start(g) <= wg (start(0) == 0).  ROWS: search row_start, else wg_start
template <bool ROWS>
__device__ __forceinline__ int crop_group_of(const o3d_crop_plan* __restrict__ G, int n_groups, int wg) {
    int lo = 0, hi = n_groups - 1;
    while (lo < hi) {                                      // at most 12 steps: register state only, every read is of the table
        const int mid = (lo + hi + 1) >> 1;
        if ((ROWS ? G[mid].row_start : G[mid].wg_start) <= wg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// AUG (o3d_track_crop_groups_aug): aug[group] = the group's augmentation records | NULL; aug itself may be NULL
template <bool SCATTER, bool AUG = false>
__global__ __launch_bounds__(CROP_WG) void crop_groups_kernel(const o3d_crop_plan* __restrict__ G, int n_groups, int32_t* __restrict__ scratch,
                                                              const o3d_crop_aug* const* __restrict__ aug = nullptr) {
    const int gi = crop_group_of<false>(G, n_groups, (int)blockIdx.x);
    const o3d_crop_plan g = G[gi];
    const int W = g.n > 0 ? (g.n + CROP_WG - 1) / CROP_WG : 1, w = (int)blockIdx.x - g.wg_start;
    if (w < 0 || w >= W) return;                           // a device table that disagrees with the planned grid: nothing is touched
    if (AUG) crop_multi_wg<SCATTER, true>(g.points, g.n, g.targets, g.n_targets, W, scratch + g.sbase, w, aug ? aug[gi] : nullptr);
    else crop_multi_wg<SCATTER>(g.points, g.n, g.targets, g.n_targets, W, scratch + g.sbase, w);
}

__global__ __launch_bounds__(CROP_WG) void crop_groups_scan_kernel(const o3d_crop_plan* __restrict__ G, int n_groups, int32_t* __restrict__ scratch) {
    const o3d_crop_plan g = G[crop_group_of<true>(G, n_groups, (int)blockIdx.x)];
    const int W = g.n > 0 ? (g.n + CROP_WG - 1) / CROP_WG : 1, k = (int)blockIdx.x - g.row_start;
    if (k < 0 || k >= g.n_targets) return;
    crop_scan_row(scratch + g.sbase + (long)k * W, W, g.targets[k].count);
}

// ---- o3d_train_select -----------------------------------------------------------------------------------------------------------------
constexpr int SELECT_WG = O3D_TRAIN_MAX_CANDIDATES;        // one thread per candidate

// MOTION (o3d_train_select_motion): counts = (in-box, previous crop, current crop); cap0 is not used
template <bool MOTION>
__global__ __launch_bounds__(SELECT_WG) void train_select_kernel(const int32_t* __restrict__ counts, int J, int B, int cap0, int cap1, int cap2,
                                                                 int32_t* __restrict__ sel, int32_t* __restrict__ n_valid,
                                                                 int32_t* __restrict__ overflow) {
    __shared__ int wave_tot[SELECT_WG / 64];
    __shared__ int list[SELECT_WG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int c0 = 0, c1 = 0, c2 = 0;
    if (tid < J) { c0 = counts[3 * tid]; c1 = counts[3 * tid + 1]; c2 = counts[3 * tid + 2]; }
    const bool valid = tid < J && (MOTION ? c0 > 10 : c0 + c1 > 20) && c2 > 20;
    const unsigned long long mask = __ballot(valid);
    if (lane == 0) wave_tot[wave] = __popcll(mask);
    __syncthreads();
    int rank = __popcll(mask & ((1ull << lane) - 1ull)), nv = 0;
    for (int v = 0; v < SELECT_WG / 64; ++v) {
        if (v < wave) rank += wave_tot[v];
        nv += wave_tot[v];
    }
    if (valid) list[rank] = tid;
    __syncthreads();
    int over = 0;
    if (tid < B) {
        const int j = nv > 0 ? list[tid % nv] : -1;
        sel[tid] = j;
        if (j >= 0) over = (MOTION ? 0 : counts[3 * j] > cap0) + (counts[3 * j + 1] > cap1) + (counts[3 * j + 2] > cap2);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) over += __shfl_xor(over, off, 64);
    __syncthreads();                                       // wave_tot is reused
    if (lane == 0) wave_tot[wave] = over;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int v = 0; v < SELECT_WG / 64; ++v) total += wave_tot[v];
        n_valid[0] = nv;
        overflow[0] = total;
    }
}

// ---- o3d_train_labels -----------------------------------------------------------------------------------------------------------------
struct LabelArgs {
    const float* gt; const float* sb; const float* tb; const float* offset; int J;
    float* search_box; float* box_label; float* bbox_size; float* model_box;
};

__global__ __launch_bounds__(256) void train_labels_kernel(LabelArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.J) return;
    const float* gt = a.gt + 15 * (long)j;
    const float* sb = a.sb + 15 * (long)j;
    float* o = a.search_box + 15 * (long)j;
    double d[3], Rs[9], R[9];
    for (int i = 0; i < 3; ++i) d[i] = (double)gt[i] - (double)sb[i];
    for (int i = 0; i < 9; ++i) { Rs[i] = sb[6 + i]; R[i] = gt[6 + i]; }
    for (int r = 0; r < 3; ++r) {                          // row r of R_sb^T = column r of R_sb
        o[r] = (float)((Rs[r] * d[0] + Rs[3 + r] * d[1]) + Rs[6 + r] * d[2]);
        for (int c = 0; c < 3; ++c) o[6 + 3 * r + c] = (float)((Rs[r] * R[c] + Rs[3 + r] * R[3 + c]) + Rs[6 + r] * R[6 + c]);
    }
    for (int i = 0; i < 3; ++i) {
        o[3 + i] = gt[3 + i];
        a.bbox_size[3 * (long)j + i] = gt[3 + i];
        a.box_label[4 * (long)j + i] = o[i];
    }
    a.box_label[4 * (long)j + 3] = -a.offset[4 * (long)j + 3];
    float* m = a.model_box + 15 * (long)j;
    for (int i = 0; i < 15; ++i) m[i] = (i == 6 || i == 10 || i == 14) ? 1.f : 0.f;
    for (int i = 0; i < 3; ++i) m[3 + i] = a.tb[15 * (long)j + 3 + i];
}

// ---- o3d_train_sample -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void train_sample_kernel(o3d_train_sample_args a) {
    const int r = blockIdx.y, cloud = blockIdx.z, i = blockIdx.x * 256 + threadIdx.x;
    const int S = cloud ? a.N : a.M;
    const int j = a.sel[r];
    const bool live = j >= 0 && j < a.J;
    if (cloud == 0 && blockIdx.x == 0) {                   // the rows of the per-candidate labels that the batch takes
        const int B = a.B;
        for (int e = threadIdx.x; e < 37; e += 256) {
            if (e < 4) a.box_label[4 * (long)r + e] = live ? a.cand_box_label[4 * (long)j + e] : 0.f;
            else if (e < 7) a.bbox_size[3 * (long)r + (e - 4)] = live ? a.cand_bbox_size[3 * (long)j + (e - 4)] : 0.f;
            else if (a.bc_boxes) {
                const int which = e < 22 ? 0 : 1, f = e - (which ? 22 : 7);      // f: the field of the (15) box
                const float v = live ? (which ? a.search_box : a.model_box)[15 * (long)j + f] : 0.f;
                float* o = a.bc_boxes + (long)which * 15 * B;
                if (f < 3) o[3 * (long)r + f] = v;
                else if (f < 6) o[3 * (long)B + 3 * (long)r + (f - 3)] = v;
                else o[6 * (long)B + 9 * (long)r + (f - 6)] = v;
            }
        }
    }
    if (i >= S) return;
    int n = 0, n_a = 0;
    if (live) {
        const int32_t* c = a.counts + 3 * (long)j;
        if (cloud) {
            n = min(c[2], a.cap_search);
        } else {
            n_a = min(c[0], a.cap_first);
            n = n_a + min(c[1], a.cap_template);
        }
    }
    const bool zero = n <= 2;
    int s = -1;
    if (!zero) {
        const int32_t* given = cloud ? a.idx_s : a.idx_t;
        if (given) {
            s = given[(long)j * S + i];
        } else {
            const unsigned key = mix32((a.seed * 0x9E3779B1u) ^
                                       (a.counter * 0x85EBCA77u + (unsigned)j * 0xC2B2AE3Du + (unsigned)cloud * 0x27D4EB2Fu + 0x165667B1u));
            s = sample_index(key, i, n, S);
        }
        if ((unsigned)s >= (unsigned)n) s = -1;
    }
    // the source of row s: the search crop, or the part of the virtual concatenation that holds it
    const float* src = nullptr;
    int n_src = 0, local = s;
    if (s >= 0) {
        if (cloud) { src = a.crop_search + 3 * (long)j * a.cap_search; n_src = n; }
        else if (s < n_a) { src = a.crop_first + 3 * (long)j * a.cap_first; n_src = n_a; }
        else { src = a.crop_template + 3 * (long)j * a.cap_template; n_src = n - n_a; local = s - n_a; }
    }
    float x, y, z;
    gather_row(src, n_src, &local, 0, s < 0, x, y, z);
    const long row = (long)r * S + i;
    float* o = (cloud ? a.search_points : a.template_points) + 3 * row;
    o[0] = x; o[1] = y; o[2] = z;
    if (cloud) {
        float qx, qy, qz;
        const bool inside = s >= 0 && crop_test(x, y, z, a.search_box + 15 * (long)j, 1.f, 0.f, O3D_CROP_SUBWINDOW, qx, qy, qz);
        a.seg_label[row] = inside ? 1.f : 0.f;
    }
    int32_t* used = cloud ? a.used_s : a.used_t;
    if (used) used[row] = s;
}

// ---- o3d_train_augment ----------------------------------------------------------------------------------------------------------------
struct AugmentArgs { const float* gt; const float* draw; const int32_t* slot_src; int K, n_slots; float* out_box; o3d_crop_aug* aug; };

__global__ __launch_bounds__(256) void train_augment_kernel(AugmentArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_slots) return;
    const int k = a.slot_src ? a.slot_src[i] : i;
    o3d_crop_aug rec;
    if (k < 0 || k >= a.K) {                               // a disabled record: all zero
        rec.enabled = 0;
        for (int e = 0; e < 15; ++e) rec.box[e] = 0.f;
        for (int e = 0; e < 9; ++e) rec.A[e] = 0.f;
        for (int e = 0; e < 3; ++e) rec.c[e] = 0.f;
        a.aug[i] = rec;
        return;
    }
    const float* gt = a.gt + 15 * (long)k;
    const float* dr = a.draw + 6 * (long)k;
    double R[9], t[3] = {dr[0], dr[1], dr[2]};
    for (int e = 0; e < 9; ++e) R[e] = gt[6 + e];
    double s, c;
    sincos((double)dr[3] * (3.14159265358979323846 / 180.0), &s, &c);
    const double fx = dr[4] != 0.f ? -1.0 : 1.0, fy = dr[5] != 0.f ? -1.0 : 1.0;
    // M = R Rz(rot): column 0 = c R0 + s R1, column 1 = -s R0 + c R1, column 2 = R2 (R0, R1, R2: the columns of R)
    double M[9];
    for (int r = 0; r < 3; ++r) {
        M[3 * r] = R[3 * r] * c + R[3 * r + 1] * s;
        M[3 * r + 1] = R[3 * r + 1] * c - R[3 * r] * s;
        M[3 * r + 2] = R[3 * r + 2];
    }
    float* o = a.out_box + 15 * (long)k;
    rec.enabled = 1;
    for (int r = 0; r < 3; ++r) {
        const float cr = (float)((double)gt[r] + ((R[3 * r] * t[0] + R[3 * r + 1] * t[1]) + R[3 * r + 2] * t[2]));
        o[r] = cr;
        rec.c[r] = cr;
        o[3 + r] = gt[3 + r];
        // the box: M Rz(180 deg) for flip_x = M diag(-1, -1, 1), exactly
        o[6 + 3 * r] = (float)(fx * M[3 * r]);
        o[6 + 3 * r + 1] = (float)(fx * M[3 * r + 1]);
        o[6 + 3 * r + 2] = (float)M[3 * r + 2];
        // the points: A = M diag(fx, fy, 1) R^T
        for (int q = 0; q < 3; ++q)
            rec.A[3 * r + q] = (float)(((fx * M[3 * r]) * R[3 * q] + (fy * M[3 * r + 1]) * R[3 * q + 1]) + M[3 * r + 2] * R[3 * q + 2]);
    }
    for (int e = 0; e < 15; ++e) rec.box[e] = gt[e];
    a.aug[i] = rec;
}

// ---- o3d_train_draw -------------------------------------------------------------------------------------------------------------------
struct DrawArgs {
    const float* gt; int R; const int32_t* rows; const int32_t* cand; int J; unsigned seed, counter; int degrees, num_candidates, mode;
    float* refs; float* first; float* offs; float* aug;
};

__device__ __forceinline__ unsigned draw_key(unsigned seed, unsigned counter, unsigned j, unsigned tag) {
    return mix32((seed * 0x9E3779B1u) ^ (counter * 0x85EBCA77u + j * 0xC2B2AE3Du + tag * 0x27D4EB2Fu + 0x165667B1u));
}
__device__ __forceinline__ unsigned draw_bits(unsigned key, unsigned c) { return mix32(key ^ (c * 0x9E3779B1u + 0x85EBCA77u)); }
__device__ __forceinline__ double draw_u(unsigned h) { return ((double)(h >> 8) + 0.5) * (1.0 / 16777216.0); }
__device__ __forceinline__ double draw_uniform(unsigned h, double lo, double hi) { return lo + (hi - lo) * draw_u(h); }
__device__ __forceinline__ double draw_normal(unsigned ha, unsigned hb) {
    return sqrt(-2.0 * log(draw_u(ha))) * cos((2.0 * 3.14159265358979323846) * ((double)(hb >> 8) * (1.0 / 16777216.0)));
}

// box `row` of the pool -> dst (15); a row outside the pool is not read
__device__ __forceinline__ void draw_gather(const float* __restrict__ gt, int R, int row, float* __restrict__ dst) {
    const bool ok = row >= 0 && row < R;
    const float* src = gt + 15 * (long)(ok ? row : 0);
    for (int e = 0; e < 15; ++e) dst[e] = ok ? src[e] : 0.f;
}

__global__ __launch_bounds__(256) void train_draw_kernel(DrawArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.J) return;
    const int J = a.J, cid = a.cand[j];
    const bool siamese = a.mode == O3D_TRAIN_DRAW_SIAMESE;
    const double ang = a.degrees ? 5.0 : 5.0 * (3.14159265358979323846 / 180.0);
    const int32_t* rows = a.rows + (siamese ? 3 : 2) * (long)j;
    if (siamese) draw_gather(a.gt, a.R, rows[0], a.first + 15 * (long)j);
    draw_gather(a.gt, a.R, rows[siamese ? 1 : 0], a.refs + 15 * (long)j);
    draw_gather(a.gt, a.R, rows[siamese ? 2 : 1], a.refs + 15 * (long)(J + j));
    float* o = a.offs + 4 * (long)j;                       // the jitter
    if (cid == 0) {
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f;
    } else {
        const unsigned key = draw_key(a.seed, a.counter, (unsigned)j, 2u);
        o[0] = (float)draw_uniform(draw_bits(key, 0u), -0.3, 0.3);
        o[1] = (float)draw_uniform(draw_bits(key, 1u), -0.3, 0.3);
        o[2] = 0.f;
        o[3] = (float)(draw_uniform(draw_bits(key, 2u), -0.3, 0.3) * ang);
    }
    if (siamese) {                                         // the search offset
        float* s = a.offs + 4 * (long)(J + j);
        if (cid == 0 && a.num_candidates > 1) {
            s[0] = 0.f; s[1] = 0.f; s[2] = 0.f; s[3] = 0.f;
        } else {
            const unsigned key = draw_key(a.seed, a.counter, (unsigned)j, 3u);
            s[0] = (float)draw_normal(draw_bits(key, 0u), draw_bits(key, 1u));
            s[1] = (float)draw_normal(draw_bits(key, 2u), draw_bits(key, 3u));
            s[2] = 0.f;
            s[3] = (float)(draw_normal(draw_bits(key, 4u), draw_bits(key, 5u)) * sqrt(ang));
        }
    } else if (a.mode == O3D_TRAIN_DRAW_MOTION_AUG) {
        for (int f = 0; f < 2; ++f) {                      // the previous frame's draw, the current frame's
            const unsigned key = draw_key(a.seed, a.counter, (unsigned)j, 4u + (unsigned)f);
            float* g = a.aug + 6 * (long)(f * J + j);
            for (unsigned c = 0; c < 3; ++c) g[c] = (float)draw_uniform(draw_bits(key, c), -0.3, 0.3);
            g[3] = (float)draw_uniform(draw_bits(key, 3u), -10.0, 10.0);
            g[4] = (float)(draw_bits(key, 4u) >> 31);
            g[5] = (float)(draw_bits(key, 5u) >> 31);
        }
    }
}

// ---- o3d_train_inside_box -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void train_inside_box_kernel(const float* __restrict__ points, int n, const float* __restrict__ box,
                                                               float factor, int32_t* __restrict__ mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float dx, dy, dz;
    mask[i] = inside_box(points[3 * (long)i], points[3 * (long)i + 1], points[3 * (long)i + 2], box, factor, dx, dy, dz) ? 1 : 0;
}

// ---- o3d_train_motion_labels ----------------------------------------------------------------------------------------------------------
struct MotionLabelArgs {
    const float* prev_gt; const float* this_gt; const float* ref_box; int J, degrees; float motion_threshold;
    float* this_box; float* prev_box; float* canon_box; float* box_label; float* box_label_prev; float* motion_label;
    int32_t* motion_state; float* bbox_size;
};

// transform_box in double: (c, R) of a box in the frame of (cr, Rr) -> centre Rr^T (c - cr), rotation Rr^T R
__device__ __forceinline__ void transform_box64(const double* c, const double* R, const double* cr, const double* Rr, double* oc, double* oR) {
    const double d[3] = {c[0] - cr[0], c[1] - cr[1], c[2] - cr[2]};
    for (int r = 0; r < 3; ++r) {                          // row r of Rr^T = column r of Rr
        oc[r] = (Rr[r] * d[0] + Rr[3 + r] * d[1]) + Rr[6 + r] * d[2];
        for (int q = 0; q < 3; ++q) oR[3 * r + q] = (Rr[r] * R[q] + Rr[3 + r] * R[3 + q]) + Rr[6 + r] * R[6 + q];
    }
}

__device__ __forceinline__ void label_row(const double* c, const double* R, int degrees, float* o) {
    const double theta = atan2(R[3], R[0]);
    o[0] = (float)c[0]; o[1] = (float)c[1]; o[2] = (float)c[2];
    o[3] = (float)(degrees ? theta * (180.0 / 3.14159265358979323846) : theta);
}

__global__ __launch_bounds__(256) void train_motion_labels_kernel(MotionLabelArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.J) return;
    const float* pg = a.prev_gt + 15 * (long)j;
    const float* tg = a.this_gt + 15 * (long)j;
    const float* rb = a.ref_box + 15 * (long)j;
    double cp[3], Rp[9], ct[3], Rt[9], cr[3], Rr[9];
    for (int e = 0; e < 3; ++e) { cp[e] = pg[e]; ct[e] = tg[e]; cr[e] = rb[e]; }
    for (int e = 0; e < 9; ++e) { Rp[e] = pg[6 + e]; Rt[e] = tg[6 + e]; Rr[e] = rb[6 + e]; }
    double c_this[3], R_this[9], c_prev[3], R_prev[9], c_mot[3], R_mot[9];
    transform_box64(ct, Rt, cr, Rr, c_this, R_this);
    transform_box64(cp, Rp, cr, Rr, c_prev, R_prev);
    transform_box64(c_this, R_this, c_prev, R_prev, c_mot, R_mot);
    float* ob = a.this_box + 15 * (long)j;
    float* pb = a.prev_box + 15 * (long)j;
    float* cb = a.canon_box + 15 * (long)j;
    for (int e = 0; e < 3; ++e) {
        ob[e] = (float)c_this[e]; pb[e] = (float)c_prev[e]; cb[e] = 0.f;
        ob[3 + e] = tg[3 + e]; pb[3 + e] = pg[3 + e]; cb[3 + e] = pg[3 + e];
        a.bbox_size[3 * (long)j + e] = tg[3 + e];
    }
    for (int e = 0; e < 9; ++e) {
        ob[6 + e] = (float)R_this[e]; pb[6 + e] = (float)R_prev[e];
        cb[6 + e] = (e == 0 || e == 4 || e == 8) ? 1.f : 0.f;
    }
    label_row(c_this, R_this, a.degrees, a.box_label + 4 * (long)j);
    label_row(c_prev, R_prev, a.degrees, a.box_label_prev + 4 * (long)j);
    label_row(c_mot, R_mot, a.degrees, a.motion_label + 4 * (long)j);
    const double dx = c_this[0] - c_prev[0], dy = c_this[1] - c_prev[1], dz = c_this[2] - c_prev[2];
    a.motion_state[j] = sqrt((dx * dx + dy * dy) + dz * dz) > (double)a.motion_threshold ? 1 : 0;
}

static bool crop_groups_plan(const o3d_crop_plan* groups, int n_groups, bool check_plan, o3d_crop_plan* fill, long& wgs, long& rows,
                             long& need) {
    if (!groups || n_groups < 1 || n_groups > O3D_CROP_MAX_GROUPS) return false;
    wgs = rows = need = 0;
    for (int g = 0; g < n_groups; ++g) {
        const o3d_crop_plan& G = groups[g];
        if (G.n < 0 || G.n > (1 << 30) || (G.n > 0 && !G.points) || !G.targets || G.n_targets < 1 ||
            G.n_targets > O3D_CROP_MULTI_MAX_TARGETS)
            return false;
        if (check_plan && (G.wg_start != wgs || G.row_start != rows || G.sbase != need)) return false;
        if (fill) { fill[g].wg_start = (int)wgs; fill[g].row_start = (int)rows; fill[g].sbase = need; }
        const int W = crop_wgs(G.n);
        wgs += W;
        rows += G.n_targets;
        need += (long)W * G.n_targets;
        if (wgs > 0x7fffffffL || rows > 0x7fffffffL) return false;
    }
    return true;
}

}  // namespace

// Host only (no HIP call): plans the HOST table `groups` in place -- wg_start, row_start and sbase of every group from the n
// and n_targets of the groups before it -- and writes grid[0] = the workgroups of the count / scatter launches, grid[1] =
// those of the scan launch (grid may be NULL).  -> the scratch length in int32, -1 for a bad table.
extern "C" long o3d_track_crop_groups_scratch(o3d_crop_plan* groups, int n_groups, int* grid) {
    long wgs, rows, need;
    if (!crop_groups_plan(groups, n_groups, false, groups, wgs, rows, need)) return -1;
    if (grid) { grid[0] = (int)wgs; grid[1] = (int)rows; }
    return need;
}

// groups: the planned HOST table (checked again here, its plan included); dev_groups: its copy on the device, which the
// launches read (its upload precedes this call in the stream).  The host cannot read the target tables: as in
// o3d_track_crop_multi, a target whose capacity is <= 0 is counted only and a mode other than O3D_CROP_MODEL crops as
// O3D_CROP_SUBWINDOW.  scratch: scratch_len >= o3d_track_crop_groups_scratch(groups, n_groups, ...) int32 on the device.
extern "C" int o3d_track_crop_groups(const o3d_crop_plan* groups, const o3d_crop_plan* dev_groups, int n_groups, int32_t* scratch,
                                     long scratch_len, void* stream) {
    long wgs, rows, need;
    if (!crop_groups_plan(groups, n_groups, true, nullptr, wgs, rows, need) || !dev_groups || !scratch || scratch_len < need)
        return O3D_EINVAL;
    hipLaunchKernelGGL(crop_groups_kernel<false>, dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), dev_groups, n_groups, scratch);
    hipLaunchKernelGGL(crop_groups_scan_kernel, dim3((int)rows), dim3(CROP_WG), 0, o3d_stream(stream), dev_groups, n_groups, scratch);
    hipLaunchKernelGGL(crop_groups_kernel<true>, dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), dev_groups, n_groups, scratch);
    return o3d_launch_status();
}

extern "C" int o3d_train_select(const int32_t* counts, int J, int B, int cap_first, int cap_template, int cap_search, int32_t* sel,
                                int32_t* n_valid, int32_t* overflow, void* stream) {
    if (!counts || !sel || !n_valid || !overflow || J < 1 || J > O3D_TRAIN_MAX_CANDIDATES || B < 1 || B > J || cap_first < 0 ||
        cap_template < 0 || cap_search < 0)
        return O3D_EINVAL;
    hipLaunchKernelGGL(train_select_kernel<false>, dim3(1), dim3(SELECT_WG), 0, o3d_stream(stream), counts, J, B, cap_first, cap_template,
                       cap_search, sel, n_valid, overflow);
    return o3d_launch_status();
}

extern "C" int o3d_train_labels(const float* gt_search, const float* sample_bb, const float* template_bb, const float* offset, int J,
                                float* search_box, float* box_label, float* bbox_size, float* model_box, void* stream) {
    if (!gt_search || !sample_bb || !template_bb || !offset || !search_box || !box_label || !bbox_size || !model_box || J < 1 ||
        J > O3D_TRAIN_MAX_CANDIDATES)
        return O3D_EINVAL;
    LabelArgs a{gt_search, sample_bb, template_bb, offset, J, search_box, box_label, bbox_size, model_box};
    hipLaunchKernelGGL(train_labels_kernel, dim3(o3d_cdiv(J, 256)), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_train_sample(const o3d_train_sample_args* args, void* stream) {
    if (!args) return O3D_EINVAL;
    const o3d_train_sample_args& a = *args;
    if (!a.sel || !a.counts || !a.crop_first || !a.crop_template || !a.crop_search || a.cap_first < 0 || a.cap_template < 0 ||
        a.cap_search < 0 || a.cap_first > (1 << 29) || a.cap_template > (1 << 29) || a.cap_search > (1 << 29) || a.J < 1 ||
        a.J > O3D_TRAIN_MAX_CANDIDATES || a.B < 1 || a.B > a.J || a.M < 1 || a.M > (1 << 20) || a.N < 1 || a.N > (1 << 20) ||
        (a.idx_t == nullptr) != (a.idx_s == nullptr) || !a.search_box || !a.model_box || !a.cand_box_label || !a.cand_bbox_size ||
        !a.template_points || !a.search_points || !a.seg_label || !a.box_label || !a.bbox_size)
        return O3D_EINVAL;
    const int rows = a.M > a.N ? a.M : a.N;
    hipLaunchKernelGGL(train_sample_kernel, dim3(o3d_cdiv(rows, 256), a.B, 2), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_track_crop_groups_aug(const o3d_crop_plan* groups, const o3d_crop_plan* dev_groups, const o3d_crop_aug* const* dev_aug,
                                         int n_groups, int32_t* scratch, long scratch_len, void* stream) {
    long wgs, rows, need;
    if (!crop_groups_plan(groups, n_groups, true, nullptr, wgs, rows, need) || !dev_groups || !scratch || scratch_len < need)
        return O3D_EINVAL;
    hipLaunchKernelGGL((crop_groups_kernel<false, true>), dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), dev_groups, n_groups, scratch,
                       dev_aug);
    hipLaunchKernelGGL(crop_groups_scan_kernel, dim3((int)rows), dim3(CROP_WG), 0, o3d_stream(stream), dev_groups, n_groups, scratch);
    hipLaunchKernelGGL((crop_groups_kernel<true, true>), dim3((int)wgs), dim3(CROP_WG), 0, o3d_stream(stream), dev_groups, n_groups, scratch,
                       dev_aug);
    return o3d_launch_status();
}

extern "C" int o3d_train_augment(const float* gt, const float* draw, const int32_t* slot_src, int K, int n_slots, float* out_box,
                                 o3d_crop_aug* aug, void* stream) {
    if (!gt || !draw || !out_box || !aug || K < 1 || K > 3 * O3D_TRAIN_MAX_CANDIDATES || n_slots < 1 ||
        n_slots > 3 * O3D_TRAIN_MAX_CANDIDATES || (!slot_src && n_slots != K))
        return O3D_EINVAL;
    AugmentArgs a{gt, draw, slot_src, K, n_slots, out_box, aug};
    hipLaunchKernelGGL(train_augment_kernel, dim3(o3d_cdiv(n_slots, 256)), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_train_draw(const float* gt, int R, const int32_t* rows, const int32_t* cand, int J, int seed, int counter, int degrees,
                              int num_candidates, int mode, float* refs, float* first, float* offs, float* aug, void* stream) {
    if (mode != O3D_TRAIN_DRAW_SIAMESE && mode != O3D_TRAIN_DRAW_MOTION && mode != O3D_TRAIN_DRAW_MOTION_AUG) return O3D_EINVAL;
    if (!gt || !rows || !cand || !refs || !offs || (mode == O3D_TRAIN_DRAW_SIAMESE && !first) || (mode == O3D_TRAIN_DRAW_MOTION_AUG && !aug) ||
        J < 1 || J > O3D_TRAIN_MAX_CANDIDATES || R < 1 || num_candidates < 1)
        return O3D_EINVAL;
    DrawArgs a{gt, R, rows, cand, J, (unsigned)seed, (unsigned)counter, degrees != 0, num_candidates, mode, refs, first, offs, aug};
    hipLaunchKernelGGL(train_draw_kernel, dim3(o3d_cdiv(J, 256)), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_train_inside_box(const float* points, int n, const float* box, float factor, int32_t* mask, void* stream) {
    if (n < 0 || n > (1 << 30) || !box || !(factor >= 0.f) || (n > 0 && (!points || !mask))) return O3D_EINVAL;
    if (n == 0) return O3D_OK;
    hipLaunchKernelGGL(train_inside_box_kernel, dim3(o3d_cdiv(n, 256)), dim3(256), 0, o3d_stream(stream), points, n, box, factor, mask);
    return o3d_launch_status();
}

extern "C" int o3d_train_motion_labels(const float* prev_gt, const float* this_gt, const float* ref_box, int J, int degrees,
                                       float motion_threshold, float* this_box, float* prev_box, float* canon_box, float* box_label,
                                       float* box_label_prev, float* motion_label, int32_t* motion_state, float* bbox_size, void* stream) {
    if (!prev_gt || !this_gt || !ref_box || !this_box || !prev_box || !canon_box || !box_label || !box_label_prev || !motion_label ||
        !motion_state || !bbox_size || J < 1 || J > O3D_TRAIN_MAX_CANDIDATES || !(motion_threshold >= 0.f))
        return O3D_EINVAL;
    MotionLabelArgs a{prev_gt, this_gt, ref_box, J, degrees != 0, motion_threshold, this_box, prev_box, canon_box, box_label,
                      box_label_prev, motion_label, motion_state, bbox_size};
    hipLaunchKernelGGL(train_motion_labels_kernel, dim3(o3d_cdiv(J, 256)), dim3(256), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_train_select_motion(const int32_t* counts, int J, int B, int cap_prev, int cap_this, int32_t* sel, int32_t* n_valid,
                                       int32_t* overflow, void* stream) {
    if (!counts || !sel || !n_valid || !overflow || J < 1 || J > O3D_TRAIN_MAX_CANDIDATES || B < 1 || B > J || cap_prev < 0 || cap_this < 0)
        return O3D_EINVAL;
    hipLaunchKernelGGL(train_select_kernel<true>, dim3(1), dim3(SELECT_WG), 0, o3d_stream(stream), counts, J, B, 0, cap_prev, cap_this, sel,
                       n_valid, overflow);
    return o3d_launch_status();
}
