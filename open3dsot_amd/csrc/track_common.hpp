// track_common.hpp -- the device functions that csrc/track.hip (the tracking front end) and csrc/train_batch.hip (the training
// batch builder) both call: ONE definition per formula.  The fp32 operation orders are written at the head of track.hip; a
// source that includes this header is compiled with -ffp-contract=off.
#pragma once
#include "o3d_common.hpp"

namespace {

constexpr int CROP_WG = 256;

// workgroups of a cloud of n points: an empty cloud keeps one, which writes count = 0
inline int crop_wgs(int n) { return n > 0 ? o3d_cdiv(n, CROP_WG) : 1; }

// keep? and q for the point p against `box` (15), in the operation order of the header comment: THE crop test, of both
// o3d_track_crop (box in global memory) and o3d_track_crop_multi (box staged in LDS)
__device__ __forceinline__ bool crop_test(float px, float py, float pz, const float* box, float scale, float offset, int mode,
                                          float& qx, float& qy, float& qz) {
    const float dx = px - box[0], dy = py - box[1], dz = pz - box[2];
    const float w = box[3], l = box[4], h = box[5];
    const float* R = box + 6;
    bool keep = true;
    if (mode == O3D_CROP_MODEL) {
        const float s4 = 4.f * scale, o2 = 2.f * offset;
        const float L = (l * s4) * 0.5f, W = (w * s4) * 0.5f, H = (h * s4) * 0.5f;
        const float e0 = ((fabsf(R[0]) * L + fabsf(R[1]) * W) + fabsf(R[2]) * H) + o2;
        const float e1 = ((fabsf(R[3]) * L + fabsf(R[4]) * W) + fabsf(R[5]) * H) + o2;
        const float e2 = ((fabsf(R[6]) * L + fabsf(R[7]) * W) + fabsf(R[8]) * H) + o2;
        keep = fabsf(dx) < e0 && fabsf(dy) < e1 && fabsf(dz) < e2;
    }
    qx = (R[0] * dx + R[3] * dy) + R[6] * dz;
    qy = (R[1] * dx + R[4] * dy) + R[7] * dz;
    qz = (R[2] * dx + R[5] * dy) + R[8] * dz;
    const float hx = (l * scale) * 0.5f + offset, hy = (w * scale) * 0.5f + offset, hz = (h * scale) * 0.5f + offset;
    return keep && fabsf(qx) < hx && fabsf(qy) < hy && fabsf(qz) < hz;
}

// (x, y, z) = row idx[i] of src (n_src,3); zeros when `zero` is set (src and idx are then not read) or the index lies
// outside the source (a caller's bug: the row stays zero)
__device__ __forceinline__ void gather_row(const float* src, int n_src, const int32_t* idx, int i, int zero, float& x, float& y, float& z) {
    x = y = z = 0.f;
    if (zero) return;
    const int s = idx[i];
    if ((unsigned)s < (unsigned)n_src) {
        const float* p = src + 3 * (long)s;
        x = p[0]; y = p[1]; z = p[2];
    }
}

// the inclusive test of points_in_box (nuscenes geometry_utils) for the point p against `box` (15) scaled by `factor`:
// d = p - c, q = R^T d in crop_test's operation order, then |qx| <= (l*factor)*0.5 and |qy| <= (w*factor)*0.5 and |qz| <=
// (h*factor)*0.5.  THE test of the augmentation mask (crop_multi_wg<.., true>) and of both seg_label halves of
// o3d_train_motion_sample; d is returned for the caller that transforms the point
__device__ __forceinline__ bool inside_box(float px, float py, float pz, const float* box, float factor, float& dx, float& dy, float& dz) {
    dx = px - box[0]; dy = py - box[1]; dz = pz - box[2];
    const float w = box[3], l = box[4], h = box[5];
    const float* R = box + 6;
    const float qx = (R[0] * dx + R[3] * dy) + R[6] * dz;
    const float qy = (R[1] * dx + R[4] * dy) + R[7] * dz;
    const float qz = (R[2] * dx + R[5] * dy) + R[8] * dz;
    return fabsf(qx) <= (l * factor) * 0.5f && fabsf(qy) <= (w * factor) * 0.5f && fabsf(qz) <= (h * factor) * 0.5f;
}

// ---- the keyed index draw of o3d_train_sample and o3d_train_motion_sample (train_batch.hip writes it down) ------------------------
__device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

// the draw of the header comment: row i of a cloud of n > 2 rows resampled to S rows
__device__ __forceinline__ int sample_index(unsigned key, int i, int n, int S) {
    if (n == S) return i;
    if (S > n) return (int)__umulhi(mix32(key ^ ((unsigned)i * 0x9E3779B1u + 0x85EBCA77u)), (unsigned)n);
    const int b = 32 - __clz(n - 1), h = (b + 1) >> 1;
    const unsigned mask = (1u << h) - 1u;
    unsigned x = (unsigned)i;
    do {
        unsigned L = x >> h, R = x & mask;
#pragma unroll
        for (unsigned round = 0; round < 4u; ++round) {
            const unsigned f = mix32(key ^ (R * 0x9E3779B1u + round * 0x85EBCA77u + 0xC2B2AE3Du)) & mask;
            const unsigned t = L ^ f;
            L = R; R = t;
        }
        x = (L << h) | R;
    } while (x >= (unsigned)n);
    return (int)x;
}

// counter-based draw from U[-1, 1): a 32-bit mix of (seed, frame, component) (the finaliser of MurmurHash3), its top 24 bits
__device__ __forceinline__ float limit_draw(unsigned seed, unsigned frame, unsigned comp) {
    unsigned x = seed * 0x9E3779B1u ^ (frame * 0x85EBCA77u + comp * 0xC2B2AE3Du + 0x27D4EB2Fu);
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return (float)(x >> 8) * (2.f / 16777216.f) - 1.f;
}

// getOffsetBB for one target, THE box update of both o3d_track_offset_box and o3d_track_offset_box_multi (ref, offset,
// yaw_state: the target's rows; rebase, seed: the target's; k: the frame) -> box (15) and the updated yaw_state.  The
// arithmetic is a 3x3 product; carried in double so that the stored fp32 box is the rounded exact result
__device__ __forceinline__ void offset_box_one(const float* ref, const float* offset, float* yaw_state, int rebase, int degrees,
                                               int use_z, int limit_box, unsigned seed, unsigned k, float* box) {
    float off[4] = {offset[0], offset[1], offset[2], offset[3]};
    const float w = ref[3], l = ref[4], h = ref[5];
    if (limit_box) {                                  // datasets/points_utils.py:70-76, literally (no abs)
        if (off[0] > w) off[0] = limit_draw(seed, k, 0u);
        if (off[1] > fminf(l, 2.f)) off[1] = limit_draw(seed, k, 1u);
        if (use_z && off[2] > h) off[2] = 0.f;
    }
    const double theta = degrees ? (double)off[3] * (3.14159265358979323846 / 180.0) : (double)off[3];
    double R0[9], yaw = theta;
    if (yaw_state && !rebase) {
        for (int i = 0; i < 9; ++i) R0[i] = yaw_state[i];
        yaw = (double)yaw_state[9] + theta;
    } else {
        for (int i = 0; i < 9; ++i) R0[i] = ref[6 + i];
    }
    // the reference box's own rotation carries the offset into the world: R = R0 Rz(yaw before the update)
    double Rr[9];
    if (yaw_state && !rebase) {
        double s, c;
        sincos((double)yaw_state[9], &s, &c);
        for (int r = 0; r < 3; ++r) {
            Rr[3 * r] = R0[3 * r] * c + R0[3 * r + 1] * s;
            Rr[3 * r + 1] = R0[3 * r + 1] * c - R0[3 * r] * s;
            Rr[3 * r + 2] = R0[3 * r + 2];
        }
    } else {
        for (int i = 0; i < 9; ++i) Rr[i] = R0[i];
    }
    const double ox = off[0], oy = off[1], oz = use_z ? (double)off[2] : 0.0;
    for (int r = 0; r < 3; ++r) box[r] = (float)((double)ref[r] + ((Rr[3 * r] * ox + Rr[3 * r + 1] * oy) + Rr[3 * r + 2] * oz));
    box[3] = w; box[4] = l; box[5] = h;
    const float yaw_f = (float)yaw;                   // the stored state: the next update starts from exactly this value
    double s, c;
    sincos(yaw_state ? (double)yaw_f : yaw, &s, &c);
    for (int r = 0; r < 3; ++r) {
        box[6 + 3 * r] = (float)(R0[3 * r] * c + R0[3 * r + 1] * s);
        box[6 + 3 * r + 1] = (float)(R0[3 * r + 1] * c - R0[3 * r] * s);
        box[6 + 3 * r + 2] = (float)R0[3 * r + 2];
    }
    if (yaw_state) {
        if (rebase)
            for (int i = 0; i < 9; ++i) yaw_state[i] = (float)R0[i];
        yaw_state[9] = yaw_f;
    }
}

// ---- one cloud against K targets (o3d_track_crop_multi, o3d_track_crop_groups) ---------------------------------------------------
constexpr int CROP_MULTI_CHUNK = O3D_CROP_MULTI_CHUNK;      // targets staged in LDS at a time (<= 32: one keep bit each)
constexpr int CROP_MULTI_WORDS = 18;                        // box (15), scale, offset, mode
constexpr int CROP_AUG_WORDS = 28;                          // o3d_crop_aug: enabled, box (15), A (9), c' (3)
static_assert(sizeof(o3d_crop_aug) == 4 * CROP_AUG_WORDS, "o3d_crop_aug: points_utils.CROP_AUG mirrors this layout");

// the point a target with the staged augmentation record `a` (CROP_AUG_WORDS words) sees in place of p: a point inside the
// record's box scaled by 1.25 becomes p'_i = ((A_i0*dx + A_i1*dy) + A_i2*dz) + c'_i with d = p - c, every other point and
// every point of a disabled record stays p (train_batch.hip writes the order down)
__device__ __forceinline__ void aug_point(const float* a, float& x, float& y, float& z) {
    if (__float_as_int(a[0]) == 0) return;
    float dx, dy, dz;
    if (!inside_box(x, y, z, a + 1, 1.25f, dx, dy, dz)) return;
    const float* A = a + 16;
    const float* c = a + 25;
    x = ((A[0] * dx + A[1] * dy) + A[2] * dz) + c[0];
    y = ((A[3] * dx + A[4] * dy) + A[5] * dz) + c[1];
    z = ((A[6] * dx + A[7] * dy) + A[8] * dz) + c[2];
}

// Workgroup w of a group (the cloud `points` (n,3), the DEVICE table T of K targets, W = crop_wgs(n), S = the group's K rows
// of W int32 in scratch): the count pass (SCATTER false: S[k][w] = this workgroup's survivors of target k) or the scatter
// pass (SCATTER true: S[k][w] holds the survivors of the workgroups before this one).  THE body of both crop_multi_kernel
// and crop_groups_kernel; every argument is the same for all threads of the workgroup.  AUG (o3d_track_crop_groups_aug): A =
// the group's K augmentation records | NULL, staged beside par; target k tests and writes aug_point(A[k], p) in place of p
template <bool SCATTER, bool AUG = false>
__device__ __forceinline__ void crop_multi_wg(const float* __restrict__ points, int n, const o3d_crop_target* __restrict__ T, int K, int W,
                                              int32_t* __restrict__ S, int w, const o3d_crop_aug* __restrict__ A = nullptr) {
    __shared__ float par[CROP_MULTI_CHUNK][CROP_MULTI_WORDS];
    __shared__ float aug[AUG ? CROP_MULTI_CHUNK : 1][CROP_AUG_WORDS];
    __shared__ int wave_cnt[CROP_MULTI_CHUNK][CROP_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = w * CROP_WG + tid;
    const bool in = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (in) {
        const float* p = points + 3 * (long)i;
        px = p[0]; py = p[1]; pz = p[2];
    }
    for (int k0 = 0; k0 < K; k0 += CROP_MULTI_CHUNK) {
        const int nc = K - k0 < CROP_MULTI_CHUNK ? K - k0 : CROP_MULTI_CHUNK;
        __syncthreads();                                   // the previous chunk's readers are done with par / wave_cnt
        for (int e = tid; e < nc * CROP_MULTI_WORDS; e += CROP_WG) {
            const int k = e / CROP_MULTI_WORDS, f = e - k * CROP_MULTI_WORDS;
            const o3d_crop_target& J = T[k0 + k];
            par[k][f] = f < 15 ? J.box[f] : f == 15 ? J.scale : f == 16 ? J.offset : __int_as_float(J.mode);
        }
        if constexpr (AUG) {
            const float* src = reinterpret_cast<const float*>(A ? A + k0 : nullptr);      // the records are 28 words each
            for (int e = tid; e < nc * CROP_AUG_WORDS; e += CROP_WG) (&aug[0][0])[e] = src ? src[e] : 0.f;      // zero: disabled
        }
        __syncthreads();
        unsigned bits = 0u;                                // bit k: this thread's point survives target k0 + k
        for (int k = 0; k < nc; ++k) {
            float qx, qy, qz;
            bool keep;
            if constexpr (AUG) {
                float x = px, y = py, z = pz;
                aug_point(aug[k], x, y, z);
                keep = in && crop_test(x, y, z, par[k], par[k][15], par[k][16], __float_as_int(par[k][17]), qx, qy, qz);
            } else {
                keep = in && crop_test(px, py, pz, par[k], par[k][15], par[k][16], __float_as_int(par[k][17]), qx, qy, qz);
            }
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
            int pos = S[(long)(k0 + k) * W + w];           // the survivors of the workgroups before this one (launch 2)
            for (int v = 0; v < wave; ++v) pos += wave_cnt[k][v];
            pos += __popcll(mask & ((1ull << lane) - 1ull));
            const o3d_crop_target& J = T[k0 + k];
            if (pos < J.capacity) {
                float qx, qy, qz;
                if constexpr (AUG) {
                    float x = px, y = py, z = pz;
                    aug_point(aug[k], x, y, z);
                    crop_test(x, y, z, par[k], par[k][15], par[k][16], __float_as_int(par[k][17]), qx, qy, qz);
                } else {
                    crop_test(px, py, pz, par[k], par[k][15], par[k][16], __float_as_int(par[k][17]), qx, qy, qz);
                }
                float* o = J.out + 3 * (long)pos;
                o[0] = qx; o[1] = qy; o[2] = qz;
            }
        }
    }
}

// One (group, target) row of W counts -> its exclusive prefix sums in place, count[0] = the row's total: THE scan of both
// crop_multi_scan_kernel and crop_groups_scan_kernel, run by one workgroup
__device__ __forceinline__ void crop_scan_row(int32_t* __restrict__ row, int W, int32_t* count) {
    __shared__ int wave_sum[CROP_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int w0 = 0; w0 < W; w0 += CROP_WG) {
        const int w = w0 + tid;
        const int v = w < W ? row[w] : 0;
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int u = 0; u < CROP_WG / 64; ++u) {
            if (u < wave) before += wave_sum[u];
            total += wave_sum[u];
        }
        if (w < W) row[w] = carry + before + incl - v;
        carry += total;
        __syncthreads();                                   // wave_sum is rewritten by the next pass
    }
    if (tid == 0) count[0] = carry;
}

}  // namespace
