// The lifecycle of a scene tracker's K slots as device work (tracking.ManagedSceneTracker / ManagedMotionSceneTracker; DESIGN.md
// section 12j): after frame t's o3d_track_offset_box_multi, ONE launch of ONE workgroup that
//
//   matches      the K tracks with the frame's detections, greedily, on the (K,D) overlap / distance matrices that
//                o3d_scene_pair_scores (csrc/metrics.hip) wrote
//   counts       each slot's missed frames and starved crops
//   retires      the slots that are lost
//   enrolls      the unmatched detections into the free slots, with the writes of tracking.SceneTracker.enroll
//   writes       the next frame's lane table and row t of the three logs
//
// ---- the written order (tests/scene_manage_oracle.py restates it in numpy) ---------------------------------------------------------
// t = frame[0] - 1;  n = has_dets ? min(max(n_det[0], 0), D) : 0.  Slot k is `active on entry` when active[k] != 0.
//   admissible(k,d)   active on entry && d < n && overlaps[k,d] >= min_iou && distances[k,d] <= max_dist   (fp32 compares)
//   order             pair p comes before pair q when, in this order of tests, p's overlap is larger, p's distance is smaller,
//                     p's k is smaller, p's d is smaller
//   match             walk the admissible pairs in that order; take a pair when match[k] and det_match[d] are both still -1
//   counters          active on entry: has_dets ? (misses = match[k] >= 0 ? 0 : misses + 1);
//                     min_points > 0 ? (starved = counts[2 k + count_col] < min_points ? starved + 1 : 0)
//   retire            active on entry && (misses > max_misses || (min_points > 0 && starved > max_starved)): active = 0, id = -1
//   enroll            (enroll != 0) the j-th (from 0) detection d < n with det_match[d] < 0 and 15 finite numbers, in ascending d,
//                     takes the j-th free slot (active == 0 after retire) in ascending k; id = next_id + j; detections beyond
//                     the free slots are `dropped`; next_id += the number enrolled
//   lanes, logs       as include/o3dsot.h states them
//
// ---- the match without a sort --------------------------------------------------------------------------------------------------------
// The order is strict and total, so the walk's result is unique.  Call a pair whose ends are both still free a mutual first when
// it comes first among the free admissible pairs of its row AND first among the free admissible pairs of its column.  The walk
// takes every mutual first: when it reaches the pair both ends are still free, because only a pair that shares an end with it
// could have used one up, and all of those come later.  Taking the mutual firsts and repeating on what is left therefore gives
// the walk's result; the first free pair of all is always a mutual first, so every round takes at least one pair until no free
// admissible pair is left.
//   kept state   per track k its row's first pair among the free detections (row_first[k] = its d), per detection d its column's
//                first pair among the free tracks (col_first[d] = its k), in LDS.  A wave scans a row or a column of the two
//                matrices in global memory, 64 entries at a time, and a wave64 butterfly picks the first.
//   a round      (k, d) is taken when row_first[k] == d and col_first[d] == k; all such pairs at once.  A kept pair stays the
//                first of its row (column) as long as its own detection (track) is free, so ONLY the rows whose kept detection
//                and the columns whose kept track were just taken are scanned again.
// Tracks that each have their own nearest detection are matched in one round; the worst case (every pair tied) is one take per
// round, min(K, n) rounds.  The matrices are never rescanned as a whole.  No atomics anywhere: every LDS or global word has one
// writer between two barriers, so the result is a function of the inputs.
//
// Thread i owns track i (i < K) and detection i (i < D); the workgroup always has 1024 threads, so that the first scan of the K rows
// and n columns is spread over 16 waves.  A round costs three barriers (four with a scan); two of them also carry a vote: whether
// any pair was taken (else the match is complete) and whether any row or column asked for a new scan.
//
// The same file holds o3d_scene_mot_walk, which scores such a run afterwards: it calls the same match,
// greedy_match below, once per frame; its own written order stands above its kernel.
#include "o3d_common.hpp"

namespace {

constexpr int SCENE_MAX = 1024;
static_assert(O3D_CROP_MULTI_MAX_TARGETS <= SCENE_MAX && O3D_SCENE_MAX_DETECTIONS <= SCENE_MAX, "one thread per track and per detection");
static_assert(O3D_SCENE_SLOT_COLS == 4, "slot = {id, misses, starved, start}");

struct ManageArgs {
    const float* overlaps; const float* distances; const float* dets; const int32_t* n_det;
    float* cur; float* yaw_state; float* canon_wlh; float* results; const int32_t* frame;
    int32_t* active; int32_t* slot; int32_t* next_id; const int32_t* counts; int32_t* bank_state_next; int32_t* lanes;
    int32_t* ids_log; int32_t* match_log; int32_t* dropped_log;
    int K, D, T, count_col, rule, max_misses, min_points, max_starved, enroll, has_dets;
    float min_iou, max_dist;
    int cost;
};

struct Cand { float ov, di; int k, d; };       // d < 0: none

__device__ __forceinline__ bool before(const Cand& p, const Cand& q) {
    if (p.d < 0) return false;
    if (q.d < 0) return true;
    if (p.ov != q.ov) return p.ov > q.ov;
    if (p.di != q.di) return p.di < q.di;
    if (p.k != q.k) return p.k < q.k;
    return p.d < q.d;
}

// the first of the 64 lanes' candidates, in every lane
__device__ __forceinline__ Cand wave_first(Cand c) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        Cand o{__shfl_xor(c.ov, m, 64), __shfl_xor(c.di, m, 64), __shfl_xor(c.k, m, 64), __shfl_xor(c.d, m, 64)};
        if (before(o, c)) c = o;
    }
    return c;
}

// the number of threads below this one whose flag is set, and the number of all: ballots per wave, the wave sums through LDS
__device__ __forceinline__ int block_rank(bool flag, int* s_cnt, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) s_cnt[w] = __popcll(b);
    __syncthreads();
    int base = 0, all = 0;
    for (int i = 0; i < nw; ++i) {
        base += i < w ? s_cnt[i] : 0;
        all += s_cnt[i];
    }
    __syncthreads();                                   // s_cnt is free again
    total = all;
    return base + __popcll(b & ((1ull << lane) - 1ull));
}

// The match without a sort (above), for both kernels of this file: rows k < K against columns d < n of two matrices of row
// stride D.  On entry, behind a barrier: s_match[k] / s_dmatch[d] = -1 for a free row / column (>= 0: taken before the call, or
// not in play), s_act[k] != 0 for a row in play, s_d = s_k = -1, s_need[k] = row k is in play and free (and n > 0), s_cneed[d] =
// column d < n is free.  On return, behind a barrier: s_match / s_dmatch hold the walk's result on the free rows and columns.
// Called by all 1024 threads.
__device__ __forceinline__ void greedy_match(const float* overlaps, const float* distances, int K, int D, int n, float min_iou,
                                             float max_dist, int* s_d, int* s_need, int* s_k, int* s_cneed, int* s_match,
                                             int* s_dmatch, const int* s_act) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    const bool mine = tid < K;
    bool scan = n > 0;                                 // the same in every thread: some row or column is to be scanned
    for (;;) {
        if (scan) {
            for (int i = w; i < K + n; i += nw) {      // the rows [0, K) and the columns [K, K + n) to scan, a wave each
                const bool row = i < K;
                const int r = row ? i : i - K;
                if (!(row ? s_need[r] : s_cneed[r])) continue;      // the same word in all 64 lanes
                Cand c{0.f, 0.f, -1, -1};
                for (int j = lane; j < (row ? n : K); j += 64) {
                    const int k = row ? r : j, d = row ? j : r;
                    if (row ? s_dmatch[d] >= 0 : (!s_act[k] || s_match[k] >= 0)) continue;
                    const Cand x{overlaps[(long)k * D + d], distances[(long)k * D + d], k, d};
                    if (x.ov >= min_iou && x.di <= max_dist && before(x, c)) c = x;
                }
                c = wave_first(c);
                if (lane == 0) {
                    if (row) { s_d[r] = c.d; s_need[r] = 0; }
                    else { s_k[r] = c.d >= 0 ? c.k : -1; s_cneed[r] = 0; }
                }
            }
            __syncthreads();
        }
        const int d = mine ? s_d[tid] : -1;            // >= 0: in play, still unmatched, and its row has a free pair
        const bool win = d >= 0 && s_k[d] == tid;      // a mutual first
        if (!__syncthreads_or(win)) break;             // no free admissible pair is left (the first of all is always mutual)
        if (win) { s_match[tid] = d; s_dmatch[d] = tid; s_d[tid] = -1; s_k[d] = -1; }
        __syncthreads();
        const bool row_again = d >= 0 && !win && s_dmatch[d] >= 0;         // its kept detection was taken by another track
        const int k = tid < n ? s_k[tid] : -1;
        const bool col_again = k >= 0 && s_match[k] >= 0;                  // its kept track took another detection
        if (row_again) s_need[tid] = 1;
        if (col_again) s_cneed[tid] = 1;
        scan = __syncthreads_or(row_again || col_again) != 0;
    }
    __syncthreads();
}

// ---- optimal_match: maximum-cardinality, minimum-cost assignment ---------------------------------------------
// The rule (tests/assign_oracle.py restates it in Python ints), on what greedy_match takes:
//   admissible(r,c)   greedy_match's test on a free row in play and a free column c < n: overlaps[r,c] >= min_iou &&
//                     distances[r,c] <= max_dist, fp32 compares, a NaN is never admissible
//   q(r,c)            the int32 cost of an admissible pair, in [0, 2^20]; each product is one rounded fp32 multiply
//                       O3D_COST_DISTANCE  (int) rintf(fminf(fmaxf(di, 0.f), 1024.f) * 1024.f)          unit 1/1024 m, >= 1024 m ties
//                       O3D_COST_OVERLAP   (int) rintf((1.f - fminf(fmaxf(ov, 0.f), 1.f)) * 1048576.f)
//   objective         of the one-to-one sets of admissible pairs: the most pairs, and among those the smallest sum of q.  That is
//                     the minimum-sum assignment of the matrix with q on the admissible pairs, one private `stay unmatched`
//                     column per row at BIG = 2^32, and the inadmissible pairs excluded.  Columns are numbered real c = c, dummy of
//                     row r = SCENE_MAX + r.  Potentials, lengths and sums are int64: at 1024 rows a sum stays under 2^42.
//   which optimum     u[r] = 0, v[c] = 0.  The free rows in play are inserted in ascending r, each by ONE shortest augmenting path
//                     on the reduced costs q(r,c) - u[r] - v[c] (BIG - u[r] for the dummy, whose v stays 0: see below):
//                       start     no column has a length or is used; the current row is i at length 0, reached from no column
//                       a step    every unused real column c admissible to the current row r0 (reached from column j0 at length
//                                 L) gets the tentative length L + q(r0,c) - u[r0] - v[c] when that is STRICTLY smaller than the
//                                 one it has, and then remembers j0 as its predecessor; the dummy of r0 gets L + BIG - u[r0].  The
//                                 next column is the unused one with a length of the smallest length; of equal lengths the lowest
//                                 column number (so a real column before a dummy one).  A dummy column or a real column that no
//                                 row holds ends the path, at length Dend.  Otherwise the column is used, its row is the next
//                                 current row, reached from this column at its length.
//                       potentials   a used column c of length d: v[c] += d - Dend and u[its row] += Dend - d; u[i] += Dend
//                       augment   from the end column backwards along the predecessors every column takes the row its predecessor
//                                 held, the first column of the path takes i.  A path that ends in the dummy of row t leaves t
//                                 unmatched for good.
// The dummy of row t is only ever reached from t, so it can only end a path, never lie inside one: it is never `used`, its v
// stays 0, a row that went to its dummy is never visited again and the matched rows only grow.  Lengths are kept absolute (the
// per-step subtraction of the textbook form shifts every unused column alike and changes no comparison).
//
// Thread c owns real column c and the dummy of row c: v, the two lengths, `used` and the row held when it became used live in
// its registers.  LDS: u as two int32 halves (in greedy_match's s_d / s_k), the predecessor of every real column (in its s_cneed,
// read into a register first), column -> row in s_dmatch and row -> column in s_match (the result arrays themselves), the rows to
// insert in s_need as handed in.  A step is one coalesced read of row r0's two entries per thread, a wave64 butterfly on (length,
// column, the row that holds it) and ONE barrier: the 16 wave results go through a double-buffered LDS table that every thread
// reads.  Thread 0 walks the augmentation while the others update the potentials (disjoint words) or are still reading the last
// step's table: nothing the augmentation writes is read between the last step's barrier and the one that ends the insertion.  Every loop has a
// bound that the data cannot move: K insertions, K + 1 steps (a step uses up a matched row, or ends), K + 1 links.  No atomics.
// Contract on entry and return: greedy_match's (s_d and s_k need not be -1).  Called by all 1024 threads.
constexpr long long ASSIGN_BIG = 1ll << 32, ASSIGN_INF = 1ll << 62;
constexpr int ASSIGN_NONE = 2 * SCENE_MAX;             // no column: after every real (c) and dummy (SCENE_MAX + r) number

__device__ __forceinline__ int assign_cost(float ov, float di, int cost) {
    return cost == O3D_COST_OVERLAP ? (int)rintf((1.f - fminf(fmaxf(ov, 0.f), 1.f)) * 1048576.f)
                                    : (int)rintf(fminf(fmaxf(di, 0.f), 1024.f) * 1024.f);
}

struct PathEnd { long long len; int col, row; };       // row: the row that holds the column (-1: none, or a dummy column)

__device__ __forceinline__ bool shorter(const PathEnd& p, const PathEnd& q) { return p.len < q.len || (p.len == q.len && p.col < q.col); }

__device__ __forceinline__ long long u_read(const int* s_ulo, const int* s_uhi, int r) {
    return (long long)(((unsigned long long)(unsigned)s_uhi[r] << 32) | (unsigned)s_ulo[r]);
}

__device__ __forceinline__ void optimal_match(const float* overlaps, const float* distances, int K, int D, int n, float min_iou,
                                              float max_dist, int cost, int* s_ulo, const int* s_need, int* s_uhi, int* s_way,
                                              int* s_match, int* s_dmatch) {
    __shared__ long long s_len[2][SCENE_MAX / 64];     // the 16 waves' shortest, double-buffered over the steps
    __shared__ int s_col[2][SCENE_MAX / 64], s_row[2][SCENE_MAX / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool col_ok = tid < n && s_way[tid] != 0;    // s_way arrives as s_cneed: column tid < n is free
    long long v = 0;
    s_ulo[tid] = 0;
    s_uhi[tid] = 0;
    __syncthreads();
    int buf = 0;
    for (int i = 0; i < K; ++i) {
        if (!s_need[i]) continue;                      // the same word in every thread
        long long dist = ASSIGN_INF, ddist = ASSIGN_INF, l0 = 0, dend = 0;
        bool used = false;
        int urow = -1, r0 = i, j0 = -1, jend = ASSIGN_NONE;
        // the row that holds column tid, read HERE, behind the barrier that ended the last augmentation: thread 0 rewrites
        // s_dmatch while slower threads are still deciding whether the path has ended, so that decision must not read it
        const int hold = col_ok ? s_dmatch[tid] : -1;
        for (int step = 0; step <= K; ++step) {
            const long long base = l0 - u_read(s_ulo, s_uhi, r0);
            if (col_ok && !used) {
                const float ov = overlaps[(long)r0 * D + tid], di = distances[(long)r0 * D + tid];
                if (ov >= min_iou && di <= max_dist) {
                    const long long cand = base + assign_cost(ov, di, cost) - v;
                    if (cand < dist) { dist = cand; s_way[tid] = j0; }
                }
            }
            if (tid == r0) ddist = base + ASSIGN_BIG;
            PathEnd p{ASSIGN_INF, ASSIGN_NONE, -1};
            if (!used && dist < ASSIGN_INF) p = PathEnd{dist, tid, hold};
            if (ddist < ASSIGN_INF && shorter(PathEnd{ddist, SCENE_MAX + tid, -1}, p)) p = PathEnd{ddist, SCENE_MAX + tid, -1};
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const PathEnd o{__shfl_xor(p.len, m, 64), __shfl_xor(p.col, m, 64), __shfl_xor(p.row, m, 64)};
                if (shorter(o, p)) p = o;
            }
            if (lane == 0) { s_len[buf][w] = p.len; s_col[buf][w] = p.col; s_row[buf][w] = p.row; }
            __syncthreads();
            p = PathEnd{s_len[buf][0], s_col[buf][0], s_row[buf][0]};
#pragma unroll
            for (int x = 1; x < SCENE_MAX / 64; ++x) {
                const PathEnd o{s_len[buf][x], s_col[buf][x], s_row[buf][x]};
                if (shorter(o, p)) p = o;
            }
            buf ^= 1;
            if (p.col >= ASSIGN_NONE) break;           // no column has a length: cannot happen, i's own dummy always has one
            const int r = p.row;
            if (r < 0) { jend = p.col; dend = p.len; break; }
            if (tid == p.col) { used = true; urow = r; }
            r0 = r;
            j0 = p.col;
            l0 = p.len;
        }
        if (jend < ASSIGN_NONE) {                      // the same in every thread
            if (used) {                                // one writer per row: a row is held by one column
                v += dist - dend;
                const long long u = u_read(s_ulo, s_uhi, urow) + (dend - dist);
                s_ulo[urow] = (int)(unsigned)(unsigned long long)u;
                s_uhi[urow] = (int)(unsigned)((unsigned long long)u >> 32);
            }
            if (tid == i) {
                const long long u = u_read(s_ulo, s_uhi, i) + dend;
                s_ulo[i] = (int)(unsigned)(unsigned long long)u;
                s_uhi[i] = (int)(unsigned)((unsigned long long)u >> 32);
            }
            if (tid == 0) {
                int c = jend;
                if (c >= SCENE_MAX) {                  // the dummy of row t: t stays, or becomes, unmatched
                    const int t = c - SCENE_MAX;
                    c = t == i ? -1 : s_match[t];
                    s_match[t] = -1;
                }
                for (int link = 0; link <= K && c >= 0; ++link) {
                    const int pc = s_way[c];
                    const int r = pc < 0 ? i : s_dmatch[pc];
                    s_dmatch[c] = r;
                    s_match[r] = c;
                    c = pc;
                }
            }
        }
        __syncthreads();
    }
}

// the match of both kernels of this file, by the rule the launch names
template <int RULE>
__device__ __forceinline__ void scene_match(const float* overlaps, const float* distances, int K, int D, int n, float min_iou,
                                            float max_dist, int cost, int* s_d, int* s_need, int* s_k, int* s_cneed, int* s_match,
                                            int* s_dmatch, const int* s_act) {
    if constexpr (RULE == O3D_ASSIGN_GREEDY)
        greedy_match(overlaps, distances, K, D, n, min_iou, max_dist, s_d, s_need, s_k, s_cneed, s_match, s_dmatch, s_act);
    else
        optimal_match(overlaps, distances, K, D, n, min_iou, max_dist, cost, s_d, s_need, s_k, s_cneed, s_match, s_dmatch);
}

template <int RULE>
__global__ __launch_bounds__(SCENE_MAX) void manage_kernel(ManageArgs a) {
    __shared__ int s_d[SCENE_MAX], s_need[SCENE_MAX];            // per track: row_first (-1: none); the row is to be scanned
    __shared__ int s_k[SCENE_MAX], s_cneed[SCENE_MAX];           // per detection: col_first (-1: none); the column is to be scanned
    __shared__ int s_match[SCENE_MAX], s_dmatch[SCENE_MAX];
    __shared__ int s_act[SCENE_MAX];                             // per track: active on entry
    __shared__ int s_free[SCENE_MAX], s_newid[SCENE_MAX];        // the free slots in ascending k; per slot: enrolled ? its id : -1
    __shared__ int s_cnt[16];
    const int tid = threadIdx.x;
    const int K = a.K, D = a.D;
    const int t = a.frame[0] - 1;
    const int n = (a.has_dets && D > 0) ? min(max(a.n_det[0], 0), D) : 0;
    const int next0 = a.next_id[0];
    const bool mine = tid < K;
    const bool act_in = mine && a.active[tid] != 0;
    s_match[tid] = -1;
    s_dmatch[tid] = -1;
    s_d[tid] = -1;
    s_k[tid] = -1;
    s_newid[tid] = -1;
    s_act[tid] = act_in;
    s_need[tid] = act_in && n > 0;
    s_cneed[tid] = tid < n;
    __syncthreads();

    scene_match<RULE>(a.overlaps, a.distances, K, D, n, a.min_iou, a.max_dist, a.cost, s_d, s_need, s_k, s_cneed, s_match, s_dmatch,
                      s_act);

    // counters and retire, slot tid
    int id = -1, misses = 0, starved = 0, start = 0;
    bool act = act_in;
    if (mine) {
        const int32_t* s = a.slot + O3D_SCENE_SLOT_COLS * tid;
        id = s[0]; misses = s[1]; starved = s[2]; start = s[3];
    }
    const int id_in = id;
    if (act_in) {
        if (a.has_dets) misses = s_match[tid] >= 0 ? 0 : misses + 1;
        if (a.min_points > 0) starved = a.counts[2 * tid + a.count_col] < a.min_points ? starved + 1 : 0;
        if (misses > a.max_misses || (a.min_points > 0 && starved > a.max_starved)) { act = false; id = -1; }
    }

    // enroll: the j-th unmatched finite detection takes the j-th free slot
    bool wants = a.enroll && tid < n && s_dmatch[tid] < 0;
    if (wants) {
        const float* b = a.dets + 15 * (long)tid;
        for (int i = 0; i < 15; ++i) wants = wants && isfinite(b[i]);
    }
    int n_free, n_want;
    const int r_free = block_rank(mine && !act, s_cnt, n_free);
    const int r_want = block_rank(wants, s_cnt, n_want);
    if (mine && !act) s_free[r_free] = tid;
    __syncthreads();
    if (wants && r_want < n_free) {
        const int k = s_free[r_want];
        const float* b = a.dets + 15 * (long)tid;
        for (int i = 0; i < 15; ++i) {
            a.cur[15 * (long)k + i] = b[i];
            if (t >= 0 && t < a.T) a.results[15 * ((long)t * K + k) + i] = b[i];
        }
        for (int i = 0; i < 9; ++i) a.yaw_state[10 * (long)k + i] = b[6 + i];
        a.yaw_state[10 * (long)k + 9] = 0.f;
        for (int i = 0; i < 3; ++i) a.canon_wlh[3 * (long)k + i] = b[3 + i];
        if (a.bank_state_next) { a.bank_state_next[2 * k] = 0; a.bank_state_next[2 * k + 1] = 0; }
        s_newid[k] = next0 + r_want;
    }
    __syncthreads();

    // the slot row, the lane row and the logs, slot tid
    if (mine) {
        const int nid = s_newid[tid];
        const bool first = nid >= 0;
        int32_t* s = a.slot + O3D_SCENE_SLOT_COLS * tid;
        s[0] = first ? nid : id;
        s[1] = first ? 0 : misses;
        s[2] = first ? 0 : starved;
        s[3] = first ? t : start;
        a.active[tid] = (first || act) ? 1 : 0;
        int32_t* l = a.lanes + O3D_LANE_COLS * tid;
        l[O3D_LANE_ACTIVE] = 1;
        l[O3D_LANE_FIRST] = first ? 1 : 0;
        l[O3D_LANE_HAS_CROP] = (first || a.rule != O3D_BANK_FIRST) ? 1 : 0;
        l[O3D_LANE_T] = 0;
        l[O3D_LANE_ROW] = -1;
        l[O3D_LANE_REF_ROW] = -1;
        l[O3D_LANE_REBASE] = 0;
        if (t >= 0 && t < a.T) {
            a.ids_log[(long)t * K + tid] = first ? nid : id_in;
            a.match_log[(long)t * K + tid] = s_match[tid];
        }
    }
    if (tid == 0) {
        const int taken = min(n_want, n_free);
        a.next_id[0] = next0 + taken;
        if (t >= 0 && t < a.T) a.dropped_log[t] = n_want - taken;
    }
}

// ---- o3d_scene_mot_walk: the CLEAR-MOT bookkeeping of a tracked run (metrics.ClearMOT) -----------------------
// One workgroup walks frames 0..F-1 of a chunk in order, the loop over the frames inside the kernel; what a frame hands to the
// next -- per ground-truth object g the id it was last matched to, whether it was matched at its most recent valid frame, whether
// it was ever matched -- lives in the registers of thread g and is read from / written back to device memory at the two ends, so
// a sequence may be walked in several calls.  Thread i owns object i (i < G) and column i (i < K).
//
// The written order per frame f (tests/mot_oracle.py restates it in numpy); ov, di = the frame's (G,K) matrices:
//   admissible(g,k)   gt_valid[f,g] != 0 && hyp_ids[f,k] >= 0 && ov[g,k] >= min_iou && di[g,k] <= max_dist   (fp32 compares; a
//                     NaN is never admissible)
//   carry             for g ascending, g valid and last_id[g] >= 0: k = the LOWEST column with hyp_ids[f,k] == last_id[g] (the
//                     non-negative ids of a frame are meant to be distinct); when k exists, (g,k) is admissible and no smaller g
//                     took column k: match[g] = k.  A kept identity wins over a better-scoring new pairing; of two objects that
//                     remember one id the lower g gets it.
//                     Here: thread g finds its k and tests the pair; thread k then takes the lowest g that asked for it.
//   rest              greedy_match (above, o3d_scene_manage's own walk: overlap descending, distance ascending, g ascending, k
//                     ascending) over the admissible pairs whose two ends are both still free
//   count             per valid g, matched: tp++; idsw++ when last_id[g] >= 0 && last_id[g] != hyp_ids[f,match[g]]; frag++ when
//                     ever[g] && !tracked_prev[g]; then last_id[g] = that id, ever[g] = 1, tracked_prev[g] = 1.  Unmatched: fn++,
//                     tracked_prev[g] = 0.  An invalid g leaves its state untouched.  fp = the columns with an id left unmatched.
//   rows              match_slot[f,g] = k | -1, match_id[f,g] = hyp_ids[f,k] | -1, match_ov / match_di[f,g] = ov / di[g,k] copied,
//                     -1 / +inf when g is invalid or unmatched; per_frame[f] = {gt, hyp, tp, fp, fn, idsw, frag, 0}
// No atomics, no flag a thread waits on: between two barriers every LDS or global word has one writer.  A column without an id is
// handed to greedy_match as taken (s_dmatch = G, no object's index).  The sums of a frame: a ballot per wave and counter, the 16
// wave counts through LDS, thread 0 adds them.
constexpr int WALK_SUMS = 6;                           // valid objects, columns with an id, tp, fp, idsw, frag

struct WalkArgs {
    const float* overlaps; const float* distances; const int32_t* gt_valid; const int32_t* hyp_ids;
    int32_t* last_id; int32_t* tracked_prev; int32_t* ever;
    int32_t* match_slot; int32_t* match_id; float* match_ov; float* match_di; int32_t* per_frame;
    int F, G, K;
    float min_iou, max_dist;
    int cost;
};

template <int RULE>
__global__ __launch_bounds__(SCENE_MAX) void mot_walk_kernel(WalkArgs a) {
    __shared__ int s_d[SCENE_MAX], s_need[SCENE_MAX];            // greedy_match's, rows = objects
    __shared__ int s_k[SCENE_MAX], s_cneed[SCENE_MAX];           // and columns = the K slots
    __shared__ int s_match[SCENE_MAX], s_dmatch[SCENE_MAX];
    __shared__ int s_act[SCENE_MAX];                             // per object: valid in this frame
    __shared__ int s_ids[SCENE_MAX], s_carry[SCENE_MAX];         // per column: its id; per object: the column it asks to keep
    __shared__ int s_cnt[16 * WALK_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    const int G = a.G, K = a.K;
    const bool mine = tid < G, col = tid < K;
    int last = -1;
    bool prev = false, ever = false;
    if (mine) { last = a.last_id[tid]; prev = a.tracked_prev[tid] != 0; ever = a.ever[tid] != 0; }
    for (int f = 0; f < a.F; ++f) {
        const float* ov = a.overlaps + (long)f * G * K;
        const float* di = a.distances + (long)f * G * K;
        const int id = col ? a.hyp_ids[(long)f * K + tid] : -1;
        const bool valid = mine && a.gt_valid[(long)f * G + tid] != 0;
        s_ids[tid] = id;
        s_act[tid] = valid;
        s_match[tid] = -1;
        s_dmatch[tid] = id >= 0 ? -1 : G;
        s_d[tid] = -1;
        s_k[tid] = -1;
        __syncthreads();

        // carry: object tid asks for the lowest column that holds the id it remembers
        int c = -1;
        if (valid && last >= 0) {
            for (int k = 0; k < K; ++k)
                if (s_ids[k] == last) { c = k; break; }
            if (c >= 0 && !(ov[(long)tid * K + c] >= a.min_iou && di[(long)tid * K + c] <= a.max_dist)) c = -1;
        }
        s_carry[tid] = c;
        __syncthreads();
        if (id >= 0) {                                 // column tid goes to the lowest object that asked for it
            for (int g = 0; g < G; ++g)
                if (s_carry[g] == tid) { s_match[g] = tid; s_dmatch[tid] = g; break; }
        }
        __syncthreads();
        s_need[tid] = valid && s_match[tid] < 0;
        s_cneed[tid] = col && s_dmatch[tid] < 0;
        __syncthreads();

        scene_match<RULE>(ov, di, G, K, K, a.min_iou, a.max_dist, a.cost, s_d, s_need, s_k, s_cneed, s_match, s_dmatch, s_act);

        // count, object tid and column tid
        const int m = valid ? s_match[tid] : -1;
        const bool matched = m >= 0;
        const int mid = matched ? s_ids[m] : -1;
        const bool flags[WALK_SUMS] = {valid, id >= 0, matched, id >= 0 && s_dmatch[tid] < 0, matched && last >= 0 && last != mid,
                                       matched && ever && !prev};
        if (valid) {
            if (matched) { last = mid; ever = true; }
            prev = matched;
        }
        if (mine) {
            const long o = (long)f * G + tid;
            a.match_slot[o] = m;
            a.match_id[o] = mid;
            a.match_ov[o] = matched ? ov[(long)tid * K + m] : -1.f;
            a.match_di[o] = matched ? di[(long)tid * K + m] : __int_as_float(0x7f800000);
        }
#pragma unroll
        for (int i = 0; i < WALK_SUMS; ++i) {
            const unsigned long long b = __ballot(flags[i]);
            if (lane == 0) s_cnt[w * WALK_SUMS + i] = __popcll(b);
        }
        __syncthreads();                               // the frame's LDS has been read by everyone: the next frame may write it
        if (tid == 0) {
            int sum[WALK_SUMS];
#pragma unroll
            for (int i = 0; i < WALK_SUMS; ++i) {
                sum[i] = 0;
                for (int j = 0; j < nw; ++j) sum[i] += s_cnt[j * WALK_SUMS + i];
            }
            int32_t* row = a.per_frame + 8 * (long)f;
            row[0] = sum[0]; row[1] = sum[1]; row[2] = sum[2]; row[3] = sum[3];
            row[4] = sum[0] - sum[2]; row[5] = sum[4]; row[6] = sum[5]; row[7] = 0;
        }
    }
    if (mine) { a.last_id[tid] = last; a.tracked_prev[tid] = prev ? 1 : 0; a.ever[tid] = ever ? 1 : 0; }
}

// ---- o3d_scene_assign: the match alone, as an operator and as the per-call pin of the two rules ---------------
// One workgroup: sets up greedy_match's entry contract from row_active / n_col, calls the rule's device function and writes
// match, col_match and summary = {pairs, the sum of q over the pairs under `cost`} (ballots would not do for an int64 sum: a
// wave64 butterfly, the 16 wave sums through LDS, thread 0 adds them in wave order).
struct AssignArgs {
    const float* overlaps; const float* distances; const int32_t* row_active; const int32_t* n_col;
    int32_t* match; int32_t* col_match; long long* summary;
    int K, D, cost;
    float min_iou, max_dist;
};

template <int RULE>
__global__ __launch_bounds__(SCENE_MAX) void assign_kernel(AssignArgs a) {
    __shared__ int s_d[SCENE_MAX], s_need[SCENE_MAX], s_k[SCENE_MAX], s_cneed[SCENE_MAX];
    __shared__ int s_match[SCENE_MAX], s_dmatch[SCENE_MAX], s_act[SCENE_MAX];
    __shared__ long long s_sum[SCENE_MAX / 64];
    __shared__ int s_cnt[SCENE_MAX / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int K = a.K, D = a.D;
    const int n = a.n_col ? min(max(a.n_col[0], 0), D) : D;
    const bool act = tid < K && (!a.row_active || a.row_active[tid] != 0);
    s_match[tid] = -1;
    s_dmatch[tid] = -1;
    s_d[tid] = -1;
    s_k[tid] = -1;
    s_act[tid] = act;
    s_need[tid] = act && n > 0;
    s_cneed[tid] = tid < n;
    __syncthreads();

    scene_match<RULE>(a.overlaps, a.distances, K, D, n, a.min_iou, a.max_dist, a.cost, s_d, s_need, s_k, s_cneed, s_match, s_dmatch, s_act);

    const int m = tid < K ? s_match[tid] : -1;
    if (tid < K) a.match[tid] = m;
    if (tid < D) a.col_match[tid] = s_dmatch[tid];
    long long q = m >= 0 ? assign_cost(a.overlaps[(long)tid * D + m], a.distances[(long)tid * D + m], a.cost) : 0;
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) q += __shfl_xor(q, x, 64);
    const unsigned long long b = __ballot(m >= 0);
    if (lane == 0) { s_sum[w] = q; s_cnt[w] = __popcll(b); }
    __syncthreads();
    if (tid == 0) {
        long long pairs = 0, sum = 0;
        for (int x = 0; x < SCENE_MAX / 64; ++x) { pairs += s_cnt[x]; sum += s_sum[x]; }
        a.summary[0] = pairs;
        a.summary[1] = sum;
    }
}

bool assign_known(int assignment, int cost) {
    return (assignment == O3D_ASSIGN_GREEDY || assignment == O3D_ASSIGN_OPTIMAL) && (cost == O3D_COST_DISTANCE || cost == O3D_COST_OVERLAP);
}

}  // namespace

extern "C" int o3d_scene_assign(const float* overlaps, const float* distances, const int32_t* row_active, const int32_t* n_col, int K,
                                int D, float min_iou, float max_dist, int assignment, int cost, int32_t* match, int32_t* col_match,
                                int64_t* summary, void* stream) {
    if (K < 1 || K > O3D_CROP_MULTI_MAX_TARGETS || D < 1 || D > O3D_SCENE_MAX_DETECTIONS || !assign_known(assignment, cost))
        return O3D_EINVAL;
    if (!overlaps || !distances || !match || !col_match || !summary) return O3D_EINVAL;
    AssignArgs a{overlaps, distances, row_active, n_col, match, col_match, (long long*)summary, K, D, cost, min_iou, max_dist};
    if (assignment == O3D_ASSIGN_OPTIMAL)
        hipLaunchKernelGGL(assign_kernel<O3D_ASSIGN_OPTIMAL>, dim3(1), dim3(SCENE_MAX), 0, o3d_stream(stream), a);
    else
        hipLaunchKernelGGL(assign_kernel<O3D_ASSIGN_GREEDY>, dim3(1), dim3(SCENE_MAX), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_scene_mot_walk_assign(const float* overlaps, const float* distances, const int32_t* gt_valid, const int32_t* hyp_ids,
                                         int F, int G, int K, float min_iou, float max_dist, int32_t* last_id, int32_t* tracked_prev,
                                         int32_t* ever, int32_t* match_slot, int32_t* match_id, float* match_ov, float* match_di,
                                         int32_t* per_frame, int assignment, int cost, void* stream) {
    if (F < 0 || F > O3D_SCENE_MOT_MAX_FRAMES || G < 1 || G > O3D_CROP_MULTI_MAX_TARGETS || K < 1 || K > O3D_CROP_MULTI_MAX_TARGETS ||
        !assign_known(assignment, cost))
        return O3D_EINVAL;
    if (!overlaps || !distances || !gt_valid || !hyp_ids || !last_id || !tracked_prev || !ever || !match_slot || !match_id ||
        !match_ov || !match_di || !per_frame)
        return O3D_EINVAL;
    if (F == 0) return O3D_OK;
    WalkArgs a{overlaps, distances, gt_valid, hyp_ids, last_id, tracked_prev, ever, match_slot, match_id, match_ov, match_di, per_frame,
               F, G, K, min_iou, max_dist, cost};
    if (assignment == O3D_ASSIGN_OPTIMAL)
        hipLaunchKernelGGL(mot_walk_kernel<O3D_ASSIGN_OPTIMAL>, dim3(1), dim3(SCENE_MAX), 0, o3d_stream(stream), a);
    else
        hipLaunchKernelGGL(mot_walk_kernel<O3D_ASSIGN_GREEDY>, dim3(1), dim3(SCENE_MAX), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_scene_mot_walk(const float* overlaps, const float* distances, const int32_t* gt_valid, const int32_t* hyp_ids, int F,
                                  int G, int K, float min_iou, float max_dist, int32_t* last_id, int32_t* tracked_prev, int32_t* ever,
                                  int32_t* match_slot, int32_t* match_id, float* match_ov, float* match_di, int32_t* per_frame,
                                  void* stream) {
    return o3d_scene_mot_walk_assign(overlaps, distances, gt_valid, hyp_ids, F, G, K, min_iou, max_dist, last_id, tracked_prev, ever,
                                     match_slot, match_id, match_ov, match_di, per_frame, O3D_ASSIGN_GREEDY, O3D_COST_DISTANCE, stream);
}

extern "C" int o3d_scene_manage_assign(const float* overlaps, const float* distances, const float* dets, const int32_t* n_det, int K,
                                       int D, float* cur, float* yaw_state, float* canon_wlh, float* results, int T,
                                       const int32_t* frame, int32_t* active, int32_t* slot, int32_t* next_id, const int32_t* counts,
                                       int count_col, int32_t* bank_state_next, int32_t* lanes, int rule, int32_t* ids_log,
                                       int32_t* match_log, int32_t* dropped_log, float min_iou, float max_dist, int max_misses,
                                       int min_points, int max_starved, int enroll, int has_dets, int assignment, int cost,
                                       void* stream) {
    if (K < 1 || K > O3D_CROP_MULTI_MAX_TARGETS || D < 0 || D > O3D_SCENE_MAX_DETECTIONS || T < 1 || (count_col != 0 && count_col != 1) ||
        rule < -1 || rule > O3D_BANK_ALL || !assign_known(assignment, cost))
        return O3D_EINVAL;
    if (D > 0 && (!overlaps || !distances || !dets || !n_det)) return O3D_EINVAL;
    if (!cur || !yaw_state || !canon_wlh || !results || !frame || !active || !slot || !next_id || !counts || !lanes || !ids_log ||
        !match_log || !dropped_log)
        return O3D_EINVAL;
    ManageArgs a{overlaps, distances, dets, n_det, cur, yaw_state, canon_wlh, results, frame, active, slot, next_id, counts,
                 bank_state_next, lanes, ids_log, match_log, dropped_log, K, D, T, count_col, rule, max_misses, min_points,
                 max_starved, enroll, has_dets, min_iou, max_dist, cost};
    if (assignment == O3D_ASSIGN_OPTIMAL)
        hipLaunchKernelGGL(manage_kernel<O3D_ASSIGN_OPTIMAL>, dim3(1), dim3(SCENE_MAX), 0, o3d_stream(stream), a);
    else
        hipLaunchKernelGGL(manage_kernel<O3D_ASSIGN_GREEDY>, dim3(1), dim3(SCENE_MAX), 0, o3d_stream(stream), a);
    return o3d_launch_status();
}

extern "C" int o3d_scene_manage(const float* overlaps, const float* distances, const float* dets, const int32_t* n_det, int K, int D,
                                float* cur, float* yaw_state, float* canon_wlh, float* results, int T, const int32_t* frame,
                                int32_t* active, int32_t* slot, int32_t* next_id, const int32_t* counts, int count_col,
                                int32_t* bank_state_next, int32_t* lanes, int rule, int32_t* ids_log, int32_t* match_log,
                                int32_t* dropped_log, float min_iou, float max_dist, int max_misses, int min_points, int max_starved,
                                int enroll, int has_dets, void* stream) {
    return o3d_scene_manage_assign(overlaps, distances, dets, n_det, K, D, cur, yaw_state, canon_wlh, results, T, frame, active, slot,
                                   next_id, counts, count_col, bank_state_next, lanes, rule, ids_log, match_log, dropped_log, min_iou,
                                   max_dist, max_misses, min_points, max_starved, enroll, has_dets, O3D_ASSIGN_GREEDY,
                                   O3D_COST_DISTANCE, stream);
}
