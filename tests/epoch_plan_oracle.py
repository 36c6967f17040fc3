"""The numpy restatement of o3d_train_draw (the formulas at the head of open3dsot_amd/csrc/train_batch.hip): the boxes a
planned batch gathers from the pool and the random numbers it draws.  Imports nothing of the package.

    key(tag) = mix32((seed * 0x9E3779B1) ^ (counter * 0x85EBCA77 + j * 0xC2B2AE3D + tag * 0x27D4EB2F + 0x165667B1))
    h(c)     = mix32(key(tag) ^ (c * 0x9E3779B1 + 0x85EBCA77))
    u(h) = ((h >> 8) + 0.5) * 2^-24;  uniform(lo, hi) = lo + (hi - lo) * u(h);  normal(ha, hb) = sqrt(-2 log u(ha)) *
    cos(2 pi ((hb >> 8) * 2^-24)), all in double and rounded to float32 once.
"""
import numpy as np

SIAMESE, MOTION, MOTION_AUG = 0, 1, 2
TAG_JITTER, TAG_SEARCH, TAG_AUG_PREV, TAG_AUG_THIS = 2, 3, 4, 5
M32 = 0xFFFFFFFF
f32 = np.float32


def mix32(x):
    """the MurmurHash3 finaliser on uint64 arrays that hold uint32 values"""
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def key(seed, counter, j, tag):
    a = (int(seed) * 0x9E3779B1) & M32
    b = ((int(counter) * 0x85EBCA77) & M32) + np.asarray(j, np.uint64) * 0xC2B2AE3D + int(tag) * 0x27D4EB2F + 0x165667B1
    return mix32(np.uint64(a) ^ (b & M32))


def bits(k, c):
    """h(c) of the keys k"""
    return mix32(np.asarray(k, np.uint64) ^ np.uint64((int(c) * 0x9E3779B1 + 0x85EBCA77) & M32))


def u(h):
    return ((h >> 8).astype(np.float64) + 0.5) * 2.0 ** -24


def uniform64(h, lo, hi):
    return lo + (hi - lo) * u(h)


def normal64(ha, hb):
    return np.sqrt(-2.0 * np.log(u(ha))) * np.cos((2.0 * np.pi) * ((hb >> 8).astype(np.float64) * 2.0 ** -24))


def angle(degrees):
    return 5.0 if degrees else 5.0 * (np.pi / 180.0)


def jitter(seed, counter, j, cand, degrees):
    """-> (J,4) float32 rows (x, y, 0, theta): uniform +-0.3, the angle times 5 | deg2rad(5); zero for candidate id 0"""
    k = key(seed, counter, j, TAG_JITTER)
    out = np.zeros((len(k), 4), np.float64)
    out[:, 0], out[:, 1] = uniform64(bits(k, 0), -0.3, 0.3), uniform64(bits(k, 1), -0.3, 0.3)
    out[:, 3] = uniform64(bits(k, 2), -0.3, 0.3) * angle(degrees)
    out[np.asarray(cand) == 0] = 0.0
    return out.astype(f32)


def search_offset(seed, counter, j, cand, degrees, num_candidates):
    """-> (J,4) float32 rows (x, y, 0, theta): standard normals times sqrt((1, 1, 5 | deg2rad(5))); zero for candidate id 0
    when num_candidates > 1"""
    k = key(seed, counter, j, TAG_SEARCH)
    out = np.zeros((len(k), 4), np.float64)
    out[:, 0], out[:, 1] = normal64(bits(k, 0), bits(k, 1)), normal64(bits(k, 2), bits(k, 3))
    out[:, 3] = normal64(bits(k, 4), bits(k, 5)) * np.sqrt(angle(degrees))
    if num_candidates > 1:
        out[np.asarray(cand) == 0] = 0.0
    return out.astype(f32)


def augmentation(seed, counter, j, tag):
    """-> (J,6) float32 rows (tx, ty, tz, rotation in degrees, flip_x, flip_y), drawn for every candidate"""
    k = key(seed, counter, j, tag)
    out = np.zeros((len(k), 6), np.float64)
    for c in range(3):
        out[:, c] = uniform64(bits(k, c), -0.3, 0.3)
    out[:, 3] = uniform64(bits(k, 3), -10.0, 10.0)
    out[:, 4], out[:, 5] = bits(k, 4) >> 31, bits(k, 5) >> 31
    return out.astype(f32)


def gather(gt, row):
    """the boxes of the pool rows `row`; a row outside the pool gives 15 zeros"""
    row = np.asarray(row, np.int64)
    ok = (row >= 0) & (row < gt.shape[0])
    return np.where(ok[:, None], gt[np.where(ok, row, 0)], f32(0)).astype(f32)


def draw(gt, rows, cand, seed, counter, degrees, num_candidates, mode):
    """o3d_train_draw -> {refs (2J,15), offs, first (siamese), aug (motion with augmentation)}"""
    rows, cand = np.asarray(rows), np.asarray(cand)
    j = np.arange(rows.shape[0])
    first = 1 if mode == SIAMESE else 0
    out = {"refs": np.concatenate([gather(gt, rows[:, first]), gather(gt, rows[:, first + 1])]),
           "offs": jitter(seed, counter, j, cand, degrees)}
    if mode == SIAMESE:
        out["first"] = gather(gt, rows[:, 0])
        out["offs"] = np.concatenate([out["offs"], search_offset(seed, counter, j, cand, degrees, num_candidates)])
    elif mode == MOTION_AUG:
        out["aug"] = np.concatenate([augmentation(seed, counter, j, TAG_AUG_PREV), augmentation(seed, counter, j, TAG_AUG_THIS)])
    return out
