"""numpy restatement of the three entry points of the free-running tracking loop (open3dsot_amd/csrc/track.hip:
o3d_track_resample_drawn, o3d_track_bank_update, o3d_track_motion_input_drawn), built from the oracles of their parts: the
keyed index draw (sampler_oracle.sample_indices / draw_key), the row gather (tracking_oracle.resample) and the motion input's
rows (motion_oracle.motion_input).  Integer arithmetic is exact and rows are copied, so the GPU tests compare bit for bit.
Test infrastructure only -- the product has no CPU path."""
import numpy as np

import motion_oracle as MO
import sampler_oracle as SO
import tracking_oracle as TO

f32 = np.float32
RULES = ("first", "previous", "firstandprevious", "all")


def keys(seed):
    """the two keys of a free-running tracker: cloud 0 (template / previous frame), cloud 1 (search / current frame)"""
    return SO.draw_key(seed, 0, 0, 0), SO.draw_key(seed, 0, 0, 1)


def bank_update(state, crop_rows, rule, first, has_crop, bank, bank_cap):
    """o3d_track_bank_update.  state = (fixed, total); crop_rows (nm,3): the staged crop, already cut to its buffer; bank
    (bank_cap,3) is written in place -> the new (fixed, total)"""
    fixed, total = int(state[0]), int(state[1])
    if not has_crop:
        return fixed, total
    assert rule in RULES
    crop_rows = np.asarray(crop_rows, f32).reshape(-1, 3)
    nm = crop_rows.shape[0]
    twice = rule == "firstandprevious" and first
    slot = total if rule == "all" else fixed if rule == "firstandprevious" and not first else 0
    for start in (slot, nm) if twice else (slot,):
        keep = max(0, min(nm, bank_cap - start))           # rows at or beyond bank_cap are dropped
        bank[start:start + keep] = crop_rows[:keep]
    return (nm if first else fixed), min(2 * nm if twice else slot + nm, bank_cap)


def resample_drawn(src, n, cap, key, S):
    """one job of o3d_track_resample_drawn: src (>= min(n, cap) rows), the device count n -> (dst (S,3) float32, used (S,) int32)"""
    n = min(int(n), int(cap))
    idx = SO.sample_indices(key, n, S)
    if idx is None:
        return TO.resample(None, None, S, zero=True), np.full(S, -1, np.int32)
    assert idx.min() >= 0 and idx.max() < n
    return TO.resample(np.asarray(src, f32)[:n], idx, S), idx.astype(np.int32)


def motion_input_drawn(prev, cur, counts, cap, key_pair, N, wlh, first_frame, with_bc=True):
    """o3d_track_motion_input_drawn -> (points (2N,5), candidate_bc (2N,9) | None, used (2N,) int32)"""
    ns = [min(int(c), int(cap)) for c in counts]
    drawn = [SO.sample_indices(k, n, N) for k, n in zip(key_pair, ns)]
    used = np.concatenate([np.full(N, -1, np.int64) if d is None else d for d in drawn]).astype(np.int32)
    pts, bc = MO.motion_input(np.asarray(prev, f32)[:ns[0]], np.asarray(cur, f32)[:ns[1]], np.maximum(used, 0), N, wlh, first_frame,
                              zero=(drawn[0] is None, drawn[1] is None), with_bc=with_bc)
    return pts, bc, used
