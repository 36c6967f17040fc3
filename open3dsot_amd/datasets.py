"""Dataset readers that leave the frames in HBM: the KITTI tracking set, the Waymo SOT set and nuScenes as
sampler.DeviceTracklets.

KittiTracklets mirrors the reference's kittiDataset (datasets/kitti.py) with coordinate_mode `velodyne` / `camera` and
preload_offset: the same scene list per split string, the same tracklet list (order of first appearance of track_id in the
category-filtered label file, frames sorted by frame number, gaps kept), the same boxes (fp64 on the host, cast to float32
only when packed as [centre | wlh | rotation row-major]) and the same preload crop per annotated object per frame
(crop_pc_axis_aligned with offset = preload_offset), bit for bit -- but the crop runs on the device (csrc/preload.hip):

    host     parse label_02/<scene>.txt and calib/<scene>.txt, compute boxes and crop bounds in fp64 (plain Python + numpy)
    host     read each distinct (scene, frame) .bin ONCE into a pinned buffer, up to chunk_frames frames per chunk
    upload   one copy per chunk (x y z intensity as they lie in the file), one small copy for the tables
    device   o3d_preload_count (2 launches), the counts read back (the chunk's one synchronisation), o3d_preload_scatter
    result   every tracklet frame is a contiguous (count,3) view of ONE pool tensor: no per-frame allocation, no copy

Quirks of the reference that are kept: a velodyne file that is missing (or whose length is no multiple of four floats) gives
the single point (0,0,0), untransformed and uncropped (its bare `except`); an existing empty file gives a (0,3) frame; a box
that keeps no point gives a (0,3) frame; the strict compares `mini < p < maxi` of the float32 coordinate against the fp64
bound; in camera mode the transformed coordinate is rounded to float32 before the compare; a calibration line whose values
do not reshape to 3x4 is skipped.  With preload_offset <= 0 the reference does not crop and all tracklets of a frame share
one cloud object; here they share one slice of the pool.

save(file) / KittiTracklets.load(file) stand in for the reference's pickle cache: one file with the pool, the row offsets,
the boxes and the meta; loading is one upload.  There is no CPU fallback: a CPU device raises.

WaymoTracklets mirrors the reference's WaymoDataset with preloading (datasets/waymo_data.py): the tracklets of
sot_infos_<category>_<split>.pkl in the dict's order, one pickle per lidar frame and one per annotation frame, every frame
with its own vehicle-to-global pose.  The host computes poses and boxes in fp64 (waymo_annotations); the device transforms
the (n,3) float32 rows by the pose of their frame and crops them (o3d_preload_posed_count / o3d_preload_posed_scatter), the
fp64 result rounded to float32 once, as the reference stores it back into its float32 array.  Quirks kept: `test` reads the
`val` files; the annotation file is the lidar file's name with EVERY `lidar` replaced by `annos`; the pose's rotation goes
through a quaternion and back; length and width of the box are swapped; with preload_offset <= 0 nothing is cropped but the
points are still transformed.  Two stated deviations: points_xyz must be float32 (ValueError otherwise; the reference would
keep a float64 array unrounded); and with preload_offset <= 0 the bounds are -inf / +inf under the same strict compares, so a
point whose transformed coordinate is NaN or infinite is dropped where the reference, which does not compare at all, keeps it.  Non-preloading access (which swaps length and width back on a second read) is not restated.

NuScenesTracklets mirrors the reference's NuScenesDataset with preloading (datasets/nuscenes_data.py) without the devkit:
nuscenes_annotations reads the nine JSON tables the reference touches, restates the one piece of the devkit's reverse indexing
it relies on (sample['data']['LIDAR_TOP']: the sample's key-frame sample_data record on that channel, the last in table order),
filters the instances (scene of the first annotation in the split, its num_lidar_pts >= min_points, category among the general
classes of the tracking class) and follows `next`; boxes are centre = translation, wlh = size, rotation = the matrix of the
normalised quaternion, in fp64.  The .pcd.bin sweeps (x y z intensity ring, 20 bytes a row) go into the pinned buffer as they
lie; the device takes every point sensor -> ego -> global by two rounded rigid steps (o3d_preload_steps_count /
o3d_preload_steps_scatter): the reference's rotate / translate pairs store into a float32 array, four roundings a point.
translate="float64" is the rule of numpy >= 2 (an np.float64 scalar added to a float32 array: an fp64 sum rounded on
assignment), translate="float32" the rule of numpy < 2 (the scalar demoted: an fp32 add).  The split lists live in the devkit:
pass scenes= where it is absent.  Quirks kept: a sweep whose length is no multiple of 20 bytes raises ValueError, a missing
one FileNotFoundError, an empty one gives a (0,3) frame; key_frame_only cannot drop a frame of a well-formed set (the index
above only holds key frames) but the flag and the reference's `continue` are kept; the same -inf / +inf bounds and the same NaN
deviation as the Waymo reader with preload_offset <= 0.  Not restated: non-preloading access, and the devkit's loading and
checking of the tables the reference never reads (attribute, visibility, log, map).

The three readers differ in how they parse and in what a raw frame is (kitti_items, waymo_items, nuscenes_items: one
PreloadItem per distinct raw frame); the rest is stated once: preload_chunks cuts the items into chunks, PreloadChunk is the
device half of a chunk, and _PoolTracklets runs the chunks, fills the row table, assembles the views and holds save / load.
"""
import ast
import collections
import json
import os
import pickle

import numpy as np
import torch

from . import points_utils as PU
from .sampler import DeviceTracklet, DeviceTracklets

_NAMED = ("Car", "Van", "Truck", "Pedestrian", "Person_sitting", "Cyclist", "Tram", "Misc")
_ALL = ("Car", "Van", "Pedestrian", "Cyclist")


def kitti_scene_list(split):
    """kittiDataset._build_scene_list: substring tests on the upper-cased split, in this order"""
    s = split.upper()
    if "TRAIN" in s:
        scenes = [0] if "TINY" in s else range(0, 17)
    elif "VALID" in s:
        scenes = [18] if "TINY" in s else range(17, 19)
    elif "TEST" in s:
        scenes = [19] if "TINY" in s else range(19, 21)
    else:
        scenes = range(21)
    return ["%04d" % i for i in scenes]


def read_kitti_calib(path):
    """_read_calib_file: name -> (3,4) float64; a line whose values are no floats or do not reshape to 3x4 is skipped"""
    data = {}
    with open(path) as f:
        for line in f:
            values = line.split()
            if not values:
                continue
            try:
                data[values[0]] = np.array([float(x) for x in values[1:]], np.float64).reshape(3, 4)
            except ValueError:
                pass
    return data


def _keep_type(category_name):
    if category_name in _NAMED:
        return lambda t: t == category_name
    if category_name == "All":
        return lambda t: t in _ALL
    return lambda t: t != "DontCare"


def _quat(axis, angle):
    """the unit quaternion (w, x, y, z) of a rotation by `angle` radians about `axis`"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


def _quat_mul(a, b):
    """the Hamilton product a b"""
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _quat_matrix(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _quat_from_matrix(m):
    """the unit quaternion (w, x, y, z) of the rotation matrix m[:3,:3] (Shepperd's method: the largest of the trace and the
    diagonal picks the branch), normalised"""
    m = np.asarray(m, np.float64)
    t = np.trace(m[:3, :3])
    if t > 0:
        s = 2 * np.sqrt(1 + t)
        q = [s / 4, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
    else:
        i = int(np.argmax([m[0, 0], m[1, 1], m[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2 * np.sqrt(1 + m[i, i] - m[j, j] - m[k, k])
        q = [0.0, 0.0, 0.0, 0.0]
        q[0] = (m[k, j] - m[j, k]) / s
        q[1 + i] = s / 4
        q[1 + j] = (m[j, i] + m[i, j]) / s
        q[1 + k] = (m[k, i] + m[i, k]) / s
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


def kitti_box(anno, velo_to_cam, coordinate_mode):
    """The box of _get_frame_from_anno in fp64 -> (15,) [centre | wlh | rotation row-major].  anno: height, width, length, x,
    y, z, rotation_y; velo_to_cam (4,4).  The rotation is composed as the reference composes it, as a product of two
    axis-angle quaternions: about (0,0,-1) by rotation_y then by 90 degrees (velodyne), about y by rotation_y then about x by
    pi/2 (camera)"""
    h, w, l, x, y, z, ry = anno
    if coordinate_mode == "velodyne":
        centre = np.dot(np.linalg.inv(velo_to_cam), np.array([x, y - h / 2, z, 1.0]))[:3]
        rot = _quat_matrix(_quat_mul(_quat([0, 0, -1], ry), _quat([0, 0, -1], 90 * np.pi / 180.0)))
    else:
        centre = np.array([x, y - h / 2, z])
        rot = _quat_matrix(_quat_mul(_quat([0, 1, 0], ry), _quat([1, 0, 0], np.pi / 2)))
    return np.concatenate([centre, [w, l, h], rot.reshape(-1)]).astype(np.float64)


def kitti_annotations(path, split, category_name="Car", coordinate_mode="velodyne"):
    """The host half of the reader (no device): -> a list of tracklets, each a dict with scene, track_id, frames (T,) int64,
    boxes (T,15) float64, in the reference's order; and {scene: velo_to_cam (4,4)}."""
    if coordinate_mode not in ("velodyne", "camera"):
        raise ValueError("coordinate_mode must be 'velodyne' or 'camera'")
    keep = _keep_type(category_name)
    tracklets, calibs = [], {}
    for scene in kitti_scene_list(split):
        rows = {}                                 # track_id -> [(frame, anno)], in order of first appearance (dicts keep it)
        with open(os.path.join(path, "label_02", scene + ".txt")) as f:
            for line in f:
                v = line.split()
                if not v:
                    continue
                if len(v) != 17:
                    raise ValueError("%s/label_02/%s.txt: a line of %d fields, not 17" % (path, scene, len(v)))
                if keep(v[2]):
                    rows.setdefault(int(v[1]), []).append((int(v[0]), tuple(float(x) for x in v[10:17])))
        if not rows:
            continue
        calib = read_kitti_calib(os.path.join(path, "calib", scene + ".txt"))
        velo_to_cam = calibs[scene] = np.vstack((calib["Tr_velo_cam"], np.array([0.0, 0.0, 0.0, 1.0])))
        for track_id, annos in rows.items():
            annos.sort(key=lambda a: a[0])
            tracklets.append({"scene": scene, "track_id": track_id, "frames": np.array([a[0] for a in annos], np.int64),
                              "boxes": np.stack([kitti_box(a[1], velo_to_cam, coordinate_mode) for a in annos])})
    return tracklets, calibs


def round_up_f32(m):
    """the smallest float32 >= m, elementwise, for fp64 m"""
    m = np.asarray(m, np.float64)
    with np.errstate(over="ignore"):
        f = m.astype(np.float32)
        return np.where(f.astype(np.float64) < m, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def round_down_f32(m):
    """the largest float32 <= m, elementwise, for fp64 m"""
    m = np.asarray(m, np.float64)
    with np.errstate(over="ignore"):
        f = m.astype(np.float32)
        return np.where(f.astype(np.float64) > m, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


_SIGNS = np.array([[1, 1, 1, 1, -1, -1, -1, -1], [1, -1, -1, 1, 1, -1, -1, 1], [1, 1, -1, -1, 1, 1, -1, -1]], np.float64)


def preload_bounds(boxes, offset):
    """boxes (B,15) fp64 -> (B,6) float32 [lo xyz | hi xyz]: min / max over the corners of Box.corners -+ offset in fp64, lo
    rounded down and hi rounded up to float32; offset <= 0: -inf / +inf (the reference does not crop)"""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 15)
    out = np.empty((boxes.shape[0], 6), np.float32)
    if offset <= 0:
        out[:, :3], out[:, 3:] = -np.inf, np.inf
        return out
    for b, box in enumerate(boxes):
        w, l, h = box[3:6]
        corners = np.dot(box[6:15].reshape(3, 3), _SIGNS * (np.array([l, w, h]) / 2)[:, None]) + box[0:3, None]
        out[b, :3] = round_down_f32(corners.min(1) - offset)
        out[b, 3:] = round_up_f32(corners.max(1) + offset)
    return out


def velodyne_rows(path):
    """rows of a velodyne .bin as the reference reads it (np.fromfile(float32).reshape(-1, 4)); -1: missing or unreadable as
    (n,4), which the reference turns into the single point (0,0,0)"""
    try:
        floats = os.path.getsize(path) // 4
    except OSError:
        return -1
    return floats // 4 if floats % 4 == 0 else -1


def copy_rows(host, rows, n):
    """the row loader for frames that are already arrays on the host: a copy into the pinned buffer"""
    host[:] = rows


def _read_rows(host, path, n):
    """the default row loader: a velodyne .bin (n rows of four floats) or a NuScenes .pcd.bin (n rows of five), straight into
    the pinned buffer"""
    with open(path, "rb") as f:
        got = f.readinto(host)
    if got != host.nbytes:
        raise OSError("%s changed while it was read" % path)


# a distinct raw frame as the planner and the chunk see it: the row loader's source, its raw rows, bounds (k,6) float32, per box
# the (tracklet, frame index) pairs that take its rows, the key a chunk may not mix (KITTI: the scene, for a chunk has one
# transform) and what the frame adds to the chunk's transform keyword (KITTI: the scene's transform, Waymo: the pose,
# NuScenes: the steps)
PreloadItem = collections.namedtuple("PreloadItem", "source n bounds users group extra", defaults=(None, None))


def frame_boxes(annos, users, preload_offset):
    """-> (bounds (k,6) float32, [[(tracklet, frame index)] per box]) of one raw frame.  preload_offset <= 0: no crop, one
    box of -inf / +inf whose slice all users share, as they share one cloud in the reference; otherwise a box per user"""
    if preload_offset <= 0:
        return preload_bounds(np.zeros((1, 15)), preload_offset), [users]
    return preload_bounds(np.stack([annos[k]["boxes"][t] for k, t in users]), preload_offset), [[u] for u in users]


def preload_chunks(items, chunk_frames, max_rows=PU.PRELOAD_MAX_ROWS, max_records=PU.PRELOAD_MAX_FRAMES, max_boxes=PU.PRELOAD_MAX_BOXES):
    """The cut rule of every reader (pure host): yields the PreloadItems of `items` in order, as lists.  A chunk holds at most
    chunk_frames items, one group, max_rows raw rows and max_records frame records (an item with k boxes takes
    max(1, ceil(k / max_boxes))); its first item is always taken, and preload_plan refuses one that is too large alone.
    `items` is pulled lazily: when a chunk is yielded, at most the one item that closed it has been pulled beyond it."""
    chunk, nrows, nrec = [], 0, 0
    for item in items:
        rec = max(1, -(-len(item.bounds) // max_boxes))
        if chunk and (item.group != chunk[0].group or nrows + item.n > max_rows or nrec + rec > max_records):
            yield chunk
            chunk, nrows, nrec = [], 0, 0
        chunk.append(item)
        nrows, nrec = nrows + item.n, nrec + rec
        if len(chunk) == chunk_frames:
            yield chunk
            chunk, nrows, nrec = [], 0, 0
    if chunk:
        yield chunk


class PreloadChunk:
    """The device half for one chunk of raw frames: plan, upload, count, read back, scatter.
      files            [(source, n rows)]; a raw row is row_floats floats
      bounds_per_file  for each file a (k,6) float32 array of bounds, k >= 0
      loader           loader(host rows (n,row_floats), source, n) fills one file's rows of the pinned buffer.  Default:
                       _read_rows (source is a path), with poses copy_rows (source is the (n,row_floats) array itself)
    and one of three transforms, which picks the pair of launches:
      transform        one (3,4) fp64 for the chunk | None; row_floats 4                              o3d_preload_*
      poses            one (3,4) fp64 PER FILE; row_floats 3 | 4                                      o3d_preload_posed_*
      steps            one (n_steps,12) fp64 block PER FILE, a chain of rounded rigid steps whose translation is added
                       in fp64 and rounded (translate32 = 0) or in fp32 (1); row_floats 3 | 4 | 5     o3d_preload_steps_*
    The stages are separate methods so that tools/preload_bench.py can time them; run() is the sequence the readers use."""

    def __init__(self, files, bounds_per_file, transform, device, pinned=None, row_floats=4, loader=None, poses=None, steps=None,
                 translate32=0):
        assert poses is None or (transform is None and len(poses) == len(files))
        assert steps is None or (transform is None and poses is None and len(steps) == len(files))
        assert row_floats == 4 or poses is not None or steps is not None
        self.device, self.transform = device, transform
        self.loader = loader if loader is not None else copy_rows if poses is not None else _read_rows
        recs, rec_file, row = [], [], 0
        for i, ((_, n), b) in enumerate(zip(files, bounds_per_file)):
            for k0 in range(0, len(b), PU.PRELOAD_MAX_BOXES):       # a frame with more boxes than a record takes: more records
                recs.append((row, n, 0, min(PU.PRELOAD_MAX_BOXES, len(b) - k0), 0, 0))
                rec_file.append(i)                                  # ... that carry the frame's pose or steps each
            row += n
        self.files, self.raw_rows = files, row
        self.frames = np.array(recs, np.int32).reshape(-1, PU.PRELOAD_COLS)
        self.need, self.wgs, self.B = PU.preload_plan(self.frames, row)
        self.bounds = np.concatenate([np.asarray(b, np.float32).reshape(-1, 6) for b in bounds_per_file] + [np.zeros((0, 6), np.float32)])
        assert self.bounds.shape[0] == self.B
        # what the launches take besides transform: nothing | poses (records,12) | steps (records,n_steps,12) and translate32
        rec_file, self.per_record, self.how = np.array(rec_file, np.int64), {}, {}
        if poses is not None:
            self.per_record["poses"] = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12)[rec_file])
        if steps is not None:
            steps = np.asarray(steps, np.float64).reshape((len(files), -1, 12) if len(files) else (0, 1, 12))
            self.per_record["steps"], self.how["translate32"] = np.ascontiguousarray(steps[rec_file]), int(translate32)
        if pinned is None or pinned.shape[0] < row or pinned.shape[1] != row_floats:
            pinned = torch.empty((max(row, 1), row_floats), dtype=torch.float32).pin_memory()
        self.pinned = pinned

    def read(self):
        host, row = self.pinned.numpy(), 0
        for source, n in self.files:
            if n > 0:
                self.loader(host[row:row + n], source, n)
            row += n

    def upload(self):
        dev = self.device
        self.raw = self.pinned[:self.raw_rows].to(dev, non_blocking=True)
        # one copy for the tables; frames and bounds are 24 bytes a row: the doubles behind them are aligned
        tables = [self.frames, self.bounds] + list(self.per_record.values())
        t = torch.from_numpy(np.concatenate([x.reshape(-1).view(np.uint8) for x in tables])).to(dev)
        nf, nb = self.frames.size * 4, self.bounds.size * 4
        self.dev_frames, self.dev_bounds = t[:nf].view(torch.int32), t[nf:nf + nb].view(torch.float32)
        for name, x in self.per_record.items():
            self.how[name] = t[nf + nb:].view(torch.float64).view(x.shape)
        self.scratch = torch.empty((self.need,), dtype=torch.int32, device=dev)
        self.counts = torch.empty((self.B,), dtype=torch.int32, device=dev)

    def count(self):
        PU.preload_count(self.raw, self.frames, self.dev_frames, self.dev_bounds, self.transform, self.scratch, self.counts, **self.how)

    def read_back(self):
        """-> counts (B,) int64 on the host; allocates the chunk's pool segment and uploads every box's first row"""
        counts = self.counts.cpu().numpy().astype(np.int64)
        self.first = np.concatenate([[0], np.cumsum(counts)])
        self.pool = torch.empty((int(self.first[-1]), 3), dtype=torch.float32, device=self.device)
        self.out_row = torch.from_numpy(self.first[:-1].copy()).to(self.device)
        return counts

    def scatter(self):
        PU.preload_scatter(self.raw, self.frames, self.dev_frames, self.dev_bounds, self.transform, self.scratch, self.out_row, self.pool,
                           **self.how)

    def run(self):
        self.read()
        self.upload()
        self.count()
        counts = self.read_back()
        self.scatter()
        return counts


def _frame_users(annos, key=lambda a, frame: int(frame)):
    """{key of a distinct raw frame: [(tracklet, frame index)] that crop it}, in order of first use"""
    users = {}
    for k, a in enumerate(annos):
        for t, frame in enumerate(a["frames"]):
            users.setdefault(key(a, frame), []).append((k, t))
    return users


_STR = (str, str)                                 # an info field as written by save and parsed by load: a string as it stands,
_LITERAL = (repr, ast.literal_eval)               # ... or a Python literal that comes back as it was given


class _PoolTracklets(DeviceTracklets):
    """what the readers share: the chunk loop, every frame a view of ONE pool tensor, the cache and the reference's counting
    accessors.  A reader declares INFO, the attributes that save writes into `info` as (name, (write, parse)), and CHUNK, the
    keywords of its PreloadChunks: kind, what the items' extras are (default "transform", one for the chunk | "poses" |
    "steps", one per file), and row_floats.  meta[k] = (key, the files of the frames) unless it overrides _pack_meta /
    _unpack_meta."""
    INFO, CHUNK = (), {}

    @classmethod
    def _device(cls, device, chunk_frames=1):
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("%s: CPU not supported (the frames live on a GPU)" % cls.__name__)
        if not 1 <= int(chunk_frames) <= PU.PRELOAD_MAX_FRAMES:
            raise ValueError("1 <= chunk_frames <= %d" % PU.PRELOAD_MAX_FRAMES)
        return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())

    @classmethod
    def preload_chunk(cls, items, device, pinned=None, **kw):
        """the PreloadChunk of one list that preload_chunks yielded"""
        kw = {**cls.CHUNK, **kw}
        kind, extras = kw.pop("kind", "transform"), [item.extra for item in items]
        if kind != "transform":
            kw[kind] = extras
        return PreloadChunk([(item.source, item.n) for item in items], [item.bounds for item in items],
                            extras[0] if kind == "transform" else None, device, pinned, **kw)

    def _preload(self, dev, annos, meta, items, chunk_frames, missing=(), **chunk_kw):
        """runs the chunks of `items` (PreloadItems, pulled lazily) and assembles the tracklets over the pool: the chunks'
        segments in order, then one origin point per (tracklet, frame index) of `missing`"""
        rows = [np.zeros((len(a["frames"]), 2), np.int64) for a in annos]
        segments, base, pinned = [], 0, None
        with torch.cuda.device(dev):
            for chunk_items in preload_chunks(items, chunk_frames):
                chunk = self.preload_chunk(chunk_items, dev, pinned, **chunk_kw)
                counts = chunk.run()
                pinned, b = chunk.pinned, 0
                for item in chunk_items:
                    for who in item.users:
                        for k, f in who:
                            rows[k][f] = (base + chunk.first[b], counts[b])
                        b += 1
                segments.append(chunk.pool)
                base += int(chunk.first[-1])
            for k, f in missing:
                rows[k][f] = (base, 1)
                base += 1
            segments.append(torch.zeros((len(missing), 3), dtype=torch.float32, device=dev))
            pool = segments[0] if len(segments) == 1 else torch.cat(segments)
        self._assemble(pool, rows, [a["boxes"] for a in annos], meta)

    def _assemble(self, pool, rows, boxes64, meta):
        self.pool, self.rows, self.boxes64, self.meta = pool, rows, boxes64, meta
        del self[:]
        for r, b in zip(rows, boxes64):
            self.append(DeviceTracklet([pool[int(s):int(s) + int(c)] for s, c in r], b.astype(np.float32).reshape(-1, 15)))

    # ---- the reference's accessors ------------------------------------------------------------------------------------------
    def get_num_tracklets(self):
        return len(self)

    def get_num_frames_total(self):
        return sum(len(t) for t in self)

    def get_num_frames_tracklet(self, tracklet_id):
        return len(self[tracklet_id])

    def get_frames(self, seq_id, frame_ids):
        t, (key, files) = self[seq_id], self.meta[seq_id]
        return [{"pc": t.frames[f], "3d_bbox": t.boxes[f], "meta": (key, files[f])} for f in frame_ids]

    # ---- the cache ----------------------------------------------------------------------------------------------------------
    def _pack_meta(self):
        return dict(keys=np.array([m[0] for m in self.meta], dtype=np.str_),
                    files=np.array([f for m in self.meta for f in m[1]], dtype=np.str_))

    def _unpack_meta(self, z, cut):
        return [(str(k), [str(f) for f in fs]) for k, fs in zip(z["keys"], cut(z["files"]))]

    def save(self, file):
        """one file: the pool, the row offsets, the boxes (fp64) and the meta"""
        cat = lambda xs, shape, dt: np.concatenate(list(xs) + [np.zeros(shape, dt)])      # noqa: E731
        arrays = dict(pool=self.pool.cpu().numpy(), lengths=np.array([len(t) for t in self], np.int64),
                      rows=cat(self.rows, (0, 2), np.int64), boxes=cat(self.boxes64, (0, 15), np.float64), **self._pack_meta(),
                      info=np.array([write(getattr(self, name)) for name, (write, _) in self.INFO]))
        with open(file, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, file, device=None):
        """the tracklets that save(file) wrote: one upload, the frames are views of the pool again"""
        dev = cls._device(device)
        self = cls.__new__(cls)
        DeviceTracklets.__init__(self)
        with np.load(file) as z:
            ends = np.cumsum(z["lengths"])
            cut = lambda a: np.split(a, ends[:-1]) if len(ends) else []      # noqa: E731
            self.path = None
            for (name, (_, parse)), s in zip(cls.INFO, z["info"]):
                setattr(self, name, parse(str(s)))
            self._assemble(torch.from_numpy(z["pool"]).to(dev), cut(z["rows"]), cut(z["boxes"]), self._unpack_meta(z, cut))
        return self


def kitti_items(path, annos, calibs, coordinate_mode, preload_offset):
    """-> (the PreloadItems of every distinct (scene, frame) in order of first use, the (tracklet, frame index) pairs whose
    velodyne file is missing or unreadable as (n,4): the reference's `except` gives those one point at the origin)"""
    items, missing = [], []
    for (scene, frame), who in _frame_users(annos, lambda a, frame: (a["scene"], int(frame))).items():
        file = os.path.join(path, "velodyne", scene, "%06d.bin" % frame)
        n = velodyne_rows(file)
        if n < 0:
            missing += who
        else:
            transform = np.ascontiguousarray(calibs[scene][:3]) if coordinate_mode == "camera" else None
            items.append(PreloadItem(file, n, *frame_boxes(annos, who, preload_offset), scene, transform))
    return items, missing


class KittiTracklets(_PoolTracklets):
    """KittiTracklets(path, split, ...): the tracklets of the KITTI tracking set under `path` (velodyne/, label_02/, calib/),
    cropped as the reference preloads them, resident in HBM.  A sampler.DeviceTracklets: goes unchanged into tracking.evaluate
    and DeviceBatchSampler.  meta[k] = (scene, track_id, frame numbers); pool = the one (rows,3) tensor all frames view;
    rows[k] = (T,2) int64 [first pool row, count] of tracklet k's frames."""
    INFO = (("split", _STR), ("category_name", _STR), ("coordinate_mode", _STR), ("preload_offset", (repr, float)))

    def __init__(self, path, split, category_name="Car", coordinate_mode="velodyne", preload_offset=-1, device=None, chunk_frames=64):
        super().__init__()
        dev = self._device(device, chunk_frames)
        self.path, self.split, self.category_name = path, split, category_name
        self.coordinate_mode, self.preload_offset = coordinate_mode, preload_offset
        annos, calibs = kitti_annotations(path, split, category_name, coordinate_mode)
        self.scene_list = kitti_scene_list(split)
        items, missing = kitti_items(path, annos, calibs, coordinate_mode, preload_offset)
        self._preload(dev, annos, [(a["scene"], a["track_id"], a["frames"]) for a in annos], items, chunk_frames, missing)

    def get_num_scenes(self):
        return len(self.scene_list)

    def get_frames(self, seq_id, frame_ids):
        t = self[seq_id]
        return [{"pc": t.frames[f], "3d_bbox": t.boxes[f], "meta": (self.meta[seq_id][0], self.meta[seq_id][1], int(self.meta[seq_id][2][f]))}
                for f in frame_ids]

    def _pack_meta(self):
        return dict(frames=np.concatenate([m[2] for m in self.meta] + [np.zeros((0,), np.int64)]),
                    scenes=np.array([m[0] for m in self.meta], dtype="U4"), track_ids=np.array([m[1] for m in self.meta], np.int64),
                    scene_list=np.array(self.scene_list, dtype="U4"))

    def _unpack_meta(self, z, cut):
        self.scene_list = [str(s) for s in z["scene_list"]]
        return [(str(s), int(t), f) for s, t, f in zip(z["scenes"], z["track_ids"], cut(z["frames"]))]


# ---- Waymo --------------------------------------------------------------------------------------------------------------------
WAYMO_TYPES = ("UNKNOWN", "VEHICLE", "PEDESTRIAN", "SIGN", "CYCLIST")
_WAYMO_CATEGORIES = ("vehicle", "pedestrian", "cyclist")


def _unpickle(file):
    with open(file, "rb") as f:
        return pickle.load(f)


def generate_waymo_sot_infos(root, category, split):
    """The reference's generate_waymo_data(root, cla, split) (datasets/generate_waymo_sot.py): walks
    <root>/infos_<split>_01sweeps_filter_zero_gt.pkl, reads every frame's annotation pickle and writes
    <root>/sot_infos_<category lower-cased>_<split>.pkl: {object name: [{'PC': the frame's lidar path, 'Box': the object's box,
    'Class': category}]}, objects in order of first appearance, frames in the order of the infos list.  `category` is the
    UPPER-CASE class (VEHICLE, PEDESTRIAN, CYCLIST), as the reference's __main__ passes it; the reference's own call from
    WaymoDataset passes the lower-cased name, which matches no object and writes an empty dict.  -> the dict"""
    data = {}
    for frame in _unpickle(os.path.join(root, "infos_%s_01sweeps_filter_zero_gt.pkl" % split)):
        for obj in _unpickle(os.path.join(root, frame["anno_path"]))["objects"]:
            if WAYMO_TYPES[obj["label"]] == category:
                data.setdefault(obj["name"], []).append({"PC": frame["path"], "Box": obj["box"], "Class": category})
    with open(os.path.join(root, "sot_infos_%s_%s.pkl" % (category.lower(), split)), "wb") as f:
        pickle.dump(data, f)
    return data


def waymo_names(split, category_name):
    """WaymoDataset.__init__: -> (split, category) lower-cased, `test` reads `val`; anything else is an error"""
    split, category = split.lower(), category_name.lower()
    split = "val" if split == "test" else split
    if split not in ("train", "val"):
        raise ValueError("split must be train, val or test, not %r" % split)
    if category not in _WAYMO_CATEGORIES:
        raise ValueError("category_name must be one of VEHICLE, PEDESTRIAN, CYCLIST, not %r" % category_name)
    return split, category


def waymo_pose(veh_to_global):
    """veh_pos_to_transform's global_from_car: eye(4) whose rotation is the pose's rotation taken through a quaternion and
    back, and whose last column is the pose's translation -> (4,4) fp64"""
    ref_pose = np.reshape(np.asarray(veh_to_global, np.float64), [4, 4])
    tm = np.eye(4)
    tm[:3, :3] = _quat_matrix(_quat_from_matrix(ref_pose[:3, :3]))
    tm[:3, 3] = ref_pose[:3, 3]
    return tm


def waymo_box(box9, global_from_car):
    """The box of WaymoDataset._get_frame_from_anno in fp64 -> (15,) [centre | wlh | rotation row-major].  box9: the float32
    annotation x y z length width height vx vy heading in the vehicle frame.  Length and width change places; the orientation
    is the pose's quaternion times the rotation about z by -heading; the centre is rotated, then translated"""
    box9 = np.asarray(box9)
    q_pose = _quat_from_matrix(global_from_car)
    centre = np.dot(_quat_matrix(q_pose), box9[0:3]) + global_from_car[:3, -1]
    rot = _quat_matrix(_quat_mul(q_pose, _quat([0, 0, 1], float(-box9[-1]))))
    return np.concatenate([centre, box9[[4, 3, 5]], rot.reshape(-1)]).astype(np.float64)


def _waymo_open(name, root):
    return name if root is None or os.path.isabs(name) else os.path.join(root, name)


def waymo_annotations(path, split, category_name="VEHICLE", tiny=False, root=None):
    """The host half of the Waymo reader (no device): -> (tracklets, files, poses).  tracklets: a list of dicts with key (the
    object name), files (the 'PC' strings of its frames), frames (T,) int64 (indices into `files`) and boxes (T,15) float64,
    in the order of the sot_infos dict; files: the distinct 'PC' strings in order of first use; poses (len(files),3,4) float64:
    the upper rows of each file's global_from_car.  Every annotation pickle is read once.  root=None opens the 'PC' strings
    as they stand, as the reference does; otherwise relative ones are resolved against root."""
    split, category = waymo_names(split, category_name)
    infos_file = os.path.join(path, "sot_infos_%s_%s.pkl" % (category, split))
    if not os.path.exists(infos_file):
        raise FileNotFoundError("%s is missing: write it with generate_waymo_sot_infos(%r, %r, %r)"
                                % (infos_file, path, category.upper(), split))
    infos = _unpickle(infos_file)
    keys = list(infos)[:100] if tiny else list(infos)
    index, files, poses, tracklets = {}, [], [], []
    for key in keys:
        frames, boxes = [], []
        for anno in infos[key]:
            pc = anno["PC"]
            if pc not in index:
                index[pc] = len(files)
                files.append(pc)
                poses.append(waymo_pose(_unpickle(_waymo_open(pc.replace("lidar", "annos"), root))["veh_to_global"]))
            frames.append(index[pc])
            boxes.append(waymo_box(anno["Box"], poses[index[pc]]))
        tracklets.append({"key": key, "files": [a["PC"] for a in infos[key]], "frames": np.array(frames, np.int64),
                          "boxes": np.array(boxes, np.float64).reshape(-1, 15)})
    return tracklets, files, np.array([p[:3] for p in poses], np.float64).reshape(-1, 3, 4)


def waymo_points(file):
    """['lidars']['points_xyz'] of a lidar pickle -> (n,3) float32, C-contiguous.  Anything but float32 raises ValueError (the
    reference would keep a float64 array unrounded: a stated deviation)"""
    pts = _unpickle(file)["lidars"]["points_xyz"]
    if not isinstance(pts, np.ndarray) or pts.dtype != np.float32 or pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("%s: points_xyz must be an (n,3) float32 array, not %s %s"
                         % (file, getattr(pts, "dtype", type(pts)), getattr(pts, "shape", "")))
    return np.ascontiguousarray(pts)


def waymo_items(annos, files, poses, preload_offset, root=None):
    """-> an iterator over the PreloadItem of every distinct lidar file in order of first use.  The bounds are computed here;
    a file's rows are known only once it is unpickled, so that happens when the planner pulls its item: once per file, and
    the array goes when its chunk is done"""
    users = _frame_users(annos)
    boxes = [frame_boxes(annos, users[f], preload_offset) for f in range(len(files))]

    def item(f):
        pts = waymo_points(_waymo_open(files[f], root))
        return PreloadItem(pts, pts.shape[0], *boxes[f], extra=poses[f])
    return map(item, range(len(files)))


class WaymoTracklets(_PoolTracklets):
    """WaymoTracklets(path, split, ...): the tracklets of <path>/sot_infos_<category>_<split>.pkl, transformed to the global
    frame and cropped as the reference's WaymoDataset preloads them, resident in HBM.  A sampler.DeviceTracklets.  meta[k] =
    (tracklet key, the 'PC' strings of its frames); pool / rows as in KittiTracklets.  With preload_offset <= 0 nothing is
    cropped: the transformed cloud of a frame is written once and its tracklets share the slice."""

    INFO = (("split", _STR), ("category_name", _STR), ("preload_offset", _LITERAL), ("tiny", _LITERAL))
    CHUNK = dict(kind="poses", row_floats=3)

    def __init__(self, path, split, category_name="VEHICLE", preload_offset=10, tiny=False, root=None, device=None, chunk_frames=64):
        super().__init__()
        dev = self._device(device, chunk_frames)
        self.path, self.preload_offset, self.tiny = path, preload_offset, bool(tiny)
        self.split, self.category_name = waymo_names(split, category_name)
        annos, files, poses = waymo_annotations(path, split, category_name, tiny, root)
        self._preload(dev, annos, [(a["key"], a["files"]) for a in annos], waymo_items(annos, files, poses, preload_offset, root),
                      chunk_frames)


# ---- NuScenes -----------------------------------------------------------------------------------------------------------------
_NUSC_TABLES = ("category", "instance", "sample_annotation", "sample", "sample_data", "scene", "sensor", "calibrated_sensor", "ego_pose")
_NUSC_LIDAR = "LIDAR_TOP"
_NUSC_ROW_BYTES = 20                              # a .pcd.bin row: x y z intensity ring, float32 each


def _general(prefix, *leaves):
    return tuple(prefix + "." + leaf for leaf in leaves) if leaves else (prefix,)


# the nuScenes tracking class -> the general (annotation) classes it covers, from the taxonomy of the tracking task
NUSCENES_TRACKING_CLASSES = {
    "void / ignore": _general("animal") + _general("human.pedestrian", "personal_mobility", "stroller", "wheelchair") +
    _general("movable_object", "barrier", "debris", "pushable_pullable", "trafficcone") + _general("static_object.bicycle_rack") +
    _general("vehicle.emergency", "ambulance", "police") + _general("vehicle.construction"),
    "bicycle": _general("vehicle.bicycle"),
    "bus": _general("vehicle.bus", "bendy", "rigid"),
    "car": _general("vehicle.car"),
    "motorcycle": _general("vehicle.motorcycle"),
    "pedestrian": _general("human.pedestrian", "adult", "child", "construction_worker", "police_officer"),
    "trailer": _general("vehicle.trailer"),
    "truck": _general("vehicle.truck"),
}


def _read_json(file):
    with open(file) as f:
        return json.load(f)


def nuscenes_split_scenes(scenes, split):
    """the scene names of `split`.  scenes: a dict split -> names | the path of a JSON file holding such a dict | an iterable of
    names (taken as the split's) | None: the devkit's create_splits_scenes(), imported here"""
    if scenes is None:
        try:
            from nuscenes.utils.splits import create_splits_scenes
        except ImportError:
            raise ValueError("the nuScenes devkit (nuscenes.utils.splits) is not installed: pass scenes=, a dict split -> scene "
                             "names, the path of a JSON file holding one, or the scene names of the split") from None
        scenes = create_splits_scenes()
    if isinstance(scenes, (str, os.PathLike)):
        scenes = _read_json(scenes)
    if isinstance(scenes, dict):
        if split not in scenes:
            raise ValueError("split %r is not among %s" % (split, sorted(scenes)))
        scenes = scenes[split]
    return set(scenes)


def nuscenes_annotations(path, split, category_name="Car", version="v1.0-trainval", key_frame_only=False, min_points=False, scenes=None):
    """The host half of the NuScenes reader (no device, no devkit): -> (tracklets, files, steps).  tracklets: a list of dicts
    with key (the instance token), files (the sweep's `filename` of every frame, relative to path), frames (T,) int64 (indices
    into `files`) and boxes (T,15) float64, instances in table order; files: the distinct sweeps in order of first use; steps
    (len(files),2,12) float64: per sweep [R | t] of its calibrated sensor, then of its ego pose.  What
    NuScenesDataset.filter_instance and _build_tracklet_anno do over the devkit's tables; every JSON table is read once."""
    general = NUSCENES_TRACKING_CLASSES.get(category_name.lower())
    if general is None:
        raise ValueError("category_name %r is no nuScenes tracking class: %s" % (category_name, ", ".join(sorted(NUSCENES_TRACKING_CLASSES))))
    in_split = nuscenes_split_scenes(scenes, split)
    tables = {name: _read_json(os.path.join(path, version, name + ".json")) for name in _NUSC_TABLES}
    by_token = {name: {r["token"]: r for r in rows} for name, rows in tables.items()}
    # the devkit's reverse index, as far as the reference relies on it: sample['data'][channel] is the key-frame sample_data
    # record of the sample on that channel, the last one in table order
    lidar_of = {}
    for sd in tables["sample_data"]:
        if sd["is_key_frame"]:
            sensor = by_token["sensor"][by_token["calibrated_sensor"][sd["calibrated_sensor_token"]]["sensor_token"]]
            if sensor["channel"] == _NUSC_LIDAR:
                lidar_of[sd["sample_token"]] = sd
    index, files, steps, tracklets = {}, [], [], []
    for instance in tables["instance"]:
        first = by_token["sample_annotation"][instance["first_annotation_token"]]
        scene = by_token["scene"][by_token["sample"][first["sample_token"]]["scene_token"]]
        if not (scene["name"] in in_split and first["num_lidar_pts"] >= min_points and
                by_token["category"][instance["category_token"]]["name"] in general):
            continue
        names, frames, boxes, token = [], [], [], instance["first_annotation_token"]
        while token != "":
            anno = by_token["sample_annotation"][token]
            token = anno["next"]
            if anno["sample_token"] not in lidar_of:
                raise ValueError("sample %s has no key-frame %s record" % (anno["sample_token"], _NUSC_LIDAR))
            sd = lidar_of[anno["sample_token"]]
            if key_frame_only and not sd["is_key_frame"]:
                continue
            file = sd["filename"]
            if file not in index:
                index[file] = len(files)
                files.append(file)
                cs, ego = by_token["calibrated_sensor"][sd["calibrated_sensor_token"]], by_token["ego_pose"][sd["ego_pose_token"]]
                steps.append([np.hstack([_quat_matrix(np.array(r["rotation"], np.float64)),
                                         np.array(r["translation"], np.float64).reshape(3, 1)]).reshape(12) for r in (cs, ego)])
            names.append(file)
            frames.append(index[file])
            boxes.append(np.concatenate([np.array(anno["translation"], np.float64), np.array(anno["size"], np.float64),
                                         _quat_matrix(np.array(anno["rotation"], np.float64)).reshape(-1)]))
        tracklets.append({"key": instance["token"], "files": names, "frames": np.array(frames, np.int64),
                          "boxes": np.array(boxes, np.float64).reshape(-1, 15)})
    return tracklets, files, np.array(steps, np.float64).reshape(-1, 2, 12)


def nuscenes_rows(file):
    """the rows of a .pcd.bin sweep as the reference reads it (np.fromfile(float32).reshape(-1, 5)): a missing file raises
    FileNotFoundError, a length that is no multiple of 20 bytes ValueError"""
    size = os.path.getsize(file)
    if size % _NUSC_ROW_BYTES:
        raise ValueError("%s: %d bytes are no rows of five float32 (x y z intensity ring)" % (file, size))
    return size // _NUSC_ROW_BYTES


def nuscenes_items(path, annos, files, steps, preload_offset):
    """-> the PreloadItems of every distinct sweep in order of first use"""
    users = _frame_users(annos)
    return [PreloadItem(full, nuscenes_rows(full), *frame_boxes(annos, users[f], preload_offset), extra=steps[f])
            for f, full in enumerate(os.path.join(path, file) for file in files)]


class NuScenesTracklets(_PoolTracklets):
    """NuScenesTracklets(path, split, ...): the tracklets of the nuScenes set under `path` (<version>/*.json, the sweeps where
    sample_data names them), taken sensor -> ego -> global and cropped as the reference's NuScenesDataset preloads them,
    resident in HBM.  A sampler.DeviceTracklets.  meta[k] = (instance token, the sweep files of its frames); pool / rows as in
    KittiTracklets.  With preload_offset <= 0 nothing is cropped: the transformed sweep is written once and its tracklets
    share the slice.  translate = "float64" (numpy >= 2: the translation is added in fp64 and rounded) | "float32" (numpy < 2:
    an fp32 add).  scenes: see nuscenes_split_scenes."""

    INFO = (("split", _STR), ("category_name", _STR), ("version", _STR), ("translate", _STR), ("preload_offset", _LITERAL),
            ("key_frame_only", _LITERAL), ("min_points", _LITERAL))
    CHUNK = dict(kind="steps", row_floats=5)

    def __init__(self, path, split, category_name="Car", version="v1.0-trainval", key_frame_only=False, min_points=False,
                 preload_offset=-1, scenes=None, translate="float64", device=None, chunk_frames=64):
        super().__init__()
        dev = self._device(device, chunk_frames)
        if translate not in ("float64", "float32"):
            raise ValueError("translate must be 'float64' or 'float32'")
        self.path, self.split, self.category_name, self.version = path, split, category_name, version
        self.key_frame_only, self.min_points, self.preload_offset, self.translate = key_frame_only, min_points, preload_offset, translate
        annos, files, steps = nuscenes_annotations(path, split, category_name, version, key_frame_only, min_points, scenes)
        self._preload(dev, annos, [(a["key"], a["files"]) for a in annos], nuscenes_items(path, annos, files, steps, preload_offset),
                      chunk_frames, translate32=int(translate == "float32"))
