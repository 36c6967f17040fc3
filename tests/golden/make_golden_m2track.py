"""Generate tests/golden/ref_m2track.npz by running the REFERENCE'S OWN M2-Track code in this container.

Run from the repo root, only where /root/reference exists:  python tests/golden/make_golden_m2track.py
Reference code executed (read-only, from /root/reference): models/m2track.py (M2TRACK.__init__ / forward /
compute_loss), models/backbone/pointnet.py (MiniPointNet, SegPointNet), datasets/points_utils.py (the
tensor box helpers).  What is stubbed because the packages are absent from the sandbox: pytorch_lightning
(`models.base_model.MotionBaseModel` -> a bare nn.Module holding `config`), torchmetrics, nuscenes,
pyquaternion, shapely (imported at module level by files we load, never called on this path);
`Tensor.cuda()` is the identity (m2track.py:171 hard-codes it).  Inputs: open3dsot_amd/synth.py.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

import fixture_io

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, ROOT)
torch.Tensor.cuda = lambda self, *a, **k: self
from oracle import ext_shim  # noqa: E402  (pointnet.py imports the SA modules, which import pointnet2_ops._ext)

ext_shim.install()
sys.path.insert(0, REF)     # for `pointnet2.utils...`


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Dummy:
    def __init__(self, *a, **k):
        pass


stub("nuscenes"); stub("nuscenes.utils"); stub("nuscenes.utils.geometry_utils")
stub("pyquaternion", Quaternion=_Dummy)
stub("datasets"); stub("datasets.data_classes", PointCloud=_Dummy, Box=_Dummy)
stub("torchmetrics", Accuracy=_Dummy)
stub("utils"); stub("utils.metrics", estimateOverlap=None, estimateAccuracy=None)
stub("models"); stub("models.backbone")


class MotionBaseModel(torch.nn.Module):
    def __init__(self, config=None, **kwargs):
        super().__init__()
        self.config = config


stub("models.base_model", MotionBaseModel=MotionBaseModel)
points_utils = load("datasets.points_utils", "datasets/points_utils.py")
sys.modules["datasets"].points_utils = points_utils
ref_pointnet = load("models.backbone.pointnet", "models/backbone/pointnet.py")
ref_m2 = load("models.m2track", "models/m2track.py")

from open3dsot_amd import m2track as ours, synth  # noqa: E402


def rotz_like_input(t):
    """datasets/points_utils.py:377-387 with the matrix in the angle's dtype (the reference writes float32 there)"""
    out = torch.zeros(tuple(list(t.shape) + [3, 3]), dtype=t.dtype, device=t.device)
    c, s = torch.cos(t), torch.sin(t)
    out[..., 0, 0], out[..., 0, 1], out[..., 1, 0], out[..., 1, 1], out[..., 2, 2] = c, -s, s, c, 1
    return out


def main():
    from types import SimpleNamespace
    import copy
    g = torch.Generator().manual_seed(77)
    torch.manual_seed(77)
    cfg = SimpleNamespace(**ours.M2_KITTI)
    net = ref_m2.M2TRACK(cfg)
    for m in net.modules():      # non-trivial BatchNorm state
        if isinstance(m, torch.nn.BatchNorm1d):
            m.weight.data = torch.empty_like(m.weight).uniform_(0.5, 1.5, generator=g)
            m.bias.data = torch.empty_like(m.bias).normal_(0, 0.1, generator=g)
            m.running_mean.data = torch.empty_like(m.running_mean).normal_(0, 0.1, generator=g)
            m.running_var.data = torch.empty_like(m.running_var).uniform_(0.5, 1.5, generator=g)
    fix = {"sd." + k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    batch = synth.make_motion_batch(11, 8, point_sample_size=128)
    for k, v in batch.items():
        fix["in." + k] = v
    tb = synth.to_torch(batch)
    for mode in ("train", "eval"):
        n2 = copy.deepcopy(net).train(mode == "train")
        out = n2({k: v.clone() for k, v in tb.items()})
        for k, v in out.items():
            fix["%s.out.%s" % (mode, k)] = v.detach().numpy()
        ld = n2.compute_loss(tb, out)
        for k, v in ld.items():
            fix["%s.loss.%s" % (mode, k)] = np.float32(float(v))
        if mode == "train":
            for k, v in n2.state_dict().items():
                if "running" in k:
                    fix["train.sd_after." + k] = v.detach().numpy().copy()
    # the tensor box helpers on their own
    pts = torch.randn(2, 16, 3, generator=g)
    ref_box = torch.randn(2, 4, generator=g)
    off_box = torch.randn(2, 4, generator=g) * 0.3
    fix["box.in.pts"], fix["box.in.ref"], fix["box.in.off"] = pts.numpy(), ref_box.numpy(), off_box.numpy()
    fix["box.offset_points"] = points_utils.get_offset_points_tensor(pts.clone(), ref_box, off_box).numpy()
    fix["box.offset_box"] = points_utils.get_offset_box_tensor(ref_box, off_box).numpy()
    fix["box.remove_transform"] = points_utils.remove_transform_points_tensor(pts.clone(), ref_box).numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_m2track.npz")
    written = fixture_io.save(path, **fix)
    print("wrote", path, "%.1f MB" % (sum(os.path.getsize(p) for p in written) / 1e6), len(fix), "arrays")
    # ---- round 4: the same reference model (the state dict above) at the BENCHMARKED batch of 48 frame pairs.  The twelve
    # Linear -> BatchNorm1d -> ReLU rows of the heads normalise over the batch: over 8 samples a 1e-7 difference of a pooled
    # feature moves a normalised value by 1e-4 (the bounds of the batch-8 fixture reflect that, not the kernels); over 48 the
    # losses are a 1e-4 quantity.  No state dict in this file: tests load the one of ref_m2track.npz.
    fix2 = {}
    batch = synth.make_motion_batch(111, 48, point_sample_size=256)
    for k, v in batch.items():
        fix2["in." + k] = v
    tb = synth.to_torch(batch)
    for mode in ("train", "eval"):
        n2 = copy.deepcopy(net).train(mode == "train")
        out = n2({k: v.clone() for k, v in tb.items()})
        for k, v in out.items():
            if mode == "train" or k in ("estimation_boxes", "motion_cls", "estimation_boxes_prev"):
                fix2["%s.out.%s" % (mode, k)] = v.detach().numpy()
        ld = n2.compute_loss(tb, out)
        for k, v in ld.items():
            fix2["%s.loss.%s" % (mode, k)] = np.float32(float(v))
        if mode == "train":
            for k, v in n2.state_dict().items():
                if "running" in k:
                    fix2["train.sd_after." + k] = v.detach().numpy().copy()
    path2 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_m2track_b48.npz")
    written = fixture_io.save(path2, **fix2)
    print("wrote", path2, "%.1f MB" % (sum(os.path.getsize(p) for p in written) / 1e6), len(fix2), "arrays")
    # ---- round 5: the fp64 YARDSTICK of both fixtures (third file; the two above stay byte-identical).  The same reference
    # model evaluated in double precision on the same inputs, with its two hard-mask decisions (`torch.argmax` of the
    # segmentation logits per point and of the motion-state logits per cloud, models/m2track.py:95,113) REPLAYED from the
    # fp32 run, so that the fp64 values are the exact evaluation of the graph the fp32 run executed (a near-tie that fp64
    # would decide differently gates everything downstream and is not a rounding question).  Tests then hold the GPU run to
    # max(1e-4, 3 x the reference's own fp32 distance to this) per output instead of a bare tolerance.
    fix3 = {}
    for tag, bt in (("b8", synth.make_motion_batch(11, 8, point_sample_size=128)),
                    ("b48", synth.make_motion_batch(111, 48, point_sample_size=256))):
        tb = synth.to_torch(bt)
        tb64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in tb.items()}
        for mode in ("train", "eval"):
            tape = []
            real_argmax = torch.argmax
            n32 = copy.deepcopy(net).train(mode == "train")
            torch.argmax = lambda *a, **k: (tape.append(real_argmax(*a, **k)), tape[-1])[1]
            try:
                out32 = n32({k: v.clone() for k, v in tb.items()})
            finally:
                torch.argmax = real_argmax
            n_dec = len(tape)
            n64 = copy.deepcopy(net).double().train(mode == "train")
            flips = []

            def replay(*a, **k):
                mine, theirs = real_argmax(*a, **k), tape.pop(0)
                flips.append(int((mine != theirs).sum()))
                return theirs
            torch.argmax = replay
            torch.set_default_dtype(torch.float64)        # m2track.py:171 builds the class weights with torch.tensor([...])
            real_rotz = points_utils.rotz_batch_tensor    # datasets/points_utils.py:379 hard-codes float32: same entries,
            points_utils.rotz_batch_tensor = rotz_like_input   # the angle's dtype
            try:
                out64 = n64({k: v.clone() for k, v in tb64.items()})
                ld64 = n64.compute_loss(tb64, out64)
            finally:
                torch.argmax = real_argmax
                torch.set_default_dtype(torch.float32)
                points_utils.rotz_batch_tensor = real_rotz
            assert not tape and len(flips) == n_dec
            for k, v in out64.items():
                assert v.dtype == torch.float64, k
                fix3["%s.%s.out.%s" % (tag, mode, k)] = v.detach().numpy()
                print("  %s %s %-22s reference fp32 vs fp64: %.2e of the scale" % (
                    tag, mode, k, float((out32[k].double() - v).abs().max() / (v.abs().max() + 1e-12))))
            for k, v in ld64.items():
                fix3["%s.%s.loss.%s" % (tag, mode, k)] = np.float64(float(v))
            fix3["%s.%s.fp64_would_flip" % (tag, mode)] = np.array(flips, np.int64)
            if mode == "train":
                for k, v in n64.state_dict().items():
                    if "running" in k:
                        fix3["%s.train.sd_after.%s" % (tag, k)] = v.detach().numpy().copy()
    path3 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_m2track_f64.npz")
    written = fixture_io.save(path3, **fix3)
    print("wrote", path3, "%.1f MB" % (sum(os.path.getsize(p) for p in written) / 1e6), len(fix3), "arrays")


if __name__ == "__main__":
    main()
