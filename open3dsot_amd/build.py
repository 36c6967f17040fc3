"""Compile the gfx950 HIP sources of this package into open3dsot_amd/_lib/libo3dsot_hip.so.

hipcc cross-compiles for gfx950 without a GPU, so this runs in the build container; the
resulting .so is git-ignored but travels with the repo snapshot to the GPU box.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "_lib")
SO = os.path.join(LIBDIR, "libo3dsot_hip.so")

# (source, extra flags).  Index ops are compiled with FP contraction OFF: their squared
# distances are explicit fmaf chains that must match the oracle bit for bit.
SOURCES = [
    ("fps.hip", ["-ffp-contract=off"]),
    ("index_ops.hip", ["-ffp-contract=off"]),
    ("mlp.hip", []),
    ("mlp_direct.hip", []),
    ("mlp_wgrad.hip", []),
    ("compact.hip", []),
    ("pointwise.hip", []),
    ("heads.hip", []),
    ("rowmlp.hip", []),
    ("xcorr.hip", []),
    ("sa_eval.hip", []),
    ("loss.hip", []),
    ("boxcloud.hip", []),
    ("track.hip", ["-ffp-contract=off"]),      # the crop's operation order is part of its contract (tests/tracking_oracle.py)
    ("train_batch.hip", ["-ffp-contract=off"]),      # calls track.hip's crop_test / gather_row (csrc/track_common.hpp): same contract
    ("metrics.hip", ["-ffp-contract=off"]),      # the scoring arithmetic's operation order is stated (tests/metrics_oracle.py)
    ("scene.hip", ["-ffp-contract=off"]),      # the lifecycle's order of decisions is stated (tests/scene_manage_oracle.py)
    ("preload.hip", ["-ffp-contract=off"]),      # the camera transform's fp64 operation order is stated (tests/kitti_oracle.py)
    ("optim.hip", ["-ffp-contract=off"]),      # the update rules' operation order is stated (tests/optim_oracle.py)
    ("capi_misc.hip", []),
]
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
          "-Wall", "-Wno-unused-function"]


def source_hash():
    """sha256 over the kernel sources (csrc/*.hip, *.hpp, include/o3dsot.h): stamps measurement artefacts
    (profiles/hbm_traffic.json) so that bench.py can refuse counters taken on other kernels"""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".h")))
    files.append(os.path.join(HERE, "..", "include", "o3dsot.h"))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "hipcc")
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h"))]
    headers.append(os.path.join(HERE, "..", "include", "o3dsot.h"))
    objs = []
    procs = []
    for src, extra in SOURCES:
        s = os.path.join(CSRC, src)
        if not os.path.exists(s):
            continue
        o = os.path.join(LIBDIR, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + headers):
            cmd = [hipcc] + COMMON + extra + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    if force or procs or _stale(SO, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + objs
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
