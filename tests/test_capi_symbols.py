"""The C-ABI library builds for gfx950, loads without a GPU and exports exactly the symbols that
include/o3dsot.h declares; the Python binding refuses CPU tensors (no CPU fallback)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "o3dsot.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(o3d_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_header():
    from open3dsot_amd import build, capi
    so = build.build()
    lib = ctypes.CDLL(so)
    names = declared_symbols()
    assert len(names) >= 11
    for n in names:
        assert hasattr(lib, n), "libo3dsot_hip.so does not export %s" % n
    assert capi.version().startswith("o3dsot-hip")
    for n in capi.SIGNATURES:  # everything the binding calls is exported as well
        assert hasattr(lib, n), n
    # and the other way round: every C entry point the library defines is declared (an export that lost its declaration
    # and its caller would otherwise stay in the library unnoticed)
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
        defined = {f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] in "Tt"}
        exported = sorted(n for n in defined if n.startswith("o3d_"))
        assert not set(exported) - set(names), "exported but not declared in include/o3dsot.h: %s" % (set(exported) - set(names))


def test_code_object_is_gfx950():
    so = os.path.join(ROOT, "open3dsot_amd", "_lib", "libo3dsot_hip.so")
    blob = open(so, "rb").read()
    assert b"gfx950" in blob
    assert b"gfx942" not in blob and b"gfx90a" not in blob   # single-target build, no fat multi-arch


def test_pointnet2_ops_ext_is_a_dropin():
    import pointnet2_ops._ext as ext
    for n in ("furthest_point_sampling", "gather_points", "gather_points_grad", "three_nn", "three_interpolate",
              "three_interpolate_grad", "ball_query", "group_points", "group_points_grad"):
        assert callable(getattr(ext, n))


def test_cpu_tensors_are_refused():
    import pointnet2_ops._ext as ext
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ext.furthest_point_sampling(torch.zeros(1, 8, 3), 4)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ext.group_points(torch.zeros(1, 2, 8), torch.zeros(1, 2, 2, dtype=torch.int32))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from open3dsot_amd import capi
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "SO_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(capi.O3DError, match="no CPU fallback"):
        capi.load()


def header_prototypes():
    """name -> list of parameter kinds ('p' pointer, 'i' int, 'l' long, 'f' float, 'd' double) from include/o3dsot.h"""
    src = open(os.path.join(ROOT, "include", "o3dsot.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(?:int|long|const char\s*\*)\s+(o3d_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        params = [p.strip() for p in m.group(2).split(",") if p.strip() and p.strip() != "void"]
        kinds = []
        for p in params:
            if "*" in p:
                kinds.append("p")
            else:
                t = p.split()
                kinds.append({"int": "i", "long": "l", "float": "f", "double": "d"}[t[-2] if len(t) > 1 else t[0]])
        protos[m.group(1)] = kinds
    return protos


KIND = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_float: "f", ctypes.c_double: "d"}


def test_ctypes_signatures_match_the_header():
    """every prototype of include/o3dsot.h is bound, and every argtypes list the binding derives has the arity and the
    argument kinds this file's own parser reads from the prototype (a silent ctypes mismatch corrupts arguments instead of
    failing)"""
    from open3dsot_amd import capi
    protos = header_prototypes()
    assert len(protos) >= 40
    assert set(capi.SIGNATURES) == set(protos) == set(declared_symbols())
    for name, argtypes in capi.SIGNATURES.items():
        got = [KIND[a] for a in argtypes]
        assert got == protos[name], (name, got, protos[name])


def test_signatures_and_return_types_hand_pinned():
    """one entry of each flavour written out by hand -- two parsers cannot be wrong the same way here -- and the return type
    of every entry: long for the *_scratch sizes and o3d_xcorr_reduce_groups, a string for o3d_version, int elsewhere"""
    from open3dsot_amd import capi
    pins = {"o3d_ball_query": "ppiiifipp",                                     # a float
            "o3d_mlp_conv_fwd_c": "ppppiilpplipppp",                           # longs between ints
            "o3d_adam_step": "pipppdddddddp",                                  # doubles
            "o3d_bn_finalize": "pip",                                          # a struct pointer and a count
            "o3d_thin_bwd_scratch": "",                                        # (void)
            "o3d_track_crop_groups_aug": "pppiplp",                            # const T* const*
            "o3d_mlp_conv_class": "iiiiii",                                    # a pure query: ints only
            "o3d_version": ""}
    for name, kinds in pins.items():
        assert "".join(KIND[a] for a in capi.SIGNATURES[name]) == kinds, name
    lib = capi.load()
    assert len(capi.RESTYPES) == len(capi.SIGNATURES)
    for name in capi.SIGNATURES:
        want = ctypes.c_char_p if name == "o3d_version" else \
            ctypes.c_long if name.endswith("_scratch") or name == "o3d_xcorr_reduce_groups" else ctypes.c_int
        assert capi.RESTYPES[name] is want, name
        fn = getattr(lib, name)
        assert fn.restype is want and list(fn.argtypes) == capi.SIGNATURES[name], name
    assert sum(n.endswith("_scratch") for n in capi.SIGNATURES) >= 7
    assert not hasattr(capi, "register")


def test_entry_points_reject_bad_arguments_before_touching_the_device():
    """argument validation comes first in every entry point: NULL pointers / impossible sizes return O3D_EINVAL (-1)
    without a launch -- checkable without a GPU (no compute call is made)"""
    from open3dsot_amd import capi, fused, fused_loss, points_utils  # noqa: F401  (they register argtypes)
    lib = capi.load()
    EINVAL = lib.o3d_boxcloud(None, None, None, None, 1.0, 1, 8, None, None)
    assert EINVAL != 0
    assert lib.o3d_boxcloud(None, None, None, None, 1.0, 0, 8, None, None) == 0            # empty batch: nothing to do
    assert lib.o3d_track_loss(*([None] * 8), 2, 8, 4, 9, 1.0, 1.0, 1.0, 1.0, 1.0, *([None] * 7)) == EINVAL
    assert lib.o3d_pack_points(None, None, 8, 8, None, None, 0, 0, 1, 3, 0, 1.0, 3, None, None) == EINVAL
    assert lib.o3d_furthest_point_sampling_pair(None, 8, 4, None, None, 8, 4, None, 1, None) == EINVAL
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.o3d_furthest_point_sampling_pair(p, 4096, 4, p, p, 8, 4, p, 1, None) == EINVAL     # > 2048 points: two calls
    assert lib.o3d_compact_build(None, 1, 8, 4, 8, 0, 0, 0, 8, *([None] * 7)) == EINVAL
    assert lib.o3d_compact_build(p, 1, 8, 3, 8, 0, 0, 0, 8, p, p, p, p, p, p, None) == EINVAL       # nsample not a power of two
    assert lib.o3d_pool_fwd_c(None, 256, None, None, None, None, 1, 8, 8, 0, None, None, None, None) == EINVAL
    assert lib.o3d_center_term(None, None, 8, 8, 3, None, None) == EINVAL
    # the compact data gradient rebuilds dY from dN AND Y: every operand valid but Y
    assert lib.o3d_mlp_conv_dgrad_c(p, None, p, p, p, p, 64, 128, 2048, p, p, 1024, 64, p, p, p, p, p, p, None) == EINVAL
    # the batched GEMM entries: exactly one of in_scale / in_shift NULL is refused (the transform would read the other)
    for sc, sh in ((p, None), (None, p)):
        assert lib.o3d_mlp_conv_fwd(p, p, sc, sh, 1, 3, 37, 128, p, None, None, None) == EINVAL
        assert lib.o3d_mlp_conv_fwd(p, p, sc, sh, 1, 16, 64, 128, p, None, None, None) == EINVAL        # the aligned shape too
        assert lib.o3d_mlp_conv_wgrad(p, None, None, None, 4, p, p, p, p, p, sc, sh, 1, 3, 37, 128, 1, p, p, None) == EINVAL
    # o3d_mlp_conv_class: which kernel those entries launch, without a launch
    c = lib.o3d_mlp_conv_class
    assert [c(0, 2, 37, 3, 128, 1), c(0, 2, 100, 3, 128, 1), c(0, 2, 300, 3, 128, 1)] == [64, 128, 256]
    assert [c(0, 2, 64, 16, 128, 1), c(0, 2, 64, 16, 128, 0), c(0, 2, 128, 64, 128, 0), c(1, 2, 64, 16, 128, 1)] == [3128, 2064, 4064, 3128]
    assert c(2, 2, 64, 16, 128, 1) == 64 and c(0, 2, 64, 16, 100, 1) == -1 and c(5, 2, 64, 16, 128, 1) == -1
    for entry, mirror in ((lib.o3d_bn_finalize, fused._BnFinArgs), (lib.o3d_bn_bwd_finalize, fused._BnBwdFinArgs)):
        jobs = (mirror * 2)()                               # zeroed jobs: `part` is NULL
        assert entry(None, 1, None) == EINVAL
        assert entry(ctypes.addressof(jobs), 0, None) == EINVAL and entry(ctypes.addressof(jobs), 3, None) == EINVAL
        assert entry(ctypes.addressof(jobs), 1, None) == EINVAL


def _valid_fin_jobs():
    """a forward and a backward finalize job that pass validation (host buffers for pointers: never dereferenced, because the
    tests below break one field each and the entry returns before any launch)"""
    from open3dsot_amd import fused
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    fwd = fused._BnFinArgs(p, 1, 8, 1.0, p, p, p, p, p, 0.1, 1e-5, p, p, p, p, p, 128, 0, 0.0)
    bwd = fused._BnBwdFinArgs(p, 1, 8, 1.0, p, p, p, p, p, p, p, p, p, 128, 0, 0.0)
    return buf, fwd, bwd


def test_finalize_job_structs_have_the_library_layout():
    """the ctypes mirrors of o3d_bn_fin_args / o3d_bn_bwd_fin_args have the sizes that csrc/mlp.hip static_asserts (a mismatched
    mirror would hand the kernels wild pointers)"""
    from open3dsot_amd import fused
    assert ctypes.sizeof(fused._BnFinArgs) == 128 and ctypes.sizeof(fused._BnBwdFinArgs) == 112
    src = open(os.path.join(ROOT, "open3dsot_amd", "csrc", "mlp.hip")).read()
    assert "static_assert(sizeof(o3d_bn_fin_args) == 128 && sizeof(o3d_bn_bwd_fin_args) == 112" in src


def test_finalize_entries_read_the_last_fields_where_python_puts_them():
    """a job that is valid except for tile = 0 beside a non-NULL meta, or except for nparts1 = -1, is refused with O3D_EINVAL
    before any launch: the fields behind the pointers sit where the mirror writes them"""
    from open3dsot_amd import capi, fused  # noqa: F401  (registers argtypes)
    lib = capi.load()
    for k, entry in ((1, lib.o3d_bn_finalize), (2, lib.o3d_bn_bwd_finalize)):
        for field, bad in (("tile", 0), ("nparts1", -1), ("nparts", 0), ("C", 0)):
            job = _valid_fin_jobs()[k]
            setattr(job, field, bad)
            assert entry(ctypes.addressof(job), 1, None) == -1, (k, field)
        job = _valid_fin_jobs()[k]
        setattr(job, "shift" if k == 1 else "A3", None)                # the last output pointer
        assert entry(ctypes.addressof(job), 1, None) == -1


def test_fused_backward_entry_validates_shapes_without_a_device():
    """o3d_mlp_conv_bwd_fused_*: the supported shapes (Cin 64, Cout 64 / 128, columns a multiple of 64) are decided on the
    host -- rows / scratch report -1 elsewhere and the launch entry refuses NULL operands and odd shapes before any HIP call;
    the gather / optimizer entries added in round 2 likewise"""
    from open3dsot_amd import capi, fused, fused_heads, optim, trackers  # noqa: F401  (they register argtypes)
    lib = capi.load()
    assert lib.o3d_mlp_conv_bwd_fused_rows(64, 64, 1179648) == 512            # 256 workgroups x two 32-position tiles
    assert lib.o3d_mlp_conv_bwd_fused_rows(64, 128, 1179648) == 256
    assert lib.o3d_mlp_conv_bwd_fused_rows(64, 64, 2048) == 16                # 32 chunks: 8 workgroups of 4 chunks
    assert lib.o3d_mlp_conv_bwd_fused_scratch(64, 64, 1179648) == 256 * 4 * 64 * 64
    assert lib.o3d_mlp_conv_bwd_fused_scratch(64, 128, 1179648) == 256 * 2 * 128 * 64
    for cin, cout, p_ in ((128, 128, 4096), (64, 256, 4096), (32, 64, 4096), (64, 64, 100), (64, 64, 0)):
        assert lib.o3d_mlp_conv_bwd_fused_rows(cin, cout, p_) == -1
        assert lib.o3d_mlp_conv_bwd_fused_scratch(cin, cout, p_) == -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL = lib.o3d_mlp_conv_bwd_fused_c(*([None] * 10), 64, 64, 4096, None, None, 0, None, None, None, None, None)
    assert EINVAL != 0
    assert lib.o3d_mlp_conv_bwd_fused_c(*([p] * 10), 128, 128, 4096, p, p, 0, p, p, p, p, None) == EINVAL      # Cin 128
    assert lib.o3d_mlp_conv_bwd_fused_c(*([p] * 10), 64, 64, 4096, p, None, 0, p, p, p, p, None) == EINVAL      # w without meta
    assert lib.o3d_mlp_conv_bwd_fused_c(*([p] * 10), 64, 64, 4096, p, p, 100, p, p, p, p, None) == EINVAL       # start1 % 256
    assert lib.o3d_gather_rows(None, None, 2, 8, 3, 4, None, None) == EINVAL
    assert lib.o3d_gather_rows(None, None, 2, 8, 3, 0, None, None) == 0                                         # nothing to gather
    assert lib.o3d_adam_step(None, 0, None, None, None, 1e-3, 0.5, 0.999, 1e-6, 0.0, 0.5, 1e-3, None) == EINVAL
    assert lib.o3d_mlp_conv_wgrad2_group(None, 1, None) == EINVAL and lib.o3d_mlp_conv_wgrad2_group(p, 9, None) == EINVAL
    assert lib.o3d_compact_build2(None, 8, 8, None, 8, 8, 1, 4, 0, 8, 16, *([None] * 7)) == EINVAL
    assert lib.o3d_best_proposal(None, 1, 64, p, None, None) == EINVAL and lib.o3d_best_proposal(p, 0, 64, p, None, None) == EINVAL
    assert lib.o3d_adam_step(p, 1, p, p, p, 1e-3, 0.5, 0.999, 1e-6, 0.0, 0.0, 1e-3, None) == EINVAL             # bc1 = 0: step 0


def test_round4_entry_points_validate_before_any_launch():
    """the entry points added in round 4 (M2-Track loss, the transforms between its stages, row-stack groups, the thin
    first-layer backward, the pooled global-max backward, P2B's similarity map) refuse NULL operands / unsupported shapes with
    O3D_EINVAL before touching the device"""
    from open3dsot_amd import box_utils, capi, fused_loss, fused_pointwise, fused_rows, fused_xcorr  # noqa: F401  (they register)
    lib = capi.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL = -1
    assert lib.o3d_m2track_loss(*([None] * 14), 2, 8, 9, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 2.0, *([None] * 10)) == EINVAL
    # BoxCloud term switched on needs both label halves and an even number of points
    assert lib.o3d_m2track_loss(p, p, p, None, None, None, None, p, p, p, None, None, p, None, 2, 8, 9, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5,
                                2.0, p, p, *([None] * 8)) == EINVAL
    assert lib.o3d_m2track_loss(p, p, p, p, p, None, None, p, p, p, None, None, p, None, 2, 7, 9, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5,
                                2.0, p, p, *([None] * 8)) == EINVAL
    assert lib.o3d_motion_merge_fwd(None, 8, 8, None, None, 1, 8, None, None, None) == EINVAL
    assert lib.o3d_motion_merge_fwd(p, 32, 8, None, p, 1, 7, p, p, None) == EINVAL               # odd N: no two halves
    assert lib.o3d_motion_merge_bwd(p, 32, 8, None, p, 1, 8, None, None, None, None, None) == EINVAL
    assert lib.o3d_offset_box(None, None, 1, None, None, None, None, None) == EINVAL
    assert lib.o3d_offset_box(p, p, 1, None, None, None, None, None) == EINVAL                    # forward without an output
    assert lib.o3d_thin_bwd_scratch() == 256 * 64 * 16
    assert lib.o3d_thin_bwd(p, p, p, p, p, p, p, 17, 64, 64, p, p, None, None) == EINVAL          # Cin > 16
    assert lib.o3d_thin_bwd(p, p, p, p, p, p, p, 12, 128, 64, p, p, None, None) == EINVAL         # Cout != 64
    assert lib.o3d_thin_bwd(p, p, p, p, p, p, p, 12, 64, 100, p, p, None, None) == EINVAL         # P % 64
    assert lib.o3d_gmax_bwd_pk(None, None, None, None, None, 1, 8, 8, None, None, None) == EINVAL
    assert lib.o3d_row_mlp_fwd_group(None, 1, None) == EINVAL and lib.o3d_row_mlp_fwd_group(p, 5, None) == EINVAL
    assert lib.o3d_row_mlp_bwd_group(None, 1, None) == EINVAL and lib.o3d_row_mlp_input_grad(p, 0, None) == EINVAL
    jobs = (fused_rows._RowFwdArgs * 1)()                   # a zeroed job: NULL operands
    assert lib.o3d_row_mlp_fwd_group(ctypes.addressof(jobs), 1, None) == EINVAL
    bjobs = (fused_rows._RowBwdArgs * 1)()
    assert lib.o3d_row_mlp_bwd_group(ctypes.addressof(bjobs), 1, None) == EINVAL
    assert lib.o3d_cosine_sim_fwd(None, 1, 1, 1, None, 1, 1, 1, 1, 32, 4, 8, None, None, None, None) == EINVAL
    assert lib.o3d_cosine_sim_fwd(p, 1, 1, 1, p, 1, 1, 1, 1, 33, 4, 8, p, p, p, None) == EINVAL      # channels % 32


def test_row_group_structs_match_the_header_layout():
    """ctypes mirrors of o3d_row_fwd_args / o3d_row_bwd_args: same field names, in the header's order"""
    from open3dsot_amd import fused_rows
    src = open(os.path.join(ROOT, "include", "o3dsot.h")).read()
    for name, cls in (("o3d_row_fwd_args", fused_rows._RowFwdArgs), ("o3d_row_bwd_args", fused_rows._RowBwdArgs)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, src).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            base, names = re.match(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl).groups()
            fields += [n.strip().lstrip("*").strip() for n in names.split(",")]
        assert fields == [f[0] for f in cls._fields_], (name, fields, [f[0] for f in cls._fields_])


def header_structs():
    """name -> field names, in order, of every `typedef struct {...} name;` of include/o3dsot.h (the field parser of
    test_row_group_structs_match_the_header_layout for all of them: comments stripped, `box[15]` is the field `box`)"""
    src = open(os.path.join(ROOT, "include", "o3dsot.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    structs = {}
    for body, name in re.findall(r"typedef struct \{([^}]*)\}\s*(\w+);", src):
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            base, names = re.match(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl).groups()
            fields += [re.sub(r"\[\d+\]", "", n).strip().lstrip("*").strip() for n in names.split(",")]
        structs[name] = fields
    return structs


# sizeof of the 17 job / argument structs on the LP64 hosts this library is built for, written out by hand
STRUCT_SIZES = {"o3d_bn_fin_args": 128, "o3d_bn_bwd_fin_args": 112, "o3d_rows_src": 40, "o3d_pw_fwd_args": 88,
                "o3d_pw_dgrad_args": 120, "o3d_wgrad_job": 104, "o3d_row_fwd_args": 128, "o3d_row_bwd_args": 168,
                "o3d_crop_job": 64, "o3d_resample_job": 40, "o3d_crop_target": 48, "o3d_crop_group": 32, "o3d_motion_job": 48,
                "o3d_crop_plan": 48, "o3d_train_sample_args": 192, "o3d_crop_aug": 112, "o3d_train_motion_sample_args": 248}


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """every struct the binding derives from the header has the size and the field offsets the host C compiler gives the same
    header, and so have the numpy records of the device tables: all 17, where the kernels' static_asserts cover 8"""
    from open3dsot_amd import capi, points_utils as PU
    structs = header_structs()
    assert set(structs) == set(STRUCT_SIZES)
    for name, fields in structs.items():
        cls = capi.struct(name)
        assert cls is capi.struct(name) and issubclass(cls, ctypes.Structure)                   # cached
        assert [f[0] for f in cls._fields_] == fields, name
        assert ctypes.sizeof(cls) == STRUCT_SIZES[name], name
    records = {"o3d_crop_target": PU.CROP_TARGET, "o3d_motion_job": PU.MOTION_JOB, "o3d_crop_plan": PU.CROP_PLAN,
               "o3d_crop_aug": PU.CROP_AUG, "o3d_resample_job": PU.RESAMPLE_JOB}
    for name, rec in records.items():
        assert rec == capi.dtype(name) and list(rec.names) == structs[name] and rec.itemsize == STRUCT_SIZES[name], name
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "o3dsot.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append('    printf("%s  %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fields]
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    compiled = {(ln.split(" ")[0], ln.split(" ")[1]): int(ln.split(" ")[2]) for ln in out.splitlines()}
    assert len(compiled) == sum(len(f) + 1 for f in structs.values())
    for name, fields in structs.items():
        cls, rec = capi.struct(name), capi.dtype(name)
        assert ctypes.sizeof(cls) == rec.itemsize == compiled[(name, "")], name
        for f in fields:
            assert getattr(cls, f).offset == rec.fields[f][1] == compiled[(name, f)], (name, f)


GOOD_HEADER = """
#ifndef X_H_
#define X_H_
#include <stdint.h>
#define O3D_LIMIT 7
#define O3D_ENEG (-3)
typedef struct { const float* p; long sb, sc; int C; float box[3]; unsigned seed; } o3d_a;  /* a comment; with ( */
const char* o3d_name(void);
long o3d_size(const o3d_a* jobs, int n);
int o3d_run(const o3d_a* const* tab, int32_t* out, float r, double lr,
            long ld, void* stream);
#endif
"""


def test_the_header_parser_refuses_what_it_does_not_understand():
    """the parser behind the binding never guesses: text outside its grammar raises at import instead of yielding a wrong
    argtypes list or layout"""
    from open3dsot_amd import capi
    sig, res, structs, consts = capi._parse_header(GOOD_HEADER)
    assert {n: "".join(KIND[a] for a in v) for n, v in sig.items()} == {"o3d_name": "", "o3d_size": "pi", "o3d_run": "ppfdlp"}
    assert res == {"o3d_name": ctypes.c_char_p, "o3d_size": ctypes.c_long, "o3d_run": ctypes.c_int}
    assert consts == {"O3D_LIMIT": 7, "O3D_ENEG": -3}
    assert structs == {"o3d_a": [("p", ctypes.c_void_p), ("sb", ctypes.c_long), ("sc", ctypes.c_long), ("C", ctypes.c_int),
                                 ("box", ctypes.c_float * 3), ("seed", ctypes.c_uint)]}
    bad = {"an unknown type": "int o3d_f(size_t n);",
           "a pointer to an unknown type": "int o3d_f(const o3d_b* jobs);",
           "a by-value struct field": "typedef struct { o3d_a inner; int n; } o3d_b;",
           "a by-value struct parameter": "int o3d_f(o3d_a job);",
           "a function-pointer parameter": "int o3d_f(int (*cb)(int), void* stream);",
           "a function-pointer field": "typedef struct { int (*cb)(int); } o3d_b;",
           "a bit-field": "typedef struct { int a : 3; } o3d_b;",
           "a two-dimensional array": "typedef struct { float rot[3][3]; } o3d_b;",
           "a nested struct": "typedef struct { struct { int a; } in; } o3d_b;",
           "a two-word type": "typedef struct { unsigned int a; } o3d_b;",
           "an array parameter": "int o3d_f(float box[15]);",
           "an unknown return type": "float o3d_f(int n);",
           "a prototype that lost its semicolon": "int o3d_f(int n)\nint o3d_g(int n);",
           "a prototype split by a stray semicolon": "int o3d_f(int n;\n void* stream);",
           "a second declaration of a name": "int o3d_run(int n);",
           "a macro with arguments": "#define O3D_MAX(a, b) ((a) > (b) ? (a) : (b))",
           "a constant that is no integer": "#define O3D_EPS 1e-5f",
           "a conditional": "#if defined(O3D_LIMIT)\nint o3d_f(int n);\n#endif"}
    for what, text in bad.items():
        with pytest.raises(capi.O3DError):
            capi._parse_header(GOOD_HEADER.replace("#endif", text + "\n#endif"))
            pytest.fail("the parser accepted %s" % what)


def test_a_missing_header_fails_loudly(monkeypatch, tmp_path):
    from open3dsot_amd import capi
    monkeypatch.setattr(capi, "HEADER", str(tmp_path / "o3dsot.h"))
    with pytest.raises(capi.O3DError, match=re.escape(str(tmp_path / "o3dsot.h"))):
        capi._read_header()


def header_constants():
    src = open(os.path.join(ROOT, "include", "o3dsot.h")).read()
    return {n: int(v) for n, v in re.findall(r"^#define\s+(O3D_\w+)\s+\(?(-?\d+)\)?", src, flags=re.M)}


def test_limits_come_from_the_header():
    """capi.CONSTANTS holds the header's integer #defines, and the Python names that used to repeat them as literals"""
    from open3dsot_amd import capi, fused, points_utils as PU
    assert capi.CONSTANTS == header_constants() and len(capi.CONSTANTS) >= 11
    assert (capi.CONSTANTS["O3D_OK"], capi.CONSTANTS["O3D_EINVAL"], capi.CONSTANTS["O3D_ELAUNCH"]) == (0, -1, -2)
    assert fused.POOL_BWD_SPLIT == capi.CONSTANTS["O3D_POOL_BWD_SPLIT"] == 8
    assert PU.CROP_MAX_JOBS == capi.CONSTANTS["O3D_CROP_MAX_JOBS"] == 4
    assert PU.CROP_SUBWINDOW == capi.CONSTANTS["O3D_CROP_SUBWINDOW"] == 0
    assert PU.CROP_MODEL == capi.CONSTANTS["O3D_CROP_MODEL"] == 1
    assert PU.CROP_MULTI_MAX_TARGETS == capi.CONSTANTS["O3D_CROP_MULTI_MAX_TARGETS"] == 1024
    assert PU.CROP_MULTI_CHUNK == capi.CONSTANTS["O3D_CROP_MULTI_CHUNK"] == 32
    assert PU.CROP_MAX_GROUPS == capi.CONSTANTS["O3D_CROP_MAX_GROUPS"] == 4096
    assert PU.TRAIN_MAX_CANDIDATES == capi.CONSTANTS["O3D_TRAIN_MAX_CANDIDATES"] == 1024


def test_no_tuning_switches_in_the_product():
    """one product path: the kernels read no environment variable, and the Python package knows exactly two `O3D_*`
    variables -- O3D_LIB_VARIANT (load an A/B build of the library, tools/build_variant.sh) and O3D_REQUIRE_GRAPH (fail
    instead of falling back to the eager step when the HIP-graph capture fails); experiments use tools/ab.sh on a scratch
    edit or the module-level test hooks (tools/ab_hook.py), and leave nothing behind"""
    import glob
    csrc = glob.glob(os.path.join(ROOT, "open3dsot_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "open3dsot_amd", "csrc", "*.hpp"))
    assert len(csrc) >= 15
    for f in csrc:
        assert "getenv" not in open(f).read(), f
    names = set()
    for f in glob.glob(os.path.join(ROOT, "open3dsot_amd", "*.py")) + glob.glob(os.path.join(ROOT, "pointnet2_ops", "*.py")):
        names |= set(re.findall(r"[\"'](O3D_[A-Z0-9_]+)[\"']", open(f).read()))
    names -= set(header_constants())      # the limits the modules read from capi.CONSTANTS are the header's #defines, not variables
    assert names <= {"O3D_LIB_VARIANT", "O3D_REQUIRE_GRAPH"}, names
