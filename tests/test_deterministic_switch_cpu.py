"""Deterministic mode, the parts that need no GPU: the switch, the two ordered entry points in the header and the binding, and
what o3d_group_reduce_gather_ordered_scratch (host code) answers for the set abstractions of bench.py's configurations."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RG_CH = 2048


def test_switch_defaults_to_off_and_round_trips():
    from open3dsot_amd import fused
    assert fused.deterministic_enabled() is False
    try:
        fused.set_deterministic(True)
        assert fused.deterministic_enabled() is True
        fused.set_deterministic(0)
        assert fused.deterministic_enabled() is False
        fused.set_deterministic(1)
        assert fused.deterministic_enabled() is True
    finally:
        fused.set_deterministic(False)
    assert fused.deterministic_enabled() is False
    assert fused.reduce_gather_enabled() is True          # the neighbouring switch is untouched


def test_ordered_entries_are_declared_and_bound():
    from open3dsot_amd import capi
    text = open(os.path.join(ROOT, "include", "o3dsot.h")).read()
    for name in ("o3d_group_reduce_gather_ordered_scratch", "o3d_group_reduce_gather_ordered"):
        assert text.count(name + "(") == 1, name
        assert name in capi.SIGNATURES
    # the argument lists of their twins
    assert capi.SIGNATURES["o3d_group_reduce_gather_ordered"] == capi.SIGNATURES["o3d_group_reduce_gather"]
    assert capi.SIGNATURES["o3d_group_reduce_gather_ordered_scratch"] == capi.SIGNATURES["o3d_group_reduce_gather_scratch"]
    assert capi.RESTYPES["o3d_group_reduce_gather_ordered_scratch"] is capi.RESTYPES["o3d_group_reduce_gather_scratch"]
    lib = capi.load()
    assert lib.o3d_group_reduce_gather_ordered.argtypes == capi.SIGNATURES["o3d_group_reduce_gather_ordered"]
    assert "ordered_reduce_oracle.py" in text             # the header says where its order is restated


def _sa_shapes(B, M, N):
    """(name, reduce_dims, spanmax) of the set abstractions of a BAT / P2B step that run the layer-0 list sums: backbone levels
    1 and 2 (template + search in one paired call; level 0 is xyz-only and takes o3d_group_dw0_xyz) and the vote aggregation"""
    from open3dsot_amd import gemm
    out = []
    for level in (1, 2):
        cl = gemm.Compact(B, 32, [M >> (level + 1), N >> (level + 1)], [M >> level, N >> level])
        out.append(("level %d" % level, cl.reduce_dims, max(cl.npoints) * 32))
    cl = gemm.Compact(B, 16, [64], [N >> 3])
    out.append(("vote aggregation", cl.reduce_dims, 64 * 16))
    return out


@pytest.mark.parametrize("B", [48, 100])
@pytest.mark.parametrize("N", [1024, 2048])
def test_bench_configurations_fit_the_ordered_kernels(B, N):
    """every set abstraction of bench.py's configurations (512/1024 and 512/2048 points, 48 and 100 pairs) fits: same scratch
    size as the default pair's.  The answer depends on the SIZES only, so the dense worst case (synth.make_dense_batch: every
    slot a distinct neighbour) is covered by the same rows."""
    from open3dsot_amd import capi
    lib = capi.load()
    for name, rd, span in _sa_shapes(B, 512, N):
        nseg, ldm = rd[1], max(rd[3], rd[5])
        nchunk = (span + 4 + RG_CH - 1) // RG_CH
        want = B * nseg * (nchunk * ldm + 1)
        assert lib.o3d_group_reduce_gather_ordered_scratch(*rd, span) == want, (name, rd, span)
        assert lib.o3d_group_reduce_gather_scratch(*rd, span) == want, (name, rd, span)


def test_ordered_budget_is_tighter_and_argument_checks():
    from open3dsot_amd import capi
    lib = capi.load()
    f, g = lib.o3d_group_reduce_gather_ordered_scratch, lib.o3d_group_reduce_gather_scratch
    assert f(1, 1, 1024, 16384, 0, 0, 32768) == -1 and g(1, 1, 1024, 16384, 0, 0, 32768) == -1
    # the reduce kernel's 80 KiB: 2*(ld + npoint)*4 + 24584 bytes by default, 3072 more with the head-piece slots
    assert g(1, 1, 1024, 5632, 0, 0, 2044) > 0 and f(1, 1, 1024, 5632, 0, 0, 2044) == 5632 + 1
    assert g(1, 1, 1024, 5888, 0, 0, 2044) > 0 and f(1, 1, 1024, 5888, 0, 0, 2044) == -1
    # the build kernel's 128 KiB: (nchunk*ld + 1025)*4 by default, 8192 more with the staged chunk
    assert g(1, 1, 64, 1024, 0, 0, 30 * 2048 - 4) > 0 and f(1, 1, 64, 1024, 0, 0, 30 * 2048 - 4) == -1
    assert f(1, 1, 64, 1024, 0, 0, 28 * 2048 - 4) == 28 * 1024 + 1
    for bad in ((0, 1, 64, 128, 0, 0, 2048), (2, 3, 64, 128, 0, 0, 2048), (2, 1, 0, 128, 0, 0, 2048), (2, 1, 64, 0, 0, 0, 2048),
                (2, 1, 64, 128, 0, 0, 0), (2, 2, 64, 128, 0, 128, 2048), (2, 2, 64, 128, 64, 0, 2048)):
        assert f(*bad) == -1, bad
