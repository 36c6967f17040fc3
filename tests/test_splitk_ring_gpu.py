"""The operand ring of the split-K GEMM tile (csrc/mlp_direct.hip: splitk_body) at every length of a wave's K slice the ring
treats differently, with the method, helpers and bounds of tests/test_gemm_kernels_gpu.py (flat layout) and
tests/test_compact_gemm_kernels_gpu.py (compact layout), imported from there: EXACT leg (dyadic inputs, equality), ROUNDED leg
(torch.randn, |err| <= (n + 8) * 2^-24 * sum|t_i|), sentinel guards, and the launch class (4) asserted before every launch.

A workgroup's four waves each contract a quarter of the K / 16 pairs of 8-k groups; a wave requests up to D groups (the ring
depth, a compile-time choice per operand mode and epilogue: SkRing) before its first MFMA and refills a set when its group is
consumed; the loop has a steady body (more than D groups left) and a last one that leaves after any pair.  Groups per wave at
the K of this file:
    112: 4 4 4 2    128: 4    144: 6 4 4 4    256: 8    320: 10    336: 12 10 10 10    528: 18 16 16 16
i.e. slices shorter than, equal to, one pair longer than and more than twice any depth up to 8, and uneven splits over the
waves.  The BatchNorm-backward operand reads its per-k constants from a per-wave LDS stage (one float4 per lane and array,
K <= 1024): K = 1040 is the first contraction that takes the kernel with the constants in registers instead (26 groups on
wave 0).
"""
import copy

import numpy as np
import pytest
import torch

import compact_gemm_oracle as G
import gemm_oracle as O
import test_compact_gemm_kernels_gpu as C
import test_gemm_kernels_gpu as T

pytestmark = pytest.mark.gpu

RING_KS = (112, 128, 144, 256, 320, 336, 528)
MS, PS = (64,), (64, 192)


@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi, fused, fused_heads, fused_pointwise  # noqa: F401  (register the signatures)
    return capi.load()


@pytest.mark.parametrize("K", RING_KS + (1040,))
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_ring_exact(lib, kind, K):
    T.sweep(lib, O.Dyadic(8000 + K), T.KINDS[kind][0], 4, MS, (K,), PS, T.KINDS[kind][1])


@pytest.mark.parametrize("K", RING_KS + (1040,))
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_ring_rounded(lib, kind, K):
    T.sweep(lib, T.Randn(8100 + K), T.KINDS[kind][0], 4, MS, (K,), PS, T.KINDS[kind][1])


@pytest.mark.parametrize("leg", ["exact", "rounded"])
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_ring_pair_two_slice_lengths(lib, kind, leg):
    """one pair launch, K = 128 (4 groups per wave: all in flight at once) next to K = 320 (10: the ring refills), 2 and 6 row
    blocks: against the oracle, and bit for bit against the two single launches"""
    k = T.KINDS[kind][0]
    variants = [(True, "part"), (False, "bias+resid")] if kind == "fwd" else [(True, "mask"), (False, "resid"), (False, "mask")]
    for n, (flag, epi) in enumerate(variants):
        draw = O.Dyadic(8200 + n) if leg == "exact" else T.Randn(8300 + n)
        T._pair(lib, k, draw, 4, 4, (64, 128, 192, flag, epi), (192, 320, 192, flag, epi))


def dead_second_segment():
    """the `paired` family with its second segment emptied (meta[1] = 0 live columns): segment 0 holds fewer than 256 live
    columns and ends inside its fourth 64-column tile; the padding up to 256 is computed, every tile of segment 1 is dead (its
    operands are NaN here) and must be left alone: sentinels in the output and in the statistics rows"""
    L = copy.deepcopy(G.layout("paired"))
    assert L.nseg == 2 and L.live[0] % 64 != 0 and L.live256[0] == 256 and L.start1 >= 512
    L.live[1], L.live256[1] = 0, 0
    L.meta[1, :2] = 0
    L.real = np.arange(L.live[0])
    L.written = np.arange(L.live256[0])
    L.cw[L.start1:] = float(np.nan)
    return L


@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_ring_compact_dead_segment(lib, kind):
    L = dead_second_segment()
    M, K = 128, 320
    C.expect_class(lib, 4, L.ldp, M, K, 64)
    Cin, Cout = G.kind_dims(kind, M, K)
    for draw in (G.Dyadic(8400), C.Randn(8401)):
        i = G.Inputs(draw, L, Cin, Cout)
        run = C.RUN[kind](lib, i, 64, 0, draw, "%s_c.c4" % kind)
        # (C.compare inside has checked: sentinel on every column and statistics row of the dead tiles, the bound on the live ones)
        rows = sorted(r[0] for r in run.ref.rows)
        assert rows == list(range(L.live256[0] // 64))
        out = run.Yf if kind == "fwd" else run.Gf
        view = out[:M * L.ldp].view(M, L.ldp)
        assert C.untouched(view[:, L.live256[0]:]), "a dead tile was written"
