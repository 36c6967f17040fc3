"""Layer 0 of the P2B template<->search fusion -- o3d_xcorr_expand / o3d_xcorr_reduce (csrc/xcorr.hip) -- called through the
C ABI with raw pointers against the plain numpy fp64 reference tests/pointwise_oracle.py (tied to the materialised
(B, 1 + 3 + f, M, N) tensor under a 1x1 convolution and autograd by tests/test_pointwise_oracle_cpu.py).  Method, helpers,
bounds and the pins file are those of tests/test_pointwise_kernels_gpu.py, imported from there: EXACT leg (dyadic inputs,
equality), ROUNDED leg (randn, (n + 8) * 2^-24 * sum|t_i|; the statistics partials against the fp64 sums over the kernel's own
stored Y0), sentinel guards around every output.

The shapes walk every template count the entries accept, M = 4 ... 64: the reduce kernel folds its per-thread sums of S in
1024 / M / 16 = 16, 8, 4, 2 and 1 rounds of 16 LDS slots; and channel counts whose share per workgroup row
(C0 / ysplit = 16, 40, 36, 32, 32 for ysplit = 1, 2, 4, 2, 4) is and is not a multiple of the 32 channels a pass of the
expand kernel's four waves covers, so the clamp at the end of a share runs.
"""
import numpy as np
import pytest
import torch

import pointwise_oracle as O
from test_pointwise_kernels_gpu import (EINVAL, EXTRA_ROWS, Randn, _pins, compare, dev, devs, host, lib, outbuf, pre, ptr,  # noqa: F401
                                        st, tail_intact, untouched)

pytestmark = pytest.mark.gpu

MODES = ("part+c", "part", "none")
PAD_Z = 64.0               # what the padding columns of Z (beyond B*M) hold: a read of one shows on both legs


def _inputs(lib, draw, B, M, N, C0, ldw):
    i = O.xcorr_inputs(draw, B, M, N, C0, ldw)
    i.Z[:, B * M:] = PAD_Z
    assert lib.o3d_xcorr_reduce_groups(C0) == C0 // 16 and (M * N) % 1024 == 0 and i.ldz > B * M
    return i


def _expand(lib, draw, B, M, N, C0, ldw):
    i = _inputs(lib, draw, B, M, N, C0, ldw)
    P, rows = B * M * N, B * M * N // 256
    Z, sim, W0, stat_c = dev(i.Z), dev(i.sim), dev(i.W0), dev(i.stat_c)
    for mode in MODES:
        sc = i.stat_c if mode == "part+c" else None
        r = O.xcorr_expand(i.Z, i.sim, i.W0[:, 0], B, M, N, sc)
        pre(draw, {"xc.Y0": r.Y0_abs, "xc.part0": r.part_abs[:, 0], "xc.part1": r.part_abs[:, 1]})
        Yf, Y0 = outbuf((C0, P))
        Pf, part = outbuf((rows + EXTRA_ROWS, 2, C0))
        assert lib.o3d_xcorr_expand(ptr(Z), i.ldz, ptr(sim), ptr(W0), ldw, B, M, N, C0, ptr(Y0), ptr(part) if mode != "none" else None,
                                    ptr(stat_c) if mode == "part+c" else None, st()) == 0
        torch.cuda.synchronize()
        tail_intact(Yf, Pf)
        got = host(Y0)
        compare("xcorr_expand.Y0", got, r.Y0, r.Y0_abs, r.n, draw)
        if mode == "none":
            assert untouched(Pf)
            continue
        assert untouched(part[rows:]), "xcorr_expand: a statistics row beyond P / 256 was written"
        gp = host(part[:rows])
        pr, pa = (r.part, r.part_abs) if draw.exact else O.stats_fwd(got, np.abs(got), 256, sc)
        compare("xcorr_expand.part_sum", gp[:, 0], pr[:, 0], pa[:, 0], 256, draw)
        compare("xcorr_expand.part_var", gp[:, 1], pr[:, 1], pa[:, 1], 256, draw)


def _reduce(lib, draw, B, M, N, C0, ldw):
    i = _inputs(lib, draw, B, M, N, C0, ldw)
    P, groups = B * M * N, C0 // 16
    r = O.xcorr_reduce(i.dN, i.Y0, i.A1, i.A2, i.A3, i.sim, i.W0[:, 0], B, M, N)
    pre(draw, {"xc.S": r.S_abs, "xc.dsim": r.dsim_abs, "xc.dw": r.dw_abs})
    Sf, S = outbuf((C0, i.lds))
    Df, dsim = outbuf((groups + EXTRA_ROWS, P))
    Wf, dw = outbuf((B, C0))
    d = devs(i.dN, i.Y0, i.A1, i.A2, i.A3, i.sim, i.W0)
    assert lib.o3d_xcorr_reduce(*map(ptr, d), ldw, B, M, N, C0, ptr(S), i.lds, ptr(dsim), ptr(dw), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Sf, Df, Wf)
    assert untouched(S[:, B * M:]), "xcorr_reduce: a padding column of S was written"
    assert untouched(dsim[groups:]), "xcorr_reduce: a dsim_part row beyond o3d_xcorr_reduce_groups(C0) was written"
    compare("xcorr_reduce.S", host(S[:, :B * M]), r.S, r.S_abs, r.S_n, draw)
    compare("xcorr_reduce.dsim_part", host(dsim[:groups]), r.dsim_part, r.dsim_abs, r.dsim_n, draw)
    compare("xcorr_reduce.dw_part", host(dw), r.dw_part, r.dw_abs, r.dw_n, draw)


@pytest.mark.parametrize("ldw", [1, 5])
@pytest.mark.parametrize("B,M,N,C0", O.XCORR_SHAPES)
def test_xcorr_expand_exact(lib, B, M, N, C0, ldw):
    _expand(lib, O.Dyadic(1100 + M + C0 + ldw), B, M, N, C0, ldw)


@pytest.mark.parametrize("B,M,N,C0", O.XCORR_SHAPES)
def test_xcorr_expand_rounded(lib, B, M, N, C0):
    _expand(lib, Randn(31 + M), B, M, N, C0, 5)


@pytest.mark.parametrize("ldw", [1, 5])
@pytest.mark.parametrize("B,M,N,C0", O.XCORR_SHAPES)
def test_xcorr_reduce_exact(lib, B, M, N, C0, ldw):
    _reduce(lib, O.Dyadic(1200 + M + C0 + ldw), B, M, N, C0, ldw)


@pytest.mark.parametrize("B,M,N,C0", O.XCORR_SHAPES)
def test_xcorr_reduce_rounded(lib, B, M, N, C0):
    _reduce(lib, Randn(37 + M), B, M, N, C0, 5)


# (B, M, N, C0, columns of Z / S short of B*M): everything xc_shape_ok and the leading-dimension checks refuse
REFUSALS = {"M=12": (1, 12, 256, 16, 0), "M=128": (1, 128, 8, 16, 0), "C0=24": (1, 4, 256, 24, 0),
            "MN%1024": (1, 4, 128, 16, 0), "ld_too_small": (2, 8, 128, 16, 1)}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_xcorr_refusals(lib, case):
    B, M, N, C0, short = REFUSALS[case]
    P, ld = B * M * N, B * M - short
    Cbuf = (C0 + 15) // 16 * 16
    z = torch.zeros(Cbuf * max(P, B * M), device="cuda")
    one = torch.ones(Cbuf, device="cuda")
    Yf, Y0 = outbuf((Cbuf, P))
    Pf, part = outbuf((P // 256 + EXTRA_ROWS, 2, Cbuf))
    assert lib.o3d_xcorr_expand(ptr(z), ld, ptr(z), ptr(one), 1, B, M, N, C0, ptr(Y0), ptr(part), ptr(one), st()) == EINVAL
    Sf, S = outbuf((Cbuf, B * M))
    Df, dsim = outbuf((Cbuf // 16 + EXTRA_ROWS, P))
    Wf, dw = outbuf((B, Cbuf))
    assert lib.o3d_xcorr_reduce(ptr(z), ptr(z), ptr(one), ptr(one), ptr(one), ptr(z), ptr(one), 1, B, M, N, C0, ptr(S), ld, ptr(dsim),
                                ptr(dw), st()) == EINVAL
    torch.cuda.synchronize()
    assert all(untouched(f) for f in (Yf, Pf, Sf, Df, Wf))
