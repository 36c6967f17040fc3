"""tests/compact_gemm_oracle.py against the operator it stands for, without a GPU:
  * the three formulas (forward, data gradient, weight gradient) and the statistics rows against Conv2d + BatchNorm2d (training)
    + ReLU in fp64 under torch.autograd on the SLOT-WISE tensors (B, C, npoint, ns), padded copies included, to 1e-12;
  * the exactness condition (sum|terms| / spacing < 2^24) of every exact-leg case of tests/test_compact_gemm_kernels_gpu.py,
    over the same inputs -- proven here, before any GPU run;
  * the restated remainder-tile plan against hand-worked values, and the branches the split cases reach together;
  * what the padding contract of include/o3dsot.h implies.
"""
import numpy as np
import pytest
import torch

import compact_gemm_oracle as G
import compact_oracle as CO

TOL = 1e-12


def close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max()))
    assert a.shape == b.shape and float(np.abs(a - b).max()) <= TOL * scale, (what, float(np.abs(a - b).max()), scale)


class Gauss:
    exact = False

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def val(self, shape, step=None, lim=None):
        return self.rng.randn(*shape)

    def coef(self, shape, zero=True):
        return self.rng.randn(*shape)


def slot_columns(L, s):
    """(B, npoint, ns) column of every slot of segment s: slot k < cnt is the ball's k-th column, a padded copy its first"""
    B, npoint, ns = L.B, L.npoint[s], L.ns
    sl = slice(L.ball_base[s], L.ball_base[s] + L.nballs_s[s])
    off, cnt = L.ball_off[sl][:, None], L.ball_cnt[sl][:, None]
    k = np.arange(ns)[None, :]
    return (off + np.where(k < cnt, k, 0)).reshape(B, npoint, ns)


@pytest.mark.parametrize("family,S", [("paired", 8), ("sparse", 2048), ("mixed", 0)])
def test_oracle_matches_conv_bn_relu_on_the_slots(family, S):
    L = G.layout(family)
    Cin, Cout, eps = 5, 7, 1e-5
    i = G.Inputs(Gauss(3), L, Cin, Cout)
    fwd = G.ref_fwd(i, 128, S)
    assert np.isnan(fwd.Y[:, L.unwritten()]).all() and np.isfinite(fwd.Y[:, L.written]).all()
    counts = G.counts_of(L)
    assert counts == [float(L.nballs_s[s] * L.ns) for s in range(L.nseg)]
    tot = np.stack([np.nansum(np.where((np.array([G.part_seg(L, r, fwd.nrows) for r in range(fwd.nrows)]) == s)[:, None, None],
                                       fwd.part, np.nan), axis=0) for s in range(L.nseg)])
    close(tot, fwd.tot, "the rows of the plan add up to the segment totals")
    mean, invstd, _, _ = G.bn_fwd_consts(L, fwd.part, counts, i.gamma_o, i.beta_o, eps, i.stat_c)
    # slot-wise upstream gradient (w.r.t. the BatchNorm output); the compact dN is its sum over the slots of a column
    rng = np.random.RandomState(5)
    dN = np.zeros((Cout, L.ldp))
    Gs, dW_t = [], 0.0
    for s in range(L.nseg):
        cols = slot_columns(L, s)
        g = rng.randn(L.B, Cout, L.npoint[s], L.ns)
        np.add.at(dN.T, cols.reshape(-1), g.transpose(0, 2, 3, 1).reshape(-1, Cout))
        Gs.append(g)
    i.dN = np.where(np.isnan(i.dN), np.nan, dN)
    i.Y = fwd.Y
    bwd_tot = np.zeros((L.nseg, 2, Cout))          # BatchNorm-backward sums of THIS layer, from the compact columns
    for s in range(L.nseg):
        sl = slice(L.start[s], L.start[s] + L.live[s])
        bwd_tot[s, 0], bwd_tot[s, 1] = dN[:, sl].sum(1), (dN[:, sl] * (fwd.Y[:, sl] - mean[s][:, None])).sum(1)
    A = G.bn_bwd_fin_ref(bwd_tot, counts, i.gamma_o, mean, invstd)
    i.A1, i.A2, i.A3 = A["A1"].ravel(), A["A2"].ravel(), A["A3"].ravel()
    i.Wt = i.W.T.copy()
    dg = G.ref_dgrad(i, 128, S)
    wg = G.ref_wgrad(i)
    for s in range(L.nseg):
        cols = torch.from_numpy(slot_columns(L, s))
        sc, sh, mu = (torch.from_numpy(np.asarray(v).reshape(L.nseg, Cin)[s]).view(1, Cin, 1, 1)
                      for v in (i.in_scale, i.in_shift, i.in_mean))
        Xs = torch.from_numpy(np.nan_to_num(i.X))[:, cols].permute(1, 0, 2, 3)             # (B, Cin, npoint, ns)
        n = (Xs * sc + sh).requires_grad_(True)
        conv = torch.nn.Conv2d(Cin, Cout, 1, bias=False).double()
        bn = torch.nn.BatchNorm2d(Cout, eps=eps).double().train()
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(i.W).view(Cout, Cin, 1, 1))
            bn.weight.copy_(torch.from_numpy(i.gamma_o)); bn.bias.copy_(torch.from_numpy(i.beta_o))
        y = conv(torch.relu(n))
        (bn(y) * torch.from_numpy(Gs[s])).sum().backward()
        # forward: every slot of a column holds the column's value; batch statistics from the oracle's partial rows
        close(fwd.Y[:, cols.numpy()].transpose(1, 0, 2, 3), y.detach().numpy(), "Y")
        close(mean[s], y.detach().mean((0, 2, 3)).numpy(), "batch mean")
        close(1.0 / invstd[s] ** 2 - eps, y.detach().var((0, 2, 3), unbiased=False).numpy(), "biased variance")
        close(A["dgamma"] if L.nseg == 1 else bwd_tot[s, 1] * invstd[s], bn.weight.grad.numpy(), "dgamma")
        # data gradient: the class sum of the slot-wise gradient w.r.t. the producer's BatchNorm output
        gn = n.grad.numpy()
        want = np.zeros((Cin, L.ldp))
        np.add.at(want.T, cols.numpy().reshape(-1), gn.transpose(0, 2, 3, 1).reshape(-1, Cin))
        sl = slice(L.start[s], L.start[s] + L.live256[s])
        close(dg.G[:, sl], want[:, sl], "dNprev")
        close(dg.tot[s, 0], gn.sum((0, 2, 3)), "sum g")
        close(dg.tot[s, 1], (gn * (Xs - mu).numpy()).sum((0, 2, 3)), "sum g*(yprev - mean)")
        dW_t = dW_t + conv.weight.grad.numpy().reshape(Cout, Cin)
    close(wg.dW, dW_t, "dW over both segments")
    part_tot = np.stack([np.nansum(np.where((np.array([G.part_seg(L, r, dg.nrows) for r in range(dg.nrows)]) == s)[:, None, None],
                                            dg.part, np.nan), axis=0) for s in range(L.nseg)])
    close(part_tot, dg.tot, "data-gradient rows add up to the segment totals")


def test_padding_contract():
    """dN == 0 on the padding columns: whatever finite values Y, X / Yprev hold there, padding adds nothing to dW and to the
    data gradient's statistics, and dNprev is 0 there; the forward's statistics do not see padding either (cw = 0), while Y is
    stored there.  A dN that breaks the contract is refused by the oracle."""
    L = G.layout("paired")
    pad = G.padding(L)
    assert len(pad) > 0 and not L.cw[pad].any()
    i = G.Inputs(G.Dyadic(1), L, 64, 64)
    a = (G.ref_fwd(i, 128, 8), G.ref_dgrad(i, 128, 8), G.ref_wgrad(i))
    assert not a[1].G[:, pad].any() and np.isfinite(a[0].Y[:, pad]).all()
    i.X[:, pad] += 3.0
    i.Y[:, pad] -= 5.0
    b = (G.ref_fwd(i, 128, 8), G.ref_dgrad(i, 128, 8), G.ref_wgrad(i))
    assert np.array_equal(a[0].part, b[0].part, equal_nan=True) and np.array_equal(a[1].part, b[1].part, equal_nan=True)
    assert np.array_equal(a[2].dW, b[2].dW) and np.array_equal(a[1].G, b[1].G, equal_nan=True)
    assert not np.array_equal(a[0].Y[:, pad], b[0].Y[:, pad])
    i.dN[0, pad[0]] = 1.0
    with pytest.raises(AssertionError, match="padding contract"):
        G.ref_dgrad(i, 128, 8)


# ---- the plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,cap,want", [
    (16, 8, 64, (16, 0, 1, "R0")),            # R == 0
    (18, 8, 32, (16, 2, 4, "f4")),            # R = 2: 8 <= 8 -> four blocks, 18 + 6 = 24 workgroups
    (2, 8, 16, (0, 2, 4, "f4")),              # fewer tiles than slots: everything is tail
    (18, 14, 32, (14, 4, 2, "f2")),           # R = 4: 16 > 14, 8 <= 14 -> two blocks
    (19, 8, 64, (16, 3, 2, "f2")),            # R = 3: 12 > 8, 6 <= 8
    (50, 9, 96, (50, 0, 1, "2R>S")),          # R = 5: 10 > 9
    (8, 32, 8, (8, 0, 1, "cap")),             # four blocks chosen, 8 + 24 > 8: refused (no retry with two)
    (6, 2048, 24, (0, 6, 4, "f4")),           # T + 3R == cap exactly: fits
    (6, 2048, 23, (6, 0, 1, "cap")),
    (0, 8, 16, (0, 0, 1, "off")), (-2, 8, 16, (-2, 0, 1, "off")),      # T <= 0
    (18, 0, 32, (18, 0, 1, "off")), (18, -1, 32, (18, 0, 1, "off")),   # S <= 0
])
def test_tail_plan_hand_worked(T, S, cap, want):
    assert G.tail_plan_why(T, S, cap) == want and G.tail_plan(T, S, cap) == want[:3]


def test_stat_rows_of_a_paired_launch_by_hand():
    """paired: segment 0 has 2 live tiles of 16, segment 1 18 of 32 from column 2048 (tile 16); 8 slots: segment 0 is all
    tail (f = 4), segment 1 keeps 16 whole tiles and cuts tiles 16, 17 in four; extra rows from 48, segment 1's block at +8"""
    L = G.layout("paired")
    assert (L.live256, L.start1, L.ldp) == ([256, 2304], 2048, 6144)
    rows, nrows = G.stat_rows(L, 128, 8)
    assert nrows == 48 + 16
    by_row = {r: (c0, c1, s) for r, c0, c1, s in rows}
    assert len(by_row) == len(rows) == 2 * 4 + 16 + 2 * 4
    assert by_row[0] == (0, 32, 0) and by_row[48] == (32, 64, 0) and by_row[50] == (96, 128, 0)
    assert by_row[1] == (128, 160, 0) and by_row[51] == (160, 192, 0) and by_row[53] == (224, 256, 0)
    assert by_row[16] == (2048, 2176, 1) and by_row[31] == (2048 + 15 * 128, 2048 + 16 * 128, 1)
    assert by_row[32] == (4096, 4128, 1) and by_row[56] == (4128, 4160, 1) and by_row[33] == (4224, 4256, 1)
    assert by_row[61] == (4224 + 96, 4224 + 128, 1)
    assert not any(r in by_row for r in (2, 15, 34, 47, 54, 55, 62, 63))
    # every written column is in exactly one row, and no other column is
    seen = np.zeros(L.ldp, int)
    for _, c0, c1, _ in rows:
        seen[c0:c1] += 1
    assert (seen[L.written] == 1).all() and seen.sum() == len(L.written)
    rows64, n64 = G.stat_rows(L, 64, 8)                       # 64-column rows never split
    assert n64 == 96 and [r for r, *_ in rows64] == list(range(4)) + list(range(32, 32 + 36))


def test_split_cases_reach_every_branch():
    """a condition on the cases of the GPU file: R == 0, f == 4 with and without whole tiles, f == 2, f == 1 because 2R > S,
    a split refused by cap -- one by the smallest margin the layouts allow (mixed at 128 slots: 50 + 50 workgroups for 96) next
    to one that fills its grid exactly (sparse: 6 + 18 for 24) --, two segments with different plans in one launch, one segment
    and two"""
    assert G.cap_margin(50, 128, 96) == 4 and G.cap_margin(6, 2048, 24) == 0 and G.cap_margin(16, 8, 64) is None
    assert G.split_coverage() == G.SPLIT_BRANCHES
    for fam, S, M, K in G.SPLIT_CASES:
        L = G.layout(fam)
        rows, nrows = G.stat_rows(L, 128, S if S is not None else G.NATURAL_SLOTS[M])
        seen = np.zeros(L.ldp, int)
        for r, c0, c1, _ in rows:
            assert 0 <= r < nrows
            seen[c0:c1] += 1
        assert len({r for r, *_ in rows}) == len(rows) and (seen[L.written] == 1).all() and seen.sum() == len(L.written)


# ---- the exactness condition of every exact-leg case of the GPU file -------------------------------------------------------
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_exact_leg_precondition_forward_and_data_gradient(kind):
    cases = [(f, M, K, tile, 0) for f, M, K, tile, _ in G.PLAIN_CASES]
    cases += [(f, M, K, 128, S if S is not None else G.NATURAL_SLOTS[M]) for f, S, M, K in G.SPLIT_CASES]
    for fam, M, K, tile, S in cases:
        Cin, Cout = G.kind_dims(kind, M, K)
        i = G.Inputs(G.Dyadic(G.case_seed(kind, fam, M, K)), G.layout(fam), Cin, Cout)
        for s in {0, S}:
            (G.exact_fwd(G.ref_fwd(i, tile, s)) if kind == "fwd" else G.exact_dgrad(G.ref_dgrad(i, tile, s)))


def test_exact_leg_precondition_weight_gradient_and_fused():
    for fam, Cout, Cin in G.WGRAD_CASES:
        i = G.Inputs(G.Dyadic(G.case_seed("wgrad", fam, Cout, Cin)), G.layout(fam), Cin, Cout)
        G.assert_exact("cg.dW", G.ref_wgrad(i).dW_abs)
    for fam, Cout, dead in G.FUSED_CASES:
        L = G.layout(fam) if isinstance(fam, str) else G.Dense(fam)
        i = G.Inputs(G.Dyadic(G.case_seed("fused", fam, Cout)), L, 64, Cout, dead_channel=dead)
        r = G.ref_dgrad(i, 64)
        G.exact_dgrad(r), G.exact_fused(i, r), G.assert_exact("cg.dW", G.ref_wgrad(i).dW_abs)
        assert not dead or (i.in_scale[3] == 0 and r.mask[3, :L.live256[0]].all())      # segment 0's channel 3


def test_inputs_poison_every_column_no_entry_may_read():
    L = G.layout("paired")
    i = G.Inputs(G.Dyadic(2), L, 64, 64)
    dead = L.unwritten()
    assert dead.any() and all(np.isnan(a[:, dead]).all() and np.isfinite(a[:, ~dead]).all() for a in (i.X, i.Y, i.dN))
    assert not i.dN[:, G.padding(L)].any() and i.dN[:, L.real].any()
    assert CO.FILL_I == L.cw[dead][0]
