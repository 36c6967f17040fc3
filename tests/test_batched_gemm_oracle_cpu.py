"""tests/batched_gemm_oracle.py against the operators it restates, and tests/test_batched_gemm_kernels_gpu.py against itself:
  * the adapter tied, to 1e-12, to Conv2d(1x1) -> BatchNorm2d (train) -> ReLU -> Conv2d(1x1) -> BatchNorm2d (train) -> ReLU ->
    max(dim=-1) on a (B, C, npoint, ns) tensor in torch fp64 under autograd, composed from the oracle's pieces with the
    BatchNorm constants derived in fp64 from the oracle's OWN statistics rows -- so it cannot merely mirror the kernels;
  * the exactness precondition of every exact-leg case of the GPU file, run here without a GPU (its case runners with
    lib = None stop after the reference and the precondition);
  * sensitivity: plausible mistakes applied to the oracle's output are rejected by the GPU file's `compare`.
No GPU."""
import numpy as np
import pytest
import torch

import batched_gemm_oracle as BO
import gemm_oracle as G
import test_batched_gemm_kernels_gpu as K

EPS = 1e-5


def rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def test_layout_is_the_flat_matrix_in_b_p_order():
    A = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)
    F = BO.flat(A)
    assert F.shape == (3, 8) and F[1, 5] == A[1, 1, 1] and np.array_equal(BO.unflat(F, 2), A)
    # statistics row b * P/128 + t is flat tile b * P/128 + t
    Y = np.random.RandomState(0).randn(2, 5, 256)
    part, _ = BO.stats_fwd(Y)
    assert part.shape == (4, 2, 5) and np.allclose(part[3, 0], Y[1, :, 128:].sum(1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("B,C0,C1,C2,npoint,ns", [(2, 5, 24, 9, 16, 8), (3, 19, 8, 40, 4, 32)])
def test_two_layer_pooled_stack_vs_autograd(B, C0, C1, C2, npoint, ns):
    torch.manual_seed(B * 10 + C0)
    P = npoint * ns
    conv1 = torch.nn.Conv2d(C0, C1, 1, bias=False).double()
    bn1 = torch.nn.BatchNorm2d(C1, eps=EPS).double().train()
    conv2 = torch.nn.Conv2d(C1, C2, 1, bias=False).double()
    bn2 = torch.nn.BatchNorm2d(C2, eps=EPS).double().train()
    with torch.no_grad():
        for bn in (bn1, bn2):
            bn.weight.copy_(torch.randn_like(bn.weight))
            bn.bias.copy_(torch.randn_like(bn.bias))
    x = torch.randn(B, C0, npoint, ns, dtype=torch.float64, requires_grad=True)
    gout = torch.randn(B, C2, npoint, dtype=torch.float64)
    pooled = torch.relu(bn2(conv2(torch.relu(bn1(conv1(x)))))).max(dim=-1)[0]
    pooled.backward(gout)

    X = x.detach().numpy().reshape(B, C0, P)
    W1, W2 = conv1.weight.detach().numpy()[:, :, 0, 0], conv2.weight.detach().numpy()[:, :, 0, 0]
    g1, b1, g2, b2 = (t.detach().numpy() for t in (bn1.weight, bn1.bias, bn2.weight, bn2.bias))
    assert P % 128 == 0
    # forward
    l1 = BO.fwd(X, W1, part=True, stat_c=np.linspace(-0.5, 0.5, C1))
    assert l1.part.shape == (B * P // 128, 2, C1) and l1.n == C0
    m1, is1, sc1, sh1 = G.bn_consts(l1.part, B * P, g1, b1, EPS, np.linspace(-0.5, 0.5, C1))
    l2 = BO.fwd(l1.Y, W2, sc1, sh1, part=True)
    m2, is2, sc2, sh2 = G.bn_consts(l2.part, B * P, g2, b2, EPS)
    pl = BO.pool_fwd(l2.Y, sc2, sh2, ns)
    assert rel(pl.out, pooled.detach().numpy()) <= 1e-12
    assert np.array_equal(pl.yarg, np.take_along_axis(l2.Y.reshape(B, C2, npoint, ns), pl.arg[..., None], -1)[..., 0])
    # backward: the pooled source, its statistics, then both layers
    dOut = gout.numpy()
    dN2 = BO.pooled_dense(dOut, pl.out, pl.arg, ns)
    p2, _ = BO.stats_bwd(dN2, l2.Y, m2)
    A = G.bn_bwd_coef(p2, B * P, g2, m2, is2)
    assert rel(p2.sum(0)[0], bn2.bias.grad.numpy()) <= 1e-12 and rel(p2.sum(0)[1] * is2, bn2.weight.grad.numpy()) <= 1e-12
    wg2 = BO.wgrad(dN2, l1.Y, l2.Y, *A, in_scale=sc1, in_shift=sh1)
    assert wg2.n == B * P and rel(wg2.dW, conv2.weight.grad.numpy()[:, :, 0, 0]) <= 1e-12
    d2 = BO.dgrad(dN2, W2, l2.Y, *A, l1.Y, sc1, sh1, m1)
    assert d2.n == C2
    A1 = G.bn_bwd_coef(d2.part, B * P, g1, m1, is1)
    assert rel(d2.part.sum(0)[0], bn1.bias.grad.numpy()) <= 1e-12
    wg1 = BO.wgrad(d2.G, X, l1.Y, *A1)
    assert rel(wg1.dW, conv1.weight.grad.numpy()[:, :, 0, 0]) <= 1e-12
    dx = BO.dgrad_plain(d2.G, W1, l1.Y, *A1)
    assert dx.n == C1 and rel(dx.G, x.grad.numpy().reshape(B, C0, P)) <= 1e-12
    # the *_abs sums dominate the values they bound
    for v, a in ((l2.Y, l2.Y_abs), (pl.out, pl.out_abs), (d2.G, d2.G_abs), (dx.G, dx.G_abs), (wg2.dW, wg2.dW_abs)):
        assert (np.abs(v) <= a * (1 + 1e-12)).all()


def test_pool_known_answers():
    Y = np.array([[[1.0, 3.0, 3.0, -2.0, -1.0, -1.0, -4.0, -3.0]]])                  # two balls of ns = 4, one channel
    r = BO.pool_fwd(Y, [1.0], [0.5], 4)
    assert r.out.tolist() == [[[3.5, 0.0]]] and r.arg.tolist() == [[[1, 0]]] and r.yarg.tolist() == [[[3.0, -1.0]]]
    assert r.out_abs.tolist() == [[[3.5, 0.0]]] and r.n == 2
    r = BO.pool_fwd(Y, [-1.0], [0.5], 4)                                              # negative scale: the smallest y wins
    assert r.out.tolist() == [[[2.5, 4.5]]] and r.arg.tolist() == [[[3, 2]]]
    r = BO.pool_fwd(Y, [0.0], [0.25], 4)                                              # dead scale: every slot ties
    assert r.out.tolist() == [[[0.25, 0.25]]] and r.arg.tolist() == [[[0, 0]]] and r.yarg.tolist() == [[[1.0, -1.0]]]


def test_pooled_source_known_answers():
    dOut = np.array([[[2.0, 3.0, 4.0, 5.0]]])
    out = np.array([[[1.0, 0.0, -0.0, -1.0]]])
    arg = np.array([[[3, 1, 0, 2]]])
    dN = BO.pooled_dense(dOut, out, arg, 4)
    assert dN.shape == (1, 1, 16) and dN[0, 0, 3] == 2.0 and np.count_nonzero(dN) == 1     # out <= 0 (and -0.0) gate to zero
    i = BO.Inputs(BO.Dyadic(0), 2, 3, 5, 128)
    for ns in (4, 8, 32):
        _, _, a = i.pooled(BO.Dyadic(1), ns)
        assert {int(v) % 4 for v in a.ravel()} == {0, 1, 2, 3} and a.min() == 0 and a.max() == ns - 1
    _, o, _ = i.pooled(BO.Dyadic(1), 4)
    assert (o > 0).any() and (o < 0).any() and (np.signbit(o) & (o == 0)).any() and (~np.signbit(o) & (o == 0)).any()


# ---- the exactness precondition of every exact case of the GPU file -------------------------------------------------------------
@pytest.mark.parametrize("Cout", K.FWD_GENERIC_COUT)
def test_exact_precondition_fwd_generic(Cout):
    K._fwd_generic(None, True, Cout)
    for Cin, Co in K.fwd_generic_shapes(Cout):
        assert Co % 64 != 0 or Cin % 16 != 0                 # shapes o3d_direct_ok refuses


def test_exact_precondition_fwd_direct_and_dgrad_direct():
    for Cin, Cout in K.FWD_DIRECT:
        assert Cout % 64 == 0 and Cin % 16 == 0
        K._fwd_direct(None, True, Cin, Cout)
    for Cin, Cout in K.DG_DIRECT:
        assert Cin % 64 == 0 and Cout % 16 == 0
        for ns in (0, 4, 32):
            K._dgrad_direct(None, True, Cin, Cout, ns)


@pytest.mark.parametrize("M", K.DG_M)
def test_exact_precondition_dgrad_generic(M):
    K._dgrad_generic(None, True, M)


def test_exact_precondition_plain_wgrad_pool_row_sum():
    for Cin in K.PLAIN_CIN:
        K._plain(None, True, Cin)
    for Cin, Cout in K.WG_SHAPES:
        K._wgrad(None, True, Cin, Cout)
    for ns in K.POOL_NS:
        K._pool(None, ns, True)
    for C in (1, 7):
        K._row_sum(None, C, True)


def test_exact_inputs_are_on_their_grids_and_cover_every_k():
    i = K.DgIn(BO.Dyadic(1), 2, 3, 128, 128)
    assert (i.W != 0).any(1).all() and ((i.W != 0).sum(0) <= 43).all()              # every co enters some output row
    i = BO.Inputs(BO.Dyadic(1), 2, 48, 37, 128)
    assert (i.W != 0).any(0).all()                                                   # every ci enters some output row
    r = K.fwd_ref(BO.Dyadic(1), i, True, "part_c")
    for v, s in ((r.Y, "gemm.Y"), (r.part[:, 1], "gemm.part1")):
        assert np.array_equal(v / G.SPACING[s], np.round(v / G.SPACING[s]))
    assert i.scale_p[1] < 0 and i.scale_p[2] == 0


# ---- sensitivity: the pins reject a subtly wrong kernel ------------------------------------------------------------------
def rejected(name, got, ref, ref_abs, n, exact):
    with pytest.raises(AssertionError):
        K.compare(name, got, ref, ref_abs, n, exact, ratios={})
    return True


def both_legs():
    return [(True, BO.Dyadic(11)), (False, K.Randn(11))]


def test_compare_accepts_the_oracle_and_fp32_rounding_of_it():
    i = BO.Inputs(K.Randn(1), 2, 19, 37, 128)
    r = K.fwd_ref(K.Randn(1), i, True, "part_c")
    K.compare("y", r.Y, r.Y, r.Y_abs, r.n, False, ratios={})
    K.compare("y", r.Y.astype(np.float32), r.Y, r.Y_abs, r.n, False, ratios={})
    i = BO.Inputs(BO.Dyadic(1), 2, 19, 37, 128)
    r = K.fwd_ref(BO.Dyadic(1), i, True, "part_c")
    K.compare("y", r.Y.astype(np.float32), r.Y, r.Y_abs, r.n, True, ratios={})


def test_rejects_a_statistics_row_of_the_neighbouring_tile():
    for exact, draw in both_legs():
        i = BO.Inputs(draw, 2, 19, 37, 384)
        r = K.fwd_ref(draw, i, True, "part_c")
        for s in (0, 1):
            assert rejected("part", np.roll(r.part, 1, axis=0)[:, s], r.part[:, s], r.part_abs[:, s], 128, exact)
        d = K.DgIn(draw, 2, 65, 17, 384)
        r = K.dgrad_ref(draw, d, d.dN)
        for s in (0, 1):
            assert rejected("gpart", np.roll(r.part, -1, axis=0)[:, s], r.part[:, s], r.part_abs[:, s], 128, exact)


def test_rejects_a_dropped_k_tail():
    for exact, draw in both_legs():
        for Cin, tail in ((19, 3), (20, 4), (3, 1)):
            i = BO.Inputs(draw, 2, Cin, 37, 128)
            r = K.fwd_ref(draw, i, False, "none")
            W = i.W.copy()
            W[:, Cin - tail:] = 0.0
            assert rejected("Y", BO.fwd(i.X, W).Y, r.Y, r.Y_abs, r.n, exact)


def test_rejects_arg_of_the_last_maximum():
    ns, plants = K.pool_ties()[1]
    Y = np.zeros((1, 1, len(plants), ns)) - 1.0
    for j, (slots, win) in plants.items():
        Y[0, 0, j, slots] = 3.0
    r = BO.pool_fwd(Y.reshape(1, 1, -1), [1.0], [0.5], ns)
    assert r.arg[0, 0].tolist() == [plants[j][1] for j in range(len(plants))]
    last = ns - 1 - r.n32[..., ::-1].argmax(-1)
    K.compare_int("arg", r.arg, r.arg)
    with pytest.raises(AssertionError):
        K.compare_int("arg", last, r.arg)


def test_rejects_a_pooled_gradient_without_the_gate():
    for exact, draw in both_legs():
        for ns in (4, 32):
            i = K.DgIn(draw, 2, 20, 16, 128)
            dN, (dOut, out, arg) = K.dg_source(draw, i, ns)
            r = K.dgrad_ref(draw, i, dN)
            ungated = BO.pooled_dense(dOut, np.ones_like(out), arg, ns)
            bad = BO.dgrad(ungated, i.W, i.Y, i.A1, i.A2, i.A3, i.Yprev, i.scale_p, i.shift_p, i.mean_p)
            assert rejected("G", bad.G, r.G, r.G_abs, r.n, exact)
            w = K.wgrad_ref(draw, i, dN, True)
            badw = BO.wgrad(ungated, i.X, i.Y, i.A1, i.A2, i.A3, in_scale=i.in_scale, in_shift=i.in_shift)
            assert rejected("dW", badw.dW, w.dW, w.dW_abs, w.n, exact)


def test_rejects_a_slice_missing_from_dw():
    for exact, draw in both_legs():
        i = BO.Inputs(draw, 2, 19, 37, 128)
        w = K.wgrad_ref(draw, i, i.dN, False)
        dN = i.dN.copy()
        dN[1, :, 96:128] = 0.0                                # the last 32-position chunk ...
        Y = i.Y.copy()
        Y[1, :, 96:128] = 0.0
        part = BO.wgrad(dN, i.X, Y, i.A1, i.A2, np.zeros_like(i.A3))
        full = BO.wgrad(i.dN, i.X, i.Y, i.A1, i.A2, np.zeros_like(i.A3))
        missing = w.dW - (full.dW - part.dW)                  # ... of the A1 / A2 terms never summed
        assert rejected("dW", missing, w.dW, w.dW_abs, w.n, exact)


def test_rejects_one_element_off_by_twice_its_bound():
    draw = K.Randn(5)
    i = K.DgIn(draw, 2, 65, 17, 128)
    f = K.fwd_ref(draw, i, True, "part_c")
    d = K.dgrad_ref(draw, i, i.dN)
    w = K.wgrad_ref(draw, i, i.dN, True)
    Y, sc, sh = K.pool_inputs(draw, 2, 5, 7, 8)
    p = K.pool_ref(draw, Y, sc, sh, 8)
    Gm, rs = K.row_sum_ref(draw, 7, 1028)
    for name, ref, ra, n in (("Y", f.Y, f.Y_abs, f.n), ("part", f.part, f.part_abs, 128), ("G", d.G, d.G_abs, d.n),
                             ("gpart", d.part, d.part_abs, 128), ("dW", w.dW, w.dW_abs, w.n), ("out", p.out, p.out_abs, p.n),
                             ("row_sum", rs.dW, rs.dW_abs, rs.n)):
        at = tuple(np.argwhere(ra > 0)[-1])
        got = ref.copy()
        got[at] += 2 * (n + 8) * K.E24 * ra[at]
        assert rejected(name, got, ref, ra, n, False)
        K.compare(name, ref, ref, ra, n, False, ratios={})


def test_case_tables_promise_what_the_issue_lists():
    assert K.FWD_GENERIC_COUT == (1, 37, 64, 65, 100, 128, 129, 200, 256, 300) and (48, 37) in K.fwd_generic_shapes(37)
    assert K.DG_M == (3, 20, 64, 65, 128, 129, 300) and K.DG_COUT == (5, 16, 17, 40) and K.DG_NS == (0, 4, 8, 32)
    assert K.PLAIN_CIN[:4] == (3, 19, 131, 259) and K.PLAIN_COUT == (64, 128)
    assert K.WG_SHAPES == ((3, 64), (19, 37), (128, 128), (131, 129), (259, 64)) and len(K.WG_INST) == 4
    assert {K.generic_class(c) for c in K.PLAIN_CIN} == {64, 128, 256}      # EPI 2 in all three row tiles
    assert K.POOL_NS == (4, 8, 32, 36, 64) and K.ROW_SUM_P == (4, 1020, 1024, 1028, 4100)
    assert any(B * C * n % 32 for B, C, n in K.POOL_SHAPES) and {C for _, C, _ in K.POOL_SHAPES} == {1, 5}
