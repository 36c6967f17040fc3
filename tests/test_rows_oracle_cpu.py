"""tests/rows_oracle.py without a GPU:
  * the composed stages against nn.Sequential(Linear, BatchNorm1d, ReLU, ...) in fp64 under autograd, to 1e-12: training and
    eval mode, with and without bias / BatchNorm / ReLU, the running statistics (unbiased variance), both gradient sources
    and the summed input gradient of two stacks;
  * the exactness condition of every exact-leg case of tests/test_rows_kernels_gpu.py, the conditions its bounds put on the
    inputs (|mean| <= 16 std per feature; no pre-activation within rounding of 0 on the rounded leg), and the case tables
    as a checklist of the sizes that file promises to execute;
  * sensitivity: plausible mistakes applied to the oracle's own output are rejected by the GPU file's `compare`.
"""
import numpy as np
import pytest
import torch

import rows_oracle as O
import test_rows_kernels_gpu as K

TOL = 1e-12


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.abs(a - b).max() <= TOL * (1 + np.abs(b).max())


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def torch_layer(i, Cin, Cout, bias, bn, relu, training):
    mods = [torch.nn.Linear(Cin, Cout, bias=bias)]
    mods[0].weight.data = t64(i.W)
    if bias:
        mods[0].bias.data = t64(i.b)
    if bn:
        b = torch.nn.BatchNorm1d(Cout, eps=O.EPS, momentum=O.MOMENTUM)
        b.weight.data, b.bias.data = t64(i.gamma), t64(i.beta)
        b.running_mean, b.running_var = t64(i.rm).clone(), t64(i.rv).clone()
        mods.append(b)
    if relu:
        mods.append(torch.nn.ReLU())
    seq = torch.nn.Sequential(*mods).double()
    return seq.train(bool(training))


@pytest.mark.parametrize("training", (1, 0))
@pytest.mark.parametrize("bias,bn,relu", [(True, True, True), (False, True, True), (True, True, False), (True, False, False),
                                          (False, False, False)])
@pytest.mark.parametrize("R", (2, 5, 33))
def test_layer_matches_torch_under_autograd(R, bias, bn, relu, training):
    Cin, Cout = 7, 6
    draw = K.Randn(R + 10 * training)
    i = O.fwd_inputs(draw, R, Cin, Cout, bias, bn)
    seq = torch_layer(i, Cin, Cout, bias, bn, relu, training)
    x = t64(i.X).requires_grad_(True)
    y = seq(x)
    g = draw.val((R, Cout))
    y.backward(t64(g))
    f = O.forward(i.X, i.W, i.b, i.gamma, i.beta, i.rm, i.rv, training, relu)
    assert close(f.Y, y.detach().numpy())
    if bn:
        assert close(f.rm, seq[1].running_mean.numpy()) and close(f.rv, seq[1].running_var.numpy())
        if training:
            assert not close(f.rv, i.rv)
    r = O.backward(g, i.X, f.Z, f.mean, f.invstd, i.gamma, i.beta, relu, training)
    assert close(r.dW, seq[0].weight.grad.numpy())
    if bias:
        assert close(r.db, seq[0].bias.grad.numpy())
    if bn:
        assert close(r.dgamma, seq[1].weight.grad.numpy()) and close(r.dbeta, seq[1].bias.grad.numpy())
    dX = O.input_grad([(r.dZ, np.asarray(i.W))])
    assert close(dX.dX, x.grad.numpy())


def test_r1_training_keeps_the_biased_variance():
    """torch refuses a BatchNorm1d over one row in training mode; the documented rule (unbiased only when R > 1)"""
    u = O.running_update(np.ones(3), np.ones(3), np.full(3, 2.0), np.zeros(3), 1)
    assert np.allclose(u.rv, 1 - O.MOMENTUM) and np.allclose(u.rm, 1 + O.MOMENTUM)


@pytest.mark.parametrize("training", (1, 0))
def test_two_stacks_on_shared_rows_match_torch(training):
    """x -> two stacks of two layers each; layer 1's gradient comes from dZup . Wup, x's from the sum over the stacks"""
    R, Cin, H, Cout = 9, 5, 8, (4, 6)
    draw = K.Randn(5 + training)
    X = draw.val((R, Cin))
    x = t64(X).requires_grad_(True)
    sources = []
    for s in range(2):
        i1, i2 = O.fwd_inputs(draw, R, Cin, H), O.fwd_inputs(draw, R, H, Cout[s])
        i1.X = X
        l1, l2 = torch_layer(i1, Cin, H, True, True, True, training), torch_layer(i2, H, Cout[s], True, True, True, training)
        y = l2(l1(x))
        g = draw.val((R, Cout[s]))
        y.backward(t64(g))
        f1 = O.forward(X, i1.W, i1.b, i1.gamma, i1.beta, i1.rm, i1.rv, training, True)
        f2 = O.forward(f1.Y, i2.W, i2.b, i2.gamma, i2.beta, i2.rm, i2.rv, training, True)
        assert close(f2.Y, y.detach().numpy())
        r2 = O.backward(g, f1.Y, f2.Z, f2.mean, f2.invstd, i2.gamma, i2.beta, True, training)
        up = O.source_up(r2.dZ, i2.W)
        r1 = O.backward(up.g, X, f1.Z, f1.mean, f1.invstd, i1.gamma, i1.beta, True, training, up.g_abs, up.n)
        assert close(r2.dW, l2[0].weight.grad.numpy()) and close(r1.dW, l1[0].weight.grad.numpy())
        assert close(r1.dgamma, l1[1].weight.grad.numpy()) and close(r1.db, l1[0].bias.grad.numpy())
        sources.append((r1.dZ, np.asarray(i1.W)))
    assert close(O.input_grad(sources).dX, x.grad.numpy())
    assert not close(O.input_grad(sources[:1]).dX, x.grad.numpy())


def test_mask_is_strict():
    """a pre-activation of exactly 0 passes no gradient (torch's threshold backward on the stored output: y > 0)"""
    c = O.BWD_CASES[0]
    i = O.bwd_inputs(O.Dyadic(2000), c)
    row, feats = i.planted
    a = O.bn_act(i.Z, i.mean, i.invstd, i.gamma, i.beta, True)
    assert (a.pre[row, feats] == 0).all() and (i.g[row, feats] != 0).all()
    r = O.bn_bwd(i.g, i.Z, i.mean, i.invstd, i.gamma, i.beta, True, False)
    assert not r.dZ[row, feats].any() and not r.mask[row, feats].any()
    z = t64(i.Z).requires_grad_(True)
    bn = torch.nn.functional.batch_norm(z, t64(i.mean), 1 / t64(i.invstd) ** 2 - O.EPS, t64(i.gamma), t64(i.beta), False, 0.0,
                                        O.EPS)
    torch.relu(bn).backward(t64(i.g))
    assert close(r.dZ, z.grad.numpy())


# ---- the conditions of the GPU file, proven here ---------------------------------------------------------------------------
def test_exact_preconditions():
    seen = O.exact_preconditions()
    names = {n for n, _ in seen}
    assert {"rows.Z", "rows.g", "rows.dZ", "rows.dW", "rows.db", "rows.dZ.eval", "rows.dW.eval", "rows.db.eval", "rows.dbeta",
            "rows.dgamma", "rows.dX"} <= names
    assert all(w < O.TWO24 for _, w in seen)


def test_exact_results_are_fp32_numbers():
    """what the exact leg compares with equality is representable in fp32, element by element"""
    for k, c in enumerate([c for c in O.BWD_CASES if O.exact_ok(c) and not c.input]):
        i = O.bwd_inputs(O.Dyadic(2000 + k), c)
        r = O.backward(i.g, i.X, i.Z, i.mean, i.invstd, i.gamma, i.beta, c.relu, c.training, i.g_abs, i.g_n)
        for a in (r.dZ, r.dW, r.db) + ((r.dgamma, r.dbeta) if c.bn else ()):
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a), O.case_id(c)


def test_forward_inputs_keep_the_mean_within_16_std():
    for k, c in enumerate(O.FWD_CASES):
        for draw in (O.Dyadic(1000 + k), K.Randn(31 + k)):
            i = O.fwd_inputs(draw, c.R, c.Cin, c.Cout, c.bias, c.bn)
            if c.bn and c.training and c.R > 1:
                assert O.feature_spread(O.linear(i.X, i.W, i.b).Z) <= 16.0, O.case_id(c)


def test_rounded_backward_inputs_keep_the_mask_off_zero():
    for k, c in enumerate(O.BWD_CASES):
        if not c.input:
            assert O.mask_margin(O.bwd_inputs(K.Randn(41 + k), c), c.relu) > 16 * K.E24, O.case_id(c)
    for C in O.GROUP_WIDTHS:
        c = O._c(R=O.GROUP_R, Cin=O.GROUP_CIN, C=C)
        assert O.mask_margin(O.bwd_inputs(K.Randn(67 + C), c), True) > 16 * K.E24


def test_case_tables_list_every_promised_size():
    F, B = O.FWD_CASES, O.BWD_CASES
    assert {c.R for c in F} == {1, 5, 31, 32, 33, 48, 64} <= {c.R for c in B}
    assert all(not c.training for c in F if c.R == 1)
    assert {c.Cout for c in F} | {c.C for c in B} >= {4, 8, 9, 40, 128}
    assert {c.Cin for c in F} == {3, 70, 72, 260, 1024} == {c.Cin for c in B}
    assert any(c.Cin == 72 and c.pad == 3 for c in F) and any(c.Cin == 72 and c.off == 1 for c in F)
    assert any(c.Cin == 72 and c.pad == 3 for c in B) and any(c.Cin == 72 and c.off == 1 for c in B)
    for flag in ("bias", "bn", "relu", "training", "running"):
        assert {bool(getattr(c, flag)) for c in F} == {True, False}, flag
    assert all(c.bn for c in F if c.relu) and all(c.running for c in F if c.bn and not c.training)
    assert any(not c.save for c in F) and any(len(c.save) == 3 for c in F)
    assert {c.lddy for c in B if not c.cup} == {0, 5} and {c.cup for c in B if c.cup and not c.input} == {4, 9, 128, 1024}
    assert any(c.input for c in B) and O.LDDX_PAD == 5
    assert {c.R for c in B if O.exact_ok(c) and c.bn and c.training and not c.input} == {32, 64}
    assert O.GROUP_WIDTHS == (4, 40, 128, 9) and O.INPUT_GRAD_CUPS == (4, 9, 128, 1024)


# ---- sensitivity: the pins reject a subtly wrong kernel ------------------------------------------------------------------
def rejected(name, got, ref, ref_abs, n):
    with pytest.raises(AssertionError):
        K.compare(name, got, ref, ref_abs, n, False, ratios={})
    return True


def test_compare_accepts_the_oracle_and_fp32_rounding_of_it():
    i = O.fwd_inputs(K.Randn(1), 33, 72, 40)
    z = O.linear(i.X, i.W, i.b)
    K.compare("z", z.Z, z.Z, z.Z_abs, z.n, False, ratios={})
    K.compare("z", z.Z.astype(np.float32), z.Z, z.Z_abs, z.n, False, ratios={})


def test_mutations_are_rejected():
    R, Cin, C = 33, 72, 40
    draw = K.Randn(2)
    i = O.fwd_inputs(draw, R, Cin, C)
    Z = O.linear(i.X, i.W, i.b).Z
    s = O.batch_stats(Z)
    want = O.invstd_of(s.var)
    # the last row left out of a batch statistic
    cut = O.batch_stats(Z[:-1])
    assert rejected("mean", cut.mean, s.mean, s.mean_abs, R)
    assert rejected("invstd", O.invstd_of(cut.var), want, want, R)
    # biased instead of unbiased running variance
    u = O.running_update(i.rm, i.rv, s.mean, s.var, R)
    assert rejected("running_var", O.running_update(i.rm, i.rv, s.mean, s.var, 1).rv, u.rv, u.rv_abs, 0)
    # the mask as >= 0: the exact leg's planted zeros (equality) and the forward -> backward case's element-wise check
    c = O.BWD_CASES[0]
    b = O.bwd_inputs(O.Dyadic(2000), c)
    for training in (True, False):
        r = O.bn_bwd(b.g, b.Z, b.mean, b.invstd, b.gamma, b.beta, True, training)
        pre = O.bn_act(b.Z, b.mean, b.invstd, b.gamma, b.beta, True).pre
        m = O.bn_bwd(b.g, b.Z, b.mean, b.invstd, b.gamma, b.beta, True, training, mask=pre >= 0)
        for name in ("dZ", "dbeta"):
            with pytest.raises(AssertionError):
                K.compare(name, getattr(m, name), getattr(r, name), None, None, True)
    # the second input_grad source dropped
    srcs = O.input_grad_sources(draw, 2)
    r = O.input_grad(srcs)
    assert rejected("dX", O.input_grad(srcs[:1]).dX, r.dX, r.dX_abs, r.n)
    # one element moved by twice its bound, of every stage of a rounded backward case
    c = O.BWD_CASES[2]
    b = O.bwd_inputs(draw, c)
    r = O.backward(b.g, b.X, b.Z, b.mean, b.invstd, b.gamma, b.beta, c.relu, c.training, b.g_abs, b.g_n)
    for name, n in (("dZ", r.dZ_n), ("dW", r.dW_n), ("db", r.dW_n), ("dgamma", r.dgamma_n), ("dbeta", r.dbeta_n)):
        ref, ra = getattr(r, name), getattr(r, name + "_abs")
        got = ref.copy()
        at = tuple(np.array(ref.shape) - 1)
        got[at] += 2 * (n + 8) * K.E24 * ra[at]
        assert ra[at] > 0 and rejected(name, got, ref, ra, n)
        K.compare(name, ref, ref, ra, n, False, ratios={})
