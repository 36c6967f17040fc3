"""tests/sa_eval_oracle.py without a GPU:
  * the oracle against F.conv2d / F.batch_norm(training=False) / amax on the grouped tensor in fp64, to 1e-12, with the
    constants of bn_eval_consts (folded conv_bias, nrep copies);
  * the exactness condition of every exact case of tests/test_sa_eval_kernels_gpu.py and the conditions on every case's
    inputs: each of the ns slot positions is the unique arg-max of some (ball, channel), at least a quarter of the pooled
    outputs are > 0, at least one is exactly 0 (all slots clamped), every padded ball repeats an index as ball_query pads;
  * sensitivity: plausible mistakes applied to the oracle's own output are rejected by the GPU file's `compare`.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sa_eval_oracle as O
import test_sa_eval_kernels_gpu as K

TOL = 1e-12


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.abs(a - b).max() <= TOL * (1 + np.abs(b).max())


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


@pytest.mark.parametrize("with_xyz,with_bias", [(True, False), (True, True), (False, False)])
def test_oracle_matches_conv_bn_relu_amax(with_xyz, with_bias):
    """grouped tensor (B, 3 + C, np, ns) = [xyz[idx] - centre ; feats[idx]] -> 3 x (conv2d 1x1, batch_norm eval, relu) -> amax;
    the oracle takes Z = W0 . [xyz ; feats] per point, as the fused path does"""
    rng = np.random.RandomState(3)
    B, N, npoint, ns, Cf, C = 2, 20, 6, 4, 5, (8, 32, 32)
    nx = 3 if with_xyz else 0
    xyz, feats = rng.randn(B, N, 3), rng.randn(B, Cf, N)
    idx = O.ball_idx(rng, B, npoint, ns, N)
    centers = rng.randn(B, npoint, 3)
    Ws = [rng.randn(C[0], nx + Cf), rng.randn(C[1], C[0]), rng.randn(C[2], C[1])]
    bns = [dict(rm=rng.randn(c), rv=0.5 + rng.rand(c), gamma=rng.randn(c), beta=rng.randn(c),
                bias=rng.randn(c) if with_bias else None) for c in C]
    bi = np.arange(B)[:, None, None]
    g = feats.transpose(0, 2, 1)[bi, idx].transpose(0, 3, 1, 2)                       # (B, Cf, np, ns)
    if with_xyz:
        gx = (xyz[bi, idx] - centers[:, :, None, :]).transpose(0, 3, 1, 2)
        g = np.concatenate([gx, g], 1)
    x = t64(g)
    for W, bn in zip(Ws, bns):
        x = F.conv2d(x, t64(W)[:, :, None, None], None if bn["bias"] is None else t64(bn["bias"]))
        x = F.relu(F.batch_norm(x, t64(bn["rm"]), t64(bn["rv"]), t64(bn["gamma"]), t64(bn["beta"]), False, 0.0, O.EPS))
    want = x.amax(3).numpy()                                                           # (B, C2, np)
    pts = np.concatenate([xyz.transpose(0, 2, 1), feats], 1) if with_xyz else feats    # (B, nx + Cf, N)
    Z = np.concatenate([Ws[0] @ pts[b] for b in range(B)], 1)                          # (C0, B*N)
    # a conv bias in front of a BatchNorm is folded into its mean
    vs = [O.bn_eval_consts(bn["rm"], bn["rv"], bn["gamma"], bn["beta"], bn["bias"], nrep=3) for bn in bns]
    assert all((v == v[:, :1]).all() and v.shape == (4, 3, c) for v, c in zip(vs, C))
    v = [u[:, 1] for u in vs]
    r = O.sa_eval(Z, idx, centers.reshape(-1, 3) if with_xyz else None, Ws[0], v[0], Ws[1], v[1], Ws[2], v[2], B, npoint, ns, N, 0)
    assert close(r.out, want)
    assert (r.bound > 0).all() and r.bound.max() < 1e-3 * (1 + np.abs(want).max())


def test_two_sets_share_one_z():
    c = O.CASES[6]
    assert c.second
    i = O.inputs(O.Dyadic(1), c, 1)
    a, b = i.sets
    assert b.pt_base == c.B * a.ld > 0 and b.ld > O.N_POINTS and i.ldz > b.pt_base + c.B * b.ld
    assert not np.array_equal(O.run(i, a).out, O.run(i, b).out)
    assert not i.used.all() and i.used.any()


def draws(k):
    return (O.Dyadic(4000 + k), K.Randn(83 + k))


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=[O.case_id(c) for c in O.CASES])
def test_input_conditions(k):
    c = O.CASES[k]
    for draw in draws(k):
        i = O.inputs(draw, c, k)
        for s in i.sets:
            r = O.run(i, s)
            m = O.input_conditions(i, s, r)
            assert m["unique_positions"] == c.ns, m
            assert m["positive"] >= 0.25 and m["zeros"] >= 1, m
            assert m["padded_have_duplicate"] and (m["padded_balls"] > 0 or c.ns == 1), m
            assert not r.out[:, 1].any(), "the clamped channel"


def test_exact_preconditions():
    seen = O.exact_preconditions()
    assert {n for n, _ in seen} == {"sa.A0", "sa.A1", "sa.A2"} and all(w < O.TWO24 for _, w in seen)
    for k, c in enumerate(O.CASES):          # and the results are fp32 numbers, element by element
        i = O.inputs(O.Dyadic(4000 + k), c, k)
        out = O.run(i, i.sets[0]).out
        assert np.array_equal(out.astype(np.float32).astype(np.float64), out)


def test_case_table_lists_every_promised_size():
    C = O.CASES
    assert {c.C0 for c in C if c.C1 == 32} >= {8, 16, 24, 32, 40, 64}
    assert {c.C1 for c in C} >= {32, 64, 160} and {c.C2 for c in C} == {32, 96, 160}
    assert any(c.C0 == 256 and c.C1 == 256 for c in C) and 4 * 32 * (256 + 4 + 256 + 4) > 48 * 1024
    assert {c.ns for c in C} == {1, 2, 4, 8, 16, 32}
    assert any((c.B, c.npoint, c.ns) == (2, 12, 4) for c in C)
    assert {c.ldw for c in C} == {0, 3, 19} and any(c.second for c in C) and any(c.ldz_pad for c in C)
    assert all((c.B * c.npoint * c.ns) % 32 == 0 and c.C0 % 8 == 0 and c.C1 % 32 == 0 and c.C2 % 32 == 0 for c in C)


# ---- sensitivity ------------------------------------------------------------------------------------------------------------
def rejected(got, ref, bound):
    with pytest.raises(AssertionError):
        K.compare("x", got, ref, bound, False, ratios={})
    return True


@pytest.mark.parametrize("k", (2, 4, 5))
def test_mutations_are_rejected(k):
    c = O.CASES[k]
    i = O.inputs(K.Randn(83 + k), c, k)
    s = i.sets[0]
    r = O.run(i, s)
    K.compare("x", r.out, r.out, r.bound, False, ratios={})
    K.compare("x", r.out.astype(np.float32), r.out, r.bound, False, ratios={})
    # the pool taken over ns / 2 slots
    half = r.A2.reshape(c.C2, c.B, c.npoint, c.ns)[..., :c.ns // 2].max(3).transpose(1, 0, 2)
    assert rejected(half, r.out, r.bound)
    # one element moved by twice its bound
    got = r.out.copy()
    at = np.unravel_index(np.argmax(r.out), r.out.shape)
    got[at] += 2 * r.bound[at]
    assert rejected(got, r.out, r.bound)
    # a stale weight group: the last 8 columns of W1 read as the 8 before them
    if c.C0 >= 16:
        W1 = i.W1.copy()
        W1[:, -8:] = W1[:, -16:-8]
        bad = O.sa_eval(i.Z, s.idx, s.centers, i.W0, i.v0, W1, i.v1, i.W2, i.v2, s.B, s.npoint, s.ns, s.ld, s.pt_base)
        assert rejected(bad.out, r.out, r.bound)
    # the last row tile left to no wave
    if c.C2 > 128:
        got = r.out.copy()
        got[:, 128:] = 0.0
        assert rejected(got, r.out, r.bound)


def test_bn_consts_mutations_are_rejected():
    rng = np.random.RandomState(0)
    C = 257
    rm, rv, gamma, beta, bias = rng.randn(C), 0.5 + rng.rand(C), rng.randn(C), rng.randn(C), rng.randn(C)
    v = O.bn_eval_consts(rm, rv, gamma, beta, bias)[:, 0]
    w = O.bn_eval_consts(rm, rv, gamma, beta, None)[:, 0]
    with pytest.raises(AssertionError):           # the conv bias not folded
        K.compare("mean", w[0], v[0], (2 + 8) * O.E24 * (np.abs(rm) + np.abs(bias)), False, ratios={})
    with pytest.raises(AssertionError):           # eps left out
        K.compare("invstd", 1 / np.sqrt(rv), v[1], (3 + 8) * O.E24 * v[1], False, ratios={})
