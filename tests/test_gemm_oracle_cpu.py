"""tests/gemm_oracle.py against the operators it restates: a two-layer stack Conv1d -> BatchNorm1d (train) -> ReLU -> Conv1d
(+ bias, + residual) in torch fp64 under torch.autograd, composed here from the oracle's pieces with the BatchNorm constants
derived in fp64 from the oracle's OWN statistics partials (forward: mean / invstd / scale / shift; backward: A1, A2, A3 from
the data gradient's partials) -- so the oracle cannot merely mirror the kernels -- plus known-answer cases small enough to
check by hand.  No GPU."""
import numpy as np
import pytest
import torch

import gemm_oracle as G

EPS = 1e-5


def flat(t):
    """(B, C, N) -> (C, B*N), column = b*N + n"""
    a = t.detach().numpy()
    return a.transpose(1, 0, 2).reshape(a.shape[1], -1)


def rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("B,C,N", [(2, 32, 24), (3, 64, 40)])
def test_two_layer_stack_vs_autograd(B, C, N):
    torch.manual_seed(B * 100 + C)
    C1 = C + 16
    conv1 = torch.nn.Conv1d(C, C1, 1, bias=False).double()
    bn = torch.nn.BatchNorm1d(C1, eps=EPS).double().train()
    conv2 = torch.nn.Conv1d(C1, C, 1, bias=True).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C1).double())
        bn.bias.copy_(torch.randn(C1).double())
    x = torch.randn(B, C, N, dtype=torch.float64, requires_grad=True)
    resid = torch.randn(B, C, N, dtype=torch.float64)
    gout = torch.randn(B, C, N, dtype=torch.float64)
    out = conv2(torch.relu(bn(conv1(x)))) + resid
    out.backward(gout)

    X, R, dOut = flat(x), flat(resid), flat(gout)
    W1, W2, b2 = conv1.weight.detach().numpy()[:, :, 0], conv2.weight.detach().numpy()[:, :, 0], conv2.bias.detach().numpy()
    gamma, beta = bn.weight.detach().numpy(), bn.bias.detach().numpy()
    P, tile = B * N, N // 2                                   # several partial rows, none spanning two clouds' worth
    stat_c = np.linspace(-0.5, 0.5, C1)                       # any shift of the second moment gives the same variance
    # forward
    l1 = G.pw_fwd(X, W1, tile=tile, stat_c=stat_c)
    assert l1.part.shape == (P // tile, 2, C1) and l1.n == C
    mean, invstd, scale, shift = G.bn_consts(l1.part, P, gamma, beta, EPS, stat_c)
    l2 = G.pw_fwd(l1.Y, W2, scale, shift, bias=b2, resid=R)
    assert l2.n == C1 + 2
    assert rel(l2.Y, flat(out)) <= 1e-12
    # backward
    wg2 = G.wgrad(dOut, l1.Y, in_scale=scale, in_shift=shift)
    assert rel(wg2.dW, conv2.weight.grad.numpy()[:, :, 0]) <= 1e-12
    assert rel(G.row_sum(dOut).dW, conv2.bias.grad.numpy()) <= 1e-12
    d2 = G.pw_dgrad(dOut, W2.T, Yprev=l1.Y, scale_p=scale, shift_p=shift, mean_p=mean, tile=tile)
    assert np.array_equal(d2.mask, l1.Y * scale[:, None] + shift[:, None] > 0)
    A1, A2, A3 = G.bn_bwd_coef(d2.part, P, gamma, mean, invstd)
    d1 = G.pw_dgrad(d2.G, W1.T, Y=l1.Y, A1=A1, A2=A2, A3=A3)
    assert rel(d1.G, flat(x.grad)) <= 1e-12
    wg1 = G.wgrad(d2.G, X, Y=l1.Y, A1=A1, A2=A2, A3=A3)
    assert rel(wg1.dW, conv1.weight.grad.numpy()[:, :, 0]) <= 1e-12
    # the BatchNorm parameters' own gradients fall out of the same partials
    s = d2.part.sum(0)
    assert rel(s[0], bn.bias.grad.numpy()) <= 1e-12 and rel(s[1] * invstd, bn.weight.grad.numpy()) <= 1e-12
    # the *_abs sums dominate the values they bound
    for v, a in ((l1.Y, l1.Y_abs), (l2.Y, l2.Y_abs), (d2.G, d2.G_abs), (d1.G, d1.G_abs), (wg1.dW, wg1.dW_abs),
                 (l1.part[:, 0], l1.part_abs[:, 0]), (d2.part[:, 1], d2.part_abs[:, 1])):
        assert (np.abs(v) <= a * (1 + 1e-12)).all()


def test_plain_dgrad_with_residual_vs_autograd():
    torch.manual_seed(3)
    conv = torch.nn.Conv1d(16, 64, 1, bias=False).double()
    x = torch.randn(2, 16, 8, dtype=torch.float64, requires_grad=True)
    g = torch.randn(2, 64, 8, dtype=torch.float64)
    (conv(x) * g).sum().backward()
    r = np.arange(16 * 16, dtype=np.float64).reshape(16, 16)
    d = G.pw_dgrad(flat(g), conv.weight.detach().numpy()[:, :, 0].T, resid=r)
    assert d.n == 65 and rel(d.G - r, flat(x.grad)) <= 1e-12


# ---- known answers: one tile, K = 16, a single non-zero weight ---------------------------------------------------------------
def _one_weight(M=64, K=16, m0=5, k0=3, w=2.0):
    W = np.zeros((M, K))
    W[m0, k0] = w
    return W


def test_known_answer_forward():
    K, M, P = 16, 64, 64
    X = np.tile(np.arange(P, dtype=np.float64) - 31.0, (K, 1)) * (1 + np.arange(K))[:, None]      # row k: (k+1) * (p - 31)
    W = _one_weight()
    r = G.pw_fwd(X, W, tile=64, stat_c=np.full(M, 1.0))
    want = 2.0 * 4 * (np.arange(P) - 31.0)                    # row 5 = 2 * row 3 of X
    assert np.array_equal(r.Y[5], want) and not r.Y[np.arange(M) != 5].any()
    assert np.array_equal(r.Y_abs[5], np.abs(want)) and r.n == 16
    assert r.part.shape == (1, 2, M)
    assert r.part[0, 0, 5] == want.sum() == 8 * 32 and r.part[0, 1, 5] == ((want - 1) ** 2).sum()
    assert r.part[0, 0, 6] == 0 and r.part[0, 1, 6] == P      # a zero row: sum (0 - 1)^2
    # transformed input: relu(x * s + t) of row 3 with s = -1, t = 2: 2 - 4*(p - 31) where positive (p <= 31)
    sc, sh = np.ones(K), np.zeros(K)
    sc[3], sh[3] = -1.0, 2.0
    r = G.pw_fwd(X, W, sc, sh, bias=np.full(M, 0.5), resid=np.full((M, P), 0.25))
    f = np.maximum(2 - 4 * (np.arange(P) - 31.0), 0)
    assert np.array_equal(r.Y[5], 2 * f + 0.75) and (r.Y[4] == 0.75).all() and r.n == 18
    assert r.Y_abs[5, 0] == 2 * (4 * 31 + 2) + 0.75 and r.Y_abs[5, 40] == 0.75


def test_known_answer_cloud_bias():
    K, M, N, B = 16, 64, 128, 3
    X = np.ones((K, B * N))
    cb = np.arange(M * B, dtype=np.float64).reshape(M, B)
    r = G.pw_fwd_cloud(X, _one_weight(), cb, N)
    for b in range(B):
        assert (r.Y[5, b * N:(b + 1) * N] == 2 + cb[5, b]).all() and (r.Y[7, b * N:(b + 1) * N] == cb[7, b]).all()
    assert r.part.shape == (B, 2, M) and r.part[1, 0, 7] == N * cb[7, 1] and r.n == 17


def test_known_answer_dgrad():
    K, M, P = 16, 64, 64
    Wt = _one_weight()                                       # G[5] = 2 * dY[3]
    dN = np.ones((K, P))
    Y = np.tile(np.arange(P, dtype=np.float64), (K, 1))
    A1, A2, A3 = np.full(K, 3.0), np.full(K, -1.0), np.full(K, 0.5)
    want = 2 * (3.0 - np.arange(P) + 0.5)
    r = G.pw_dgrad(dN, Wt, Y, A1, A2, A3)
    assert np.array_equal(r.G[5], want) and not r.G[4].any() and r.n == 16
    assert np.array_equal(r.G_abs[5], 2 * (3.0 + np.arange(P) + 0.5))
    Yprev = np.tile(np.arange(P, dtype=np.float64), (M, 1))
    r = G.pw_dgrad(dN, Wt, Y, A1, A2, A3, Yprev=Yprev, scale_p=np.ones(M), shift_p=np.full(M, -10.0), mean_p=np.full(M, 1.0),
                   tile=64)
    live = np.arange(P) > 10                                  # strictly positive: column 10 is masked
    assert np.array_equal(r.G[5], np.where(live, want, 0)) and np.array_equal(r.mask[5], live)
    assert r.part[0, 0, 5] == want[live].sum() and r.part[0, 1, 5] == (want[live] * (np.arange(P)[live] - 1.0)).sum()
    assert np.array_equal(G.pw_dgrad(dN, Wt).G[5], np.full(P, 2.0))


def test_known_answer_wgrad():
    P = 64
    dN = np.zeros((64, P))
    dN[5] = 1.0
    X = np.zeros((64, P))
    X[3] = np.arange(P) - 31.0
    r = G.wgrad(dN, X)
    assert r.dW[5, 3] == 32 and np.count_nonzero(r.dW) == 1 and r.n == P and r.dW_abs[5, 3] == np.abs(X[3]).sum()
    sc, sh = np.ones(64), np.zeros(64)
    r = G.wgrad(dN, X, Y=dN, A1=np.full(64, 2.0), A2=np.full(64, 1.0), A3=np.full(64, 0.5), in_scale=sc, in_shift=sh)
    assert r.dW[5, 3] == 3.5 * np.arange(1, 33).sum() and r.dW[6, 3] == 0.5 * np.arange(1, 33).sum()
    s = G.row_sum(X)
    assert s.dW[3] == 32 and s.dW_abs[3] == np.abs(X[3]).sum() and s.n == P


def test_exact_inputs_stay_below_the_exactness_limit():
    """the grids of gemm_oracle.Inputs: the tightest output (the second-moment partials) at the widest K and tile the GPU
    tests use"""
    for K, tile, P in ((272, 64, 192), (16, 128, 256)):
        i = G.Inputs(G.Dyadic(1), 64, K, P)
        assert ((i.W != 0).sum(1) == 16).all() and (i.W != 0).any(0).all()
        r = G.pw_fwd(i.X, i.W, i.in_scale, i.in_shift, tile=tile, stat_c=i.stat_c)
        assert G.assert_exact("gemm.part1", r.part_abs[:, 1]) < G.TWO24
        for v, s in ((r.Y, "gemm.Y"), (r.part[:, 1], "gemm.part1")):
            assert np.array_equal(v / G.SPACING[s], np.round(v / G.SPACING[s]))
