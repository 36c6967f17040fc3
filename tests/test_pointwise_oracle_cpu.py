"""tests/pointwise_oracle.py against the operators it restates, in torch fp64 under torch.autograd:
  * a two-layer per-point stack Conv1d -> BatchNorm1d (train) -> ReLU twice, once ending in the activation and once in
    amax(dim=2) (and in AdaptiveMaxPool1d(1), which says where the gradient of a tie goes), composed here from the
    oracle's pieces with gemm_oracle.pw_fwd / bn_consts / bn_bwd_coef in between -- the
    BatchNorm constants come from the oracle's OWN partials, so it cannot merely mirror the kernels; the gmax end goes
    through the packed source (gmax_bwd_pk -> expand_pk -> gemm_oracle.wgrad / pw_dgrad), layer 0 through thin_bwd;
  * a per-cloud bias, whose gradient is cloud_sum_dy;
  * the materialised (B, 1 + 3 + f, M, N) fusion tensor of P2B through a 1x1 convolution, against xcorr_expand /
    xcorr_reduce;
plus hand-written known answers of gmax_fwd and the exactness condition of every exact-leg input set of
tests/test_pointwise_kernels_gpu.py and tests/test_xcorr_kernels_gpu.py, so a grid that is too coarse is found here.  No GPU."""
import numpy as np
import pytest
import torch

import gemm_oracle as G
import pointwise_oracle as O

EPS = 1e-5


def flat(t):
    """(B, C, N) -> (C, B*N), column = b*N + n"""
    a = t.detach().numpy()
    return a.transpose(1, 0, 2).reshape(a.shape[1], -1)


def rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def w2(conv):
    return conv.weight.detach().numpy().reshape(conv.weight.shape[0], conv.weight.shape[1])


def dominated(*pairs):
    for v, a in pairs:
        assert (np.abs(v) <= a * (1 + 1e-12)).all()


@pytest.mark.parametrize("end", ["act", "amax", "maxpool"])
@pytest.mark.parametrize("B,Cin,C1,N", [(2, 3, 24, 12), (3, 13, 40, 20)])
def test_two_layer_chain_vs_autograd(end, B, Cin, C1, N):
    """end = "amax": act.amax(dim=2); "maxpool": AdaptiveMaxPool1d(1), the operator of the reference (models/backbone/
    pointnet.py).  The two differ only where the maximum is met more than once: amax spreads the gradient evenly over the
    ties, the max-pool gives it to the FIRST one, which is what o3d_gmax_fwd's argq records -- so the dead channel
    (scale == 0: every column ties) is part of the "act" and "maxpool" chains only."""
    torch.manual_seed(B * 100 + Cin + len(end))
    conv0 = torch.nn.Conv1d(Cin, 64, 1, bias=False).double()
    conv1 = torch.nn.Conv1d(64, C1, 1, bias=False).double()
    bn0 = torch.nn.BatchNorm1d(64, eps=EPS).double().train()
    bn1 = torch.nn.BatchNorm1d(C1, eps=EPS).double().train()
    with torch.no_grad():
        for bn in (bn0, bn1):
            bn.weight.copy_(torch.randn_like(bn.weight))      # negative gammas too: scale < 0
            bn.bias.copy_(torch.randn_like(bn.bias))
        if end != "amax":
            bn1.weight[1] = 0.0                               # a dead channel: scale == 0
            bn1.bias[1] = 0.5
    x = torch.randn(B, Cin, N, dtype=torch.float64, requires_grad=True)
    act = torch.relu(bn1(conv1(torch.relu(bn0(conv0(x))))))
    out = act if end == "act" else act.amax(dim=2) if end == "amax" else torch.nn.functional.adaptive_max_pool1d(act, 1)[:, :, 0]
    gout = torch.randn_like(out)
    out.backward(gout)

    X, W0, W1, P, tile = flat(x), w2(conv0), w2(conv1), B * N, N // 2
    g0, b0, g1, b1 = (p.detach().numpy() for p in (bn0.weight, bn0.bias, bn1.weight, bn1.bias))
    # forward
    l0 = G.pw_fwd(X, W0, tile=tile)
    mean0, invstd0, scale0, shift0 = G.bn_consts(l0.part, P, g0, b0, EPS)
    l1 = G.pw_fwd(l0.Y, W1, scale0, shift0, tile=tile)
    mean1, invstd1, scale1, shift1 = G.bn_consts(l1.part, P, g1, b1, EPS)
    assert (scale1[1] == 0.0 or end == "amax") and (scale1 < 0).any()
    if end == "act":
        f = O.bn_relu_apply(l1.Y, scale1, shift1)
        assert rel(f.out, flat(out)) <= 1e-12
        a = O.act_bwd_partials(flat(gout), l1.Y, scale1, shift1, mean1, tile=tile)
        assert a.part.shape == (P // tile, 2, C1) and np.array_equal(a.mask, f.out > 0)
        dN1, part1 = a.dN, a.part
        dominated((f.out, f.out_abs), (a.part[:, 0], a.part_abs[:, 0]), (a.part[:, 1], a.part_abs[:, 1]))
    else:
        f = O.gmax_fwd(l1.Y, scale1, shift1, B, N)
        assert rel(f.out, out.detach().numpy()) <= 1e-12
        assert (f.argq // N == np.arange(B)[:, None]).all() and np.array_equal(f.yarg, l1.Y.T[f.argq, np.arange(C1)[None, :]])
        if end == "maxpool":
            assert (f.argq[:, 1] == N * np.arange(B)).all() and (f.out[:, 1] == 0.5).all()      # every column ties: the first
        k = O.gmax_bwd_pk(gout.numpy(), f.out, f.argq, f.yarg, mean1, B, N)
        assert k.part.shape == (1, 2, C1) and k.pk_g.shape == (C1, B) and k.part_n == B
        dN1, part1 = O.expand_pk(k.pk_g, k.pk_slot, N, P), k.part
        assert np.array_equal(np.sort(dN1[dN1 != 0]), np.sort(k.pk_g[k.pk_g != 0]))
        dominated((f.out, f.out_abs), (k.part[0, 0], k.part_abs[0, 0]), (k.part[0, 1], k.part_abs[0, 1]))
    # backward of layer 1 (the GEMM oracles on the dense or expanded gradient), then of the thin layer 0
    A = G.bn_bwd_coef(part1, P, g1, mean1, invstd1)
    wg1 = G.wgrad(dN1, l0.Y, l1.Y, *A, in_scale=scale0, in_shift=shift0)
    assert rel(wg1.dW, conv1.weight.grad.numpy()[:, :, 0]) <= 1e-12
    d1 = G.pw_dgrad(dN1, W1.T, l1.Y, *A, Yprev=l0.Y, scale_p=scale0, shift_p=shift0, mean_p=mean0, tile=tile)
    A0 = G.bn_bwd_coef(d1.part, P, g0, mean0, invstd0)
    t = O.thin_bwd(d1.G, l0.Y, *A0, X, W0)
    assert t.dW_n == P and t.dX_n == 64 and t.dW.shape == (64, Cin) and t.dX.shape == (Cin, P)
    assert rel(t.dW, conv0.weight.grad.numpy()[:, :, 0]) <= 1e-12
    assert rel(t.dX, flat(x.grad)) <= 1e-12
    dominated((t.dW, t.dW_abs), (t.dX, t.dX_abs))
    # the BatchNorm parameters' own gradients fall out of the same partials
    for part, bn, invstd in ((part1, bn1, invstd1), (d1.part, bn0, invstd0)):
        s = part.sum(0)
        assert rel(s[0], bn.bias.grad.numpy()) <= 1e-12 and rel(s[1] * invstd, bn.weight.grad.numpy()) <= 1e-12


def test_cloud_bias_gradient_vs_autograd():
    torch.manual_seed(5)
    B, Cin, C, N = 3, 16, 24, 8
    conv = torch.nn.Conv1d(Cin, C, 1, bias=False).double()
    bn = torch.nn.BatchNorm1d(C, eps=EPS).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C).double())
        bn.bias.copy_(torch.randn(C).double())
    x = torch.randn(B, Cin, N, dtype=torch.float64)
    cb = torch.randn(B, C, dtype=torch.float64, requires_grad=True)
    gout = torch.randn(B, C, N, dtype=torch.float64)
    torch.relu(bn(conv(x) + cb[:, :, None])).backward(gout)
    P = B * N
    l = G.pw_fwd_cloud(flat(x), w2(conv), cb.detach().numpy().T, N, tile=N)
    mean, invstd, scale, shift = G.bn_consts(l.part, P, bn.weight.detach().numpy(), bn.bias.detach().numpy(), EPS)
    a = O.act_bwd_partials(flat(gout), l.Y, scale, shift, mean, tile=N)
    A = G.bn_bwd_coef(a.part, P, bn.weight.detach().numpy(), mean, invstd)
    r = O.cloud_sum_dy(a.dN, l.Y, *A, B, N)
    assert r.out.shape == (C, B) and r.n == N
    assert rel(r.out.T, cb.grad.numpy()) <= 1e-12
    dominated((r.out, r.out_abs))


@pytest.mark.parametrize("B,M,N,C0,f", [(2, 4, 6, 16, 5), (1, 8, 3, 32, 2)])
def test_xcorr_split_vs_materialised_tensor(B, M, N, C0, f):
    """the reference materialises x[b, :, i, j] = [sim(t_i, s_j) ; xyz_i ; feat_i] and runs a 1x1 convolution over it"""
    torch.manual_seed(B + M)
    conv = torch.nn.Conv2d(1 + 3 + f, C0, 1, bias=False).double()
    tpl = torch.randn(B, 3 + f, M, dtype=torch.float64, requires_grad=True)       # [xyz ; feat] of the template points
    simt = torch.randn(B, M, N, dtype=torch.float64, requires_grad=True)          # sim[b, i, j]
    x = torch.cat([simt[:, None], tpl[:, :, :, None].expand(B, 3 + f, M, N)], dim=1)
    Yt = conv(x)                                                                   # (B, C0, M, N)
    to_cols = lambda t: t.detach().numpy().transpose(1, 0, 3, 2).reshape(t.shape[1], -1)    # noqa: E731  q = (b*N + j)*M + i
    W0 = w2(conv)
    F = flat(tpl)                                                                  # (3 + f, B*M), column b*M + i
    sim = simt.detach().numpy().transpose(0, 2, 1).reshape(-1)                     # (B, N, M)
    Z = W0[:, 1:] @ F
    P = B * M * N
    _, zc = O.xcorr_cols(B, M, N)                  # (xcorr_expand itself, whose statistics tiles are 256 columns: next test)
    Y0 = Z[:, zc] + W0[:, :1] * sim[None, :]
    assert rel(Y0, to_cols(Yt)) <= 1e-12
    # backward with a folded BatchNorm: dY0 = A1*dN + A2*Y0 + A3
    rng = np.random.RandomState(3)
    dN, A1, A2, A3 = rng.randn(C0, P), rng.randn(C0), rng.randn(C0), rng.randn(C0)
    dY0 = A1[:, None] * dN + A2[:, None] * Y0 + A3[:, None]
    Yt.backward(torch.from_numpy(dY0.reshape(C0, B, N, M).transpose(1, 0, 3, 2).copy()))
    r = O.xcorr_reduce(dN, Y0, A1, A2, A3, sim, W0[:, 0], B, M, N)
    assert r.S.shape == (C0, B * M) and r.dsim_part.shape == (C0 // 16, P) and r.dw_part.shape == (B, C0)
    assert (r.S_n, r.dsim_n, r.dw_n) == (N, 16, M * N)
    gW = conv.weight.grad.numpy()[:, :, 0, 0]
    assert rel(r.dw_part.sum(0), gW[:, 0]) <= 1e-12
    assert rel(r.S @ F.T, gW[:, 1:]) <= 1e-12
    assert rel(W0[:, 1:].T @ r.S, flat(tpl.grad)) <= 1e-12
    assert rel(r.dsim_part.sum(0), simt.grad.numpy().transpose(0, 2, 1).reshape(-1)) <= 1e-12
    dominated((r.S, r.S_abs), (r.dsim_part, r.dsim_abs), (r.dw_part, r.dw_abs))


def test_xcorr_expand_vs_materialised_tensor_with_partials():
    """xcorr_expand itself at a shape with whole 256-column statistics tiles"""
    torch.manual_seed(9)
    B, M, N, C0, f = 2, 4, 64, 16, 3
    conv = torch.nn.Conv2d(1 + 3 + f, C0, 1, bias=False).double()
    tpl = torch.randn(B, 3 + f, M, dtype=torch.float64)
    simt = torch.randn(B, M, N, dtype=torch.float64)
    Yt = conv(torch.cat([simt[:, None], tpl[:, :, :, None].expand(B, 3 + f, M, N)], dim=1))
    W0 = w2(conv)
    Z = W0[:, 1:] @ flat(tpl)
    sim = simt.numpy().transpose(0, 2, 1).reshape(-1)
    stat_c = np.linspace(-1, 1, C0)
    e = O.xcorr_expand(Z, sim, W0[:, 0], B, M, N, stat_c)
    cols = Yt.detach().numpy().transpose(1, 0, 3, 2).reshape(C0, -1)
    assert rel(e.Y0, cols) <= 1e-12 and e.n == 2 and e.part_n == 256
    t = cols.reshape(C0, -1, 256)
    assert e.part.shape == (B * M * N // 256, 2, C0)
    assert rel(e.part[:, 0], t.sum(2).T) <= 1e-12 and rel(e.part[:, 1], ((t - stat_c[:, None, None]) ** 2).sum(2).T) <= 1e-12
    # Z with padding columns (ldz > B*M): they are never read
    Zp = np.concatenate([Z, np.full((C0, 3), 1e30)], axis=1)
    assert np.array_equal(O.xcorr_expand(Zp, sim, W0[:, 0], B, M, N).Y0, e.Y0)
    dominated((e.Y0, e.Y0_abs), (e.part[:, 0], e.part_abs[:, 0]), (e.part[:, 1], e.part_abs[:, 1]))


# ---- known answers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", O.gmax_known_answers(), ids=lambda c: c[0])
def test_gmax_fwd_known_answers(case):
    _, Y, scale, shift, B, N, out, argq, yarg = case
    r = O.gmax_fwd(Y, scale, shift, B, N)
    assert np.array_equal(r.out, out) and np.array_equal(r.argq, argq) and np.array_equal(r.yarg, yarg)
    assert r.n == 2


def test_known_answer_packed_source():
    B, N = 2, 8
    out = np.array([[1.5, 0.0, 2.0], [0.0, 0.25, 1.0]])                 # (B, C = 3)
    dOut = np.array([[2.0, 5.0, -1.0], [7.0, 4.0, 3.0]])
    argq = np.array([[3, 0, 7], [8 + 2, 8 + 5, 8 + 0]])
    yarg = np.array([[1.0, 9.0, -2.0], [9.0, 2.0, 0.5]])
    mean = np.array([0.5, 1.0, -1.0])
    r = O.gmax_bwd_pk(dOut, out, argq, yarg, mean, B, N)
    assert np.array_equal(r.pk_g, [[2.0, 0.0], [0.0, 4.0], [-1.0, 3.0]])            # (C, B): masked where out == 0
    assert np.array_equal(r.pk_slot, [[3, 2], [0, 5], [7, 0]])
    assert np.array_equal(r.part[0, 0], [2.0, 4.0, 2.0])
    assert np.array_equal(r.part[0, 1], [2.0 * 0.5, 4.0 * 1.0, -1.0 * -1.0 + 3.0 * 1.5])
    dN = O.expand_pk(r.pk_g, r.pk_slot, N, B * N)
    want = np.zeros((3, 16))
    want[0, 3], want[1, 8 + 5], want[2, 7], want[2, 8] = 2.0, 4.0, -1.0, 3.0
    assert np.array_equal(dN, want)
    # one cloud of 5 balls in 2 shares of 3 and 2, and in 4 shares of 2, 2, 1 and 0
    g = np.array([[1.0, 2.0, 4.0, 8.0, 16.0]])
    ones = np.ones((1, 5))
    arg = np.array([[0, 1, 2, 3, 0]])
    s = O.pool_bwd_partials_split(g, ones, arg, 2 * ones, [0.5], 5, 2)
    assert np.array_equal(s.part[:, 0, 0], [7.0, 24.0]) and np.array_equal(s.part[:, 1, 0], [10.5, 36.0]) and s.part_n == 3
    s = O.pool_bwd_partials_split(g, np.array([[1.0, 0.0, 1.0, 1.0, 1.0]]), arg, 2 * ones, [0.5], 5, 4)
    assert np.array_equal(s.part[:, 0, 0], [1.0, 12.0, 16.0, 0.0]) and s.part_n == 2
    assert np.array_equal(s.pk_g, [[1.0, 0.0, 4.0, 8.0, 16.0]]) and np.array_equal(s.pk_slot, arg)


def test_known_answer_pointwise():
    Y = np.array([[1.0, -1.0, 0.5, 2.0] * 32])                           # (1, 128)
    g = np.arange(128, dtype=np.float64)[None]
    a = O.act_bwd_partials(g, Y, [2.0], [-1.0], [0.5])                    # 2y - 1 > 0: y = 1 and 2; y = 0.5 gives exactly 0
    live = np.array([True, False, False, True] * 32)
    assert np.array_equal(a.mask[0], live) and np.array_equal(a.dN[0], np.where(live, g[0], 0))
    assert a.part[0, 0, 0] == g[0][live].sum() and a.part[0, 1, 0] == (g[0] * (Y[0] - 0.5))[live].sum()
    r = O.bn_relu_apply(Y, [2.0], [-1.0])
    assert np.array_equal(r.out[0, :4], [1.0, 0.0, 0.0, 3.0]) and np.array_equal(r.out_abs[0, :4], [3.0, 0.0, 0.0, 5.0])
    c = O.cloud_sum_dy(np.ones((1, 8)), np.arange(8.0)[None], [2.0], [1.0], [-0.5], 2, 4)
    assert np.array_equal(c.out, [[4 * 1.5 + 6, 4 * 1.5 + 22]]) and c.n == 4


# ---- the exact legs of the GPU files -------------------------------------------------------------------------------------
def test_exact_inputs_stay_below_the_exactness_limit():
    seen = O.exact_preconditions()
    names = {n for n, _ in seen}
    assert set(O.SPACING) <= names and {"gemm.dW", "gemm.G", "gemm.gpart0", "gemm.gpart1"} <= names
    assert all(w < O.TWO24 for _, w in seen)


def test_exact_outputs_lie_on_their_grids():
    d = O.Dyadic(2)

    def on_grid(name, v):
        assert np.array_equal(v / O.SPACING[name], np.round(v / O.SPACING[name])), name

    i = O.chain_end_inputs(d, 9, 2 * 1028, dead=3)
    on_grid("pw.apply", O.bn_relu_apply(i.Y, i.scale, i.shift).out)
    f = O.gmax_fwd(i.Y, i.scale, i.shift, 2, 1028)
    on_grid("pw.gmax", f.out)
    assert (f.argq[:, 3] == [0, 1028]).all()                              # the dead channel
    # ties are plentiful on these grids: the maximum is met more than once in most (cloud, channel) pairs
    n = (i.Y * i.scale[:, None] + i.shift[:, None]).reshape(9, 2, 1028)
    assert ((n == n.max(2, keepdims=True)).sum(2) > 1).mean() > 0.9
    r = O.gmax_bwd_pk(i.g[:, :2].T, f.out, f.argq, f.yarg, i.mean, 2, 1028)
    on_grid("pw.pk0", r.part[:, 0]), on_grid("pw.pk1", r.part[:, 1])
    i = O.chain_end_inputs(d, 9, 384)
    a = O.act_bwd_partials(i.g, i.Y, i.scale, i.shift, i.mean)
    on_grid("pw.act0", a.part[:, 0]), on_grid("pw.act1", a.part[:, 1])
    assert ((i.Y * i.scale[:, None] + i.shift[:, None]) == 0).any()       # pre-activations exactly at the mask boundary
    on_grid("pw.cloud", O.cloud_sum_dy(i.g, i.Y, i.A1, i.A2, i.A3, 3, 128).out)
    i = O.thin_inputs(d, 192)
    t = O.thin_bwd(i.dN, i.Y, i.A1, i.A2, i.A3, i.X[:15], i.W[:, :15])
    on_grid("pw.thin_dW", t.dW), on_grid("pw.thin_dX", t.dX)
    B, M, N, C0 = O.XCORR_SHAPES[1]
    i = O.xcorr_inputs(d, B, M, N, C0, 5)
    e = O.xcorr_expand(i.Z, i.sim, i.W0[:, 0], B, M, N, i.stat_c)
    on_grid("xc.Y0", e.Y0), on_grid("xc.part0", e.part[:, 0]), on_grid("xc.part1", e.part[:, 1])
    r = O.xcorr_reduce(i.dN, i.Y0, i.A1, i.A2, i.A3, i.sim, i.W0[:, 0], B, M, N)
    on_grid("xc.S", r.S), on_grid("xc.dsim", r.dsim_part), on_grid("xc.dw", r.dw_part)
