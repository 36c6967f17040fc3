"""tests/compact_oracle.py against the operator it stands for, on the CPU.

The compact layout keeps one column per DISTINCT neighbour of a ball and gives the first hit the weight of its copies
(csrc/compact.hip).  Here every compact quantity of the oracle is compared with the slot-faithful fp64 computation on the
(B, C, npoint, ns) grouped tensor -- QueryAndGroup + layer 0 (pointnet2_utils.py:299-339) and the max over nsample
(pointnet2_modules.py:69-73), restated with torch ops as tests/test_fused_gpu.py::shadow64 does -- on dyadic inputs, so that
the two summation orders agree exactly.  The file also holds the self-checks of the hand-built index families and of the
exactness condition (sum|terms| / spacing < 2^24) of every input set that tests/test_compact_kernels_gpu.py compares
bit for bit.
"""
import numpy as np
import pytest
import torch

import compact_oracle as O


def _small(two):
    rng = np.random.RandomState(5 + two)
    B, ns = 2, 8
    segs = [(O._idx_from_counts(rng, rng.randint(1, ns + 1, B * 6), B, 6, ns, 20, hub=3), 20, 24)]
    if two:
        segs.append((O._idx_from_counts(rng, rng.randint(1, ns + 1, B * 10), B, 10, ns, 30), 30, 32))
    return segs, B, ns


def _slotwise(idx, xyz, new_xyz, feats, W0):
    """(B, C0, npoint, ns) fp64 layer-0 output and the relative coordinates (B, 3, npoint, ns), slot by slot"""
    B, npoint, ns = idx.shape
    flat = torch.from_numpy(idx).long().reshape(B, 1, npoint * ns)
    x, n, f = (torch.from_numpy(t) for t in (xyz, new_xyz, feats))
    g = x.transpose(1, 2).gather(2, flat.expand(B, 3, -1)).reshape(B, 3, npoint, ns) - n.transpose(1, 2).unsqueeze(-1)
    gf = f.gather(2, flat.expand(B, f.shape[1], -1)).reshape(B, -1, npoint, ns)
    y = torch.einsum("ok,bkjs->bojs", torch.from_numpy(W0), torch.cat([g, gf], dim=1))
    return y.numpy(), g.numpy()


@pytest.mark.parametrize("two", [0, 1])
def test_compact_quantities_equal_the_slotwise_operator(two):
    segs, B, ns = _small(two)
    L = O.Layout([(idx, ld) for idx, _, ld in segs], start1=256 * two, ldp=256 * (1 + two))
    d = O.Dyadic(3)
    C0, Cf = 6, 2
    W0 = d.coef((C0, 3 + Cf))
    xyzs = [d.val((B, N, 3), 0.5, 1.0) for _, N, _ in segs]
    feats = [d.val((B, Cf, N), 0.5, 1.0) for _, N, _ in segs]
    news = [d.val((B, idx.shape[1], 3), 0.5, 1.0) for idx, _, _ in segs]
    stat_c, scale, shift = d.val((L.nseg * C0,), 0.25, 0.5), d.coef((L.nseg * C0,)), d.val((L.nseg * C0,), 0.25, 1.0)
    A1, A2, A3 = (d.coef((L.nseg * C0,)) for _ in range(3))
    # compact side: per-point operand, Z = W0 . X0, expand
    X0 = O.pack_points(xyzs[0], feats[0], segs[0][1], segs[0][2], xyzs[-1] if two else None, feats[-1] if two else None,
                       segs[-1][1] if two else 0, segs[-1][2] if two else 0, B, 3, Cf, 1.0, 3 + Cf)
    centers = np.concatenate([n.reshape(-1, 3) for n in news] + [np.zeros((1, 3))])
    Y0, Ya = O.expand(L, W0, centers, Z=W0 @ X0)
    Y3, _ = O.expand(L, W0, centers, X3=X0[:3])
    part, _, live = O.expand_part(L, Y0, Ya, stat_c)
    out, argq, yarg = O.pool_fwd(L, Y0, scale, shift)
    dNslot = [d.val((B, C0, idx.shape[1], ns), 0.25, 2.0) for idx, _, _ in segs]
    dN = np.zeros((C0, L.ldp))
    S_ref, T_ref, dW_ref = np.zeros((C0, L.ldz)), np.zeros((C0, L.nballs)), np.zeros((C0, 3))
    for s, (idx, N, ld) in enumerate(segs):
        npoint = idx.shape[1]
        y, g = _slotwise(idx, xyzs[s], news[s], feats[s], W0)
        k = slice(s * C0, (s + 1) * C0)
        bc = lambda v: v[None, :, None, None]
        # layer-0 output: every slot of a class carries the class's column value
        cnt = L.ball_cnt[L.ball_base[s]:L.ball_base[s] + B * npoint].reshape(B, npoint)
        off = L.ball_off[L.ball_base[s]:L.ball_base[s] + B * npoint].reshape(B, npoint)
        slot = np.arange(ns)[None, None, :]
        col = off[:, :, None] + np.where(slot < cnt[:, :, None], slot, 0)           # (B, npoint, ns): the slot's column
        assert np.array_equal(y, Y0[:, col].transpose(1, 0, 2, 3))
        if s == 0:
            xyz_only = np.einsum("ok,bkjs->bojs", W0[:, :3], g)
            assert np.array_equal(xyz_only, Y3[:, col].transpose(1, 0, 2, 3))
        # weighted statistics == statistics over all slots
        rows = np.nonzero(live & (L.seg_of_col(np.arange(len(live)) * 256) == s))[0]
        assert np.array_equal(part[rows, 0].sum(0), y.sum((0, 2, 3)))
        assert np.array_equal(part[rows, 1].sum(0), ((y - bc(stat_c[k])) ** 2).sum((0, 2, 3)))
        # pool == max over ns of relu(fma)
        ref = np.maximum((y * bc(scale[k]) + bc(shift[k])).max(-1), 0.0)                 # (B, C0, npoint)
        blk = out[:, L.ball_base[s]:L.ball_base[s] + B * npoint].reshape(C0, B, npoint).transpose(1, 0, 2)
        assert np.array_equal(blk, ref)
        # backward: the class sum of the slot gradients rides on the column, dY_q = sum of the slots' dY
        np.add.at(dN.T, col.reshape(-1), dNslot[s].transpose(0, 2, 3, 1).reshape(-1, C0))
        dYslot = bc(A1[k]) * dNslot[s] + bc(A2[k]) * y + bc(A3[k])
        pts = (L.pt_base[s] + np.arange(B)[:, None, None] * ld + idx).reshape(-1)
        np.add.at(S_ref.T, pts, dYslot.transpose(0, 2, 3, 1).reshape(-1, C0))
        T_ref[:, L.ball_base[s]:L.ball_base[s] + B * npoint] = dYslot.sum(-1).transpose(1, 0, 2).reshape(C0, -1)
        dW_ref += np.einsum("bcjs,bkjs->ck", dYslot, g)
    dY, _ = O.layer0_dy(L, dN, Y0, A1, A2, A3)
    S, T = O.reduce_sums(L, dY)
    assert np.array_equal(S, S_ref) and np.array_equal(T, T_ref)
    assert np.array_equal(O.dw0_xyz(L, dY, X0, centers), dW_ref)
    # the two ways to the layer-0 weight gradient agree: S . xyz^T minus the centre term
    dW = np.zeros((C0, 5))
    dW[:, :3] = S @ X0[:3].T
    assert np.array_equal(O.center_term(T, centers, dW)[:, :3], dW_ref)
    # pool backward: D carries dOut at the arg-max column where out > 0, the totals are the sums over the balls
    dOut, mean = d.val((C0, L.nballs), 0.25, 2.0), d.val((L.nseg * C0,), 0.25, 0.5)
    D, tot, _, _ = O.pool_bwd(L, dOut, out, argq, yarg, mean)
    g = np.where(out > 0, dOut, 0.0)
    assert np.array_equal(np.nansum(D, axis=1), g.sum(1)) and np.isnan(D[:, L.unwritten()]).all()
    assert np.array_equal(np.add.reduceat(D[:, L.real], L.rstart, axis=1), g)
    assert np.array_equal(tot[:, 0].sum(0), g.sum(1))
    assert np.array_equal(L.from_pooled(L.to_pooled(out), C0), out)


FAMILIES = ["singles", "full", "mixed", "paired", "wide"]


@pytest.mark.parametrize("name", FAMILIES)
def test_layout_contract(name):
    """every family: padded like ball_query, the layout of o3d_compact_build[2]'s contract"""
    fam, L = O.family(name), O.family_layout(name)
    for s, (idx, N, ld) in enumerate(fam["segs"]):
        assert idx.min() >= 0 and idx.max() < N <= ld
        n = L.nballs_s[s]
        cnt = L.ball_cnt[L.ball_base[s]:L.ball_base[s] + n]
        flat = idx.reshape(n, -1)
        for i in range(n):          # cnt distinct entries, then copies of the first hit
            assert len(set(flat[i, :cnt[i]])) == cnt[i] and (flat[i, cnt[i]:] == flat[i, 0]).all()
        assert tuple(L.meta[s]) == ((L.live[s] + 255) // 256 * 256, L.live[s], n, 0) and L.live[s] == cnt.sum()
        pad = np.arange(L.start[s] + L.live[s], L.start[s] + L.live256[s])
        assert (L.gp[pad] == 0).all() and (L.cball[pad] == L.dummy_ball).all() and (L.cw[pad] == 0).all()
        assert (fam["B"] * idx.shape[1] * fam["ns"]) % 256 == 0          # o3d_compact_build's slot granularity
    assert L.start1 % 512 == 0 and L.ldp % 512 == 0 and L.dummy_ball == L.nballs
    assert (L.gp[L.unwritten()] == O.FILL_I).all()
    # the weights of a ball add up to ns, its columns are consecutive and carry its id
    assert np.array_equal(np.add.reduceat(L.cw[L.real], L.rstart), np.full(L.nballs, float(fam["ns"])))
    assert np.array_equal(L.cball[L.real], np.repeat(np.arange(L.nballs), L.ball_cnt))
    assert np.array_equal(L.real[L.rstart], L.ball_off)


@pytest.mark.parametrize("B,ns,npoints,Ns", [(1, 32, [8], [40]), (3, 16, [64], [128]), (2, 8, [32, 64], [64, 129]),
                                            (48, 32, [256, 512], [512, 1024])])
def test_host_record_states_the_oracles_sizes(B, ns, npoints, Ns):
    """open3dsot_amd.gemm.Compact, the host side's one statement of the layout's sizes and tensor shapes, against the
    oracle's independent one (clouds padded to 128 point columns, the worst case of all slots distinct)"""
    from open3dsot_amd import gemm
    ld = [(n + 127) // 128 * 128 for n in Ns]
    L = O.Layout([(np.zeros((B, npt, ns), np.int64), l) for npt, l in zip(npoints, ld)])
    c = gemm.Compact(B, ns, npoints, Ns)
    assert (c.nseg, c.B, c.ns, c.npoints, c.Ns, c.Npads) == (L.nseg, B, ns, npoints, Ns, ld)
    assert (c.starts, c.start1, c.pt_bases, c.ball_bases, c.nballs_s) == (L.start, L.start1, L.pt_base, L.ball_base, L.nballs_s)
    assert (c.ldp, c.ldz, c.nballs) == (L.ldp, L.ldz, L.nballs) and c.Pmaxs == [n * ns for n in L.nballs_s]
    assert c.np1 == (npoints[1] if len(npoints) == 2 else 0)
    assert c.reduce_dims == (B, L.nseg, npoints[0], ld[0], npoints[-1], ld[-1])
    shapes = {k: sh for k, (sh, _) in c.tensors.items()}
    assert shapes == {"centers": (L.dummy_ball + 1, 3), "ball_cnt": L.ball_cnt.shape, "ball_off": (L.nballs + 1,),
                      "gp": L.gp.shape, "cball": L.cball.shape, "cw": L.cw.shape, "meta": L.meta.shape}
    assert {k for k, (_, dt) in c.tensors.items() if dt == torch.float32} == {"centers", "cw"}
    assert {k for k, (_, dt) in c.tensors.items() if dt == torch.int32} == set(c.tensors) - {"centers", "cw"}
    given = {k: torch.empty(sh, dtype=dt) for k, (sh, dt) in c.tensors.items()}
    cpu = torch.device("cpu")
    assert c.fits(given, cpu) and c.take(given).gp is given["gp"]
    assert not c.fits({k: v for k, v in given.items() if k != "meta"}, cpu)
    assert not c.fits(dict(given, cw=given["cw"].double()), cpu) and not c.fits(dict(given, gp=given["gp"][:-1]), cpu)
    assert not c.fits(dict(given, centers=given["centers"].t().contiguous().t()), cpu) and not c.fits(given, torch.device("meta"))


def _balls_starting(L, lo, hi):
    return int(((L.ball_off >= lo) & (L.ball_off < hi)).sum())


def test_family_singles():
    L = O.family_layout("singles")
    assert (L.ball_cnt == 1).all() and L.ns == 8 and L.B == 2 and L.npoint == [320]
    assert _balls_starting(L, 0, 512) == 512          # four staging passes of pool_bwd_dense (PBD_BALLS = 128)
    assert _balls_starting(L, 0, 128) == 128          # four output batches of pool_t (PT_RB = 32)
    for b in range(2):                                # every ball of a cloud a different point
        assert len(set(L.gp[b * 320:(b + 1) * 320])) == 320


def test_family_full():
    L = O.family_layout("full")
    assert (L.ball_cnt == 32).all() and L.live == [1024] and L.ldp == 1024 and L.live256 == [1024]
    assert L.live[0] % 512 == 0 and not L.unwritten().any() and (L.cw == 1.0).all()


def test_family_mixed():
    fam, L = O.family("mixed"), O.family_layout("mixed")
    assert L.B == 3 and L.npoint == [128] and L.ns == 32
    assert sorted(set(L.ball_cnt)) == list(range(1, 33))
    for m in (128, 256, 512, 2048):
        assert O.straddlers(L, m), m
    assert L.ball_off[128] % 4 != 0                   # cloud 1 starts off a float4 boundary: the q0a = q0 & ~3 path
    spans = [L.ball_cnt[b * 128:(b + 1) * 128].sum() for b in range(3)]
    assert max(spans) > 2048                          # two RG_CH chunks in one cloud
    assert L.live[0] % 256 != 0
    idx, N, ld = fam["segs"][0]
    assert (idx == O.HUB).any(-1).all()               # one point in every ball (the balanced run flush)
    assert N < ld and idx.max() < N                   # points N .. ld-1: referenced by none


def test_family_paired():
    fam, L = O.family("paired"), O.family_layout("paired")
    assert L.nseg == 2 and L.npoint == [64, 128] and L.ld == [128, 256] and L.B == 2 and L.ns == 16
    assert L.start1 == 2 * 64 * 16 and L.start1 % 512 == 0
    assert set(L.ball_cnt[:128]) == {1, 2} and L.live[0] < 256 and L.live256[0] == 256
    assert L.pt_base == [0, 256] and L.ball_base == [0, 128] and L.ldz == 2 * (128 + 256)
    assert L.gp[L.start1:L.start1 + L.live[1]].min() >= 256


def test_family_wide():
    L = O.family_layout("wide")
    assert L.ns == 64 and L.B == 1 and L.npoint == [64]
    assert sorted(L.ball_cnt) == list(range(1, 65)) and (L.ball_cnt > 32).sum() == 32
    assert L.live[0] > 2048 and L.live[0] % 256 != 0


POOL_C = [12, 32, 96, 8, 24]
L0_C = [5, 64]
EXPAND_C = [5, 64, 136]


@pytest.mark.parametrize("name", FAMILIES)
def test_exact_leg_inputs_meet_the_exactness_condition(name):
    """sum|terms| / (grid spacing of the terms) < 2^24 for every output the GPU test compares for equality: all partial
    sums of a correct kernel are then exact in fp32 in any order"""
    L = O.family_layout(name)
    worst = {}
    for C0 in EXPAND_C:
        i = O.expand_inputs(L, C0, O.Dyadic(100 + C0))
        for kw in (dict(Z=i["Z"]), dict(X3=i["X3"])):
            Y0, Ya = O.expand(L, i["W0"], i["centers"], **kw)
            _, pabs, _ = O.expand_part(L, Y0, Ya, i["stat_c"])
            worst["Y0"] = O.assert_exact("Y0", Ya)
            worst["part0"] = O.assert_exact("part0", pabs[:, 0])
            worst["part1"] = O.assert_exact("part1", pabs[:, 1])
    for C in POOL_C:
        i = O.pool_inputs(L, C, O.Dyadic(200 + C))
        plants = O.plant_pool(L, i["Y"], i["scale"], i["shift"])
        seg = L.seg_of_col(L.real)
        n_abs = np.abs(i["Y"][:, L.real] * L.per_channel(i["scale"], C, seg)) + np.abs(L.per_channel(i["shift"], C, seg))
        worst["pool"] = O.assert_exact("pool", n_abs)
        out, argq, yarg = O.pool_fwd(L, i["Y"], i["scale"], i["shift"])
        for what, c, ball, q, o in plants:             # the plants do what they claim
            assert out[c, ball] == o and (q is None or argq[c, ball] == q), (what, c, ball)
        _, _, tabs, _ = O.pool_bwd(L, i["dOut"], out, argq, yarg, i["mean"])
        worst["bwd0"] = O.assert_exact("bwd0", tabs[:, 0])
        worst["bwd1"] = O.assert_exact("bwd1", tabs[:, 1])
    for C0 in L0_C:
        i = O.layer0_inputs(L, C0, O.Dyadic(300 + C0))
        _, dYa = O.layer0_dy(L, i["dN"], i["Y0"], i["A1"], i["A2"], i["A3"])
        Sa, Ta = O.reduce_sums(L, dYa)
        worst["S"], worst["T"] = O.assert_exact("S", Sa), O.assert_exact("T", Ta)
        worst["dW0"] = O.assert_exact("dW0", O.dw0_xyz(L, dYa, i["X"], i["centers"], absolute=True))
    assert len(worst) == 9


def test_plants_cover_every_edge():
    """mixed / paired / wide hold every planted case of the pool tests; the sign cases exist everywhere"""
    for name in FAMILIES:
        L = O.family_layout(name)
        i = O.pool_inputs(L, 8, O.Dyadic(1))
        kinds = {p[0] for p in O.plant_pool(L, i["Y"], i["scale"], i["shift"])}
        assert {"all_negative", "max_is_zero"} <= kinds
        if name in ("mixed", "paired", "wide"):
            assert kinds == {"boundary128-", "boundary128+", "boundary512-", "boundary512+", "first", "last", "all_equal",
                             "tie", "tie_adjacent", "all_negative", "max_is_zero"}


@pytest.mark.parametrize("nballs", [1, 1025])
def test_centre_inputs_meet_the_exactness_condition(nballs):
    i = O.center_inputs(nballs, 7, 6, O.Dyadic(400 + nballs))
    O.assert_exact("center_term", O.center_term(i["T"], i["centers"], i["dW"], absolute=True))
    O.assert_exact("center_grad", O.center_grad(i["T"], i["W0"], 0.5, absolute=True))
    ref = O.center_term(i["T"], i["centers"], i["dW"])
    assert np.array_equal(ref[:, 3:], i["dW"][:, 3:])
    assert np.array_equal(O.center_term_out(i["T"], i["centers"], i["dW"], 5), ref[:, :5])
    assert np.array_equal(O.center_grad(i["T"], i["W0"], 0.5), 0.5 * np.einsum("ck,cb->kb", i["W0"][:, :3], i["T"]))


@pytest.mark.parametrize("nxyz", [0, 3])
@pytest.mark.parametrize("two", [False, True])
def test_pack_inputs_meet_the_exactness_condition(two, nxyz):
    i = O.pack_inputs(two, O.Dyadic(500 + nxyz + two))
    ref = O.pack_points(i["xyz"][0], i["feats"][0], i["N0"], i["ld0"], i["xyz"][1], i["feats"][1], i["N1"], i["ld1"], 2, nxyz, 3,
                        0.5, nxyz + 5)
    O.assert_exact("pack", np.abs(ref))
    assert i["N0"] < i["ld0"] and (not two or i["N1"] < i["ld1"])
    assert (ref[nxyz + 3:] == 0).all() and (ref[:, i["N0"]:i["ld0"]] == 0).all() and np.abs(ref).sum() > 0
