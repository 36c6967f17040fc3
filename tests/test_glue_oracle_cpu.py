"""tests/glue_oracle.py against the operators it restates, and tests/test_glue_kernels_gpu.py against itself:
  * the cosine map tied, to 1e-12, to nn.CosineSimilarity(dim=1, eps=1e-8) on the expanded (B, f, M, N) tensors in fp64
    under autograd (no zero vectors), and -- stated separately -- what torch gives on a zero vector next to the kernel's rule;
  * the copies (centres, row gather, row stacking, weight preparation) against torch.gather / cat / transposes;
  * the exactness precondition of every exact case of the GPU file, and its case tables as a checklist;
  * sensitivity: plausible mistakes applied to the oracle's output are rejected by the GPU file's comparisons.
No GPU."""
import numpy as np
import pytest
import torch

import glue_oracle as GO
import test_glue_kernels_gpu as K


def rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def torch_cosine(t, s, dsim):
    """nn.CosineSimilarity on the expanded tensors, as models/head/xcorr.py builds them -> sim (B, N, M), dt, ds"""
    tt = torch.tensor(t, dtype=torch.float64, requires_grad=True)
    ss = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    B, f, M = tt.shape
    N = ss.shape[2]
    sim = torch.nn.CosineSimilarity(dim=1, eps=1e-8)(tt[:, :, :, None].expand(B, f, M, N), ss[:, :, None, :].expand(B, f, M, N))
    sim = sim.transpose(1, 2)                                 # (B, N, M)
    sim.backward(torch.tensor(dsim, dtype=torch.float64))
    return sim.detach().numpy(), tt.grad.numpy(), ss.grad.numpy()


@pytest.mark.parametrize("B,f,M,N", [(1, 32, 4, 1), (2, 96, 12, 33), (3, 32, 60, 100)])
def test_cosine_map_vs_cosine_similarity_under_autograd(B, f, M, N):
    rng = np.random.RandomState(B + M)
    t, s, dsim = rng.randn(B, f, M), rng.randn(B, f, N), rng.randn(B, N, M)
    sim, dt, ds = torch_cosine(t, s, dsim)
    r = GO.cosine_sim(t, s)
    assert rel(r.sim, sim) <= 1e-12 and rel(r.tn, np.linalg.norm(t, axis=1)) <= 1e-12
    rb = GO.cosine_sim_bwd(dsim, r.sim, r.tn, r.sn, t, s)
    assert rel(rb.dt, dt) <= 1e-12 and rel(rb.ds, ds) <= 1e-12
    assert (np.abs(r.sim) <= 1 + 1e-12).all() and (r.sim_bound > 0).all() and (rb.dt_bound > 0).all()


def test_zero_vectors_torch_and_the_kernels_rule():
    """A zero template column and a zero search column.  The kernel's rule: the norm is clamped at eps = 1e-8 (as fp32) and the
    clamped norm is a constant, so sim = 0 there and the gradient w.r.t. the zero vector is sum_j dsim s_j / (eps sn_j) --
    no term through the norm.  torch (2.x: each norm clamped separately, clamp_min passing no gradient where it clamps)
    gives the same up to the value of eps: the oracle uses float32(1e-8), torch the double 1e-8, 6e-9 relative apart; with
    that one constant swapped the two agree to 1e-12."""
    rng = np.random.RandomState(0)
    B, f, M, N = 2, 32, 4, 5
    t, s, dsim = rng.randn(B, f, M), rng.randn(B, f, N), rng.randn(B, N, M)
    t[:, :, 1], s[:, :, 0] = 0.0, 0.0
    sim, dt, ds = torch_cosine(t, s, dsim)
    assert np.isfinite(sim).all() and np.isfinite(dt).all() and np.isfinite(ds).all()
    assert not sim[:, :, 1].any() and not sim[:, 0, :].any()
    r = GO.cosine_sim(t, s)
    assert (r.tn[:, 1] == GO.EPS).all() and (r.sn[:, 0] == GO.EPS).all() and not r.sim[:, :, 1].any()
    live_t, live_s = [0, 2, 3], [1, 2, 3, 4]
    assert rel(r.sim[:, live_s][:, :, live_t], sim[:, live_s][:, :, live_t]) <= 1e-12
    old = GO.EPS
    try:
        GO.EPS = 1e-8                                         # torch's constant instead of the kernel's fp32 one
        r8 = GO.cosine_sim(t, s)
        rb = GO.cosine_sim_bwd(dsim, r8.sim, r8.tn, r8.sn, t, s)
    finally:
        GO.EPS = old
    assert rel(rb.dt, dt) <= 1e-12 and rel(rb.ds, ds) <= 1e-12            # zero columns included: the rules agree
    assert abs(GO.EPS / 1e-8 - 1) < 1e-8
    # and the mistake of keeping the gradient through the clamped norm differs from torch only where t != 0 (never here):
    # with a zero vector the extra term t * a_i is itself zero, which is why the exact leg pins the rule on inputs of its own
    kept = GO.cosine_sim_bwd(dsim, r.sim, r.tn, r.sn, t, s, keep_clamped=True)
    rb32 = GO.cosine_sim_bwd(dsim, r.sim, r.tn, r.sn, t, s)
    assert np.array_equal(kept.dt, rb32.dt) and np.array_equal(kept.ds, rb32.ds)


def test_copies_vs_torch():
    rng = np.random.RandomState(1)
    B, N = 3, 20
    xyz = rng.rand(B, N, 3).astype(np.float32)
    si = np.stack([rng.permutation(N)[:7] for _ in range(B)])
    c, per = GO.sample_query_centers([(xyz, si, 7), (xyz, None, 5)])
    want = torch.gather(torch.from_numpy(xyz), 1, torch.from_numpy(si)[:, :, None].expand(-1, -1, 3)).numpy()
    assert np.array_equal(per[0], want) and np.array_equal(per[1], xyz[:, :5])
    assert c.shape == (B * 12 + 1, 3) and np.array_equal(c[:B * 7], want.reshape(-1, 3)) and not c[-1].any()
    assert c.dtype == np.float32
    a, b = rng.randn(B, N, 9).astype(np.float32), rng.randn(B, N, 3).astype(np.float32)
    idx = rng.randint(0, N, size=(B, 11))
    ra, rb = GO.gather_rows2(a, b, idx, 7)
    ii = torch.from_numpy(idx[:, :7])[:, :, None]
    assert np.array_equal(ra, torch.gather(torch.from_numpy(a), 1, ii.expand(-1, -1, 9)).numpy())
    assert np.array_equal(rb, torch.gather(torch.from_numpy(b), 1, ii.expand(-1, -1, 3)).numpy())
    s1, s2 = torch.randn(B, 3, N), torch.randn(B, 5, N)
    X = GO.pack_rows([s1.numpy(), s2.numpy()], 10)
    want = torch.cat([s1, s2], 1).permute(1, 0, 2).reshape(8, B * N).numpy()
    assert np.array_equal(X[:8], want) and not X[8:].any()
    W = rng.randn(3, 5).astype(np.float32)
    d = GO.prep_weights(np.full(5 * 4, K.SENT, np.float32), W, 4, 1).reshape(5, 4)
    assert np.array_equal(d[:, :3], W.T) and (d[:, 3] == np.float32(K.SENT)).all()
    d = GO.prep_weights(np.full(3 * 7, K.SENT, np.float32), W, 7, 0).reshape(3, 7)
    assert np.array_equal(d[:, :5], W) and (d[:, 5:] == np.float32(K.SENT)).all()


# ---- exactness preconditions and case tables -------------------------------------------------------------------------------
def test_exact_forward_inputs_have_power_of_two_norms():
    for n, (f, M, N) in enumerate(K.COS_SHAPES):
        rng = np.random.RandomState(50 + n)
        zt, zs = K.zero_cols(M, N)
        t, s = GO.pow2_columns(rng, 3, f, M, zt), GO.pow2_columns(rng, 3, f, N, zs)
        assert ((t != 0).sum(1) == np.where(np.isin(np.arange(M), zt), 0, 4)[None, :]).all()
        r = GO.cosine_sim(t, s)
        for v in (r.tn, r.sn):
            live = v > GO.EPS
            assert np.array_equal(np.log2(v[live]), np.round(np.log2(v[live])))
        # every dot product: at most four terms on the grid 2^-4, magnitudes up to 2^4 -> exact in fp32 in any order
        assert np.array_equal(r.dot * 16, np.round(r.dot * 16)) and r.dot_abs.max() * 16 < 2.0 ** 24
        assert np.array_equal(r.sim.astype(np.float32).astype(np.float64), r.sim)


def test_exact_backward_inputs_keep_every_sum_exact():
    for n, (f, M, N) in enumerate(K.COS_SHAPES):
        rng = np.random.RandomState(50 + n)
        for clamped in (False, True):
            i = GO.exact_bwd_inputs(rng, 3, f, M, N, clamped_t=clamped)
            r = GO.cosine_sim_bwd(i.dsim, i.sim, i.tn, i.sn, i.t, i.s)
            assert GO.assert_exact_bwd(i, r) < 2.0 ** 24
            assert (i.tn <= GO.EPS).all() == clamped
            if clamped:                                       # the clamp has something to drop, and b_j nothing to add
                kept = GO.cosine_sim_bwd(i.dsim, i.sim, i.tn, i.sn, i.t, i.s, keep_clamped=True)
                assert not r.bj.any() and kept.ai[:, :2].all() and not r.ai.any()
            for v in (r.dt, r.ds):
                assert np.array_equal(v.astype(np.float32).astype(np.float64), v)


def test_case_tables_promise_what_the_issue_lists():
    assert {f for f, _, _ in K.COS_SHAPES} == {32, 96} and {M for _, M, _ in K.COS_SHAPES} == {4, 12, 60, 64}
    assert {N for _, _, N in K.COS_SHAPES} == {1, 31, 32, 33, 100, 128} and (96, 64, 128) in K.COS_SHAPES
    assert K.WRAP_B * K.WRAP_NPOINT == 65540 and K.WRAP_N == 8 and K.WRAP_NS == 4
    sizes = sorted({r * c for r, c in K.PREP_SHAPES})
    assert sizes[:4] == [1, 8191, 8192, 8193] and sizes[-1] > 2 * 8192
    jobs = K.prep_jobs(np.random.RandomState(0), K.PREP_SHAPES)
    assert {j[4] for j in jobs} == {0, 1} and any(j[3] > (j[1] if j[4] else j[2]) for j in jobs)


# ---- sensitivity -----------------------------------------------------------------------------------------------------------
def rejected(name, got, ref, bound, exact):
    with pytest.raises(AssertionError):
        K.compare(name, got, ref, bound, exact, ratios={})
    return True


def test_rejects_swapped_norms_and_one_element_off():
    rng = np.random.RandomState(2)
    t, s, dsim = rng.randn(2, 32, 12).astype(np.float32), rng.randn(2, 32, 12).astype(np.float32), rng.randn(2, 12, 12)
    s *= 1.5
    r = GO.cosine_sim(t, s)
    K.compare("tn", r.tn, r.tn, r.tn_bound, False, ratios={})
    K.compare("tn", r.tn.astype(np.float32), r.tn, r.tn_bound, False, ratios={})
    assert rejected("tn", r.sn, r.tn, r.tn_bound, False) and rejected("sn", r.tn, r.sn, r.sn_bound, False)
    rb = GO.cosine_sim_bwd(dsim, r.sim, r.tn, r.sn, t, s)
    sw = GO.cosine_sim_bwd(dsim, r.sim, r.sn, r.tn, t, s)                 # (M == N here: the swap has the right shape)
    assert rejected("dt", sw.dt, rb.dt, rb.dt_bound, False) and rejected("ds", sw.ds, rb.ds, rb.ds_bound, False)
    for name, ref, bound in (("tn", r.tn, r.tn_bound), ("sim", r.sim, r.sim_bound), ("dt", rb.dt, rb.dt_bound),
                             ("ds", rb.ds, rb.ds_bound)):
        got = ref.copy()
        at = tuple(np.array(ref.shape) - 1)
        got[at] += 2 * bound[at]
        assert bound[at] > 0 and rejected(name, got, ref, bound, False)
        K.compare(name, ref.astype(np.float32), ref, bound, False, ratios={})


def test_rejects_the_gradient_through_a_clamped_norm():
    rng = np.random.RandomState(3)
    i = GO.exact_bwd_inputs(rng, 2, 32, 12, 31, clamped_t=True)
    r = GO.cosine_sim_bwd(i.dsim, i.sim, i.tn, i.sn, i.t, i.s)
    kept = GO.cosine_sim_bwd(i.dsim, i.sim, i.tn, i.sn, i.t, i.s, keep_clamped=True)
    assert rejected("dt", kept.dt, r.dt, None, True)
    K.compare("ds", kept.ds, r.ds, None, True, ratios={})     # (the search norms are live in both)


def test_rejects_a_centre_row_off_by_one_and_a_transposed_job_copied_plain():
    rng = np.random.RandomState(4)
    xyz = rng.rand(2, 9, 3).astype(np.float32)
    si = np.stack([rng.permutation(9)[:4] for _ in range(2)])
    c, _ = GO.sample_query_centers([(xyz, si, 4)])
    K.same_bits("centers", c, c)
    with pytest.raises(AssertionError):
        K.same_bits("centers", np.roll(c, 1, axis=0), c)
    with pytest.raises(AssertionError):
        K.same_bits("centers", GO.sample_query_centers([(xyz, (si + 1) % 9, 4)])[0], c)
    with pytest.raises(AssertionError):                       # -0.0 where 0.0 is expected: bit for bit
        K.same_bits("centers", np.where(np.arange(len(c))[:, None] == len(c) - 1, np.float32(-0.0), c), c)
    W = rng.randn(8, 8).astype(np.float32)
    dst = np.full(8 * 9, K.SENT, np.float32)
    with pytest.raises(AssertionError):
        K.same_bits("prep", GO.prep_weights(dst, W, 9, 0), GO.prep_weights(dst, W, 9, 1))
    a = rng.randn(2, 9, 3).astype(np.float32)
    idx = rng.randint(0, 9, size=(2, 6))
    with pytest.raises(AssertionError):                       # the index read with ld_idx = npoint instead of 6
        K.same_bits("gather", GO.gather_rows2(a, None, idx.reshape(-1)[:8].reshape(2, 4), 4)[0], GO.gather_rows2(a, None, idx, 4)[0])
