"""tests/ordered_reduce_oracle.py (the float32 restatement of the ordered layer-0 list sums) against the fp64 reference
compact_oracle.reduce_sums, and its new index families against the shapes they are there for.  No GPU."""
import numpy as np
import pytest

import compact_oracle as O
import ordered_reduce_oracle as R

FAMILIES = ["singles", "full", "mixed", "paired", "wide"] + R.NEW_FAMILIES


def _dy(L, C0, draw):
    i = O.layer0_inputs(L, C0, draw)
    return O.layer0_dy(L, i["dN"], i["Y0"], i["A1"], i["A2"], i["A3"])


@pytest.mark.parametrize("name", FAMILIES)
def test_restatement_is_exact_on_dyadic_inputs(name):
    L = R.family_layout(name)
    dY, dYa = _dy(L, 5, O.Dyadic(300))
    S, T = O.reduce_sums(L, dY)
    Sa, Ta = O.reduce_sums(L, dYa)
    O.assert_exact("S", Sa)
    O.assert_exact("T", Ta)
    assert (dY.astype(np.float32) == dY).all()
    So, To = R.ordered_sums(L, dY)
    assert So.dtype == np.float32 and To.dtype == np.float32
    assert np.array_equal(So.astype(np.float64), S) and np.array_equal(To.astype(np.float64), T)


@pytest.mark.parametrize("name", FAMILIES)
def test_restatement_is_within_the_rounding_bound(name):
    """randn: |err| <= (n + 8) * 2^-24 * sum|t_i|, the bound of tests/test_compact_kernels_gpu.py"""
    L = R.family_layout(name)
    rng = np.random.RandomState(5)
    dY = rng.randn(3, len(L.real)).astype(np.float32).astype(np.float64)
    S, T = O.reduce_sums(L, dY)
    Sa, Ta = O.reduce_sums(L, np.abs(dY))
    nS, _ = O.reduce_sums(L, np.ones((1, len(L.real))))
    So, To = R.ordered_sums(L, dY)
    for got, ref, ra, n in ((So, S, Sa, nS), (To, T, Ta, L.ball_cnt[None, :])):
        bound = (np.asarray(n, np.float64) + 8) * 2.0 ** -24 * ra
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bound).all(), (name, float((err - bound).max()))


@pytest.mark.parametrize("name", FAMILIES)
def test_ordered_index_is_a_sorted_permutation(name):
    L = R.family_layout(name)
    perm, poff = R.ordered_index(L)
    nchunk = R.nchunk_of(L)
    written = np.zeros(L.ldp, bool)
    for cl in R.clouds(L):
        c, pbase, _, _, ld, q0, q1, q0a = cl
        written[q0:q1] = True
        po = poff[c]
        assert po[0] == 0 and po[nchunk * ld] == q1 - q0 and (np.diff(po[:nchunk * ld + 1]) >= 0).all()
        cols = []
        for k in range(nchunk):
            for n in range(ld):
                lst = perm[q0 + po[k * ld + n]:q0 + po[k * ld + n + 1]]
                assert ((lst >> 16) == n).all() and (np.diff(lst) > 0).all()          # one point, ascending column
                q = q0a + k * R.RG_CH + (lst & 0xffff)
                assert (L.gp[q] == pbase + n).all()
                cols.append(q)
        assert np.array_equal(np.sort(np.concatenate(cols)), np.arange(q0, q1))       # every column once
    assert (perm[~written] == O.FILL_I).all()


def test_new_families_reach_what_they_are_for():
    # (a) a cloud longer than a chunk, and a point's list on both sides of the boundary
    L = R.family_layout("chunkcut")
    for cl in R.clouds(L):
        chunks = R.cloud_chunks(L, cl)
        assert len(chunks) >= 2 and all((n == O.HUB).any() for _, _, _, n, _ in chunks[:2])
    # (b) a run of more than 2 * 256 entries in one chunk: it covers whole thread shares
    L = R.family_layout("hubrun")
    for cl in R.clouds(L):
        _, _, _, n, q = R.cloud_chunks(L, cl)[0]
        per = -(-len(q) // R.THREADS)
        assert (n == O.HUB).sum() > 2 * R.THREADS and (n == O.HUB).sum() >= 3 * per
    # (c) segment 1, second cloud: q0 off the float4 grid and more than one chunk
    L = R.family_layout("misaligned")
    assert L.nseg == 2
    cl = R.clouds(L)[3]
    assert cl[5] != cl[7] and len(R.cloud_chunks(L, cl)) >= 2
    for name in R.NEW_FAMILIES:
        f = R.family(name)
        assert f["B"] == 2 and len(f["segs"]) <= 2 and all(ld <= 1024 for _, _, ld in f["segs"])
