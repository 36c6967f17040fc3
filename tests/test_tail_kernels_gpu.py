"""The kernels at the tail of a training step and of a tracked frame, called through the C ABI with raw pointers, launch by
launch, against the plain numpy fp64 reference tests/tail_oracle.py (tied to the trackers' compute_loss, torch.optim.Adam and
the reference's box helpers under autograd by tests/test_tail_oracle_cpu.py): o3d_track_loss, o3d_m2track_loss (csrc/loss.hip),
o3d_adam_step, o3d_best_proposal, o3d_rpn_votes_fwd, o3d_rpn_votes_bwd, o3d_box_assemble (csrc/heads.hip), o3d_motion_merge_fwd,
o3d_motion_merge_bwd, o3d_offset_box (csrc/boxcloud.hip).  Same method as tests/test_pointwise_kernels_gpu.py and
tests/test_rows_kernels_gpu.py, whose helpers this file imports.  e = 2^-24 below.

EXACT leg (equality): inputs on a dyadic grid, so a correct kernel is exact in fp32 whatever its summation order (with or
without FMA contraction); the CPU file evaluates the same formulas in numpy float32 and finds them equal to fp64.  Compared for
equality: the three counts of o3d_track_loss and its vote, BoxCloud and box smooth-L1 sums (|d| exactly 0, exactly 1, just
inside and outside 1: the coordinates of a seed share one |d|, so that v = 3 sl1(d) times fl(1/3) and c = K sl1(d) over K round
back to sl1(d)); of o3d_m2track_loss the class-weight sum, the BoxCloud sum, the moving count, the four centre sums, the four
angle sums (all angles 0: sinf(0) = 0) and, where B and B*N*K are powers of two, w_center = 3 and no motion state is given,
g_bc and the centre columns of g_motion, g_aux, g_est, g_prev (a clamp times a power of two); o3d_motion_merge and o3d_offset_box
with all angles 0 (sincosf(0) = (0, 1)); the copies of the vote head's glue and o3d_box_assemble (bit-equal to numpy float32
off + centre on both legs); o3d_best_proposal entirely; o3d_adam_step with beta1 = 0.5, beta2 = 0.75, bc1 = 0.5, bc2 = 0.25,
lr = 2^-10, eps = 0, g = +-2^k, v in {0, g^2} (sqrtf of a perfect square and a division by a power of two are exact: the build
keeps clang's correctly rounded fp32 divide and sqrt, asserted on build.COMMON).  NOT exact, compared on the ROUNDED leg's bound
also when the inputs are dyadic: every gradient of o3d_track_loss (1 / (count + 1e-6) is never a power of two), every loss,
the BCE / NLL sums, g_seg, g_mcls, the angle columns, and the gradients of o3d_m2track_loss when a motion state is given.

ROUNDED leg: torch.randn inputs, |err| <= (n + 8) * e * sum|t_i| per output and per stage; a stage behind a reduction is compared
against fp64 over the sums the kernel itself stored (`partial`, read back and added in fp64), so no stage's bound carries
another's.  n per output, from the kernels' code (tail_oracle has the same figures next to the formulas):
  loss sums    a thread adds r = ceil(elements / 16384) terms (o3d_m2track_loss: ceil(B / 64) * ceil(N / 256), the BoxCloud sum
               ceil(B / 64) * ceil(N K / 256), the per-sample sums ceil(B / 256)), a wave folds in 6 butterfly steps, the four wave
               rows are added in order: depth r + 10.  A term adds its own roundings: 0 for the counts; 3 for the segmentation BCE
               (x y, the subtraction, the softplus' addition); 10 for the vote term (per coordinate the difference -- whose
               rounding costs at most 2 e sl1(d) -- and the two products of sl1, three additions, fl(1/3), y); K + 8 for the
               BoxCloud term; 4 for the objectness BCE; 8 for the box term; 6 for a 2-class NLL (difference, sum of the two
               exponentials, m + log, - x_y, the weight); 5 for an angle term; 4 for an element of M2-Track's BoxCloud sum.
  losses       from the fp64 sum of the stored rows: the kernel adds the 64 rows one after the other (64), then 2 to 4 roundings
               of the quotient (a count is exact; 1 / (count + 1e-6) is an addition and a division); the weighted total adds its
               products and additions (13 resp. 16); M2-Track's segmentation loss is a quotient of two such sums (2 * 64 + 2).
  gradients    from the same fp64 sums: 5 for g_cla (c_seg, 1 + exp, the division, - y, the product), 7 / 8 for g_vote / g_bc
               (1 / (count + 1e-6), w, fl(1/3) or / K, the difference, the product), 7 for the box columns, 9 for the objectness
               column; M2-Track: 64 + 9 for g_seg (the class-weight sum enters through the 64 additions), 5 for g_bc and the
               centre columns of g_aux / g_est / g_prev, 8 for g_motion and g_mcls.
  adam         m: 5 (fma(wd, p, g), (1 - beta1) g, the fma, the two float hyper-parameters); v: 8 (g twice, (1 - beta2), the
               fma); p against the update computed in fp64 from the STORED m and v: 8 (lr / bc1, the product, sqrtf, 1 / sqrt(bc2),
               + eps, the division, the subtraction), sum|t| = |p| + |update|.
  glue         score: 2 (1 + exp, the division); dcla: 3; boxes: 1 -- and bit-equal to float32 off + centre.
  motion       merged x, y of the previous half: 20 roundings of the chain + 4 rotations' sine / cosine + |aux_t| (the angle
               prev_t + motion_t is rounded before its sincosf: e |aux_t| in the angle); current half 8 + 2 rotations + |aux_t|;
               z: 5 / 2; aux: 4 + one rotation.  Backward: depth ceil(N / 256) + 9, 8 to 16 roundings of the per-point term and
               the chain behind the sums, three rotations.  sum|t_i| is carried through the chain term by term.
A transcendental adds U_f * e * |f| where it enters (propagated with the derivative of what follows it): U_exp = 2, U_log1p = 2,
U_log = 4, U_sin = 3, U_cos = 4, i.e. twice the worst error of torch.exp / log1p / log / sin / cos on the MI355X against fp64 over
about 10^6 fp32 arguments in the ranges used here, in fp32 ulp of the fp64 value, rounded up (U_MEASURED below; the figures are
in the header of profiles/tail_kernel_pins.txt; an ulp is at most 2 e |f|, so the sweep's worst error lies inside U_f e |f|).
That torch's functions and the kernels' expf / log1pf / logf / sinf / cosf / sincosf are the same device math library is a
SUPPOSITION: nothing here verifies it.  A value below the normal range may be flushed (whether this build flushes fp32
denormals is not known): every bound has the floor (n + 8) * 2^-126; Adam's inputs keep |g| in [1e-15, 1e15] and stay out of
that range altogether.

GUARDS on every launch: every output has a 256-element sentinel tail, and EXTRA_ROWS more rows where it is a matrix, that must
stay untouched; the scratch of the two loss entries has exactly the documented size (512 and 1024 floats), is filled with NaN
before the call and must be finite after it, with an untouched tail behind it; strided sources live in NaN-filled buffers; every
output is finite.  The worst err / bound per kernel and output is printed and, when O3D_TAIL_PINS names a file, written there
(profiles/tail_kernel_pins.txt is such a run).
"""
import os

import numpy as np
import pytest
import torch

import tail_oracle as O
from test_pointwise_kernels_gpu import SENT, TAIL, Randn, dev, devs, host, ibuf, lib, outbuf, ptr, st, tail_intact, untouched  # noqa: F401
from test_rows_kernels_gpu import EXTRA_ROWS, compare

pytestmark = pytest.mark.gpu

RATIOS = {}
FLOOR = 2.0 ** -126 / O.E24
NAN = float("nan")
# worst error of the device math library (torch.exp, log1p, log, sin, cos on the MI355X against fp64, 1.3 to 2.1 * 10^6 fp32
# arguments each): (fp32 ulp of the fp64 value, units of 2^-24 |f|) -> U_f = ceil(2 * the first figure), at least 2
U_MEASURED = {"exp": (0.8314, 1.3738), "log1p": (0.5660, 1.0449), "log": (1.7517, 2.4944), "sin": (1.3965, 1.9210),
              "cos": (1.5369, 2.0293)}
U_RANGES = {"exp": "[-87, 88]", "log1p": "[1e-30, 1]", "log": "[1, 2]", "sin": "[-8, 8]", "cos": "[-8, 8]"}


@pytest.fixture(scope="module", autouse=True)
def _pins():
    yield
    path = os.environ.get("O3D_TAIL_PINS")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |err| / bound per kernel and output, rounded legs of tests/test_tail_kernels_gpu.py;\n"
                    "# bound = (n + 8) * 2^-24 * sum|t_i| + U_f * 2^-24 * |f| per transcendental; every ratio must be <= 1\n"
                    "# device math library on the MI355X against fp64 (torch.exp / log1p / log / sin / cos, about 10^6 fp32\n"
                    "# arguments each; that the kernels' expf ... sincosf are the same library is a supposition):\n")
            for k in sorted(U_MEASURED):
                f.write("#   %-6s on %-11s worst %.4f ulp = %.4f * 2^-24 |f|  ->  U_%s = %d\n" % (
                    k, U_RANGES[k], U_MEASURED[k][0], U_MEASURED[k][1], k, O.U[k]))
            for k in sorted(RATIOS):
                f.write("%-36s %.4f\n" % (k, RATIOS[k]))


def test_allowances_are_the_measured_ones():
    for k, (ulp, rel) in U_MEASURED.items():
        assert O.U[k] == max(2, int(np.ceil(2 * ulp))) and rel <= O.U[k], k


def cmp(name, got, ref, ref_abs, n, exact=False):
    """exact: equality; else the bound of the header with its denormal floor (where sum|t_i| is 0 the value must be 0)"""
    if not exact:
        ref_abs = np.asarray(ref_abs, np.float64) + 0.0 * np.asarray(ref, np.float64)
        ref_abs = np.where(ref_abs > 0, ref_abs + FLOOR, 0.0)
    compare(name, got, ref, ref_abs, n, exact, RATIOS)


class Out:
    """a float output of `shape` with EXTRA_ROWS more rows (a matrix) and a TAIL, all prefilled with the sentinel"""

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.n = int(np.prod(shape))
        extra = EXTRA_ROWS * (self.n // self.shape[0]) if len(self.shape) > 1 else 0
        self.flat, _ = outbuf((self.n + extra,))

    @property
    def ptr(self):
        return self.flat.data_ptr()

    def host(self, finite=True):
        assert untouched(self.flat[self.n:]), "write beyond the output"
        a = self.flat[:self.n].cpu().numpy().reshape(self.shape)
        assert (a != np.float32(SENT)).all(), "an element was not written"
        if finite:
            assert np.isfinite(a).all()
        return a.astype(np.float64)

    def bits(self):
        self.host(finite=False)
        return self.flat[:self.n].cpu().numpy().reshape(self.shape).view(np.int32)

    def untouched(self):
        return untouched(self.flat)


def optr(o):
    return None if o is None else o.ptr


def scratch(n):
    t = torch.full((n + TAIL,), SENT, dtype=torch.float32, device="cuda")
    t[:n] = NAN
    return t


def devl(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def devn(a):
    return None if a is None else dev(a)


def nanbuf(shape):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device="cuda")


def bits(a):
    return np.asarray(a, np.float32).view(np.int32)


# ---- o3d_track_loss -----------------------------------------------------------------------------------------------------
def run_track(lib, i, with_bc, grads, weights=O.TRACK_W):
    B, N = i.cla.shape
    P, K = i.centers.shape[1], i.bc_label.shape[2]
    held = devs(i.cla, i.seg, i.vote, i.box_label, i.centers, i.boxes)
    bcp, bcl = (dev(i.bc_pred) if with_bc else None), dev(i.bc_label)
    sc = scratch(O.TRACK_SCRATCH)
    losses = Out((6,))
    g = [Out((B, N)), Out((B, N, 3)), Out((B, P, 5)), Out((B, N, K)) if with_bc else None] if grads else [None] * 4
    rc = lib.o3d_track_loss(*[ptr(t) for t in held], ptr(bcp), ptr(bcl), B, N, P, K, *weights, sc.data_ptr(), losses.ptr,
                            *[optr(o) for o in g], st())
    assert rc == 0
    torch.cuda.synchronize()
    tail_intact(sc)
    part = host(sc[:O.TRACK_SCRATCH]).reshape(O.LG, 8)
    assert np.isfinite(part).all(), "a row of the scratch was not written"
    names = ("g_cla", "g_vote", "g_boxes", "g_bc")
    return O.Ref(partial=part, losses=losses.host(), **{k: None if o is None else o.host() for k, o in zip(names, g)})




def check_track(k, i, got, with_bc, grads, draw, weights=O.TRACK_W):
    args = O.track_args(i, with_bc)
    B, N = i.cla.shape
    P = i.centers.shape[1]
    r = O.track_sums(*args)
    tot = got.partial.sum(0)
    assert np.array_equal(tot[:3], r.sums[:3]), ("counts", tot[:3], r.sums[:3])
    for j, name in enumerate(O.TRACK_SUMS):
        ex = draw.exact and j in O.track_spacing(i)
        if ex:
            assert r.sums_abs[j] / O.track_spacing(i)[j] < O.TWO24
        cmp("%s.sum.%s" % (k, name), tot[j], r.sums[j], r.sums_abs[j], r.sums_n[j], ex)
    f = O.track_finish(tot, B * N, B * P, weights, with_bc)
    for j, name in enumerate(O.TRACK_LOSSES):
        cmp("%s.loss.%s" % (k, name), got.losses[j], f.losses[j], f.losses_abs[j], f.losses_n[j])
    if not with_bc:
        assert got.losses[5] == 0.0 and tot[5] == 0.0
    if not grads:
        return
    g = O.track_grads(*args, weights, tot)
    for name in ("g_cla", "g_vote", "g_boxes") + (("g_bc",) if with_bc else ()):
        cmp("%s.%s" % (k, name), getattr(got, name), getattr(g, name), getattr(g, name + "_abs"), getattr(g, name + "_n"))


def _track(lib, draw, shape, kind="plain"):
    """BoxCloud and bc_pred = NULL, each with gradients and losses-only: the losses-only launch stores the same bits"""
    i = O.track_inputs(draw, *shape, kind=kind)
    for with_bc in (True, False):
        full = run_track(lib, i, with_bc, True)
        check_track("track_loss", i, full, with_bc, True, draw)
        only = run_track(lib, i, with_bc, False)
        assert np.array_equal(only.partial, full.partial) and np.array_equal(only.losses, full.losses)
    return i, full


@pytest.mark.parametrize("case", O.TRACK_EXACT, ids=str)
def test_track_loss_exact(lib, case):
    _track(lib, O.Dyadic(case[0]), case[1])


@pytest.mark.parametrize("case", O.TRACK_ROUNDED[:5], ids=str)
def test_track_loss_rounded(lib, case):
    _track(lib, Randn(case[0]), case[1])


def test_track_loss_no_foreground_seed_and_no_near_proposal(lib):
    """the 1e-6 of the three denominators alone: every loss but the segmentation BCE is 0, and so are g_vote, g_bc and the box
    columns; the objectness mask is empty, so its column's gradient is 0 as well"""
    i, got = _track(lib, Randn(O.TRACK_ROUNDED[5][0]), O.TRACK_ROUNDED[5][1], kind="empty")
    assert not got.partial[:, :3].any()
    assert not got.g_vote.any() and not got.g_boxes.any() and got.losses[1] == 0 and got.losses[2] == 0 and got.losses[4] == 0


def test_track_loss_proposals_next_to_the_thresholds(lib):
    i, got = _track(lib, Randn(O.TRACK_ROUNDED[6][0]), O.TRACK_ROUNDED[6][1], kind="edge")
    d = O.track_dist(i.centers, i.box_label)
    assert all((np.abs(d - e) < 2e-6).any() for e in O.EDGE_DIST)


def test_track_loss_saturated_logits(lib):
    """logits +-30 and +-88: expf(88) is finite, 1 + expf(88) is not 1, expf(-88) is below the normal range"""
    _track(lib, Randn(O.TRACK_ROUNDED[7][0]), O.TRACK_ROUNDED[7][1], kind="logits")


# ---- o3d_m2track_loss ---------------------------------------------------------------------------------------------------
M2_EXACT_SUMS = (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)


def run_m2(lib, i, K, grads, weights=O.M2_W):
    B, _, N = i.seg_logits.shape
    a = O.m2_args(i)
    held = [devl(x) if j in (1, 6) else devn(x) for j, x in enumerate(a)]
    sc = scratch(O.M2_SCRATCH)
    losses = Out((12,))
    shapes = {"g_seg": (B, 2, N), "g_bc": (B, N, K), "g_mcls": (B, 2), "g_motion": (B, 4), "g_aux": (B, 4), "g_est": (B, 4),
              "g_prev": (B, 4)}
    on = {"g_seg": True, "g_bc": i.bc_pred is not None, "g_mcls": i.motion_cls is not None, "g_motion": True, "g_aux": True,
          "g_est": i.est is not None, "g_prev": i.prev is not None}
    g = {k: Out(shapes[k]) if grads and on[k] else None for k in O.M2_GRADS}
    rc = lib.o3d_m2track_loss(*[ptr(t) for t in held], B, N, K, *weights, 0.5, 2.0, sc.data_ptr(), losses.ptr,
                              *[optr(g[k]) for k in O.M2_GRADS], st())
    assert rc == 0
    torch.cuda.synchronize()
    tail_intact(sc)
    part = host(sc[:O.M2_SCRATCH]).reshape(O.LG, 16)
    assert np.isfinite(part).all(), "a row of the scratch was not written"
    assert not part[:, 13:].any()
    return O.Ref(partial=part, losses=losses.host(), **{k: None if o is None else o.host() for k, o in g.items()})


def check_m2(k, i, K, got, grads, draw, weights=O.M2_W, exact_grads=False):
    a = O.m2_args(i)
    B, _, N = i.seg_logits.shape
    r = O.m2_sums(*a)
    tot = got.partial.sum(0)[:13]
    for j, name in enumerate(O.M2_SUMS):
        ex = draw.exact and j in M2_EXACT_SUMS
        if ex:
            assert r.sums_abs[j] / O.m2_spacing(i)[j] < O.TWO24
        cmp("%s.sum.%s" % (k, name), tot[j], r.sums[j], r.sums_abs[j], r.sums_n[j], ex)
    f = O.m2_finish(tot, B, N, K, weights, i.bc_pred is not None, i.motion_cls is not None, i.state is not None,
                    i.est is not None, i.prev is not None)
    for j, name in enumerate(O.M2_LOSSES):
        cmp("%s.loss.%s" % (k, name), got.losses[j], f.losses[j], f.losses_abs[j], f.losses_n[j])
    if not grads:
        return
    g = O.m2_grads(*a, weights, tot)
    for name in O.M2_GRADS:
        if getattr(g, name) is None:
            assert getattr(got, name) is None
            continue
        ref, have = getattr(g, name), getattr(got, name)
        cmp("%s.%s" % (k, name), have, ref, getattr(g, name + "_abs"), getattr(g, name + "_n"))
        if exact_grads and name == "g_bc":
            cmp(k + ".g_bc", have, ref, None, None, True)
        if exact_grads and name in ("g_motion", "g_aux", "g_est", "g_prev"):
            cmp("%s.%s" % (k, name), have[:, :3], ref[:, :3], None, None, True)
            assert not have[:, 3].any()


def _m2(lib, draw, shape, flags=(1, 1, 1, 1), kind="plain", weights=O.M2_W, exact_grads=False, grads=True):
    B, N, K = shape
    i = O.m2_inputs(draw, B, N, K, flags, kind)
    got = run_m2(lib, i, K, grads, weights)
    check_m2("m2track_loss", i, K, got, grads, draw, weights, exact_grads)
    return i, got


def _m2_case(lib, case, exact, **kw):
    seed, shape, flags, kind = case
    return _m2(lib, O.Dyadic(seed) if exact else Randn(seed), shape, flags, kind, **kw)


@pytest.mark.parametrize("k", range(4), ids=[str(s) for s in O.M2_SHAPES])
@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounded"))
def test_m2track_loss(lib, k, exact):
    _m2_case(lib, (O.M2_EXACT if exact else O.M2_ROUNDED)[k], exact)


@pytest.mark.parametrize("k", range(16), ids=["bc%d_cls%d_est%d_prev%d" % f for f in O.M2_FLAGS])
def test_m2track_loss_every_combination_of_the_optional_terms(lib, k):
    assert O.M2_EXACT[4 + k][2] == O.M2_ROUNDED[4 + k][2] == O.M2_FLAGS[k]
    _m2_case(lib, O.M2_EXACT[4 + k], True)
    _m2_case(lib, O.M2_ROUNDED[4 + k], False)


@pytest.mark.parametrize("case", O.M2_EXACT_GRADS, ids=str)
def test_m2track_loss_exact_gradients(lib, case):
    """B and B*N*K powers of two, w_center = 3, w_bc = 2, no motion state: every constant in front of a clamp is a power of two"""
    _m2_case(lib, case, True, weights=O.M2_W_EXACT, exact_grads=True)


def test_m2track_loss_odd_n_without_boxcloud(lib):
    _m2_case(lib, O.M2_EXACT[20], True)
    _m2_case(lib, O.M2_ROUNDED[20], False)


def test_m2track_loss_no_moving_sample(lib):
    """the 1e-6 of the moving count alone: the motion pair's losses and g_motion are 0"""
    i, got = _m2_case(lib, O.M2_ROUNDED[21], False)
    assert got.losses[8] == 0 and got.losses[10] == 0 and not got.g_motion.any()


def test_m2track_loss_labels_that_are_not_one(lib):
    """labels 2, -1 and states 3, -5 are class 1: the same bits as with 1 in their place"""
    i, got = _m2_case(lib, O.M2_ROUNDED[22], False)
    assert (np.abs(i.seg_label) > 1).any() or (i.seg_label < 0).any()
    i.seg_label, i.state = (i.seg_label != 0).astype(np.int64), (i.state != 0).astype(np.int64)
    ones = run_m2(lib, i, 9, True)
    assert np.array_equal(ones.partial, got.partial) and np.array_equal(ones.losses, got.losses)
    assert all(np.array_equal(getattr(ones, k), getattr(got, k)) for k in O.M2_GRADS)


def test_m2track_loss_losses_only(lib):
    i, got = _m2_case(lib, O.M2_ROUNDED[23], False)
    only = run_m2(lib, i, 9, False)
    check_m2("m2track_loss", i, 9, only, False, Randn(0))
    assert np.array_equal(only.partial, got.partial) and np.array_equal(only.losses, got.losses)


# ---- o3d_adam_step ------------------------------------------------------------------------------------------------------
class AdamRun:
    """the jobs of O.ADAM_JOBS laid into the flat buffers in the order O.ADAM_ORDER with gaps of sentinels between them; the
    gradients in one buffer of their own at odd element offsets (4-byte aligned, no more)"""

    def __init__(self, jobs):
        self.sizes = [len(j[0]) for j in jobs]
        self.off, pos = {}, O.ADAM_GAP
        for j in O.ADAM_ORDER:
            self.off[j] = pos
            pos += self.sizes[j] + O.ADAM_GAP
        self.total = pos
        self.P, self.M, self.V = (outbuf((self.total,))[0] for _ in range(3))
        self.goff, gpos = [], 1
        for n in self.sizes:
            self.goff.append(gpos)
            gpos += n + n % 2 + 2
        self.G = nanbuf((gpos,))
        assert self.G.data_ptr() % 256 == 0 and all(o % 2 == 1 for o in self.goff)
        for j, (p, m, v, g) in enumerate(jobs):
            sl = slice(self.off[j], self.off[j] + self.sizes[j])
            self.P[sl], self.M[sl], self.V[sl] = dev(p), dev(m), dev(v)
        self.set_grads([j[3] for j in jobs])
        tab = [[self.G.data_ptr() + 4 * self.goff[j], self.off[j], n] for j, n in enumerate(self.sizes)]
        self.tab = torch.tensor(tab, dtype=torch.int64).cuda()

    def set_grads(self, gs):
        for j, g in enumerate(gs):
            self.G[self.goff[j]:self.goff[j] + self.sizes[j]] = dev(g)

    def step(self, lib, lr, beta1, beta2, eps, wd, bc1, bc2):
        assert lib.o3d_adam_step(self.tab.data_ptr(), len(self.sizes), self.P.data_ptr(), self.M.data_ptr(), self.V.data_ptr(),
                                 lr, beta1, beta2, eps, wd, bc1, bc2, st()) == 0
        torch.cuda.synchronize()

    def read(self):
        """-> [(p, m, v)] per job, after checking the gaps and the tails"""
        out = []
        live = torch.zeros(self.total + TAIL, dtype=torch.bool, device="cuda")
        for j, n in enumerate(self.sizes):
            live[self.off[j]:self.off[j] + n] = True
        for buf in (self.P, self.M, self.V):
            assert untouched(buf[~live]), "write into a gap between the jobs or beyond the buffer"
        for j, n in enumerate(self.sizes):
            sl = slice(self.off[j], self.off[j] + n)
            out.append(tuple(host(b[sl]) for b in (self.P, self.M, self.V)))
        return out


def adam_exact_jobs(wd):
    jobs = []
    for k, n in enumerate(O.ADAM_JOBS):
        draw = O.Dyadic(6000 + k)
        e = np.abs(draw.val((n,), 1.0, 1.0 if wd else 3.0))
        g = O._signs(draw, (n,)) * 2.0 ** e
        m = draw.val((n,), 0.25, 4.0)
        if wd:       # p a multiple of g / wd: the effective gradient g + wd p is again a power of two
            p = g / wd * O._pick(draw, (0.0, 1.0, 3.0), (n,))
        else:
            p = draw.val((n,), 0.125, 4.0)
        ge = g + wd * p
        v = np.where(draw.val((n,), 1.0, 1.0) > 0, ge * ge, 0.0)
        jobs.append((p, m, v, g))
    return jobs


@pytest.mark.parametrize("wd", (0.0, 0.125))
def test_adam_step_exact(lib, wd):
    from open3dsot_amd import build
    assert not any(("correctly-rounded" in f and "no-" in f) or "fast-math" in f or f in ("-Ofast", "-freciprocal-math",
                                                                                          "-funsafe-math-optimizations")
                   for f in build.COMMON), "the build no longer keeps the correctly rounded fp32 divide and sqrt"
    jobs = adam_exact_jobs(wd)
    run = AdamRun(jobs)
    run.step(lib, wd=wd, **O.ADAM_EXACT)
    for j, ((p, m, v, g), (gp, gm, gv)) in enumerate(zip(jobs, run.read())):
        r = O.adam_step(p, m, v, g, wd=wd, **O.ADAM_EXACT)
        cmp("adam.m", gm, r.m, None, None, True)
        cmp("adam.v", gv, r.v, None, None, True)
        cmp("adam.p", gp, r.p, None, None, True)


@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_adam_step_rounded_two_steps(lib, wd):
    """|g| in [1e-15, 1e15] (odd jobs spread over that range, even jobs of order 1): denormals and overflow are out of reach.
    Elements [0, n/8) of every job have g = 0, m = 0, v = 0 and wd p is added to a zero gradient: with wd = 0 the parameter
    keeps its bits.  The second step runs on the first's output with a new gradient and the bias corrections of t = 2."""
    h = O.ADAM_ROUNDED
    jobs = [O.adam_inputs(Randn(600 + k), n, k) for k, n in enumerate(O.ADAM_JOBS)]
    run = AdamRun(jobs)
    state = [(f32(p), f32(m), f32(v)) for p, m, v, _ in jobs]
    grads = [f32(j[3]) for j in jobs]
    for t in (1, 2):
        bc1, bc2 = 1 - h["beta1"] ** t, 1 - h["beta2"] ** t
        run.step(lib, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, bc1, bc2)
        got = run.read()
        for j, ((p, m, v), g, (gp, gm, gv)) in enumerate(zip(state, grads, got)):
            assert (np.abs(g[g != 0]) >= 1e-15).all() and (np.abs(g) <= 1e15).all()
            r = O.adam_moments(m, v, g, p, h["beta1"], h["beta2"], wd)
            cmp("adam.m", gm, r.m, r.m_abs, r.m_n)
            cmp("adam.v", gv, r.v, r.v_abs, r.v_n)
            u = O.adam_update(p, gm, gv, h["lr"], h["eps"], bc1, bc2)
            cmp("adam.p", gp, u.p, u.p_abs, u.p_n)
            z = len(p) // 8
            if wd == 0.0 and t == 1 and z:
                assert np.array_equal(bits(gp[:z]), bits(p[:z])), "g = 0, v = 0: the parameter moved"
        state = got
        grads = [f32(O.adam_inputs(Randn(650 + k), n, k)[3]) for k, n in enumerate(O.ADAM_JOBS)]
        run.set_grads(grads)


def f32(a):
    return O.f32(a)


# ---- o3d_best_proposal ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", O.BEST_KINDS)
def test_best_proposal(lib, kind):
    """the FIRST maximum, and the four box values of that row bit for bit; the same with out_idx == NULL"""
    for B in O.BEST_B:
        for P in O.BEST_P:
            draw = O.Dyadic(7000 + 10 * B + P)
            boxes = draw.val((B, P, 5), 0.125, 8.0)
            boxes[:, :, 4] = O.best_scores(kind, B, P, draw)
            r = O.best_proposal(boxes)
            src = nanbuf((B * P * 5 + 64,))
            src[:B * P * 5] = dev(boxes).reshape(-1)
            out, out2 = Out((B, 4)), Out((B, 4))
            iflat, idx = ibuf((B,))
            assert lib.o3d_best_proposal(src.data_ptr(), B, P, out.ptr, idx.data_ptr(), st()) == 0
            assert lib.o3d_best_proposal(src.data_ptr(), B, P, out2.ptr, None, st()) == 0
            torch.cuda.synchronize()
            tail_intact(iflat)
            assert np.array_equal(idx.cpu().numpy(), r.idx), (kind, B, P, idx.cpu().numpy()[:4], r.idx[:4])
            assert np.array_equal(out.bits(), bits(r.out)) and np.array_equal(out2.bits(), bits(r.out)), (kind, B, P)


# ---- the vote head's glue ------------------------------------------------------------------------------------------------
def strided(a, layout):
    """a (B,C,N) on the device as a view into a NaN-filled buffer -> (buffer to hold, pointer, sb, sc, sn)
    layout "slice": channels 2.. of a (B, C + 4, N + 3) tensor; "permuted": a (B, N, C + 2) tensor seen as (B, C, N);
    "step2": every second point of a (B, C, 2 N) tensor"""
    B, C, N = a.shape
    t = dev(a)
    if layout == "slice":
        buf = nanbuf((B, C + 4, N + 3))
        view = buf[:, 2:2 + C, :N]
    elif layout == "permuted":
        buf = nanbuf((B, N, C + 2))
        view = buf[:, :, :C].permute(0, 2, 1)
    elif layout == "step2":
        buf = nanbuf((B, C, 2 * N))
        view = buf[:, :, ::2]
    else:
        buf = nanbuf((B, C, N))
        view = buf
    view.copy_(t)
    return buf, view.data_ptr(), view.stride(0), view.stride(1), view.stride(2)


def _draw(exact, seed):
    return O.Dyadic(seed) if exact else Randn(seed)


def _val(draw, shape):
    return draw.val(shape, 0.25, 4.0)


@pytest.mark.parametrize("layout", ("slice", "permuted"))
@pytest.mark.parametrize("shape", O.RPN_SHAPES, ids=str)
@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounded"))
def test_rpn_votes_fwd(lib, shape, layout, exact):
    B, N, f = shape
    draw = _draw(exact, 800 + N)
    cla, vote = 2.0 * _val(draw, (B, 1, N)), _val(draw, (B, 3 + f, N))
    r = O.rpn_votes_fwd(cla[:, 0], vote)
    cb, cp, csb, _, csn = strided(cla, "step2")
    vb, vp, vsb, vsc, vsn = strided(vote, layout)
    score, vxyz, vfeat = Out((B, N)), Out((B, N, 3)), Out((B, 1 + f, N))
    assert lib.o3d_rpn_votes_fwd(cp, csb, csn, vp, vsb, vsc, vsn, B, N, f, score.ptr, vxyz.ptr, vfeat.ptr, st()) == 0
    torch.cuda.synchronize()
    cmp("rpn_votes_fwd.score", score.host(), r.score, r.score_abs, r.score_n)
    assert np.array_equal(vfeat.bits()[:, 0], score.bits()), "the score row of vote_feature is not the score"
    assert np.array_equal(vfeat.bits()[:, 1:], bits(vote[:, 3:])) and np.array_equal(vxyz.bits(), bits(r.vote_xyz))


@pytest.mark.parametrize("null", ("none", "dvf", "dvx", "both"))
@pytest.mark.parametrize("shape", O.RPN_SHAPES, ids=str)
@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounded"))
def test_rpn_votes_bwd(lib, shape, null, exact):
    """dvf as a channel slice of a wider tensor, dvx as the permuted (B,N,3) view; a NULL gradient is zeros"""
    B, N, f = shape
    draw = _draw(exact, 820 + N)
    s = f32(O.sigmoid(2.0 * _val(draw, (B, N))))
    dvf = None if null in ("dvf", "both") else _val(draw, (B, 1 + f, N))
    dvx = None if null in ("dvx", "both") else _val(draw, (B, 3, N))
    r = O.rpn_votes_bwd(s, dvf, dvx, f)
    sd = dev(s)
    fb, fp, fsb, fsc, fsn = strided(dvf, "slice") if dvf is not None else (None, None, 0, 0, 0)
    xb, xp, xsb, xsc, xsn = strided(dvx, "permuted") if dvx is not None else (None, None, 0, 0, 0)
    dcla, dvote = Out((B, N)), Out((3 + f, B * N))
    assert lib.o3d_rpn_votes_bwd(sd.data_ptr(), fp, fsb, fsc, fsn, xp, xsb, xsc, xsn, B, N, f, dcla.ptr, dvote.ptr, st()) == 0
    torch.cuda.synchronize()
    cmp("rpn_votes_bwd.dcla", dcla.host(), r.dcla, r.dcla_abs, r.dcla_n)
    assert np.array_equal(dvote.bits(), bits(r.dvote))
    if dvf is None:
        assert not dcla.host().any()


@pytest.mark.parametrize("layout", ("slice", "permuted"))
@pytest.mark.parametrize("shape", O.ASSEMBLE_SHAPES, ids=str)
@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounded"))
def test_box_assemble(lib, shape, layout, exact):
    B, P = shape
    draw = _draw(exact, 840 + P)
    off, ctr = _val(draw, (B, 5, P)), _val(draw, (B, P, 3))
    r = O.box_assemble(off, ctr)
    ob, op, osb, osc, osn = strided(off, layout)
    cd = dev(ctr)
    boxes = Out((B, P, 5))
    assert lib.o3d_box_assemble(op, osb, osc, osn, cd.data_ptr(), B, P, boxes.ptr, st()) == 0
    torch.cuda.synchronize()
    cmp("box_assemble.boxes", boxes.host(), r.boxes, r.boxes_abs, r.boxes_n, exact)
    want = np.asarray(off, np.float32).transpose(0, 2, 1).copy()
    want[:, :, :3] = want[:, :, :3] + np.asarray(ctr, np.float32)
    assert np.array_equal(boxes.bits(), want.view(np.int32))


# ---- o3d_motion_merge_fwd / _bwd, o3d_offset_box ------------------------------------------------------------------------------
def wide_points(pts):
    """xyz as channels 0..2 of a (B, 5, N) tensor whose other channels hold NaN"""
    B, _, N = pts.shape
    buf = nanbuf((B, 5, N))
    buf[:, :3] = dev(pts)
    return buf, 5 * N, N


@pytest.mark.parametrize("with_prev", (True, False), ids=("prev", "noprev"))
@pytest.mark.parametrize("N", O.MERGE_N)
@pytest.mark.parametrize("B", O.MERGE_B)
@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounded"))
def test_motion_merge_fwd(lib, B, N, with_prev, exact):
    i = O.merge_inputs(_draw(exact, 900 + N + B), B, N, zero_angles=exact)
    prev = i.prev if with_prev else None
    r = O.motion_merge_fwd(i.pts, prev, i.motion)
    buf, bs, cs = wide_points(i.pts)
    pd, md = devn(prev), dev(i.motion)
    merged, aux = Out((B, 3, N)), Out((B, 4))
    assert lib.o3d_motion_merge_fwd(buf.data_ptr(), bs, cs, ptr(pd), md.data_ptr(), B, N, merged.ptr, aux.ptr, st()) == 0
    torch.cuda.synchronize()
    cmp("motion_merge_fwd.merged", merged.host(), r.merged, r.merged_abs, r.merged_n, exact)
    cmp("motion_merge_fwd.aux", aux.host(), r.aux, r.aux_abs, r.aux_n, exact)


@pytest.mark.parametrize("with_prev", (True, False), ids=("prev", "noprev"))
@pytest.mark.parametrize("with_gprev", (True, False), ids=("gprev", "nogprev"))
@pytest.mark.parametrize("with_gaux", (True, False), ids=("gaux", "nogaux"))
@pytest.mark.parametrize("N", O.MERGE_N)
@pytest.mark.parametrize("B", O.MERGE_B)
@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounded"))
def test_motion_merge_bwd(lib, B, N, with_gaux, with_gprev, with_prev, exact):
    """prev = NULL stands for a previous box of zeros: g_prev, when asked for, is the gradient at those zeros"""
    i = O.merge_inputs(_draw(exact, 950 + N + B), B, N, zero_angles=exact)
    prev = i.prev if with_prev else None
    g_aux = i.g_aux if with_gaux else None
    r = O.motion_merge_bwd(i.pts, prev, i.motion, i.g, g_aux)
    buf, bs, cs = wide_points(i.pts)
    pd, md, gd, gad = devn(prev), dev(i.motion), dev(i.g), devn(g_aux)
    g_prev, g_motion = (Out((B, 4)) if with_gprev else None), Out((B, 4))
    assert lib.o3d_motion_merge_bwd(buf.data_ptr(), bs, cs, ptr(pd), md.data_ptr(), B, N, gd.data_ptr(), ptr(gad), optr(g_prev),
                                    g_motion.ptr, st()) == 0
    torch.cuda.synchronize()
    cmp("motion_merge_bwd.g_motion", g_motion.host(), r.g_motion, r.g_motion_abs, r.g_motion_n, exact)
    if with_gprev:
        cmp("motion_merge_bwd.g_prev", g_prev.host(), r.g_prev, r.g_prev_abs, r.g_prev_n, exact)


@pytest.mark.parametrize("B", O.OFFSET_B)
@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounded"))
def test_offset_box(lib, B, exact):
    """forward; backward with g_ref only, with g_off only and with both: what a launch writes does not depend on the other"""
    i = O.offset_inputs(_draw(exact, 980 + B), B, zero_angles=exact)
    f, b = O.offset_box(i.ref, i.off), O.offset_box_bwd(i.ref, i.off, i.g)
    rd, od, gd = devs(i.ref, i.off, i.g)
    box = Out((B, 4))
    assert lib.o3d_offset_box(rd.data_ptr(), od.data_ptr(), B, box.ptr, None, None, None, st()) == 0
    torch.cuda.synchronize()
    cmp("offset_box.box", box.host(), f.box, f.box_abs, f.box_n, exact)
    seen = {}
    for want_ref, want_off in ((True, False), (False, True), (True, True)):
        g_ref, g_off, nobox = (Out((B, 4)) if want_ref else None), (Out((B, 4)) if want_off else None), Out((B, 4))
        assert lib.o3d_offset_box(rd.data_ptr(), od.data_ptr(), B, nobox.ptr, gd.data_ptr(), optr(g_ref), optr(g_off), st()) == 0
        torch.cuda.synchronize()
        assert nobox.untouched(), "the backward wrote the forward's output"
        for name, o in (("g_ref", g_ref), ("g_off", g_off)):
            if o is None:
                continue
            cmp("offset_box." + name, o.host(), getattr(b, name), getattr(b, name + "_abs"), getattr(b, name + "_n"), exact)
            assert np.array_equal(seen.setdefault(name, o.bits()), o.bits())
