"""The GEMM launches of the fused operators: the ONE place that maps a GEMM shape to a C entry of csrc/mlp_direct.hip /
csrc/mlp_wgrad.hip / csrc/mlp.hip, to the statistics partial rows that entry writes, to its weight-gradient scratch and to
the launch's row in `fused.profile_step`'s roofline accounting.

One function per launch kind and layout -- flat (C, P) operands: `flat_fwd`, `flat_fwd_cloud`, `flat_dgrad`, `flat_wgrad`,
`flat_wgrad_job`; the compact (distinct-neighbour) layout of csrc/compact.hip: `compact_fwd`, `compact_dgrad`,
`compact_wgrad`, `compact_bwd_fused`.  Each returns a `Launch`: the (name, flops, entry, args, dims) description
`fused_heads._drive` consumes, plus `out` -- the `Partials` the launch writes (what `fused.bn_fin_job` / `bn_bwd_fin_job` are
handed: tensor, rows per segment, live-row rule), or the scratch a weight gradient needs alive until it has been issued.
`issue(launch)` launches at once and returns `out`; a generator of the heads yields the launch instead.
The compact launchers take the layout as a `Compact`: the one record of its sizes and tensors, which also builds it.

`family` names the roofline family of the caller: "pw" (1-D conv stacks: pw_conv_*), "grouped" (positions of a grouped
MLP: conv_*), "points" (its per-point layer 0: conv_*_points).
"""
import collections
import ctypes

import torch

from . import capi

TILE = 128   # point columns are padded to this (the widest wave tile of the GEMM kernels, csrc/mlp_direct.hip)

# ---- optional per-kernel timing (bench.py's roofline leg) ---------------------------------
_PROF = {"on": False, "events": []}


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, flops, fn, *args, dims=None):
    """Launch one C-ABI entry; when profiling, bracket it with HIP events on the launch stream.
    dims = (Cin, Cout[, pooled]) of a GEMM launch: only used for the per-launch roofline table of `profile_step`."""
    if _PROF["on"]:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        _PROF["events"].append((name, flops, e0, e1, dims))
    else:
        rc = fn(*args)
    capi.check(rc, name)


def _up(v, m):
    return -(-v // m) * m


def _const_vec(dev, n, value):
    key = (str(dev), n, value)
    v = _CONST.get(key)
    if v is None:
        v = _CONST[key] = torch.full((n,), float(value), device=dev, dtype=torch.float32)
    return v


_CONST = {}

Launch = collections.namedtuple("Launch", "name flops entry args dims out")
# statistics partials of a launch: part (sum(rows), 2, C); rows: one count per segment; live: () = every row is live, or
# (meta, tile) = compact layout, ceil(meta[4 * s] / tile) rows of a segment are (the trailing arguments of fused.bn_fin_job)
Partials = collections.namedtuple("Partials", "part rows live")


def issue(la):
    _call(la.name, la.flops, getattr(capi.load(), la.entry), *la.args, dims=la.dims)
    return la.out


class Layer:
    """a layer's raw output Y with its BatchNorm constants vec (4, [nseg,] C) = mean, invstd, scale, shift: the consumer
    applies BatchNorm + ReLU while loading.  vec None: an operand that is read as stored"""
    __slots__ = ("Y", "vec")

    def __init__(self, Y, vec=None):
        self.Y, self.vec = Y, vec

    mean = property(lambda self: self.vec[0])
    invstd = property(lambda self: self.vec[1])
    scale = property(lambda self: self.vec[2])
    shift = property(lambda self: self.vec[3])

    def consts(self):
        """(scale, shift, mean) pointers, NULL for an operand read as stored"""
        return (None, None, None) if self.vec is None else (self.vec[2].data_ptr(), self.vec[3].data_ptr(), self.vec[0].data_ptr())


class Grad:
    """gradient source of a backward launch, dY = A1 * dN + A2 * Y + A3 (A: the three pointers of `fused.bn_bwd_coef`) with
    dN dense, or the packed {masked gradient, arg-max slot} pairs `pk` of a max over `ns` columns instead of dN.
    light: the per-launch roofline table charges no Y row for this source"""
    __slots__ = ("dN", "Y", "A", "pk", "ns", "unpacked", "light")

    def __init__(self, dN, Y, A, light=False):
        self.dN, self.Y, self.A, self.pk, self.ns, self.unpacked, self.light = dN, Y, A, None, 4, (None, None, None), light

    @classmethod
    def plain(cls, dN):
        """dY = dN: Y is dN, A1 = ones, A2 = A3 = zeros over dN's rows (entries that take a NULL Y instead get that)"""
        one, zero = _const_vec(dN.device, dN.shape[0], 1.0), _const_vec(dN.device, dN.shape[0], 0.0)
        return cls(dN, dN, (one.data_ptr(), zero.data_ptr(), zero.data_ptr()), light=True)

    @classmethod
    def pooled(cls, pk, ns, Y, A, unpacked=(None, None, None), light=False):
        """unpacked: (dOut, out, arg) of the pool as well, for the entry that still takes them (the xcorr stage hands them
        over and counts the source as light; the per-point stacks do neither)"""
        g = cls(None, Y, A, light)
        g.pk, g.ns, g.unpacked = pk, ns, unpacked
        return g


def _name(family, kind):
    return {"pw": "pw_conv_%s", "grouped": "conv_%s", "points": "conv_%s_points"}[family] % kind


def _dims(Cin, Cout, light=False):
    return (Cin, Cout, True) if light else (Cin, Cout)


def _partials(rows, C, like):
    return Partials(torch.empty((rows, 2, C), device=like.device, dtype=torch.float32), [rows], ())


def _pw_tile(lib, M, K, P):
    """the wave tile of the flat-layout entry points of csrc/mlp_direct.hip (o3d_pw_fwd / o3d_pw_dgrad), which they pick from
    the size of the launch -- and with it the number of statistics partial rows, P // tile; 0: they do not take the shape"""
    tile = lib.o3d_pw_tile(P, M)
    return tile if M % 64 == 0 and K % 16 == 0 and P % tile == 0 else 0


# ---- flat layout ------------------------------------------------------------------------------------------------------
def flat_fwd(family, src, W, Cin, Cout, P, Y, stat_c=None, bias=None, resid=None, tile128=False, kind="fwd", row=True):
    """Y (Cout, P) = W . f(src) (+ bias + resid), src a `Layer`.  stat_c (the shift of the second moment): the launch also
    writes statistics partials -> out.  o3d_pw_fwd where it takes the shape, else the B = 1 form of o3d_mlp_conv_fwd, whose
    statistics tiles are 128 columns; tile128: that entry whatever the shape (the per-point layer 0 of the grouped MLPs).
    kind "dgrad": a plain data gradient W^T . S run -- and accounted -- as a forward GEMM; row False: no row in the
    per-launch roofline table"""
    lib = capi.load()
    sc, sh, _ = src.consts()
    head = (_name(family, kind), 2.0 * Cin * Cout * P)
    dims = _dims(Cin, Cout) if row else None
    tile = 0 if tile128 else _pw_tile(lib, Cout, Cin, P)
    p = _partials(P // (tile or TILE), Cout, Y) if stat_c is not None else None
    if tile:
        return Launch(*head, "o3d_pw_fwd", [src.Y.data_ptr(), W.data_ptr(), sc, sh, _ptr(bias), _ptr(resid), Cin, Cout, P,
                                            Y.data_ptr(), _ptr(p and p.part), _ptr(stat_c), _stream()], dims, p)
    assert bias is None and resid is None
    return Launch(*head, "o3d_mlp_conv_fwd", [src.Y.data_ptr(), W.data_ptr(), sc, sh, 1, Cin, Cout, P, Y.data_ptr(),
                                              _ptr(p and p.part), _ptr(stat_c), _stream()], dims, p)


def flat_fwd_cloud(X, W, cbias, B, N, Cin, Cout, Y, stat_c=None):
    """Y (Cout, B*N) = W . X + cbias[:, cloud of the column] (the per-cloud bias of fused_pointwise.chain_cloud); 128-column
    statistics tiles"""
    p = _partials(B * N // TILE, Cout, Y) if stat_c is not None else None
    return Launch("pw_conv_fwd", 2.0 * Cin * Cout * B * N, "o3d_pw_fwd_cloud",
                  [X.data_ptr(), W.data_ptr(), cbias.data_ptr(), B, N, Cin, Cout, Y.data_ptr(), _ptr(p and p.part), _ptr(stat_c),
                   _stream()], _dims(Cin, Cout), p)


def flat_dgrad(family, g, Wt, Cin, Cout, P, dst, prev=None, W=None, resid=None, staged=False, row=True):
    """dst (Cin, P) = W^T . dY of the `Grad` g.  prev (the producer's `Layer`): masked by its ReLU, BatchNorm-backward
    partials of the producer -> out; prev None: the gradient of an operand that is no BN + ReLU output (+ resid).
    A packed source runs o3d_mlp_conv_dgrad_wt (128-column tiles); a dense one o3d_pw_dgrad where it takes the shape, else
    o3d_mlp_conv_dgrad_wt.  staged: the LDS-staged o3d_mlp_conv_dgrad_plain (reads W, not Wt; prev None only)"""
    lib = capi.load()
    head = (_name(family, "dgrad"), 2.0 * Cin * Cout * P)
    dims = _dims(Cin, Cout, g.light) if row else None
    if staged:
        return Launch(*head, "o3d_mlp_conv_dgrad_plain", [g.dN.data_ptr(), g.Y.data_ptr(), *g.A, W.data_ptr(), 1, Cin, Cout, P,
                                                          dst.data_ptr(), _stream()], dims, None)
    pv = prev if prev is not None else Layer(None)
    tile = _pw_tile(lib, Cin, Cout, P) if g.pk is None else 0
    p = _partials(P // (tile or TILE), Cin, dst) if prev is not None else None
    sc, sh, mean = pv.consts()
    if tile:
        Y, A = (None, (None, None, None)) if g.Y is g.dN else (g.Y.data_ptr(), g.A)
        return Launch(*head, "o3d_pw_dgrad", [g.dN.data_ptr(), Y, *A, Wt.data_ptr(), Cin, Cout, P, _ptr(pv.Y), sc, sh, mean,
                                              _ptr(resid), dst.data_ptr(), _ptr(p and p.part), _stream()], dims, p)
    assert resid is None and prev is not None
    return Launch(*head, "o3d_mlp_conv_dgrad_wt",
                  [_ptr(g.dN), *[_ptr(t) for t in g.unpacked], g.ns, g.Y.data_ptr(), *g.A, W.data_ptr(), Wt.data_ptr(),
                   _ptr(g.pk), 1, Cin, Cout, P, pv.Y.data_ptr(), sc, sh, mean, dst.data_ptr(), p.part.data_ptr(), _stream()],
                  dims, p)


def _wgrad2_scratch(lib, Cin, Cout, P, like):
    return torch.empty((lib.o3d_mlp_conv_wgrad2_scratch(1, Cin, Cout, P),), device=like.device, dtype=torch.float32)


def flat_wgrad(family, g, src, Cin, Cout, P, dW, row=True):
    """dW (Cout, Cin) = dY . f(src)^T.  Aligned shapes run the tile-matched MFMA kernel (o3d_mlp_conv_wgrad2), the rest the
    generic one, split over `nsl` slices of the columns; out: the scratch (alive until the launch is issued)"""
    lib = capi.load()
    sc, sh, _ = src.consts()
    head = (_name(family, "wgrad"), 2.0 * Cin * Cout * P)
    if Cin % 64 == 0 and Cout % 64 == 0:
        scratch = _wgrad2_scratch(lib, Cin, Cout, P, dW)
        return Launch(*head, "o3d_mlp_conv_wgrad2", [_ptr(g.dN), _ptr(g.pk), g.ns, g.Y.data_ptr(), *g.A, src.Y.data_ptr(), sc, sh,
                                                     1, Cin, Cout, P, scratch.data_ptr(), dW.data_ptr(), _stream()],
                      _dims(Cin, Cout, g.light) if row else None, scratch)
    tiles = ((Cin + 127) // 128) * ((Cout + 127) // 128)
    nsl = max(1, min(P // 32 // 4, 768 // tiles))
    scratch = torch.empty((nsl + 16, Cout, Cin), device=dW.device, dtype=torch.float32)
    # (the per-point layer 0 on the generic kernel has never had a row in the per-launch table)
    return Launch(*head, "o3d_mlp_conv_wgrad", [g.dN.data_ptr(), None, None, None, 4, g.Y.data_ptr(), *g.A, src.Y.data_ptr(), sc, sh,
                                                1, Cin, Cout, P, nsl, scratch.data_ptr(), dW.data_ptr(), _stream()],
                  _dims(Cin, Cout) if row and family != "points" else None, scratch)


# ---- grouped weight gradients: ONE launch (+ one reduction launch) for up to 8 jobs (csrc/mlp_wgrad.hip::wgrad2_group_kernel)
_WgradJob = capi.struct("o3d_wgrad_job")
_MAXJOBS = 8                # WG_MAXJOBS of csrc/mlp_wgrad.hip


def flat_wgrad_job(g, src, Cin, Cout, P, dW, out=(0, 0)):
    """the `flat_wgrad` of an aligned shape as a job of the grouped launch: (flops, o3d_wgrad_job fields), scratch.  out:
    dW is the compact (out_rows, out_cols) top-left block of the (Cout, Cin) gradient"""
    sc, sh, _ = src.consts()
    scratch = _wgrad2_scratch(capi.load(), Cin, Cout, P, dW)
    return (2.0 * Cin * Cout * P, (g.dN.data_ptr(), g.Y.data_ptr(), *g.A, src.Y.data_ptr(), sc, sh, Cin, Cout, P,
                                   scratch.data_ptr(), dW.data_ptr(), *out)), scratch


def row_sum_job(G, rows, P, out):
    """out (rows) = row sums of G (rows, P) as a job of the grouped launch (the bias gradient of a stack's last layer)"""
    return (0.0, (G.data_ptr(), None, None, None, None, None, None, None, 0, rows, P, None, out.data_ptr(), 0, 0))


def flush_wgrad_jobs(jobs, st):
    for j0 in range(0, len(jobs), _MAXJOBS):
        chunk = jobs[j0:j0 + _MAXJOBS]
        arr = (_WgradJob * len(chunk))(*[_WgradJob(*j[1]) for j in chunk])
        _call("pw_conv_wgrad", sum(j[0] for j in chunk), capi.load().o3d_mlp_conv_wgrad2_group, ctypes.addressof(arr), len(chunk), st)


# ---- compact layout -----------------------------------------------------------------------------------------------------
class Compact:
    """The distinct-neighbour layout of csrc/compact.hip for one or two segments (sets of B clouds: the template and the
    search branch of a paired call): the ONE place that turns (B, ns, npoints, Ns) into its sizes, and the holder of its
    tensors.  Per segment (lists): npoints balls of ns slots per cloud, Ns points per cloud padded to Npads columns of the
    per-point operand, Pmaxs worst-case columns (every slot distinct), starts / pt_bases / ball_bases = first column / point
    column / ball id, nballs_s balls; start1 = first column of segment 1 (0: one segment); ldp / ldz / nballs = columns /
    point columns / balls of all segments.  Tensors (`tensors`: name -> (shape, dtype)): ball_cnt, ball_off per ball; gp
    (source point), cball (ball id), cw (weight) per column; meta: the live column counts, on the device; centers: the ball
    centres + the dummy ball of the padding columns (None without coordinates)."""

    def __init__(self, B, ns, npoints, Ns):
        self.B, self.ns, self.npoints, self.Ns, self.nseg = B, ns, list(npoints), list(Ns), len(npoints)
        nseg = self.nseg
        self.Npads = [_up(n, TILE) for n in self.Ns]
        self.nballs_s = [B * npt for npt in self.npoints]
        self.Pmaxs = [nb * ns for nb in self.nballs_s]
        self.starts = [0, self.Pmaxs[0]][:nseg]
        self.pt_bases = [0, B * self.Npads[0]][:nseg]
        self.ball_bases = [0, self.nballs_s[0]][:nseg]
        self.start1 = self.starts[1] if nseg == 2 else 0
        self.ldp, self.ldz, self.nballs = sum(self.Pmaxs), sum(B * n for n in self.Npads), sum(self.nballs_s)
        self.np1 = self.npoints[1] if nseg == 2 else 0            # (the pool entries' "no second segment")
        # B, nseg, npoint and point columns of the first and the last segment: the argument group of the reduce entries
        self.reduce_dims = (B, nseg, self.npoints[0], self.Npads[0], self.npoints[-1], self.Npads[-1])
        f32, i32 = torch.float32, torch.int32
        self.tensors = {"centers": ((self.nballs + 1, 3), f32), "ball_cnt": ((self.nballs,), i32),
                        "ball_off": ((self.nballs + 1,), i32), "gp": ((self.ldp,), i32), "cball": ((self.ldp,), i32),
                        "cw": ((self.ldp,), f32), "meta": ((nseg, 4), i32)}
        self.centers = self.ball_cnt = self.ball_off = self.gp = self.cball = self.cw = self.meta = None

    def fits(self, given, dev):
        """`given` (a dict) holds every tensor of the layout with the table's shape and dtype, contiguous, on `dev`"""
        return all(k in given and torch.is_tensor(given[k]) and tuple(given[k].shape) == sh and given[k].dtype == dt and
                   given[k].device == dev and given[k].is_contiguous() for k, (sh, dt) in self.tensors.items())

    def take(self, given):
        """hold the tensors of `given` (which `fits`) -> self"""
        for k in self.tensors:
            setattr(self, k, given[k])
        return self

    def alloc(self, dev, centers=True):
        """fresh tensors (centers: that one as well) -> self"""
        for k, (sh, dt) in self.tensors.items():
            if centers or k != "centers":
                setattr(self, k, torch.empty(sh, device=dev, dtype=dt))
        return self

    def build(self, idxs, st):
        """fill ball_cnt ... meta from the grouping indices idxs[s] (B, npoints[s], ns) int32: three launches"""
        lib = capi.load()
        out = [t.data_ptr() for t in (self.ball_cnt, self.ball_off, self.gp, self.cball, self.cw, self.meta)]
        if self.nseg == 2:
            _call("compact_build", 0.0, lib.o3d_compact_build2, idxs[0].data_ptr(), self.npoints[0], self.Npads[0],
                  idxs[1].data_ptr(), self.npoints[1], self.Npads[1], self.B, self.ns, self.start1, self.pt_bases[1], self.nballs,
                  *out, st)
        else:
            _call("compact_build", 0.0, lib.o3d_compact_build, idxs[0].data_ptr(), self.B, self.npoints[0], self.ns, self.Npads[0],
                  0, 0, 0, self.nballs, *out, st)

    def pooled(self, flat, C):
        """the segments' (B, C, npoint_s) blocks of a flat pooled buffer (nballs * C), back to back"""
        return [flat[b * C:(b + n) * C].view(self.B, C, npt) for b, n, npt in zip(self.ball_bases, self.nballs_s, self.npoints)]


_TAIL = {"on": True, "applied": -1}       # "on": False = no split (tools/ab_hook.py fused._TAIL.on flips it for the same-box A/B)


def set_tail_split(slots):
    """TEST hook for the remainder-tile split of the large GEMM launches: -1 automatic (default), 0 off, S > 0 pretend S
    resident slots (small problems then meet every branch of csrc/mlp_common.hpp::tail_plan)"""
    capi.load().o3d_direct_tail_override(int(slots))
    _TAIL["on"], _TAIL["applied"] = int(slots) != 0, int(slots)


def _compact_partials(lib, c, M, like):
    """(tile, Partials) of a direct GEMM launch with M output rows over the compact layout: one row per wave tile of
    o3d_direct_tile columns, and behind them the rows of a 128-column launch's remainder tiles cut into column blocks
    (csrc/mlp_common.hpp::tail_plan): one block of resident-slot size per segment"""
    tile = lib.o3d_direct_tile(c.ldp, M, 1)
    if not _TAIL["on"] and _TAIL["applied"] != 0:          # switched off through the dict (A/B tool): tell the library
        lib.o3d_direct_tail_override(0)
        _TAIL["applied"] = 0
    tail = len(c.Pmaxs) * lib.o3d_direct_tail_slots(M) if tile == 128 else 0
    part = torch.empty((c.ldp // tile + tail, 2, M), device=like.device, dtype=torch.float32)
    return tile, Partials(part, [pm // tile for pm in c.Pmaxs], (c.meta, tile))


def compact_fwd(c, src, W, Cin, Cout, Y, stat_c=None):
    """Y (Cout, ldp) = W . relu(bn(src)) on the live columns (layers >= 1 of a grouped MLP)"""
    lib = capi.load()
    tile, p = _compact_partials(lib, c, Cout, Y) if stat_c is not None else (lib.o3d_direct_tile(c.ldp, Cout, 1), None)
    sc, sh, _ = src.consts()
    return Launch("conv_fwd", (2.0 * Cin * Cout, c.meta, c.ldp), "o3d_mlp_conv_fwd_c",
                  [src.Y.data_ptr(), W.data_ptr(), sc, sh, Cin, Cout, c.ldp, c.cw.data_ptr(), c.meta.data_ptr(), c.start1, tile,
                   Y.data_ptr(), _ptr(p and p.part), _ptr(stat_c), _stream()], _dims(Cin, Cout), p)


def compact_dgrad(c, g, Wt, Cin, Cout, prev, dst):
    """dst (Cin, ldp) = W^T . dY masked by prev's ReLU, BatchNorm-backward partials of prev -> out"""
    tile, p = _compact_partials(capi.load(), c, Cin, dst)
    sc, sh, mean = prev.consts()
    return Launch("conv_dgrad", (2.0 * Cin * Cout, c.meta, c.ldp), "o3d_mlp_conv_dgrad_c",
                  [g.dN.data_ptr(), g.Y.data_ptr(), *g.A, Wt.data_ptr(), Cin, Cout, c.ldp, c.cw.data_ptr(), c.meta.data_ptr(),
                   c.start1, tile, prev.Y.data_ptr(), sc, sh, mean, dst.data_ptr(), p.part.data_ptr(), _stream()],
                  _dims(Cin, Cout), p)


def compact_wgrad(c, g, src, Cin, Cout, dW):
    """dW (Cout, Cin) = dY . relu(bn(src))^T over the live columns; executed FLOPs = per live column (count read back when
    profiling)"""
    scratch = _wgrad2_scratch(capi.load(), Cin, Cout, c.ldp, dW)
    sc, sh, _ = src.consts()
    return Launch("conv_wgrad", (2.0 * Cin * Cout, c.meta, c.ldp), "o3d_mlp_conv_wgrad2_c",
                  [g.dN.data_ptr(), g.Y.data_ptr(), *g.A, src.Y.data_ptr(), sc, sh, Cin, Cout, c.ldp, c.cw.data_ptr(),
                   c.meta.data_ptr(), c.start1, scratch.data_ptr(), dW.data_ptr(), _stream()], _dims(Cin, Cout), scratch)


# data + weight gradient of a 64-input-channel inner layer in ONE kernel (csrc/mlp_wgrad.hip::fused_bwd_kernel: SA level 0's
# 64 -> 64 and 64 -> 128 layers); wider outputs take the wgrad2 + direct-dgrad pair
FUSED_BWD_MAX_COUT = 128


def compact_bwd_fused(c, g, Wt, Cin, Cout, prev, dW, dst):
    """`compact_wgrad` + `compact_dgrad` in one launch, or None for a shape the kernel does not take.  out: partials of
    `rows` rows per segment block, all live"""
    lib = capi.load()
    rows = lib.o3d_mlp_conv_bwd_fused_rows(Cin, Cout, c.ldp) if Cout <= FUSED_BWD_MAX_COUT else -1
    if rows <= 0:
        return None
    scratch = torch.empty((lib.o3d_mlp_conv_bwd_fused_scratch(Cin, Cout, c.ldp),), device=dW.device, dtype=torch.float32)
    part = torch.empty((2, rows, 2, Cin), device=dW.device, dtype=torch.float32)
    sc, sh, mean = prev.consts()
    return Launch("conv_bwd_fused", (4.0 * Cin * Cout, c.meta, c.ldp), "o3d_mlp_conv_bwd_fused_c",
                  [g.dN.data_ptr(), g.Y.data_ptr(), *g.A, prev.Y.data_ptr(), sc, sh, mean, Wt.data_ptr(), Cin, Cout, c.ldp,
                   c.cw.data_ptr(), c.meta.data_ptr(), c.start1, scratch.data_ptr(), dW.data_ptr(), part.data_ptr(),
                   dst.data_ptr(), _stream()], _dims(Cin, Cout), (Partials(part, [rows] * len(c.Pmaxs), ()), scratch))
