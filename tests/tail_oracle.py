"""Plain numpy fp64 reference of the kernels at the tail of a training step and of a tracked frame -- no torch, no GPU:
csrc/loss.hip (o3d_track_loss, o3d_m2track_loss), the second half of csrc/heads.hip (o3d_adam_step, o3d_best_proposal,
o3d_rpn_votes_fwd / _bwd, o3d_box_assemble) and the motion / offset kernels of csrc/boxcloud.hip (o3d_motion_merge_fwd / _bwd,
o3d_offset_box).  One function per entry point, taking the arrays the C ABI takes; next to every value `x` it returns
`x_abs` = sum|t_i| of the terms that make it up and `x_n` = the number of roundings a value of the kernel passes through
(derived from the kernel's code in the docstring of tests/test_tail_kernels_gpu.py), the two figures of the bound
|err| <= (n + 8) * 2^-24 * sum|t_i|.  A transcendental f adds U[f] * 2^-24 * |f| at the place it enters; the allowance is
folded into `x_abs` as allow / (n + 8).  tests/test_tail_oracle_cpu.py ties every function to the torch modules the project
treats as specification.
"""
from types import SimpleNamespace as Ref

import numpy as np

from compact_oracle import Dyadic, TWO24  # noqa: F401  (re-exported for the tests)

E24 = 2.0 ** -24
# allowance of the device math library per function, in units of 2^-24 * |f|: twice the worst error, in fp32 ulp of the fp64
# value, of a sweep of about 10^6 fp32 arguments on an MI355X, rounded up (profiles/tail_kernel_pins.txt has the measured
# figures); an ulp is at most 2^-23 |f|, so the sweep's worst error is inside the allowance
U = {"exp": 2, "log1p": 2, "log": 4, "sin": 3, "cos": 4}
UT = max(U["sin"], U["cos"])
LG, LT = 64, 256                       # workgroups and threads of the two loss launches
TRACK_SCRATCH, M2_SCRATCH = LG * 8, LG * 16
TREE = 6 + 4                           # six butterfly steps of a wave, then the four wave rows of a workgroup
TOT = LG                               # the gradient kernel adds the LG stored rows one after the other


DT = [np.float64]


def f64(a):
    return None if a is None else np.asarray(a, DT[-1])


class precision:
    """with precision(np.float32): the formulas below run on float32 arrays (the CPU file's check of the bounds)"""

    def __init__(self, dt):
        self.dt = dt

    def __enter__(self):
        DT.append(self.dt)

    def __exit__(self, *exc):
        DT.pop()


def cdiv(a, b):
    return -(-a // b)


def sl1(d):
    a = np.abs(d)
    return np.where(a < 1.0, 0.5 * d * d, a - 0.5)


def clamp1(d):
    return np.clip(d, -1.0, 1.0)


def softplus_neg_abs(x):
    return np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def fold(abs_sum, n, allow):
    """sum|t_i| with the transcendental allowance (units of 2^-24) folded in: (n + 8) * e * result = the whole bound"""
    return abs_sum + allow / (np.asarray(n, np.float64) + 8)


# ---- o3d_track_loss -----------------------------------------------------------------------------------------------------
TRACK_SUMS = ("seg_count", "near_count", "mask_count", "seg_bce", "vote", "bc", "obj_bce", "box")
TRACK_LOSSES = ("total", "objective", "box", "seg", "vote", "bc")


def track_dist(centers, box_label):
    d = f64(centers) - f64(box_label)[:, None, :3]
    return np.sqrt((d * d).sum(-1) + 1e-6)


def track_sums(cla, seg, vote, box_label, centers, boxes, bc_pred, bc_label):
    """the 8 sums the first launch reduces -> sums, sums_abs, sums_n (8 each)"""
    cla, seg, vote, box_label, centers, boxes = map(f64, (cla, seg, vote, box_label, centers, boxes))
    B, N = cla.shape
    P = centers.shape[1]
    sp = softplus_neg_abs(cla)
    t3 = np.maximum(cla, 0) - cla * seg + sp
    a3 = fold(np.maximum(cla, 0) + np.abs(cla * seg) + sp, 3, U["exp"] * np.exp(-np.abs(cla)) + U["log1p"] * sp)
    t4 = sl1(vote - box_label[:, None, :3]).sum(-1) / 3.0 * seg
    if bc_pred is not None:
        K = bc_pred.shape[2]
        t5 = sl1(f64(bc_pred) - f64(bc_label)).sum(-1) / K * seg
    else:
        K, t5 = 0, np.zeros_like(seg)
    dist = track_dist(centers, box_label)
    near = f64(dist < 0.3)
    mask = np.minimum(near + f64(dist > 0.6), 1.0)
    x = boxes[:, :, 4]
    spx = softplus_neg_abs(x)
    t6 = (1 - near) * x + (1 + near) * (spx + np.maximum(-x, 0))
    a6 = fold((1 - near) * np.abs(x) + (1 + near) * (spx + np.maximum(-x, 0)), 4,
              (1 + near) * (U["exp"] * np.exp(-np.abs(x)) + U["log1p"] * spx))
    t7 = sl1(boxes[:, :, :4] - box_label[:, None, :]).sum(-1) * 0.25 * near
    ds, dp = cdiv(B * N, LG * LT) + TREE, cdiv(B * P, LG * LT) + TREE
    terms = (seg, near, mask, t3, t4, t5, t6, t7)
    absv = (np.abs(seg), near, mask, a3, np.abs(t4), np.abs(t5), a6, np.abs(t7))
    n = np.array([ds, dp, dp, ds + 3, ds + 10, ds + K + 8, dp + 4, dp + 8], np.float64)
    return Ref(sums=np.array([t.sum() for t in terms]), sums_abs=np.array([a.sum() for a in absv]), sums_n=n,
               dist=dist, near=near, mask=mask)


def track_finish(sums, nseed, nprop, weights, with_bc):
    """the 6 losses from the 8 sums (the second launch's head) -> losses, losses_abs, losses_n and the constants"""
    s = f64(sums)
    w_obj, w_box, w_seg, w_vote, w_bc = [float(w) for w in weights]
    inv_seg, inv_near = 1.0 / (s[0] + 1e-6), 1.0 / (s[1] + 1e-6)
    mask_ratio = s[2] / (s[2] + 1e-6)
    l_seg, l_vote = s[3] / nseed, s[4] * inv_seg
    l_bc = s[5] * inv_seg if with_bc else 0.0
    l_obj, l_box = s[6] / nprop * mask_ratio, s[7] * inv_near
    parts = np.array([l_obj * w_obj, l_box * w_box, l_seg * w_seg, l_vote * w_vote, l_bc * w_bc])
    losses = np.array([parts.sum(), l_obj, l_box, l_seg, l_vote, l_bc])
    labs = np.abs(losses)
    labs[0] = np.abs(parts).sum()
    n = np.array([TOT + 13, TOT + 4, TOT + 4, TOT + 2, TOT + 4, TOT + 4], np.float64)
    return Ref(losses=losses, losses_abs=labs, losses_n=n, inv_seg=inv_seg, inv_near=inv_near, mask_ratio=mask_ratio)


def track_grads(cla, seg, vote, box_label, centers, boxes, bc_pred, bc_label, weights, sums):
    """the four gradients of the weighted total, with the denominators taken from `sums`"""
    cla, seg, vote, box_label, centers, boxes = map(f64, (cla, seg, vote, box_label, centers, boxes))
    B, N = cla.shape
    P = centers.shape[1]
    w_obj, w_box, w_seg, w_vote, w_bc = [float(w) for w in weights]
    c = track_finish(sums, B * N, B * P, weights, bc_pred is not None)
    r = Ref()
    sig = sigmoid(cla)
    c_seg = w_seg / (B * N)
    r.g_cla, r.g_cla_n = c_seg * (sig - seg), 5
    r.g_cla_abs = fold(abs(c_seg) * (sig + np.abs(seg)), 5, abs(c_seg) * U["exp"] * sig * (1 - sig))
    c_vote = w_vote * c.inv_seg / 3.0
    r.g_vote = c_vote * seg[:, :, None] * clamp1(vote - box_label[:, None, :3])
    r.g_vote_abs, r.g_vote_n = np.abs(r.g_vote), 7
    if bc_pred is not None:
        c_bc = w_bc * c.inv_seg / bc_pred.shape[2]
        r.g_bc = c_bc * seg[:, :, None] * clamp1(f64(bc_pred) - f64(bc_label))
        r.g_bc_abs, r.g_bc_n = np.abs(r.g_bc), 8
    else:
        r.g_bc = r.g_bc_abs = None
    near = f64(track_dist(centers, box_label) < 0.3)
    c_obj, c_box = w_obj * c.mask_ratio / (B * P), w_box * c.inv_near * 0.25
    sx = sigmoid(boxes[:, :, 4])
    r.g_boxes = np.empty_like(boxes)
    r.g_boxes_abs = np.empty_like(boxes)
    r.g_boxes_n = np.array([7, 7, 7, 7, 9], np.float64)
    r.g_boxes[:, :, 4] = c_obj * ((1 - near) - (1 + near) * (1 - sx))
    r.g_boxes_abs[:, :, 4] = fold(abs(c_obj) * ((1 - near) + (1 + near) * (1 + sx)), 9,
                                  abs(c_obj) * (1 + near) * U["exp"] * sx * (1 - sx))
    r.g_boxes[:, :, :4] = c_box * near[:, :, None] * clamp1(boxes[:, :, :4] - box_label[:, None, :])
    r.g_boxes_abs[:, :, :4] = np.abs(r.g_boxes[:, :, :4])
    return r


def track_loss(cla, seg, vote, box_label, centers, boxes, bc_pred, bc_label, weights):
    """-> the 8 raw sums, the 6 losses and the four gradients (models/base_model.py:122-164, models/bat.py:57-65; the
    objectness BCE is a scalar mean that the mask rescales by mask / (mask + 1e-6), as the reference has it)"""
    r = track_sums(cla, seg, vote, box_label, centers, boxes, bc_pred, bc_label)
    B, N = np.shape(cla)
    f = track_finish(r.sums, B * N, B * np.shape(centers)[1], weights, bc_pred is not None)
    g = track_grads(cla, seg, vote, box_label, centers, boxes, bc_pred, bc_label, weights, r.sums)
    r.__dict__.update(f.__dict__)
    r.__dict__.update(g.__dict__)
    return r


# ---- o3d_m2track_loss ---------------------------------------------------------------------------------------------------
M2_SUMS = ("class_weight", "seg_nll", "bc", "moving", "center_motion", "angle_motion", "center", "angle", "center_prev",
           "angle_prev", "center_aux", "angle_aux", "motion_cls_nll")
M2_LOSSES = ("total", "motion_cls", "center", "angle", "center_prev", "angle_prev", "seg", "center_aux", "center_motion",
             "angle_aux", "angle_motion", "bc")
M2_GRADS = ("g_seg", "g_bc", "g_mcls", "g_motion", "g_aux", "g_est", "g_prev")


def nll2(x0, x1, y):
    """2-class -log softmax(x)[y] and softmax(x)[1] with the pieces of their bounds"""
    m = np.maximum(x0, x1)
    e0, e1 = np.exp(x0 - m), np.exp(x1 - m)
    S = e0 + e1
    xy = np.where(y, x1, x0)
    nll = m + np.log(S) - xy
    pieces = np.abs(m) + np.abs(xy) + np.log(S) + 1.0
    allow = U["exp"] * np.minimum(e0, e1) / S + U["log"] * np.log(S)
    p1 = e1 / S
    return Ref(nll=nll, abs=pieces, allow=allow, p1=p1, p_allow=2 * U["exp"] * p1 * (1 - p1))


def _angle(pred, lab):
    """smooth-L1 on the sines: value, allowance of the two sines (units of 2^-24), cos(pred) * clamp"""
    sp, sl = np.sin(pred), np.sin(lab)
    d = sp - sl
    return sl1(d), U["sin"] * (np.abs(sp) + np.abs(sl)) * np.minimum(np.abs(d), 1.0), d


def m2_sums(seg_logits, seg_label, bc_pred, bc_a, bc_b, motion_cls, state, motion, motion_lab, aux, est, prev, box_lab, prev_lab,
            cw=(0.5, 2.0)):
    seg_logits = f64(seg_logits)
    B, _, N = seg_logits.shape
    y = np.asarray(seg_label) != 0
    q = nll2(seg_logits[:, 0], seg_logits[:, 1], y)
    w = f64(np.where(y, cw[1], cw[0]))
    dseg, db = cdiv(B, LG) * cdiv(N, LT) + TREE, cdiv(B, LT) + TREE
    s, a, n = np.zeros(13), np.zeros(13), np.zeros(13)
    s[0], a[0], n[0] = w.sum(), np.abs(w).sum(), dseg
    s[1], a[1], n[1] = (w * q.nll).sum(), fold(np.abs(w) * q.abs, dseg + 6, np.abs(w) * q.allow).sum(), dseg + 6
    if bc_pred is not None:
        K = bc_pred.shape[2]
        t = sl1(f64(bc_pred) - np.concatenate([f64(bc_a), f64(bc_b)], axis=1))
        s[2], a[2], n[2] = t.sum(), t.sum(), cdiv(B, LG) * cdiv(N * K, LT) + TREE + 4
    st = f64(np.asarray(state) != 0) if state is not None else f64(np.ones(B))
    s[3], a[3], n[3] = st.sum(), st.sum(), db
    motion, motion_lab = f64(motion), f64(motion_lab)
    t = st * sl1(motion[:, :3] - motion_lab[:, :3]).sum(-1) / 3.0
    s[4], a[4], n[4] = t.sum(), t.sum(), db + 10
    v, al, _ = _angle(motion[:, 3], motion_lab[:, 3])
    s[5], a[5], n[5] = (st * v).sum(), fold(st * v, db + 5, st * al).sum(), db + 5
    for k, (row, lab) in enumerate(((est, box_lab), (prev, prev_lab), (aux, box_lab))):
        if row is None:
            continue
        row, lab = f64(row), f64(lab)
        t = sl1(row[:, :3] - lab[:, :3]).sum(-1)
        s[6 + 2 * k], a[6 + 2 * k], n[6 + 2 * k] = t.sum(), t.sum(), db + 8
        v, al, _ = _angle(row[:, 3], lab[:, 3])
        s[7 + 2 * k], a[7 + 2 * k], n[7 + 2 * k] = v.sum(), fold(v, db + 5, al).sum(), db + 5
    if motion_cls is not None:
        mc = f64(motion_cls)
        qm = nll2(mc[:, 0], mc[:, 1], np.asarray(state) != 0)
        s[12], a[12], n[12] = qm.nll.sum(), fold(qm.abs, db + 6, qm.allow).sum(), db + 6
    return Ref(sums=s, sums_abs=a, sums_n=n)


def m2_finish(sums, B, N, K, weights, with_bc, with_mcls, with_state, with_est, with_prev):
    s = f64(sums)
    w_center, w_angle, w_seg, w_bc, w_mcls = [float(w) for w in weights]
    l_seg = s[1] / s[0]
    l_bc = s[2] / (float(B) * N * K) if with_bc else 0.0
    inv_mov = 1.0 / (s[3] + 1e-6) if with_state else 1.0 / B
    l_cm, l_am = s[4] * inv_mov, s[5] * inv_mov
    l_c, l_a = (s[6] / (3.0 * B), s[7] / B) if with_est else (0.0, 0.0)
    l_cp, l_ap = (s[8] / (3.0 * B), s[9] / B) if with_prev else (0.0, 0.0)
    l_cx, l_ax = s[10] / (3.0 * B), s[11] / B
    l_mcls = s[12] / B if with_mcls else 0.0
    parts = np.array([l_mcls * w_mcls, l_c * w_center, l_cp * w_center, l_cx * w_center, l_cm * w_center, l_a * w_angle,
                      l_ap * w_angle, l_ax * w_angle, l_am * w_angle, l_seg * w_seg, l_bc * w_bc])
    losses = np.array([parts.sum(), l_mcls, l_c, l_a, l_cp, l_ap, l_seg, l_cx, l_cm, l_ax, l_am, l_bc])
    labs = np.abs(losses)
    labs[0] = np.abs(parts).sum()
    n = np.full(12, TOT + 4.0)
    n[0], n[6] = 2 * TOT + 16, 2 * TOT + 2
    return Ref(losses=losses, losses_abs=labs, losses_n=n, inv_mov=inv_mov)


def m2_grads(seg_logits, seg_label, bc_pred, bc_a, bc_b, motion_cls, state, motion, motion_lab, aux, est, prev, box_lab, prev_lab,
             weights, sums, cw=(0.5, 2.0)):
    seg_logits = f64(seg_logits)
    B, _, N = seg_logits.shape
    w_center, w_angle, w_seg, w_bc, w_mcls = [float(w) for w in weights]
    K = bc_pred.shape[2] if bc_pred is not None else 0
    c = m2_finish(sums, B, N, K, weights, bc_pred is not None, motion_cls is not None, state is not None, est is not None,
                  prev is not None)
    r = Ref(**{g: None for g in M2_GRADS})
    y = np.asarray(seg_label) != 0
    q = nll2(seg_logits[:, 0], seg_logits[:, 1], y)
    w = f64(np.where(y, cw[1], cw[0])) * (w_seg / f64(sums)[0])
    r.g_seg = np.stack([w * ((1 - q.p1) - (~y)), w * (q.p1 - y)], axis=1)
    r.g_seg_n = TOT + 9
    r.g_seg_abs = np.stack([fold(2 * np.abs(w), TOT + 9, np.abs(w) * q.p_allow)] * 2, axis=1)
    if bc_pred is not None:
        c_bc = w_bc / (float(B) * N * K)
        r.g_bc = c_bc * clamp1(f64(bc_pred) - np.concatenate([f64(bc_a), f64(bc_b)], axis=1))
        r.g_bc_abs, r.g_bc_n = np.abs(r.g_bc), 5
    st = f64(np.asarray(state) != 0) if state is not None else f64(np.ones(B))

    def row(pred, lab, cc, ca, n):
        pred, lab = f64(pred), f64(lab)
        g = np.empty_like(pred)
        g[:, :3] = cc[:, None] * clamp1(pred[:, :3] - lab[:, :3])
        _, _, d = _angle(pred[:, 3], lab[:, 3])
        cosp = np.cos(pred[:, 3])
        g[:, 3] = ca * cosp * clamp1(d)
        ga = np.abs(g)
        allow = np.abs(ca) * np.abs(cosp) * (U["cos"] * np.abs(clamp1(d)) + U["sin"] * (np.abs(np.sin(pred[:, 3])) +
                                                                                    np.abs(np.sin(lab[:, 3]))))
        ga[:, 3] = fold(ga[:, 3], n, allow)
        return g, ga, n

    r.g_motion, r.g_motion_abs, r.g_motion_n = row(motion, motion_lab, w_center * st * c.inv_mov / 3.0, w_angle * st * c.inv_mov, 8)
    ones = np.ones(B)
    r.g_aux, r.g_aux_abs, r.g_aux_n = row(aux, box_lab, ones * w_center / (3.0 * B), ones * w_angle / B, 5)
    if est is not None:
        r.g_est, r.g_est_abs, r.g_est_n = row(est, box_lab, ones * w_center / (3.0 * B), ones * w_angle / B, 5)
    if prev is not None:
        r.g_prev, r.g_prev_abs, r.g_prev_n = row(prev, prev_lab, ones * w_center / (3.0 * B), ones * w_angle / B, 5)
    if motion_cls is not None:
        mc = f64(motion_cls)
        ym = np.asarray(state) != 0
        qm = nll2(mc[:, 0], mc[:, 1], ym)
        cm = w_mcls / B
        r.g_mcls = np.stack([cm * ((1 - qm.p1) - (~ym)), cm * (qm.p1 - ym)], axis=1)
        r.g_mcls_n = 8
        r.g_mcls_abs = np.stack([fold(2 * abs(cm) + 0 * qm.p1, 8, abs(cm) * qm.p_allow)] * 2, axis=1)
    return r


def m2track_loss(seg_logits, seg_label, bc_pred, bc_a, bc_b, motion_cls, state, motion, motion_lab, aux, est, prev, box_lab,
                 prev_lab, weights, cw=(0.5, 2.0)):
    """-> the 13 raw sums, the 12 losses and the 7 gradients (models/m2track.py:153-231); a NULL-able term is None.  A label
    is class 1 where it is non-zero, as the kernel reads it.  state None: plain means over the batch for the motion pair."""
    args = (seg_logits, seg_label, bc_pred, bc_a, bc_b, motion_cls, state, motion, motion_lab, aux, est, prev, box_lab, prev_lab)
    r = m2_sums(*args, cw=cw)
    B, _, N = np.shape(seg_logits)
    K = bc_pred.shape[2] if bc_pred is not None else 0
    f = m2_finish(r.sums, B, N, K, weights, bc_pred is not None, motion_cls is not None, state is not None, est is not None,
                  prev is not None)
    g = m2_grads(*args, weights, r.sums, cw=cw)
    r.__dict__.update(f.__dict__)
    r.__dict__.update(g.__dict__)
    return r


# ---- o3d_adam_step ------------------------------------------------------------------------------------------------------
def adam_moments(m, v, g, p, beta1, beta2, wd):
    m, v, g, p = map(f64, (m, v, g, p))
    gi = g + wd * p
    m2 = beta1 * m + (1 - beta1) * gi
    v2 = beta2 * v + (1 - beta2) * gi * gi
    return Ref(m=m2, m_abs=np.abs(beta1 * m) + abs(1 - beta1) * (np.abs(g) + np.abs(wd * p)), m_n=5, v=v2, v_abs=v2, v_n=8)


def adam_update(p, m2, v2, lr, eps, bc1, bc2):
    p, m2, v2 = map(f64, (p, m2, v2))
    u = (lr / bc1) * m2 / (np.sqrt(v2) / float(np.sqrt(bc2)) + eps)
    return Ref(p=p - u, p_abs=np.abs(p) + np.abs(u), p_n=8)


def adam_step(p, m, v, g, lr, beta1, beta2, eps, wd, bc1, bc2):
    """torch.optim.Adam's update without amsgrad / maximize; bc1 = 1 - beta1^t and bc2 = 1 - beta2^t are passed, as in the ABI"""
    r = adam_moments(m, v, g, p, beta1, beta2, wd)
    r.__dict__.update(adam_update(p, r.m, r.v, lr, eps, bc1, bc2).__dict__)
    return r


# ---- o3d_best_proposal ----------------------------------------------------------------------------------------------------
def best_proposal(boxes):
    """boxes (B,P,5) -> out (B,4) of the FIRST maximum of column 4, idx (B)"""
    boxes = np.asarray(boxes)
    idx = np.empty(boxes.shape[0], np.int64)
    for b in range(boxes.shape[0]):
        best = 0
        for j in range(1, boxes.shape[1]):
            if boxes[b, j, 4] > boxes[b, best, 4]:
                best = j
        idx[b] = best
    return Ref(out=boxes[np.arange(boxes.shape[0]), idx, :4], idx=idx)


# ---- the vote head's glue ------------------------------------------------------------------------------------------------
def rpn_votes_fwd(cla, vote):
    """cla (B,N), vote (B,3+f,N) -> score (B,N), vote_xyz (B,N,3), vote_feature (B,1+f,N)"""
    cla, vote = f64(cla), f64(vote)
    s = sigmoid(cla)
    return Ref(score=s, score_abs=fold(s, 2, U["exp"] * s * (1 - s)), score_n=2, vote_xyz=vote[:, :3].transpose(0, 2, 1).copy(),
               vote_feature=np.concatenate([s[:, None, :], vote[:, 3:]], axis=1))


def rpn_votes_bwd(score, dvf, dvx, f):
    """score (B,N), dvf (B,1+f,N) | None, dvx (B,3,N) | None -> dcla (B,N), dvote (3+f, B*N); a missing gradient is zeros"""
    score = f64(score)
    B, N = score.shape
    dvote = np.zeros((3 + f, B * N))
    if dvx is not None:
        dvote[:3] = f64(dvx).transpose(1, 0, 2).reshape(3, B * N)
    dcla = np.zeros((B, N))
    if dvf is not None:
        dvf = f64(dvf)
        dvote[3:] = dvf[:, 1:].transpose(1, 0, 2).reshape(f, B * N)
        dcla = dvf[:, 0] * score * (1 - score)
    return Ref(dcla=dcla, dcla_abs=np.abs(dcla if dvf is None else dvf[:, 0] * score), dcla_n=3, dvote=dvote)


def box_assemble(offsets, centers):
    """offsets (B,5,P), centers (B,P,3) -> boxes (B,P,5)"""
    o, c = f64(offsets).transpose(0, 2, 1), f64(centers)
    boxes = o.copy()
    boxes[:, :, :3] += c
    a = np.abs(o)
    a[:, :, :3] += np.abs(c)
    return Ref(boxes=boxes, boxes_abs=a, boxes_n=1)


# ---- o3d_offset_box -------------------------------------------------------------------------------------------------------
def offset_box(ref, off):
    ref, off = f64(ref), f64(off)
    c, s = np.cos(ref[:, 3]), np.sin(ref[:, 3])
    box = np.stack([c * off[:, 0] - s * off[:, 1] + ref[:, 0], s * off[:, 0] + c * off[:, 1] + ref[:, 1], off[:, 2] + ref[:, 2],
                    ref[:, 3] + off[:, 3]], axis=1)
    rot = np.abs(c * off[:, 0]) + np.abs(s * off[:, 1])
    rot2 = np.abs(s * off[:, 0]) + np.abs(c * off[:, 1])
    a = np.stack([rot + np.abs(ref[:, 0]), rot2 + np.abs(ref[:, 1]), np.abs(off[:, 2]) + np.abs(ref[:, 2]),
                  np.abs(ref[:, 3]) + np.abs(off[:, 3])], axis=1)
    return Ref(box=box, box_abs=a, box_n=np.array([4 + UT, 4 + UT, 1, 1], np.float64))


def offset_box_bwd(ref, off, g):
    ref, off, g = f64(ref), f64(off), f64(g)
    c, s = np.cos(ref[:, 3]), np.sin(ref[:, 3])
    ox, oy = off[:, 0], off[:, 1]
    gx, gy = g[:, 0], g[:, 1]
    g_ref = g.copy()
    g_ref[:, 3] = g[:, 3] + gx * (-s * ox - c * oy) + gy * (c * ox - s * oy)
    ra = np.abs(g)
    ra[:, 3] = np.abs(g[:, 3]) + np.abs(gx) * (np.abs(s * ox) + np.abs(c * oy)) + np.abs(gy) * (np.abs(c * ox) + np.abs(s * oy))
    g_off = g.copy()
    g_off[:, 0], g_off[:, 1] = c * gx + s * gy, -s * gx + c * gy
    oa = np.abs(g)
    oa[:, 0], oa[:, 1] = np.abs(c * gx) + np.abs(s * gy), np.abs(s * gx) + np.abs(c * gy)
    return Ref(g_ref=g_ref, g_ref_abs=ra, g_ref_n=np.array([0, 0, 0, 8 + UT], np.float64), g_off=g_off, g_off_abs=oa,
               g_off_n=np.array([3 + UT, 3 + UT, 0, 0], np.float64))


# ---- o3d_motion_merge_fwd / _bwd --------------------------------------------------------------------------------------------
class _V:
    """a 2-D vector per (cloud, point) with the sum of the absolute values of the terms it was made of"""

    def __init__(self, x, y, ax=None, ay=None):
        self.x, self.y = x, y
        self.ax, self.ay = (np.abs(x) if ax is None else ax), (np.abs(y) if ay is None else ay)

    def rot(self, t):
        """by the angle t (B,) or (B,1)"""
        c, s = np.cos(t), np.sin(t)
        return _V(c * self.x - s * self.y, s * self.x + c * self.y, np.abs(c) * self.ax + np.abs(s) * self.ay,
                  np.abs(s) * self.ax + np.abs(c) * self.ay)

    def add(self, o, sign=1.0):
        return _V(self.x + sign * o.x, self.y + sign * o.y, self.ax + o.ax, self.ay + o.ay)


def motion_merge_fwd(pts, prev, motion):
    """pts (B,3,N) xyz channel-major, the first N/2 points of the previous frame; prev (B,4) | None (zeros); motion (B,4) ->
    merged (B,3,N), aux (B,4): the reference's chain step by step (datasets/points_utils.py:390-452)"""
    pts, motion = f64(pts), f64(motion)
    B, _, N = pts.shape
    h = N // 2
    prev = np.zeros_like(motion) if prev is None else f64(prev)
    col = lambda a: a[:, None]      # noqa: E731
    pc, pt = _V(col(prev[:, 0]), col(prev[:, 1])), col(prev[:, 3])
    mc, mt = _V(col(motion[:, 0]), col(motion[:, 1])), col(motion[:, 3])
    # get_offset_box_tensor: aux = prev moved by the motion given in prev's frame
    ac, at = mc.rot(pt).add(pc), pt + mt
    az = motion[:, 2] + prev[:, 2]
    aux = np.stack([ac.x[:, 0], ac.y[:, 0], az, at[:, 0]], axis=1)
    aux_abs = np.stack([ac.ax[:, 0], ac.ay[:, 0], np.abs(motion[:, 2]) + np.abs(prev[:, 2]), np.abs(pt[:, 0]) + np.abs(mt[:, 0])], axis=1)
    # get_offset_points_tensor on the previous half: into the box, along the motion, back to the world
    p0 = _V(pts[:, 0, :h], pts[:, 1, :h])
    moved = p0.add(pc, -1.0).rot(-pt).rot(mt).add(mc).rot(pt).add(pc)
    z0 = ((pts[:, 2, :h] - col(prev[:, 2])) + col(motion[:, 2])) + col(prev[:, 2])
    z0a = np.abs(pts[:, 2, :h]) + 2 * col(np.abs(prev[:, 2])) + col(np.abs(motion[:, 2]))
    p1 = _V(pts[:, 0, h:], pts[:, 1, h:])
    # remove_transform_points_tensor: both halves in the frame of aux
    o0, o1 = moved.add(ac, -1.0).rot(-at), p1.add(ac, -1.0).rot(-at)
    zaux = col(np.abs(motion[:, 2]) + np.abs(prev[:, 2]))
    merged = np.stack([np.concatenate([o0.x, o1.x], 1), np.concatenate([o0.y, o1.y], 1),
                       np.concatenate([z0 - col(az), pts[:, 2, h:] - col(az)], 1)], axis=1)
    mabs = np.stack([np.concatenate([o0.ax, o1.ax], 1), np.concatenate([o0.ay, o1.ay], 1),
                     np.concatenate([z0a + zaux, np.abs(pts[:, 2, h:]) + zaux], 1)], axis=1)
    ang = np.ceil(np.abs(at))                                   # the rounding of prev_t + motion_t, as an angle
    n = np.empty((B, 3, N))
    n[:, :2, :h], n[:, :2, h:] = col(20 + 4 * UT + ang), col(8 + 2 * UT + ang)
    n[:, 2, :h], n[:, 2, h:] = 5, 2
    return Ref(merged=merged, merged_abs=mabs, merged_n=n, aux=aux, aux_abs=aux_abs,
               aux_n=np.array([4 + UT, 4 + UT, 1, 1], np.float64))


def _rot_vjp(t, vx, vy, gx, gy):
    """o = Rz(t) v: -> (g_v x, g_v y, g_t)"""
    c, s = np.cos(t), np.sin(t)
    return c * gx + s * gy, -s * gx + c * gy, gx * (-s * vx - c * vy) + gy * (c * vx - s * vy)


def motion_merge_bwd(pts, prev, motion, g_merged, g_aux):
    """gradients of motion_merge_fwd's chain w.r.t. prev and motion by reverse accumulation through its steps, in fp64
    -> g_prev (B,4), g_motion (B,4); the bounds' sum|t_i| follow the sums the kernel forms (per half: S = sum g,
    T = sum g . d/dtheta)"""
    pts, motion, g = f64(pts), f64(motion), f64(g_merged)
    B, _, N = pts.shape
    h = N // 2
    prev = np.zeros_like(motion) if prev is None else f64(prev)
    col = lambda a: a[:, None]      # noqa: E731
    pcx, pcy, pcz, pt = (col(prev[:, k]) for k in range(4))
    mcx, mcy, mcz, mt = (col(motion[:, k]) for k in range(4))
    cp, sp = np.cos(pt), np.sin(pt)
    acx, acy, at = cp * mcx - sp * mcy + pcx, sp * mcx + cp * mcy + pcy, pt + mt
    # forward of the previous half, keeping every step's input
    x0, y0 = pts[:, 0, :h] - pcx, pts[:, 1, :h] - pcy
    x1, y1 = np.cos(-pt) * x0 - np.sin(-pt) * y0, np.sin(-pt) * x0 + np.cos(-pt) * y0
    x2, y2 = np.cos(mt) * x1 - np.sin(mt) * y1 + mcx, np.sin(mt) * x1 + np.cos(mt) * y1 + mcy
    x3, y3 = cp * x2 - sp * y2 + pcx, sp * x2 + cp * y2 + pcy
    x4, y4 = x3 - acx, y3 - acy
    g_pc, g_mc, g_ac = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros((B, 3))
    g_pt, g_mt, g_at = np.zeros(B), np.zeros(B), np.zeros(B)
    # ---- previous half, backwards
    gx, gy, gt = _rot_vjp(-at, x4, y4, g[:, 0, :h], g[:, 1, :h])
    g_at -= gt.sum(1)
    g_ac[:, 0] -= gx.sum(1); g_ac[:, 1] -= gy.sum(1)                                  # noqa: E702
    gz = g[:, 2, :h]
    g_ac[:, 2] -= gz.sum(1)
    g_pc[:, 0] += gx.sum(1); g_pc[:, 1] += gy.sum(1)                                  # noqa: E702   (x3 = ... + pc)
    gx, gy, gt = _rot_vjp(pt, x2, y2, gx, gy)
    g_pt += gt.sum(1)
    g_mc[:, 0] += gx.sum(1); g_mc[:, 1] += gy.sum(1)                                  # noqa: E702   (x2 = ... + mc)
    gx, gy, gt = _rot_vjp(mt, x1, y1, gx, gy)
    g_mt += gt.sum(1)
    gx, gy, gt = _rot_vjp(-pt, x0, y0, gx, gy)
    g_pt -= gt.sum(1)
    g_pc[:, 0] -= gx.sum(1); g_pc[:, 1] -= gy.sum(1)                                  # noqa: E702
    # z of the previous half: ((z - pcz) + mcz) + pcz - acz
    g_mc[:, 2] += gz.sum(1)
    # ---- current half
    u, v = pts[:, 0, h:] - acx, pts[:, 1, h:] - acy
    gx, gy, gt = _rot_vjp(-at, u, v, g[:, 0, h:], g[:, 1, h:])
    g_at -= gt.sum(1)
    g_ac[:, 0] -= gx.sum(1); g_ac[:, 1] -= gy.sum(1); g_ac[:, 2] -= g[:, 2, h:].sum(1)   # noqa: E702
    # ---- aux = (Rz(pt) mc + pc, mcz + pcz, pt + mt), with the gradient that arrives at aux itself
    if g_aux is not None:
        ga = f64(g_aux)
        g_ac += ga[:, :3]
        g_at += ga[:, 3]
    gx, gy, gt = _rot_vjp(pt[:, 0], mcx[:, 0], mcy[:, 0], g_ac[:, 0], g_ac[:, 1])
    g_mc[:, 0] += gx; g_mc[:, 1] += gy; g_mc[:, 2] += g_ac[:, 2]                      # noqa: E702
    g_pt += gt + g_at
    g_mt += g_at
    g_pc += g_ac
    g_prev, g_motion = np.concatenate([g_pc, g_pt[:, None]], 1), np.concatenate([g_mc, g_mt[:, None]], 1)
    # ---- sum|t_i| along the kernel's sums
    ag = np.abs(g)
    S0, S1 = ag[:, :, :h].sum(2), ag[:, :, h:].sum(2)                                 # (B,3) each

    def tsum(gs, px, py, cx, cy):
        r = np.abs(px) + np.abs(cx) + np.abs(py) + np.abs(cy)
        return ((gs[:, 0] + gs[:, 1]) * r).sum(1)

    T0 = tsum(ag[:, :, :h], pts[:, 0, :h], pts[:, 1, :h], pcx, pcy)
    T1 = tsum(ag[:, :, h:], pts[:, 0, h:], pts[:, 1, h:], np.abs(cp * mcx) + np.abs(sp * mcy) + np.abs(pcx),
              np.abs(sp * mcx) + np.abs(cp * mcy) + np.abs(pcy))
    gaa = np.zeros((B, 4)) if g_aux is None else np.abs(f64(g_aux))
    xy0, xy1 = S0[:, 0] + S0[:, 1], S1[:, 0] + S1[:, 1]
    gac_xy = xy1 + gaa[:, 0] + gaa[:, 1]
    gat = T1 + gaa[:, 3]
    m_abs = np.stack([gac_xy, gac_xy, S1[:, 2] + gaa[:, 2], gat], axis=1)
    mm = np.abs(motion[:, 0]) + np.abs(motion[:, 1])
    p_abs = np.stack([xy0 + gac_xy, xy0 + gac_xy, S0[:, 2] + S1[:, 2] + gaa[:, 2], T0 + gat + gac_xy * mm], axis=1)
    depth = cdiv(N, LT) + 6 + 3
    ang = np.ceil(np.abs(at[:, 0]))
    nn = np.stack([depth + 8 + 3 * UT + ang, depth + 8 + 3 * UT + ang, np.full(B, depth + 2.0), depth + 12 + 3 * UT + ang], axis=1)
    return Ref(g_prev=g_prev, g_prev_abs=p_abs, g_prev_n=nn + 4, g_motion=g_motion, g_motion_abs=m_abs, g_motion_n=nn)


# ---- case tables and inputs of tests/test_tail_kernels_gpu.py (checked without a GPU by tests/test_tail_oracle_cpu.py) --------
TRACK_SHAPES = [(1, 1, 1, 1), (2, 7, 3, 9), (3, 100, 5, 2), (5, 3300, 70, 9), (260, 64, 64, 9)]       # (B, N, P, K)
TRACK_KINDS = ("plain", "empty", "edge", "logits")
TRACK_W = (1.5, 0.2, 0.2, 1.0, 1.0)                 # objectness, box, seg, vote, bc: the BAT configuration
M2_SHAPES = [(1, 2, 1), (3, 6, 9), (65, 258, 9), (257, 4, 3)]                                           # (B, N, K)
M2_EXACT_GRAD_SHAPES = [(1, 2, 1), (4, 8, 4)]       # B * N * K and B powers of two: the gradients' constants are too
M2_W = (2.0, 10.0, 0.1, 1.0, 0.1)                   # center, angle, seg, bc, motion_cls: the KITTI configuration
M2_W_EXACT = (3.0, 4.0, 0.5, 2.0, 0.25)             # w_center / (3 B) a power of two when B is
M2_FLAGS = [(bc, cls, est, prev) for bc in (0, 1) for cls in (0, 1) for est in (0, 1) for prev in (0, 1)]
ADAM_JOBS = (1, 255, 256, 257, 8192, 8193, 20000)   # one sweep of the 32 x 256 grid is 8192 elements
ADAM_ORDER = (4, 0, 6, 2, 5, 1, 3)                  # where the jobs lie in the flat buffers
ADAM_GAP = 37
ADAM_EXACT = dict(lr=2.0 ** -10, beta1=0.5, beta2=0.75, eps=0.0, bc1=0.5, bc2=0.25)
ADAM_ROUNDED = dict(lr=1e-3, beta1=0.5, beta2=0.999, eps=1e-6)
BEST_B, BEST_P = (1, 3, 70), (1, 2, 63, 64, 65, 128, 200)
RPN_SHAPES = [(1, 1, 1), (2, 5, 3), (3, 100, 4), (2, 300, 7)]                                           # (B, N, f)
ASSEMBLE_SHAPES = [(1, 1), (2, 7), (3, 64), (5, 103)]                                                   # (B, P)
MERGE_B, MERGE_N = (1, 3), (2, 6, 254, 256, 258, 514, 1024)
OFFSET_B = (1, 63, 64, 65, 130)
# (seed, shape, kind) of every o3d_track_loss launch set, (seed, shape, flags, kind) of every o3d_m2track_loss one
TRACK_ROUNDED = [(400 + s[1], s, "plain") for s in TRACK_SHAPES] + [(411, (3, 100, 5, 2), "empty"), (412, (3, 100, 5, 2), "edge"),
                                                                    (413, (2, 7, 3, 9), "logits")]
TRACK_EXACT = [(4000 + s[1], s, "plain") for s in TRACK_SHAPES]
ALL_ON = (1, 1, 1, 1)
M2_ROUNDED = [(500 + s[1], s, ALL_ON, "plain") for s in M2_SHAPES] + [(510, (3, 6, 9), f, "plain") for f in M2_FLAGS] + \
    [(530, (2, 7, 0), (0, 1, 1, 1), "plain"), (531, (3, 6, 9), ALL_ON, "still"), (532, (3, 6, 9), ALL_ON, "labels"),
     (533, (65, 258, 9), ALL_ON, "plain")]
M2_EXACT = [(5000 + s[1], s, ALL_ON, "plain") for s in M2_SHAPES] + [(5100, (3, 6, 9), f, "plain") for f in M2_FLAGS] + \
    [(5300, (2, 7, 0), (0, 1, 1, 1), "plain")]
M2_EXACT_GRADS = [(5200 + s[0], s, (1, 0, 1, 1), "plain") for s in M2_EXACT_GRAD_SHAPES]
EDGE_DIST = (0.3 - 1e-4, 0.3 + 1e-4, 0.6 - 1e-4, 0.6 + 1e-4)
LOGITS = (30.0, -30.0, 88.0, -88.0)


def _signs(draw, shape):
    return np.where(draw.val(shape, 1.0, 1.0) >= 0, 1.0, -1.0)


def _pick(draw, values, shape):
    """entries of `values`, every one present when there is room (the first len(values) slots cycle through them)"""
    v = np.asarray(values, np.float64)
    k = np.abs(draw.val(shape, 1.0, 1000.0)).astype(np.int64) % len(v) if draw.exact else \
        (np.abs(draw.val(shape)) * 1000).astype(np.int64) % len(v)
    flat = k.reshape(-1)
    flat[:len(v)] = np.arange(len(v))[:flat.size]
    return v[k]


def exact_mags(count):
    """|d| of the exact leg's smooth-L1 arguments: 0, 1, just inside and outside 1, and both branches; the step next to 1
    shrinks with the number of terms so that their sum stays exact -> (values, grid spacing of a smooth-L1 value)"""
    k = 8 if count <= 1024 else 3
    eps = 2.0 ** -k
    return (0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 1.0 - eps, 1.0 + eps), 2.0 ** -(2 * k + 1)


def track_inputs(draw, B, N, P, K, kind="plain"):
    """-> Ref(cla, seg, vote, box_label, centers, boxes, bc_pred, bc_label [, spacing on the exact leg])"""
    i = Ref()
    if draw.exact:
        mags, i.spacing = exact_mags(max(B * N, B * P))
        i.box_label = draw.val((B, 4), 0.125, 2.0)
        i.cla = draw.val((B, N), 0.25, 4.0)
        i.seg = (draw.val((B, N), 1.0, 1.0) > 0).astype(np.float64)
        # one |d| for the coordinates of a seed: v = 3 sl1(d) and c = K sl1(d), whose products with fl(1/3) and quotients by K
        # round back to sl1(d) exactly
        i.vote = i.box_label[:, None, :3] + _signs(draw, (B, N, 3)) * _pick(draw, mags, (B, N, 1))
        i.bc_label = draw.val((B, N, K), 0.125, 2.0)
        i.bc_pred = i.bc_label + _signs(draw, (B, N, K)) * _pick(draw, mags, (B, N, 1))
        off = _pick(draw, (0.0, 0.125, -0.125, 0.25, -0.25, 0.5, -0.5, 1.0), (B, P, 3))
        i.centers = i.box_label[:, None, :3] + off
        i.boxes = np.concatenate([i.box_label[:, None, :] + _signs(draw, (B, P, 4)) * _pick(draw, mags, (B, P, 4)),
                                  draw.val((B, P, 1), 0.25, 4.0)], axis=2)
        return i
    i.box_label = draw.val((B, 4))
    i.cla = 2.0 * draw.val((B, N))
    i.seg = (draw.val((B, N)) > 0.3).astype(np.float64)
    i.vote = f32(i.box_label[:, None, :3] + 0.8 * draw.val((B, N, 3)))
    i.bc_label = draw.val((B, N, K))
    i.bc_pred = f32(i.bc_label + draw.val((B, N, K)))
    u = draw.val((B, P, 3)) + 1e-3
    u /= np.sqrt((u * u).sum(-1, keepdims=True))
    radius = _pick(draw, (0.05, 0.15, 0.25, 0.4, 0.5, 0.75, 1.5), (B, P, 1))
    if kind == "edge":
        radius = np.sqrt(_pick(draw, EDGE_DIST, (B, P, 1)) ** 2 - 1e-6)
    if kind == "empty":
        i.seg[:] = 0.0
        radius = _pick(draw, (0.4, 0.45, 0.5), (B, P, 1))
    i.centers = f32(i.box_label[:, None, :3] + u * radius)
    i.boxes = f32(np.concatenate([i.box_label[:, None, :] + 0.7 * draw.val((B, P, 4)), 2.0 * draw.val((B, P, 1))], axis=2))
    if kind == "logits":
        i.cla = _pick(draw, LOGITS, (B, N))
        i.boxes[:, :, 4] = _pick(draw, LOGITS, (B, P))
    return i


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def track_spacing(i):
    """grid spacing of the terms of the exactly compared sums of o3d_track_loss (the box term is a quarter of four sl1)"""
    return {0: 1.0, 1: 1.0, 2: 1.0, 4: i.spacing, 5: i.spacing, 7: i.spacing / 4}


def m2_spacing(i):
    """the same for o3d_m2track_loss: class weights 0.5 and 2, a count, smooth-L1 values; the angle sums are 0"""
    return {0: 0.5, 2: i.spacing, 3: 1.0, 4: i.spacing, 5: 1.0, 6: i.spacing, 7: 1.0, 8: i.spacing, 9: 1.0, 10: i.spacing, 11: 1.0}


def track_args(i, with_bc=True):
    return (i.cla, i.seg, i.vote, i.box_label, i.centers, i.boxes, i.bc_pred if with_bc else None, i.bc_label)


def m2_inputs(draw, B, N, K, flags=(1, 1, 1, 1), kind="plain"):
    """flags = (BoxCloud, motion_cls + state, refined box, previous box) -> the 14 arrays of o3d_m2track_loss, None where off"""
    bc, cls, est, prev = flags
    i = Ref()
    h = N // 2
    if draw.exact:
        mags, i.spacing = exact_mags(B * N * K)
        lab = lambda: np.concatenate([draw.val((B, 3), 0.125, 2.0), np.zeros((B, 1))], axis=1)      # noqa: E731  (angles 0)
        near = lambda L, same: L + np.concatenate([_signs(draw, (B, 3)) * _pick(draw, mags, (B, 1) if same else (B, 3)),  # noqa: E731
                                                   np.zeros((B, 1))], axis=1)
        i.seg_logits = draw.val((B, 2, N), 0.25, 4.0)
        i.bc_a, i.bc_b = draw.val((B, h, K), 0.125, 2.0), draw.val((B, N - h, K), 0.125, 2.0)
        i.bc_pred = np.concatenate([i.bc_a, i.bc_b], axis=1) + _signs(draw, (B, N, K)) * _pick(draw, mags, (B, N, K))
        i.motion_cls = draw.val((B, 2), 0.25, 4.0)
        i.motion_lab, i.box_lab, i.prev_lab = lab(), lab(), lab()
        i.motion, i.aux, i.est, i.prev = near(i.motion_lab, True), near(i.box_lab, False), near(i.box_lab, False), near(i.prev_lab, False)
        pos = draw.val((B, N), 1.0, 1.0) > 0
        mov = draw.val((B,), 1.0, 1.0) >= 0
    else:
        lab = lambda: draw.val((B, 4))      # noqa: E731
        near = lambda L, same: f32(L + 0.8 * draw.val((B, 4)))      # noqa: E731
        i.seg_logits = 2.0 * draw.val((B, 2, N))
        i.bc_a, i.bc_b = draw.val((B, h, K)), draw.val((B, N - h, K))
        i.bc_pred = f32(np.concatenate([i.bc_a, i.bc_b], axis=1) + draw.val((B, N, K)))
        i.motion_cls = 2.0 * draw.val((B, 2))
        i.motion_lab, i.box_lab, i.prev_lab = lab(), lab(), lab()
        i.motion, i.aux, i.est, i.prev = near(i.motion_lab, True), near(i.box_lab, False), near(i.box_lab, False), near(i.prev_lab, False)
        pos = draw.val((B, N)) > 0.3
        mov = draw.val((B,)) > -0.3
    i.seg_label = pos.astype(np.int64)
    i.state = mov.astype(np.int64)
    if kind == "still":
        i.state[:] = 0
    if kind == "labels":                   # non-zero labels that are not 1: class 1 all the same
        i.seg_label = i.seg_label * np.where(np.arange(N) % 2 == 0, 2, -1)[None, :]
        i.state = i.state * np.where(np.arange(B) % 2 == 0, 3, -5)
    if not bc:
        i.bc_pred = i.bc_a = i.bc_b = None
    if not cls:
        i.motion_cls = i.state = None
    if not est:
        i.est = None
    if not prev:
        i.prev = None
    return i


def m2_args(i):
    return (i.seg_logits, i.seg_label, i.bc_pred, i.bc_a, i.bc_b, i.motion_cls, i.state, i.motion, i.motion_lab, i.aux, i.est,
            i.prev, i.box_lab, i.prev_lab)


def adam_inputs(draw, n, k=0):
    """-> p, m, v, g of one job.  Exact leg: g = +-2^k, v in {0, g^2}, m and p dyadic; elements [0, n/8) of an even job hold
    g = 0, v = 0 (m dyadic): p is then bit-unchanged when m is 0 there too.  Rounded leg: |g| in [1e-15, 1e15] on a log grid --
    denormals (whether the build flushes them is not known) and overflow stay out of reach"""
    if draw.exact:
        e = np.abs(draw.val((n,), 1.0, 3.0))
        g = _signs(draw, (n,)) * 2.0 ** e
        v = np.where(draw.val((n,), 1.0, 1.0) > 0, g * g, 0.0)
        m = draw.val((n,), 0.25, 4.0)
        p = draw.val((n,), 0.125, 4.0)
    else:
        scale = 10.0 ** np.clip(5.0 * draw.val((n,)), -15, 15) if k % 2 else 1.0
        g = draw.val((n,)) * scale
        g = np.where(np.abs(g) < 1e-15, 1e-15, np.clip(g, -1e15, 1e15))
        m = 0.5 * draw.val((n,)) * scale
        v = f32(np.maximum((0.3 * draw.val((n,)) * scale) ** 2, 1e-30))
        p = draw.val((n,))
        g, m = f32(g), f32(m)
    z = n // 8
    g[:z], v[:z], m[:z] = 0.0, 0.0, 0.0
    return p, m, v, g


def best_scores(kind, B, P, draw):
    """(B,P) objectness scores of the planted cases"""
    s = draw.val((B, P), 0.25, 8.0) if draw.exact else draw.val((B, P))
    top = np.abs(s).max() + 1.0
    if kind == "lane_rounds" and P > 64:          # the maximum twice in one lane: j and j + 64
        j = min(3, P - 65)
        s[:, j], s[:, j + 64] = top, top
    elif kind == "lanes" and P > 1:               # across lanes
        s[:, P - 1], s[:, (P - 1) // 2] = top, top
    elif kind == "first_last":
        s[:, 0], s[:, P - 1] = top, top
    elif kind == "last":
        s[:, P - 1] = top
    elif kind == "equal":
        s[:] = 0.75
    elif kind == "neg_inf":
        s[:] = -np.inf
    elif kind == "pos_inf":
        s[:, P // 2] = np.inf
    elif kind == "zeros":                          # -0.0 before +0.0: equal, the first wins
        s[:] = -np.abs(s) - 1.0
        s[:, P // 3] = -0.0
        if P // 3 + 1 < P:
            s[:, P // 3 + 1:] = np.where(np.arange(P - P // 3 - 1) % 2 == 0, 0.0, -0.0)
    return s


BEST_KINDS = ("random", "lane_rounds", "lanes", "first_last", "last", "equal", "neg_inf", "pos_inf", "zeros")


def merge_inputs(draw, B, N, zero_angles=False):
    if draw.exact:
        pts = draw.val((B, 3, N), 0.25, 4.0)
        prev, motion = draw.val((B, 4), 0.25, 2.0), draw.val((B, 4), 0.25, 2.0)
        g, g_aux = draw.val((B, 3, N), 0.25, 2.0), draw.val((B, 4), 0.25, 2.0)
    else:
        pts = 3.0 * draw.val((B, 3, N))
        prev, motion = draw.val((B, 4)), draw.val((B, 4))
        g, g_aux = draw.val((B, 3, N)), draw.val((B, 4))
    if zero_angles:
        prev[:, 3], motion[:, 3] = 0.0, 0.0
    return Ref(pts=pts, prev=prev, motion=motion, g=g, g_aux=g_aux)


def offset_inputs(draw, B, zero_angles=False):
    if draw.exact:
        ref, off, g = draw.val((B, 4), 0.25, 4.0), draw.val((B, 4), 0.25, 4.0), draw.val((B, 4), 0.25, 2.0)
    else:
        ref, off, g = draw.val((B, 4)), draw.val((B, 4)), draw.val((B, 4))
    if zero_angles:
        ref[:, 3] = 0.0
    return Ref(ref=ref, off=off, g=g)
