"""Train from a config: the reference's entry point (main.py:66-86) without Lightning.

`fit(model, train, val, epochs=..., batch_size=...)` is main.py's training run as a composition of what the package already
has, and nothing new below it:

    batches      sampler.SiameseBatchBuilder / MotionBatchBuilder (by model type) inside a
                 sampler.DeviceBatchSampler(shuffle=True, plan_batches=P, rank, world): DataLoader(shuffle=True, drop_last=True)
    steps        dist.DataParallelStep(graph=True, grad_clip=config.gradient_clip_val), `next_batch` passed so that the
                 sampling prefetch runs beside the step
    schedule     DataParallelStep.epoch_end(): the StepLR of the model's configure_optimizers, once per epoch
    validation   tracking.evaluate(model, val, **val_kwargs) after every check_val_every_n_epoch-th epoch
    checkpoints  last.ckpt every epoch, epoch={e}-step={s}.ckpt kept by save_top_k on `precision` (mode max):
                 ModelCheckpoint(monitor='precision/test', mode='max', save_last=True, save_top_k=k) of main.py:78-79

Order of events of an epoch: begin the sampler's epoch; the steps (the total loss of every step is added on the device and read
back ONCE, after the last step: no per-step .item()); epoch_end() (the schedule is stepped BEFORE anything is saved, so a
resumed run continues with the next epoch's learning rate); sync_buffers(); validation on every rank (model.eval(), a FRESH
tracker per validation -- tracking.evaluate builds one -- so no graph captured before later training steps is replayed,
model.train()); rank 0 writes last.ckpt and, by the top-k rule, the epoch's file.  There are no sanity validation steps
(main.py:84 asks Lightning for two; they compute nothing that is kept).

Checkpoint files are torch.save of tensors, numbers, strings, lists and dicts only (they load with weights_only=True), keyed
like a Lightning 1.3.8 checkpoint: epoch, global_step, state_dict, optimizer_states, lr_schedulers, hyper_parameters (the
config as a plain dict) -- plus `sampler` (seed, epoch, the builder's build counter), `monitor` (the kept files and their
scores) and `history`.  Lightning is not a dependency and was not available when this was written: the key layout is restated
from memory and UNPINNED against a real Lightning checkpoint; `epoch` counts finished epochs and `global_step` optimizer steps.
load_checkpoint accepts any dict with a `state_dict` (weights only), which is what a pretrained reference checkpoint reduces to.

More than one rank: every rank validates, rank 0 writes; this path is UNTESTED on more than one rank.
"""
import os

import torch

CKPT_KEYS = ("epoch", "global_step", "state_dict", "optimizer_states", "lr_schedulers", "hyper_parameters")
MONITOR, MODE = "precision", "max"


# ---- pure host pieces (tests/test_optim_oracle_cpu.py) ------------------------------------------------------------------------
def validates_after(epoch, check_val_every_n_epoch):
    """does validation run after (0-based) epoch `epoch`?  Lightning's rule: (epoch + 1) % check_val_every_n_epoch == 0"""
    n = int(check_val_every_n_epoch)
    if n < 1:
        raise ValueError("check_val_every_n_epoch must be >= 1")
    return (int(epoch) + 1) % n == 0


def top_k_update(kept, name, score, k):
    """ModelCheckpoint's save_top_k bookkeeping with mode max.  kept: [[score, name], ...] of the files on disk, best first;
    (name, score): this epoch's candidate; score None: the epoch did not validate.  k = -1 keeps every epoch's file, 0 none, k > 0
    the best k by score -- a new file enters only when fewer than k are kept or it is STRICTLY better than the worst kept one.
    -> (new kept list, save this one?, names to delete)"""
    k = int(k)
    kept = [list(x) for x in kept]
    if k == 0:
        return kept, False, []
    if k < 0:
        return kept + [[score, name]], True, []
    if score is None or score != score:                   # nothing to rank by (no validation, or a NaN metric)
        return kept, False, []
    if len(kept) >= k and not score > kept[-1][0]:
        return kept, False, []
    kept.append([score, name])
    kept.sort(key=lambda x: -x[0])                      # stable: among equals the older file stays in front
    drop = kept[k:]
    return kept[:k], True, [x[1] for x in drop]


def checkpoint_name(epoch, global_step):
    return "epoch=%d-step=%d.ckpt" % (epoch, global_step)


def _plain(x):
    """tuples -> lists, recursively; anything but tensors, numbers, strings, None, lists and dicts is refused"""
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if torch.is_tensor(x):
        return x.detach().cpu()
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if hasattr(x, "item") and getattr(x, "shape", None) == ():      # a numpy scalar
        return x.item()
    raise TypeError("checkpoint: a %s does not belong in a checkpoint file" % type(x).__name__)


# ---- checkpoints ------------------------------------------------------------------------------------------------------------
def checkpoint_dict(model, step, epoch, global_step, sampler=None, monitor=None, history=None):
    config = getattr(model, "config", None)
    hyper = dict(config) if isinstance(config, dict) else dict(vars(config)) if config is not None else {}
    ckpt = {"epoch": int(epoch), "global_step": int(global_step),
            "state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
            "optimizer_states": [step.optimizer.state_dict()],
            "lr_schedulers": [step.scheduler.state_dict()] if step.scheduler is not None else [],
            "hyper_parameters": hyper,
            "monitor": {"monitor": MONITOR, "mode": MODE, "kept": monitor or []},
            "history": history or []}
    if sampler is not None:
        ckpt["sampler"] = {"seed": sampler.seed, "epoch": sampler.epoch, "counter": sampler.builder.counter}
    return _plain(ckpt)


def save_checkpoint(path, model, step, epoch, global_step, sampler=None, monitor=None, history=None):
    """model: the tracker; step: its DataParallelStep (optimizer and schedule); epoch: finished epochs; global_step: optimizer
    steps taken; sampler: the DeviceBatchSampler whose seed, epoch and build counter a resumed run continues from"""
    tmp = str(path) + ".tmp"
    torch.save(checkpoint_dict(model, step, epoch, global_step, sampler, monitor, history), tmp)
    os.replace(tmp, str(path))


def load_checkpoint(path):
    """-> the checkpoint dict of `path`, every key of a full checkpoint present: a file that holds weights only -- any dict with
    a `state_dict` -- comes back with epoch 0, global_step 0 and no optimizer, schedule, sampler or monitor state"""
    ckpt = torch.load(str(path), map_location="cpu", weights_only=True)
    if not isinstance(ckpt, dict) or not isinstance(ckpt.get("state_dict"), dict):
        raise ValueError("load_checkpoint: %s holds no `state_dict`" % path)
    out = {"epoch": 0, "global_step": 0, "optimizer_states": [], "lr_schedulers": [], "hyper_parameters": {},
           "monitor": {"monitor": MONITOR, "mode": MODE, "kept": []}, "history": [], "sampler": None}
    out.update(ckpt)
    return out


# ---- the loop ---------------------------------------------------------------------------------------------------------------
def make_sampler(model, train, batch_size, candidates=None, capacity=None, seed=0, plan_batches=8, rank=0, world=1):
    """the planned, shuffled epoch of `train` (a sampler.DeviceTracklets) for `model`: MotionBatchBuilder for M2-Track, else
    SiameseBatchBuilder, both reading the data keys of model.config"""
    from . import m2track, sampler as S
    motion = isinstance(model, m2track.M2TRACK)
    cls = S.MotionBatchBuilder if motion else S.SiameseBatchBuilder
    kw = {} if capacity is None else {"capacity": capacity}
    builder = cls(model.config, batch_size, candidates=candidates, seed=seed, **kw)
    return S.DeviceBatchSampler(train, builder, seed=seed, shuffle=True, plan_batches=plan_batches, rank=rank, world=world)


def fit(model, train, val=None, *, epochs, batch_size, candidates=None, capacity=None, plan_batches=8, seed=0,
        check_val_every_n_epoch=1, val_kwargs=None, ckpt_dir=None, save_top_k=-1, resume=None, graph=True, graph_warmup=3,
        require_graph=None, rank=None, world=None, on_step=None):
    """Train `model` (on its GPU, in train mode) for `epochs` epochs on `train` and validate on `val` (both
    sampler.DeviceTracklets; val None: no validation) -> history, one dict per epoch of THIS and, after `resume`, the earlier
    runs: {"epoch", "global_step", "steps", "loss" (mean total loss of the epoch's steps), "lr" (the epoch's learning rate),
    "val" (tracking.evaluate's dict | None)}.  epochs, batch_size, save_top_k, check_val_every_n_epoch, resume (a checkpoint
    path) are main.py's --epoch, --batch_size, --save_top_k, --check_val_every_n_epoch, --checkpoint; gradient_clip_val,
    optimizer, lr, wd, lr_decay_step, lr_decay_rate come from model.config.  ckpt_dir None: nothing is written.
    candidates / capacity / plan_batches / seed: the batch builder's and the planned epoch's; val_kwargs: tracking.evaluate's.
    on_step(epoch, batch, loss): called after every step with the batch dict and the step's loss (a device tensor), for
    logging; whatever it reads back is its own synchronisation."""
    from . import dist as D, tracking
    if rank is None or world is None:
        r, _, w = D.env_rank()
        rank, world = (r if rank is None else rank), (w if world is None else world)
    ckpt = load_checkpoint(resume) if resume is not None else None
    if ckpt is not None:
        model.load_state_dict(ckpt["state_dict"])
    clip = getattr(model.config, "gradient_clip_val", None) if not isinstance(model.config, dict) \
        else model.config.get("gradient_clip_val")
    it = make_sampler(model, train, batch_size, candidates, capacity, seed, plan_batches, rank, world)
    step = D.DataParallelStep(model, world=world, graph=graph, graph_warmup=graph_warmup, require_graph=require_graph,
                              grad_clip=clip)
    first, global_step, kept, history = 0, 0, [], []
    if ckpt is not None:
        first, global_step = int(ckpt["epoch"]), int(ckpt["global_step"])
        if ckpt["optimizer_states"]:
            step.optimizer.load_state_dict(ckpt["optimizer_states"][0])
        if ckpt["lr_schedulers"] and step.scheduler is not None:
            step.scheduler.load_state_dict(ckpt["lr_schedulers"][0])
        kept, history = [list(x) for x in ckpt["monitor"]["kept"]], list(ckpt["history"])
        if ckpt["sampler"] is not None:
            if int(ckpt["sampler"]["seed"]) != it.seed:
                raise ValueError("fit(resume=...): the checkpoint's epochs were drawn with seed %d, this run asks for %d"
                                 % (ckpt["sampler"]["seed"], it.seed))
            it.epoch, it.builder.counter = int(ckpt["sampler"]["epoch"]), int(ckpt["sampler"]["counter"])
    if ckpt_dir is not None and rank == 0:
        os.makedirs(str(ckpt_dir), exist_ok=True)
    model.train()
    dev = next(model.parameters()).device
    for epoch in range(first, int(epochs)):
        lr = float(step.optimizer.param_groups[0]["lr"])
        batches = iter(it)                                # begins the sampler's next epoch
        total, steps = torch.zeros((), device=dev, dtype=torch.float32), 0
        cur = next(batches, None)
        while cur is not None:
            nxt = next(batches, None)                     # built before the step: its sampling prefetch runs beside it
            loss = step.step(cur, next_batch=nxt)
            total += loss
            steps += 1
            if on_step is not None:
                on_step(epoch, cur, loss)
            cur = nxt
        global_step += steps
        step.epoch_end()
        row = {"epoch": epoch, "global_step": global_step, "steps": steps,
               "loss": float(total) / steps if steps else None, "lr": lr, "val": None}        # THE read-back of the epoch
        step.sync_buffers()
        if val is not None and validates_after(epoch, check_val_every_n_epoch):
            model.eval()
            try:
                row["val"] = _plain(tracking.evaluate(model, val, **(val_kwargs or {})))
            finally:
                model.train()
        history.append(row)
        if ckpt_dir is not None and rank == 0:
            name = checkpoint_name(epoch, global_step)
            score = row["val"][MONITOR] if row["val"] is not None else None
            kept, save, drop = top_k_update(kept, name, score, save_top_k)
            for path in [os.path.join(str(ckpt_dir), "last.ckpt")] + ([os.path.join(str(ckpt_dir), name)] if save else []):
                save_checkpoint(path, model, step, epoch + 1, global_step, it, kept, history)
            for old in drop:
                if os.path.exists(os.path.join(str(ckpt_dir), old)):
                    os.remove(os.path.join(str(ckpt_dir), old))
    return history
