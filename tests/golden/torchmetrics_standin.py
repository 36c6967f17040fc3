"""A small stand-in for torchmetrics for the metrics fixture generator (TEST ONLY): torchmetrics is not installed where the
fixtures are made, and the reference's utils/metrics.py (TorchSuccess, TorchPrecision) needs only this much of it -- a `Metric`
base with `add_state` and `__call__` -> `update`, and `utilities.data.dim_zero_cat`.  The arithmetic of the two metrics
(`value`, `compute`) is the reference's own and runs unchanged on top of this."""
import copy
import types

import torch


class Metric:
    def __init__(self, dist_sync_on_step=False, **kwargs):
        self._defaults = {}

    def add_state(self, name, default, dist_reduce_fx=None, persistent=False):
        self._defaults[name] = default
        setattr(self, name, copy.deepcopy(default))

    def reset(self):
        for name, default in self._defaults.items():
            setattr(self, name, copy.deepcopy(default))

    def __call__(self, *args, **kwargs):
        return self.update(*args, **kwargs)


def dim_zero_cat(x):
    """torchmetrics.utilities.data.dim_zero_cat: a list of tensors -> their concatenation along dim 0 (0-dim ones as
    1-element); an empty list -> an empty tensor"""
    if isinstance(x, torch.Tensor):
        return x
    x = [y.unsqueeze(0) if y.numel() == 1 and y.ndim == 0 else y for y in x]
    if not x:
        return torch.empty(0)
    return torch.cat(x, dim=0)


utilities = types.ModuleType("torchmetrics.utilities")
utilities.data = types.ModuleType("torchmetrics.utilities.data")
utilities.data.dim_zero_cat = dim_zero_cat
