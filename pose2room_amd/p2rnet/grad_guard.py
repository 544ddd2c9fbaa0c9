"""Gradient clipping and a non-finite step guard on the device, without a host synchronisation.

Between `backward()` and `optimizer.step()` the reference clips by the global norm (models/training.py:35-37,
`optimizer.clip_norm`), which torch does with a norm per tensor, a stack, a second norm, a few scalar operations and one
more pass over every gradient; and nothing keeps an `inf` or a NaN in one gradient from reaching AdamW, whose moments it
poisons for the rest of the run.  `GradGuard` does both with one reduction over the gradients (csrc/grad_guard.hip,
include/p2r_grad_guard.h): two launches for up to 160 tensors yield the global L2 norm accumulated in float64, the count
of non-finite entries per parameter, the clipping divisor and a skip flag -- all of them in device memory, which the
optimizer reads there.

  * torch's fused Adam / AdamW takes the two numbers itself: `optimizer.grad_scale` and `optimizer.found_inf`, the
    attributes that `torch.amp.GradScaler` sets (torch/optim/adam.py reads them with getattr).  With `grad_scale` the
    fused kernel divides every gradient by it and writes the quotient back into `p.grad`; with `found_inf == 1` it leaves
    the parameters, both moments and the step counters as they were.  No further pass, no further launch.
  * any other optimizer gets the clipped gradients from `p2r_grad_scale` (in place, one launch per 160 tensors, which
    returns at once when nothing is to clip).  It cannot skip: zeroed gradients are no skipped step -- AdamW would still
    decay the moments, apply the weight decay and count the step -- so `nonfinite='skip'` is refused for it.

`grad_guard_reference` is the contract in float64 on the host; the tests compare the kernels with it.  There is no CPU
fallback: parameters on the CPU are refused, a missing library is a `P2RLibraryError`.
"""
import math

import torch

from .. import _lib

CHUNK = 16384           # P2R_GG_CHUNK of include/p2r_grad_guard.h: elements per partial sum
GROUP = 160             # P2R_GG_GROUP: table entries per launch
NONFINITE = ('ignore', 'skip', 'raise')
_DTYPES = {torch.float32: 0, torch.float64: 1}      # P2R_GG_F32, P2R_GG_F64

_library = _lib.extension("grad_guard")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib = _library.lib


def entry_type():
    """the ctypes.Structure of p2r_grad_entry, from the header"""
    return _library.struct("p2r_grad_entry")


# ---- the contract ---------------------------------------------------------------------------------------------------------
def grad_guard_reference(grads, max_norm):
    """The float64 mirror of p2r_grad_measure and of the clipped gradients.

    grads: an ordered list of float32 / float64 tensors of any numel >= 0, or None (skipped, keeps its slot);
    max_norm: <= 0 measures only.
    -> {'sumsq': [S_i] (python floats), 'nonfinite': [c_i] (ints), 'norm': float, 'found': 0.0 | 1.0,
        'scale': float (a float32 value), 'clipped': [g / scale in g's own precision, or None]}
    S_i runs over the finite elements of gradient i only, so the norms stay readable on the step that went bad."""
    sumsq, bad, clipped = [], [], []
    for g in grads:
        if g is None:
            sumsq.append(0.0)
            bad.append(0)
            continue
        if g.dtype not in _DTYPES:
            raise ValueError(f"grad_guard_reference: float32 or float64 gradients, got {g.dtype}")
        x = g.detach().cpu().reshape(-1).double()
        fin = torch.isfinite(x)
        x = torch.where(fin, x, torch.zeros_like(x))
        sumsq.append(float((x * x).sum(dtype=torch.float64)) if x.numel() else 0.0)
        bad.append(int(x.numel() - int(fin.sum())))
    total = 0.0
    for s in sumsq:
        total += s
    norm = math.sqrt(total)
    found = 1.0 if sum(bad) > 0 else 0.0
    if max_norm > 0:
        scale = float(torch.tensor(max(1.0, (norm + 1e-6) / float(max_norm)), dtype=torch.float64).float())
    else:
        scale = 1.0
    for g in grads:
        if g is None:
            clipped.append(None)
        else:
            c = g.detach().cpu()
            clipped.append(c / torch.tensor(scale, dtype=c.dtype))
    return {'sumsq': sumsq, 'nonfinite': bad, 'norm': norm, 'found': found, 'scale': scale, 'clipped': clipped}


# ---- the launches -----------------------------------------------------------------------------------------------------------
def n_chunks(numels):
    """chunks of a table: every entry owns at least one (p2r_grad_guard.h)"""
    return sum(max(1, -(-int(n) // CHUNK)) for n in numels)


def _table(grads, names=None):
    """-> (ctypes array of p2r_grad_entry, numels, device) of a list of gradients / None; every tensor is checked"""
    E = entry_type()
    table = (E * max(len(grads), 1))()
    numels, device = [], None
    for i, g in enumerate(grads):
        if g is None:
            numels.append(0)
            continue
        who = names[i] if names is not None else f"gradient {i}"
        if not g.is_cuda:
            raise RuntimeError(f"grad_guard: the gradient of {who} must be a GPU tensor (no CPU fallback)")
        if g.dtype not in _DTYPES:
            raise ValueError(f"grad_guard: the gradient of {who} is {g.dtype}; float32 or float64 expected")
        if not g.is_contiguous():
            raise ValueError(f"grad_guard: the gradient of {who} is not contiguous")
        if device is None:
            device = g.device
        elif g.device != device:
            raise RuntimeError(f"grad_guard: the gradient of {who} is on {g.device}, others on {device}")
        n = g.numel()
        table[i].data = g.data_ptr() if n else None
        table[i].numel = n
        table[i].dtype = _DTYPES[g.dtype]
        numels.append(n)
    return table, numels, device


class Measured(object):
    """The device tensors of one `measure`: sumsq (n) f64, nonfinite (n) i32, norm (1) f64, scale (1) f32, found (1) f32,
    steps (1) i64, skipped (1) i64, and the work buffers part_sumsq / part_count (chunks), first_chunk (n)."""
    _FIELDS = ('sumsq', 'nonfinite', 'norm', 'scale', 'found', 'steps', 'skipped', 'part_sumsq', 'part_count',
               'first_chunk')

    def __init__(self, n, chunks, device):
        self.n, self.chunks, self.device = n, chunks, device
        self.sumsq = torch.empty((n,), dtype=torch.float64, device=device)
        self.nonfinite = torch.empty((n,), dtype=torch.int32, device=device)
        self.norm = torch.empty((1,), dtype=torch.float64, device=device)
        self.scale = torch.empty((1,), dtype=torch.float32, device=device)
        self.found = torch.empty((1,), dtype=torch.float32, device=device)
        self.steps = torch.zeros((1,), dtype=torch.int64, device=device)
        self.skipped = torch.zeros((1,), dtype=torch.int64, device=device)
        self.part_sumsq = torch.empty((chunks,), dtype=torch.float64, device=device)
        self.part_count = torch.empty((chunks,), dtype=torch.int32, device=device)
        self.first_chunk = torch.empty((n,), dtype=torch.int32, device=device)

    def tensors(self):
        return {f: getattr(self, f) for f in self._FIELDS}


def measure(grads, max_norm, count_skips=False, out=None, device=None, names=None):
    """p2r_grad_measure over a list of GPU gradients / None on the current stream: no synchronisation, the gradients are
    not modified.  `out`: the `Measured` of an earlier call over a list of the same numels (its buffers are written again
    and its counters move on); None allocates one, with counters at zero.  `device`: needed only when every entry is None.
    -> Measured"""
    table, numels, dev = _table(grads, names)
    dev = dev if dev is not None else (out.device if out is not None else device)
    if dev is None:
        raise ValueError("grad_guard.measure: no gradient and no device")
    dev = torch.device(dev)
    chunks = n_chunks(numels)
    if out is None:
        out = Measured(len(grads), chunks, dev)
    elif out.n != len(grads) or out.chunks != chunks or out.device != dev:
        raise ValueError(f"grad_guard.measure: `out` was made for {out.n} gradients in {out.chunks} chunks on {out.device}, "
                         f"got {len(grads)} in {chunks} on {dev}")
    _library.launch("p2r_grad_measure", dev, table, len(grads), float(max_norm), int(bool(count_skips)), chunks,
                    out.part_sumsq, out.part_count, out.first_chunk, out.sumsq, out.nonfinite, out.norm, out.scale,
                    out.found, out.steps, out.skipped)
    return out


def scale_grads(grads, scale, names=None):
    """p2r_grad_scale: g = g / scale in place for every gradient of the list, `scale` (1) f32 on the device; returns at
    once on the device when scale == 1.  No synchronisation."""
    table, numels, dev = _table(grads, names)
    if dev is None or not any(numels):
        return
    if not (torch.is_tensor(scale) and scale.dtype == torch.float32 and scale.numel() == 1 and scale.device == dev):
        raise ValueError(f"grad_guard.scale_grads: scale must be one float32 on {dev}")
    _library.launch("p2r_grad_scale", dev, table, len(grads), scale)


# ---- the guard --------------------------------------------------------------------------------------------------------------
def takes_found_inf(optimizer):
    """True for the optimizers that read `grad_scale` / `found_inf` on the device themselves: torch's fused Adam / AdamW"""
    return (isinstance(optimizer, torch.optim.Adam) and len(optimizer.param_groups) > 0
            and all(bool(g.get('fused')) for g in optimizer.param_groups))


class GradGuard(object):
    """Measures the gradients of `named_params` before every optimizer step, clips them to `max_norm` (<= 0: measure
    only) and treats a step with a non-finite gradient as `nonfinite` says:
      'ignore'  the step is taken as today;
      'skip'    the optimizer leaves parameters, moments and step counters untouched (fused Adam / AdamW only);
      'raise'   like 'skip' where the optimizer can, then one synchronisation per step and a FloatingPointError that
                names the first parameter, in the order of `named_params`, with a non-finite gradient entry.
    `step(optimizer)` replaces clip + `optimizer.step()`; `report()` reads the numbers of the last step.  Only `report`
    and 'raise' synchronise.  `optimizer`: checked at construction when given (a 'skip' that cannot be is a ValueError)."""

    def __init__(self, named_params, max_norm, nonfinite='ignore', optimizer=None):
        if nonfinite not in NONFINITE:
            raise ValueError(f"GradGuard: nonfinite must be one of {NONFINITE}, got {nonfinite!r}")
        self.nonfinite = nonfinite
        self._checked = None
        if optimizer is not None:
            self._check_optimizer(optimizer)
        named = [(n, p) for n, p in named_params if p.requires_grad]
        if not named:
            raise ValueError("GradGuard: no parameter that takes a gradient")
        for name, p in named:
            if not p.is_cuda:
                raise RuntimeError(f"GradGuard: parameter {name} must be on a GPU (no CPU fallback)")
            if p.dtype not in _DTYPES:
                raise ValueError(f"GradGuard: parameter {name} is {p.dtype}; float32 or float64 expected")
        if len({p.device for _, p in named}) > 1:
            raise RuntimeError("GradGuard: all parameters must be on one device")
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        self.max_norm = float(max_norm)
        self.device = self.params[0].device
        self._out = None
        lib()

    def _check_optimizer(self, optimizer):
        if self._checked is not optimizer:
            if self.nonfinite == 'skip' and not takes_found_inf(optimizer):
                raise ValueError(f"GradGuard: nonfinite='skip' needs an optimizer that reads found_inf on the device (torch's "
                                 f"fused Adam / AdamW); {type(optimizer).__name__} cannot leave a step out, and zeroed "
                                 "gradients are no skipped step")
            self._checked = optimizer
        return takes_found_inf(optimizer)

    def measure(self):
        """the reduction alone, over the parameters' current gradients -> Measured (device tensors, no synchronisation)"""
        grads = [p.grad for p in self.params]
        self._out = measure(grads, self.max_norm, self.nonfinite != 'ignore', self._out, self.device, self.names)
        return self._out

    def step(self, optimizer):
        fused = self._check_optimizer(optimizer)
        out = self.measure()
        clip = self.max_norm > 0
        guard = self.nonfinite != 'ignore'
        if fused:
            try:
                # 0-dim views: the optimizer subtracts found_inf from its 0-dim step counters in place
                if clip:
                    optimizer.grad_scale = out.scale.view(())
                if guard:
                    optimizer.found_inf = out.found.view(())
                optimizer.step()
            finally:        # the guard is in use for this call only
                for attr in ('grad_scale', 'found_inf'):
                    if attr in optimizer.__dict__:
                        delattr(optimizer, attr)
            if self.nonfinite == 'raise':
                self._raise_if_found(out)
        else:
            if self.nonfinite == 'raise':
                self._raise_if_found(out)
            if clip:
                scale_grads([p.grad for p in self.params], out.scale, self.names)
            optimizer.step()

    def _raise_if_found(self, out):
        counts = out.nonfinite.tolist()             # the one synchronisation of 'raise'
        for name, c in zip(self.names, counts):
            if c:
                raise FloatingPointError(f"GradGuard: the gradient of {name} has {c} non-finite "
                                         f"entr{'y' if c == 1 else 'ies'} ({sum(1 for k in counts if k)} parameter(s) "
                                         "affected)")

    def report(self):
        """-> {'steps', 'skipped', 'norm', 'scale', 'per_parameter': {name: (norm_i, nonfinite_i)}} of the last measured
        step; synchronises."""
        if self._out is None:
            raise RuntimeError("GradGuard.report: no step was measured yet")
        out = self._out
        sumsq, counts = out.sumsq.tolist(), out.nonfinite.tolist()
        return {'steps': int(out.steps.item()), 'skipped': int(out.skipped.item()), 'norm': float(out.norm.item()),
                'scale': float(out.scale.item()),
                'per_parameter': {n: (math.sqrt(s), int(c)) for n, s, c in zip(self.names, sumsq, counts)}}
