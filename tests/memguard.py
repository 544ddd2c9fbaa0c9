"""Memory-contract harness: guard bands, poisoned allocations and a three-way contract check for op wrappers.

A kernel may be right in every value a test compares and still break what it is allowed to read and write: a store a few
elements past its output lands in the caching allocator's padding, a tile load past the end of a ragged tensor reaches a
sum, a partial slot nobody wrote holds the right number from the previous identical call.  This module makes each of the
three visible without provoking a fault: every access it can expose stays inside a buffer allocated here.

* `guarded(shape, dtype, device, fill, halo, offset_bytes)` -> `(buf, view)`: `view` lies inside the 1-D `buf` with
  `GUARD` elements of halo on either side.  `view` is NOT an autograd view of `buf` (it shares the storage through
  `Tensor.set_`), so it behaves like a freshly allocated tensor: it can be a leaf, an output of an autograd Function, and
  `handoff` entries -- which live on the tensor object -- stay with it.
* poison is a fixed bit pattern compared through an integer view (a computed NaN has another payload): quiet NaN
  0x7FC0BEEF for fp32, 0x7EEF for fp16, 0xA5 for bytes.  Halos of float inputs come as zeros, poison or +3.0e38 (a max-type
  reduction drops NaN but not 3e38); halos of integer inputs are always the valid index 0.
* `poisoned_allocations()` replaces `torch.empty`, `torch.empty_like` and `Tensor.new_empty` for tensors of one device type
  by poison-filled guarded views and records them; `.check()` (also run on a clean exit) asserts every halo is intact,
  `.assert_clean(...)` that no element handed back still carries poison.  `torch.zeros` / `torch.full` are untouched.
* `run_contract(fn, inputs, device, ...)` runs `fn` once plainly over zero halos, then once per halo fill under
  `poisoned_allocations()` and asserts (a) halos of all recorded allocations and inputs intact, inputs unmodified,
  (b) returned tensors and gradients poison-free, (c) every returned tensor and gradient bit-identical across all runs.

Kernels with float atomics, where (c) holds only to the tolerance their own test applies (`tol=` of `run_contract`):
  csrc/interpolate.hip    three_interpolate gradient: atomicAdd(gp + id[k], go * w[k]) (and into LDS, s_acc)
  csrc/group_gather.hip   group / gather gradient, the scatter forms taken when an index list does not fit LDS:
                          atomicAdd(grad_points + bl * n + ii, grad_out[t]); the gather forms the other shapes run are
                          atomic-free and stay exact
  csrc/stgcn_gcn.hip      first-generation adjacency gradient (skeletons other than 53 joints, ragged lengths):
                          atomicAdd(dcs_row + j * V, part[j])
(csrc/stgcn_tconv.hip, the first-generation temporal conv, has no atomic and stays exact.)
"""
import contextlib

import torch

# at least the 4096 elements of the older write-only tests and one 16-frame tile of 53 joints (848 floats); a multiple of
# 512 bytes for every dtype, so that a view at offset 0 keeps the allocator's alignment
GUARD = max(4096, 16 * 53)
assert GUARD % 512 == 0

FILLS = ('zero', 'poison', 'big')
BIG = 3.0e38

_INT_VIEW = {1: (torch.uint8, 0xA5), 2: (torch.int16, 0x7EEF), 4: (torch.int32, 0x7FC0BEEF),
             8: (torch.int64, 0x7FF8BEEF7FC0BEEF)}

_ORIG_EMPTY = torch.empty
_ORIG_EMPTY_LIKE = torch.empty_like
_ORIG_NEW_EMPTY = torch.Tensor.new_empty


class ContractViolation(AssertionError):
    """`kind` names the broken clause: 'halo' (a), 'input-modified' (a), 'poison' (b), 'differs' (c)."""

    def __init__(self, kind, message):
        super().__init__(f"[{kind}] {message}")
        self.kind = kind


def _bits(t):
    """integer view of the same width (bit patterns compare exactly, NaN included)"""
    return t.view(_INT_VIEW[t.element_size()][0])


def poison_value(dtype):
    return _INT_VIEW[_ORIG_EMPTY(0, dtype=dtype).element_size()][1]


def _paint(t, kind):
    if kind == 'poison':
        _bits(t).fill_(poison_value(t.dtype))
    elif kind == 'big' and t.is_floating_point():
        t.fill_(min(BIG, torch.finfo(t.dtype).max))
    elif kind in ('zero', 'big'):
        _bits(t).zero_()
    else:
        raise ValueError(kind)


def _expected_bits(dtype, kind):
    one = _ORIG_EMPTY(1, dtype=dtype)
    _paint(one, kind)
    return int(_bits(one).item())


def guarded(shape, dtype, device, fill='poison', halo='poison', offset_bytes=0, strides=None):
    """-> (buf, view).  fill: 'zero' | 'poison' | 'big' | a tensor to copy | None (leave); halo: 'zero' | 'poison' | 'big'.
    offset_bytes shifts the view's start: 0 keeps the allocator's alignment, 16 gives data_ptr() % 32 == 16, 4 a pointer
    that is not 16-byte aligned."""
    shape = tuple(int(s) for s in shape)
    item = _ORIG_EMPTY(0, dtype=dtype).element_size()
    assert offset_bytes % item == 0, "offset_bytes must be whole elements"
    off = offset_bytes // item
    if strides is None:
        n = 1
        for s in shape:
            n *= s
        strides, acc = [], 1
        for s in reversed(shape):
            strides.append(acc)
            acc *= max(s, 1)
        strides = tuple(reversed(strides))
    else:       # dense non-overlapping layouts only (what empty_like preserves)
        n = 1 + sum((s - 1) * st for s, st in zip(shape, strides)) if all(s > 0 for s in shape) else 0
    buf = _ORIG_EMPTY(n + 2 * GUARD + off, dtype=dtype, device=device)
    _paint(buf, halo)
    view = _ORIG_EMPTY(0, dtype=dtype, device=buf.device).set_(buf.untyped_storage(), GUARD + off, shape, strides)
    if isinstance(fill, torch.Tensor):
        view.copy_(fill)
    elif fill is not None and (fill != halo or not view.is_contiguous()):
        _paint(buf[GUARD + off:GUARD + off + n], fill)
    return buf, view


def _span(buf, view):
    start = view.storage_offset()
    n = buf.numel() - start - GUARD
    return start, n


def halo_damage(buf, view, halo):
    """number of halo elements (0-d device tensor) that no longer hold the pattern"""
    start, n = _span(buf, view)
    want = _expected_bits(buf.dtype, halo)
    b = _bits(buf)
    return (b[:start] != want).sum() + (b[start + n:] != want).sum()


def _describe_damage(buf, view, halo):
    start, n = _span(buf, view)
    want = _expected_bits(buf.dtype, halo)
    b = _bits(buf)
    before = (b[:start] != want).nonzero().flatten()
    after = (b[start + n:] != want).nonzero().flatten()
    parts = []
    if before.numel():
        parts.append(f"{before.numel()} element(s) before the start, nearest at offset {int(before.max()) - start}")
    if after.numel():
        parts.append(f"{after.numel()} element(s) past the end, nearest at offset +{int(after.min())}")
    return "; ".join(parts)


def poison_count(t):
    """number of elements of `t` (0-d tensor) that carry the poison bit pattern"""
    if t.numel() == 0:
        return torch.zeros((), dtype=torch.int64, device=t.device)
    t = t.detach()
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.is_complex() or t.element_size() not in _INT_VIEW:
        return torch.zeros((), dtype=torch.int64, device=t.device)
    tc = t if t.is_contiguous() else t.contiguous()
    return (_bits(tc) == poison_value(t.dtype)).sum()


def _device_or_default(device):
    if device is not None:
        return device
    return torch.get_default_device() if hasattr(torch, 'get_default_device') else 'cpu'


class poisoned_allocations(contextlib.AbstractContextManager):
    """Within the block, `torch.empty` / `torch.empty_like` / `Tensor.new_empty` of tensors on a `device_type` device return
    poison-filled guarded views at the allocator's alignment; everything else passes through."""

    def __init__(self, device_type='cuda'):
        self.device_type = device_type
        self.records = []           # (buf, view)
        self._saved = None

    # -- replacements ----------------------------------------------------------------------------------------------
    def _wants(self, device):
        return torch.device(_device_or_default(device)).type == self.device_type

    def _make(self, shape, dtype, device, requires_grad=False, strides=None):
        buf, view = guarded(shape, dtype, _device_or_default(device), fill='poison', halo='poison', strides=strides)
        if requires_grad:
            view.requires_grad_(True)
        self.records.append((buf, view))
        return view

    @staticmethod
    def _plain(kw):
        return (kw.get('out') is None and kw.get('layout', torch.strided) is torch.strided and not kw.get('pin_memory')
                and kw.get('names') is None
                and kw.get('memory_format', torch.contiguous_format) is torch.contiguous_format)

    def _empty(self, *size, **kw):
        if not (self._plain(kw) and self._wants(kw.get('device'))):
            return _ORIG_EMPTY(*size, **kw)
        if 'size' in kw:
            size = (kw['size'],)
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        return self._make(shape, kw.get('dtype') or torch.get_default_dtype(), kw.get('device'), kw.get('requires_grad', False))

    def _empty_like(self, t, **kw):
        device = kw.get('device', t.device)
        ok = (kw.get('layout', torch.strided) is torch.strided and t.layout is torch.strided and not kw.get('pin_memory')
              and not t.is_quantized and self._wants(device))
        if not ok:
            return _ORIG_EMPTY_LIKE(t, **kw)
        meta = _ORIG_EMPTY_LIKE(t, **{**kw, 'device': 'meta', 'requires_grad': False})     # shape, dtype, preserved strides
        return self._make(meta.shape, meta.dtype, device, kw.get('requires_grad', False), strides=meta.stride())

    def _new_empty(self, t, *size, **kw):
        device = kw.get('device', t.device)
        if not (self._plain(kw) and self._wants(device)):
            return _ORIG_NEW_EMPTY(t, *size, **kw)
        if 'size' in kw:
            size = (kw['size'],)
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        return self._make(shape, kw.get('dtype') or t.dtype, device, kw.get('requires_grad', False))

    # -- context ---------------------------------------------------------------------------------------------------
    def __enter__(self):
        assert self._saved is None
        self._saved = (torch.empty, torch.empty_like, torch.Tensor.__dict__.get('new_empty'))
        me = self
        torch.empty = lambda *a, **k: me._empty(*a, **k)
        torch.empty_like = lambda t, **k: me._empty_like(t, **k)
        torch.Tensor.new_empty = lambda t, *a, **k: me._new_empty(t, *a, **k)
        return self

    def __exit__(self, et, ev, tb):
        torch.empty, torch.empty_like, own = self._saved
        if own is None:
            del torch.Tensor.new_empty
        else:
            torch.Tensor.new_empty = own
        self._saved = None
        if et is None:
            self.check()
        return False

    # -- assertions ------------------------------------------------------------------------------------------------
    def check(self):
        """(a): the halo of every recorded allocation still holds the poison pattern"""
        if not self.records:
            return
        bad = torch.stack([halo_damage(buf, view, 'poison').cpu() for buf, view in self.records])
        for i in bad.nonzero().flatten().tolist():
            buf, view = self.records[i]
            raise ContractViolation('halo', f"allocation #{i} {tuple(view.shape)} {view.dtype}: written outside -- "
                                    + _describe_damage(buf, view, 'poison'))

    def assert_clean(self, *tensors, names=None):
        """(b): no element of a tensor handed back to the caller carries the poison pattern"""
        for i, t in enumerate(tensors):
            if t is None:
                continue
            n = int(poison_count(t))
            if n:
                what = names[i] if names else f"tensor #{i}"
                flat = t.detach().contiguous().view(-1)
                first = int((_bits(flat if flat.dtype != torch.bool else flat.view(torch.uint8))
                             == poison_value(t.dtype)).nonzero()[0])
                raise ContractViolation('poison', f"{what} {tuple(t.shape)}: {n} element(s) never written "
                                        f"(or computed from unwritten memory), first at flat index {first}")


class Input:
    """One input of `run_contract`: a CPU tensor, whether it is a leaf that takes a gradient, and its own offset_bytes
    (None: the call's)."""

    def __init__(self, tensor, grad=False, offset_bytes=None):
        self.tensor, self.grad, self.offset_bytes = tensor, grad, offset_bytes


def guard_module(module, device, halo, registry, offset_bytes=0):
    """deep copy of `module` on `device` with every parameter and buffer inside its own guarded view (recorded in
    `registry` as (name, buf, view, halo, source))"""
    import copy
    m = copy.deepcopy(module)
    for name, p in list(m.named_parameters()) + list(m.named_buffers()):
        h = halo if p.is_floating_point() else 'zero'
        buf, view = guarded(p.shape, p.dtype, device, fill=p.detach(), halo=h, offset_bytes=offset_bytes if p.is_floating_point() else 0)
        p.data = view
        registry.append((name, buf, view, h, None))
    return m


def _flatten(out, prefix='out'):
    """tensor -> {'out': t}; tuple -> {'out.0': ...}; dict -> {'out.<key>': ...}; None entries are dropped"""
    if out is None:
        return {}
    if isinstance(out, torch.Tensor):
        return {prefix: out}
    items = out.items() if isinstance(out, dict) else enumerate(out)
    res = {}
    for k, v in items:
        res.update(_flatten(v, f"{prefix}.{k}"))
    return res


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if a.dtype == torch.bool or a.element_size() not in _INT_VIEW or a.is_complex():
        return bool(torch.equal(a, b))
    return bool(torch.equal(_bits(a), _bits(b)))


def run_contract(fn, inputs, device, offset_bytes=0, fills=FILLS, tol=None, const_inputs=True):
    """fn(**inputs) -> tensor / tuple / dict of tensors; `inputs`: name -> CPU tensor | Input | nn.Module.  Every tensor is
    rebuilt per run inside a guarded view on `device` (float halos: the run's fill; integer halos: 0), modules are copied
    with their parameters and buffers in guarded views.  Gradients of `Input(grad=True)` leaves and of module parameters,
    and module buffers (running statistics), count as returned tensors.
    tol: None = (c) is exact; else a float, or {name: float} for the named results only: |a - b| <= tol * max|b| for float
    tensors (kernels with float atomics only).
    -> the plain run's {name: tensor}."""
    device = torch.device(device)
    dev_type = device.type
    baseline = None
    for run in ('plain',) + tuple(fills):
        halo = 'zero' if run == 'plain' else run
        registry, views, modules = [], {}, {}
        for name, spec in inputs.items():
            if isinstance(spec, torch.nn.Module):
                views[name] = modules[name] = guard_module(spec, device, halo, registry, offset_bytes)
                continue
            if not isinstance(spec, Input):
                spec = Input(spec)
            src = spec.tensor
            isf = src.is_floating_point()
            ob = offset_bytes if spec.offset_bytes is None else spec.offset_bytes
            h = halo if isf else 'zero'
            buf, view = guarded(src.shape, src.dtype, device, fill=src, halo=h, offset_bytes=ob if isf else 0)
            if spec.grad:
                view.requires_grad_(True)
            registry.append((name, buf, view, h, src))
            views[name] = view
        pa = poisoned_allocations(dev_type) if run != 'plain' else None
        with (pa if pa is not None else contextlib.nullcontext()):
            out = fn(**views)
            if dev_type == 'cuda':
                torch.cuda.synchronize(device)
        named = _flatten(out)
        for name, v in views.items():
            if isinstance(v, torch.nn.Module):
                for k, p in v.named_parameters():
                    if p.grad is not None:
                        named[f"grad:{name}.{k}"] = p.grad
                for k, b in v.named_buffers():
                    named[f"buf:{name}.{k}"] = b
            elif v.requires_grad and v.grad is not None:
                named[f"grad:{name}"] = v.grad
        # (a) halos of the inputs (allocation halos were checked on leaving the block), inputs unmodified
        bad = [halo_damage(buf, view, h).cpu() for _, buf, view, h, _ in registry]
        for (name, buf, view, h, src), nbad in zip(registry, bad):
            if int(nbad):
                raise ContractViolation('halo', f"run '{run}': input {name}: written outside -- " + _describe_damage(buf, view, h))
            if const_inputs and src is not None and not same_bits(view.detach().cpu(), src):
                raise ContractViolation('input-modified', f"run '{run}': input {name} was written to")
        # (b)
        if pa is not None:
            keys = list(named)
            pa.assert_clean(*[named[k] for k in keys], names=[f"run '{run}': {k}" for k in keys])
        # (c)
        got = {k: v.detach().clone() for k, v in named.items()}
        if baseline is None:
            baseline = got
            continue
        if set(got) != set(baseline):
            raise ContractViolation('differs', f"run '{run}' returned {sorted(got)}, the plain run {sorted(baseline)}")
        for k, v in got.items():
            ref = baseline[k]
            if same_bits(v, ref):
                continue
            ktol = tol.get(k) if isinstance(tol, dict) else tol
            if ktol is not None and v.is_floating_point() and v.shape == ref.shape:
                err = (v.double() - ref.double()).abs().max().item()
                if err <= ktol * (ref.double().abs().max().item() + 1e-30):
                    continue
            detail = ""
            if v.shape == ref.shape and v.numel():
                diff = (_bits(v.contiguous()) != _bits(ref.contiguous())).view(-1) if v.element_size() in _INT_VIEW and v.dtype != torch.bool \
                    else (v != ref).view(-1)
                idx = diff.nonzero().flatten()
                detail = f": {idx.numel()} of {v.numel()} element(s), first at flat index {int(idx[0])}"
            raise ContractViolation('differs', f"{k} with '{run}' halos differs from the plain run{detail} -- memory outside "
                                    "the tensors reached a result")
    return baseline
