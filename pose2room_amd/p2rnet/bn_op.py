"""BatchNorm (+ residual) (+ ReLU) as one fused op on the HIP kernels of csrc/bn_act.hip.

`fused_bn_act(x, bn, res=None, relu=True)` is numerically the reference's chain
`relu(bn(x) + res)` (stgcn_layers.py:399-439) for an `nn.BatchNorm2d` module `bn`, in train
mode (batch statistics, running-stat update with the module's momentum, unbiased running
variance) and eval mode (running statistics), differentiable w.r.t. x, bn.weight, bn.bias
and res.
"""
import torch
from torch.autograd import Function

from .. import _lib
from . import handoff, math_mode


def _rows(x):
    N, C = x.shape[0], x.shape[1]
    L = x.numel() // max(N * C, 1)
    return N, C, L


def _stats_partial(x):
    """per-(sample, channel) (count, mean, M2) rows [N, C, 3] from one HBM pass (see `moments`)."""
    N, C, L = _rows(x)
    part = torch.empty((N, C, 3), dtype=torch.float32, device=x.device)
    _lib.launch("p2r_bn_stats", x.device, N * C, L, x, part)
    return part


def _stats(x):
    """per-channel (mean, biased var) in fp64 from one HBM pass."""
    N, C, L = _rows(x)
    return moments(_stats_partial(x), N * L)


def finalize(part, M, bn):
    """Kernel partials [P, C, 3] or [P, C, 2] (see `moments`) -> fin [4, C] = (mean, invstd, scale, shift) of
    BatchNorm module `bn` in one launch, which also applies the running-statistics update (momentum, unbiased
    variance) in place."""
    part = part.contiguous()
    P, C, width = part.shape
    fin = torch.empty((4, C), dtype=torch.float32, device=part.device)
    if bn.momentum is None:      # cumulative moving average: the factor depends on the step counter
        mom = 1.0 / float(bn.num_batches_tracked + 1)
    else:
        mom = float(bn.momentum)
    _lib.launch("p2r_bn_finalize", part.device, P, C, width, part, float(M), bn.weight, bn.bias, float(bn.eps), mom,
                bn.running_mean, bn.running_var, bn.num_batches_tracked, fin)
    return fin


def bwd_finalize(part, M):
    """Backward partials [P, C, 2] = (sum g, sum g*xhat) -> [4, C] = (dbeta, dgamma, m1, m2)."""
    part = part.contiguous()
    P, C = part.shape[0], part.shape[1]
    out = torch.empty((4, C), dtype=torch.float32, device=part.device)
    _lib.launch("p2r_bn_bwd_finalize", part.device, P, C, part, float(M), out)
    return out


def moments(part, M):
    """(mean, biased var) in fp64 from kernel partials over M elements per channel.

    [P, C, 3] = (count, mean, M2 = sum of squared differences from that mean) per entry: the statistics pass and the
    third-generation conv epilogues, which take their sums about a pivot so that the variance survives
    |mean| >> std in fp32; merged as p2r_bn_finalize does.  [P, C, 2] = (sum, sum of squares): the first- and
    second-generation conv epilogues (fallback shapes)."""
    part = part.double()
    if part.shape[-1] == 3:
        n = part[..., 0]
        tot = n.sum(0)
        mean = (n * part[..., 1]).sum(0) / tot
        m2 = (part[..., 2] + n * (part[..., 1] - mean) ** 2).sum(0)
        return mean, m2 / tot, float(M)
    tot = part.sum(0)
    mean = tot[:, 0] / M
    var = (tot[:, 1] / M - mean * mean).clamp_(min=0.0)
    return mean, var, float(M)


def _apply(x, scale, shift, res, relu, want_mask=False):
    N, C, L = _rows(x)
    y = torch.empty_like(x)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if (want_mask and relu) else None
    if relu and want_mask and math_mode.split16() and x.dim() == 4 and N > 0:
        # split16 mode: y is (typically) the next block's graph-conv input -- its range word leaves with it
        word = math_mode.new_word(x.device)
        _lib.launch("p2r_bn_apply_amax", x.device, N, C, L, x, scale, shift, res, y, mask, word)
        math_mode.announce(y, word)
    else:
        _lib.launch("p2r_bn_apply", x.device, N, C, L, x, scale, shift, res, int(relu), y, mask)
    return (y, mask) if want_mask else y


# Inspection hook for the ReLU gates behind a BatchNorm: callable(bn_module, x, scale, shift, res) called with the
# BatchNorm's input, its per-channel affine constants (batch or running statistics folded in) and the residual (or None)
# right before the fused kernel evaluates relu(x * scale + shift + res); it may adjust x IN PLACE.  The parity tests use it
# to find the gates whose pre-activation is within rounding of zero and pin them to the reference's recorded state
# (tests/test_model_cpu.py: GateForcer) -- one flipped gate moves the gradients upstream of it by far more than rounding.
GATE_HOOK = None

OVERLAP_APPLY = True      # BatchNorm-backward apply pass on a side stream under the graph conv's gradient kernels
OVERLAP_REDUCE = True     # ... and its reduction pass too (the data-gradient kernel then runs without the sums epilogue)
SIDE_INLINE = False       # tests only: the very same launches as with the overlap on, but issued on the MAIN stream -- what
#                           the side-stream schedule must reproduce bit for bit (a missed join would not)
_SIDE = {}


def _side_stream(dev):
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    st = _SIDE.get(key)
    if st is None:
        st = _SIDE[key] = torch.cuda.Stream(device=dev, priority=-1)
    return st


class BNLink(object):
    """Handshake between a fused BatchNorm (+res) + ReLU and the graph conv that consumes its output y.

    When every use of y goes through one `gcn_op.graph_conv` call (st_gcn_block chains: y is the next block's
    input and identity branch), that op's data-gradient kernel produces the whole gradient of y, so it can also
    emit the two per-channel sums of this BatchNorm's backward from its row epilogue, which replaces the reduction
    pass over the gradient and the saved input.  It leaves them on the gradient it returns (handoff 'bn_sums'), so the
    BatchNorm backward uses them only for that very tensor in that very state (a second consumer of y would make
    autograd hand over a different tensor, or accumulate into this one in place, which bumps the counter)."""
    __slots__ = ('u', 'mask', 'fin', 'versions', 'used')

    def __init__(self):
        self.u = self.mask = self.fin = self.versions = None
        self.used = 0           # how many backward passes took the sums from the graph conv (tests)

    def attach(self, u, mask, fin):
        """The BatchNorm's saved input, ReLU mask bytes and constants.  They are plain references (the consumer is
        another autograd Function, so they cannot ride in ITS saved tensors): the version counters recorded here
        stand in for autograd's saved-tensor check."""
        self.u, self.mask, self.fin = u, mask, fin
        self.versions = (u._version, mask._version, fin._version)

    def intact(self):
        """False when u / mask / fin were modified in place after the forward: the sums would be computed from other
        values than the BatchNorm backward itself reads, so the consumer must not emit them (the BatchNorm then runs
        its own reduction pass, and autograd's own check on ITS saved tensors raises as for any in-place change)."""
        return (self.u is not None and self.versions is not None and
                self.versions == (self.u._version, self.mask._version, self.fin._version))


class _FusedBNAct(Function):
    """Train-mode BatchNorm (+res) (+ReLU).  `fin` [4, C] = (mean, invstd, scale, shift) from `finalize`.

    lazy_res = True (only when `res` is the identity branch handed out by gcn_op.graph_conv(with_residual=True,
    lazy_res=True), whose backward is the one consumer of its gradient): the residual gradient g = dy * mask is not
    written by the backward apply pass; the incoming gradient dy itself is returned for `res` with the mask bytes left on
    it (handoff 'res_mask'), and the graph conv's data-gradient kernel multiplies while it adds (444 MB less written per
    block)."""

    @staticmethod
    def forward(ctx, x, weight, bias, res, fin, relu, link=None, lazy_res=False):
        x = x.contiguous()
        res_c = res.contiguous() if res is not None else None
        # the ReLU mask is kept as one byte per element, so the backward does not re-read y (4 bytes) twice
        y, mask = _apply(x, fin[2], fin[3], res_c, relu, want_mask=True)
        ctx.save_for_backward(x, mask, fin)
        ctx.relu = relu
        ctx.split = math_mode.split16() and relu and x.dim() == 4
        ctx.has_res = res is not None
        ctx.lazy_res = bool(lazy_res) and relu and res is not None
        ctx.link = link if relu else None
        if ctx.link is not None:
            link.attach(x, mask, fin)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mask, fin = ctx.saved_tensors
        mean, invstd, kscale = fin[0], fin[1], fin[2]
        mode = 3 if ctx.relu else 0
        dy = dy.contiguous()
        N, C, L = _rows(x)
        dev = x.device
        link, part, ready = ctx.link, None, None
        sums = handoff.take(dy, 'bn_sums') if link is not None else None
        if sums is not None and sums[0] is link:
            # dy is the gradient the graph conv's data-gradient kernel wrote (gcn_op._GraphConv.backward), in the state
            # it left it in: `part` = the two sums from that kernel's epilogue (or None: reduce here, see below),
            # `ready` = the event recorded right behind that launch
            _, part, ready = sums
            link.used += 1
        side_ok = OVERLAP_APPLY and ready is not None

        def reduce_pass():
            part_ = torch.empty((N, C, 2), dtype=torch.float32, device=dev)
            _lib.launch("p2r_bn_bwd_reduce", dev, N, C, L, dy, mask, x, mean, invstd, mode, None, None, part_)
            return part_

        if part is None and not side_ok:
            part = reduce_pass()

        def apply_pass():
            part_ = part if part is not None else reduce_pass()
            tot_ = bwd_finalize(part_, N * L)                 # (dbeta, dgamma, m1, m2)
            dx_ = torch.empty_like(x)
            dres_ = torch.empty_like(x) if (ctx.has_res and not ctx.lazy_res) else None
            word_ = math_mode.new_word(dev) if ctx.split else None
            if word_ is not None:
                # split16 mode: dx is the incoming gradient of the temporal conv's data-gradient kernel
                _lib.launch("p2r_bn_bwd_apply_amax", dev, N, C, L, dy, mask, x, mean, invstd, kscale, tot_[2], tot_[3], dx_,
                            dres_, word_)
                math_mode.announce(dx_, word_)
            else:
                _lib.launch("p2r_bn_bwd_apply", dev, N, C, L, dy, mask, x, mean, invstd, kscale, tot_[2], tot_[3], mode,
                            None, None, dx_, dres_)
            return tot_, dx_, dres_, word_

        if side_ok and SIDE_INLINE:
            tot, dx, dres, word = apply_pass()
        elif side_ok:
            # dy and the sums were complete at `ready` (recorded right behind the graph conv's data-gradient launch), but
            # this stream still has that op's weight- and adjacency-gradient kernels queued in front of us: ~2 ms of
            # MFMA-bound work that nothing here depends on and that leaves 100+ VGPRs per SIMD and two thirds of the
            # HBM rate unused.  The finalisation and the streaming apply pass go to a side stream that waits for
            # `ready` only and run UNDER those kernels; this stream joins before anything reads the results.
            main, side = torch.cuda.current_stream(dev), _side_stream(dev)
            side.wait_event(ready)
            with torch.cuda.stream(side):
                tot, dx, dres, word = apply_pass()
                done = torch.cuda.Event()
                done.record(side)
            main.wait_event(done)
            for t_ in (tot, dx, dres, word):
                if t_ is not None:
                    t_.record_stream(main)                    # allocated from the side stream's pool, consumed here
        else:
            tot, dx, dres, word = apply_pass()
        if ctx.lazy_res:
            handoff.put(dy, 'res_mask', mask)
            dres = dy
        return dx, tot[1], tot[0], dres, None, None, None, None


class _EvalBNAct(Function):
    """eval mode: fixed statistics, y = relu(x*scale + shift + res).  scale / shift are torch expressions of
    bn.weight / bn.bias and the running statistics, so returning their gradients (sum g*x, sum g per channel)
    lets autograd carry them on to the affine parameters like nn.BatchNorm2d does in eval mode."""

    @staticmethod
    def forward(ctx, x, scale, shift, res, relu):
        x = x.contiguous()
        y = _apply(x, scale.contiguous(), shift.contiguous(), res.contiguous() if res is not None else None, relu)
        ctx.save_for_backward(x, y, scale)
        ctx.relu, ctx.has_res = relu, res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, scale = ctx.saved_tensors
        g = dy * (y > 0) if ctx.relu else dy
        dims = [d for d in range(dy.dim()) if d != 1]
        dscale = dshift = None
        if ctx.needs_input_grad[1]:
            dscale = (g.double() * x).sum(dims).float()
        if ctx.needs_input_grad[2]:
            dshift = g.double().sum(dims).float()
        dx = g * scale.view(1, -1, *([1] * (dy.dim() - 2))) if ctx.needs_input_grad[0] else None
        return dx, dscale, dshift, (g if ctx.has_res else None), None


def supported(x, bn):
    return x.is_cuda and x.dtype == torch.float32 and bn.affine and bn.track_running_stats and x.dim() >= 3


def fused_bn_act(x, bn, res=None, relu=True, stats=None, link=None, lazy_res=False):
    """stats: optional kernel partials [P, C, 3 | 2] of x (see `moments`) replacing the statistics pass.
    link: a `BNLink` to hang on the result (train mode) for the graph conv that consumes it.
    lazy_res: True when the graph conv that handed out `res` takes its gradient unmasked, see `_FusedBNAct` (train mode
    only)."""
    if bn.training:
        part = _stats_partial(x.contiguous()) if stats is None else stats
        fin = finalize(part, x.numel() // x.shape[1], bn)
        if GATE_HOOK is not None and relu:
            GATE_HOOK(bn, x, fin[2], fin[3], res)
        y = _FusedBNAct.apply(x, bn.weight, bn.bias, res, fin, relu, link, lazy_res)
        if link is not None and relu:
            y._p2r_bn_link = link
        return y
    invstd = torch.rsqrt(bn.running_var + bn.eps)
    scale = bn.weight * invstd
    shift = bn.bias - bn.running_mean * scale
    if GATE_HOOK is not None and relu:
        GATE_HOOK(bn, x, scale.detach(), shift.detach(), res)
    return _EvalBNAct.apply(x, scale, shift, res, relu)
