"""Side outputs handed from the op that produced a tensor to the op that consumes it, carried on the tensor itself: the
range word of a split16 operand (math_mode), the BatchNorm-backward sums of a graph-conv data gradient and the ReLU mask
of a residual gradient handed over unmasked (bn_op).

This is sound because the entry lives in the tensor object's own attribute dict, and PyTorch keeps a tensor's Python
object alive for as long as anything (autograd included) holds the tensor: a value put on a Function's forward output
reaches the consumer's forward, one put on the gradient a backward returns reaches the upstream backward.  It cannot
outlive its tensor or pass to a new tensor in the same memory; a view, `detach()` or summed gradient is another object
and gets nothing; the version counter stored with the value voids it after any in-place change."""

_ATTR = '_p2r_handoff'


def put(t, key, value):
    """leave `value` on tensor `t` under `key`, valid for `t` in its current state"""
    t.__dict__.setdefault(_ATTR, {})[key] = (t._version, value)


def _valid(t, entry):
    return entry[1] if entry is not None and entry[0] == t._version else None


def peek(t, key):
    """the value left on `t` under `key`, or None when there is none or `t` was modified in place since"""
    return _valid(t, t.__dict__.get(_ATTR, {}).get(key))


def take(t, key):
    """`peek`, and the entry is gone afterwards"""
    return _valid(t, t.__dict__.get(_ATTR, {}).pop(key, None))
