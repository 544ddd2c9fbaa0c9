"""Bernoulli-gated mixture sampling for multi-hypothesis generation (csrc/mdn_sample.hip: p2r_mdn_sample,
p2r_mdn_sample_ex).

`sample(heads, pis, n_samples, seed, h_offset)` draws H hypotheses of up to three mixture heads in one launch:

    out[h, b, l, d] = (1 / n_h) sum_{s < n_h} sum_g [u(h,b,l,g,s) < pi[b,g,l]] (mu[g,d] + exp(log_sigma[g,d]) eps(h,b,l,g,s,d))

-- `MixtureDensityHead.generate_point_predictions(pi, n_h, sample_pi=True)` (mdn.py:49-61, central tendency 'mean')
with the draws taken from an in-kernel Philox4x32-10 stream instead of torch's generator.  `readout='median'` returns the
lower median of the n_h draws instead (the order statistic of rank (n_h - 1) // 2, `torch.median`'s choice) and
`return_draws=True` the draws themselves, `mdn.py`'s `generate_samples`: draw s of a hypothesis is the inner sum over g
above, added in double with g ascending and rounded once to the head's type.  `sample_reference` is the NumPy mirror of
that stream (counter / key layout: the header comment of csrc/mdn_sample.hip); the kernel matches it to rounding, with
identical gate decisions.
"""
import ctypes

import numpy as np
import torch

from .. import _lib

PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
MAX_HEADS, MAX_G, MAX_D, MAX_N = 3, 256, 4, 256


READOUTS = {'mean': 0, 'median': 1}


_SampleHead, _SampleHeadEx = _lib.struct('p2r_mdn_sample_head'), _lib.struct('p2r_mdn_sample_head_ex')


def readout_code(readout):
    if readout not in READOUTS:
        raise ValueError(f"mdn_sample: readout must be 'mean' or 'median', got {readout!r}")
    return READOUTS[readout]


def _pi_layout(pis, G):
    """-> (list of (B, G, L) f32 device tensors sharing one channel stride, ctot)"""
    B, _, L = pis[0].shape
    strided = all(p.stride(2) == 1 and p.stride(1) == L and p.stride(0) == pis[0].stride(0) for p in pis)
    if strided and pis[0].stride(0) % L == 0 and pis[0].stride(0) // L >= G:
        return pis, pis[0].stride(0) // L
    return [p.contiguous() for p in pis], G


def sample(heads, pis, n_samples, seed, h_offset=0, head_ids=None, readout='mean', return_draws=False):
    """heads: up to three MixtureDensityHead modules (their `mu`, `log_sigma`); pis: their (B, G, L) f32 mixture weights
    on one GPU (views into one tensor with a channel stride are passed as they are); n_samples: H counts in 1..256;
    seed: 64-bit int; h_offset: stream index of the first hypothesis; head_ids: stream index of each head (default
    0, 1, 2 in order); readout: 'mean' or 'median' (the lower median of the n_h draws).
    -> [out_i (H, B, L, D_i) in mu_i's dtype] -- per hypothesis the (B, K, D) memory order of `pw_op.proposal_heads`'
    predictions; with return_draws ([out_i], [draws_i (H, B, L, Nmax, D_i)]), Nmax = max(n_samples), the slots
    s >= n_h of hypothesis h zero."""
    code = readout_code(readout)
    if not 1 <= len(heads) <= MAX_HEADS or len(pis) != len(heads):
        raise ValueError(f"mdn_sample: 1..{MAX_HEADS} heads with one pi each, got {len(heads)} / {len(pis)}")
    head_ids = list(range(len(heads))) if head_ids is None else list(head_ids)
    pi0 = pis[0]
    if not all(torch.is_tensor(p) and p.is_cuda and p.dtype == torch.float32 and p.dim() == 3 for p in pis):
        raise RuntimeError("mdn_sample: pi must be (B, G, L) float32 tensors on a GPU")
    if any(p.shape != pi0.shape or p.device != pi0.device for p in pis):
        raise RuntimeError("mdn_sample: every head's pi must have one shape on one device")
    B, G, L = pi0.shape
    ns = [int(n) for n in np.atleast_1d(np.asarray(n_samples))]
    H = len(ns)
    if H < 1:
        raise RuntimeError("mdn_sample: at least one hypothesis")
    dev = pi0.device
    pis, ctot = _pi_layout(list(pis), G)
    ex = return_draws or code != 0          # the plain mean goes through the entry point it always had
    n_max = max(ns) if return_draws else 0
    keep, outs, hs, draws = [], [], [], []
    for i, (mdn, p) in enumerate(zip(heads, pis)):
        mu, ls = mdn.mu.detach(), mdn.log_sigma.detach()
        if mu.device != dev or ls.device != dev or mu.dtype not in (torch.float32, torch.float64) or \
                ls.dtype != torch.float32 or mu.dim() != 2 or mu.shape[0] != G or ls.shape != mu.shape:
            raise RuntimeError(f"mdn_sample: head {i}: mu [G][D] f32/f64 and log_sigma [G][D] f32 on {dev}, G = {G}")
        mu, ls = mu.contiguous(), ls.contiguous()
        D = mu.shape[1]
        out = torch.empty((H, B, L, D), dtype=mu.dtype, device=dev)
        keep += [mu, ls]
        outs.append(out)
        fields = dict(pi=p.data_ptr(), log_sigma=ls.data_ptr(), mu=mu.data_ptr(), out=out.data_ptr(), D=D,
                      f64=int(mu.dtype == torch.float64), head_id=head_ids[i])
        if return_draws:
            draws.append(torch.empty((H, B, L, n_max, D), dtype=mu.dtype, device=dev))
            fields['draws'] = draws[-1].data_ptr()
        hs.append(_SampleHeadEx(**fields) if ex else _SampleHead(**fields))
    arr = (type(hs[0]) * len(hs))(*hs)
    narr = (ctypes.c_int * H)(*ns)
    key = int(seed) & 0xffffffffffffffff
    if ex:
        _lib.launch('p2r_mdn_sample_ex', dev, len(hs), arr, B, G, L, ctot, H, narr, key, int(h_offset), code, n_max)
    else:
        _lib.launch('p2r_mdn_sample', dev, len(hs), arr, B, G, L, ctot, H, narr, key, int(h_offset))
    return (outs, draws) if return_draws else outs


def resolve_draws(num_hypotheses, n_samples=None, seed=None):
    """The defaults of `P2RNet.generate_hypotheses` -> (seed as an unsigned 64-bit int, [n_h] * H).
    seed None: drawn from torch's default CPU generator (so `torch.manual_seed` reproduces a call); n_samples None:
    each n_h uniform in 1..99 (the reference's per-run rule, proposal_net.py:56-59) drawn from that seed; an int or a
    length-H sequence fixes them."""
    H = int(num_hypotheses)
    if H < 1:
        raise ValueError("num_hypotheses must be >= 1")
    if seed is None:
        seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    seed = int(seed) & 0xffffffffffffffff
    if n_samples is None:
        ns = [int(v) for v in np.random.Generator(np.random.PCG64(seed)).integers(1, 100, size=H)]
    elif np.ndim(n_samples) == 0:
        ns = [int(n_samples)] * H
    else:
        ns = [int(v) for v in n_samples]
    if len(ns) != H or not all(1 <= n <= MAX_N for n in ns):
        raise ValueError(f"n_samples: {H} counts in 1..{MAX_N} wanted, got {ns}")
    return seed, ns


# ------------------------------------------------------------------------------------------------------------------
# NumPy mirror of the stream
# ------------------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays (broadcastable), key: 2 uint32 arrays -> 4 uint32 arrays (Random123's philox4x32_10)."""
    c = [np.asarray(x, dtype=np.uint64) for x in ctr]
    k0, k1 = (np.asarray(x, dtype=np.uint64) for x in key)
    m32 = np.uint64(0xffffffff)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(PHILOX_W[0])) & m32
            k1 = (k1 + np.uint64(PHILOX_W[1])) & m32
        p0 = np.uint64(PHILOX_M[0]) * c[0]
        p1 = np.uint64(PHILOX_M[1]) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
    return [x.astype(np.uint32) for x in c]


def _u24(x):
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _u53(a, b):
    return ((a >> np.uint32(5)).astype(np.float64) * 67108864.0 + (b >> np.uint32(6)).astype(np.float64)) * 2.0 ** -53


def _box_muller_f32(u1, u2):
    r = np.sqrt(np.float32(-2.0) * np.log(np.float32(1.0) - u1))
    ang = 2.0 * np.pi * u2.astype(np.float64)
    return r * np.cos(ang).astype(np.float32), r * np.sin(ang).astype(np.float32)


def _box_muller_f64(u1, u2):
    r = np.sqrt(-2.0 * np.log(1.0 - u1))
    ang = 2.0 * np.pi * u2
    return r * np.cos(ang), r * np.sin(ang)


def sample_reference(pi, mu, log_sigma, n_samples, seed, h_offset=0, head_id=0, readout='mean', return_draws=False):
    """Host mirror of one head of `sample`: pi (B, G, L) f32, mu [G][D] f32 or f64, log_sigma [G][D] f32 (NumPy arrays)
    -> (H, B, L, D) in mu's dtype, with return_draws (that, draws (H, B, L, max(n_samples), D)).  Same counters, same
    gate decisions; the mean's sums in double in another order; a draw is the sum over g in double, g ascending,
    rounded to mu's dtype, and the median `np.sort` of the draws at (n - 1) // 2."""
    code = readout_code(readout)
    pi = np.asarray(pi, dtype=np.float32)
    mu = np.asarray(mu)
    ls = np.asarray(log_sigma, dtype=np.float32)
    f64 = mu.dtype == np.float64
    B, G, L = pi.shape
    D = mu.shape[1]
    rows = B * L
    pi_r = pi.transpose(0, 2, 1).reshape(rows, G)                         # [row][g]
    sigma = np.exp(ls.astype(np.float64)) if f64 else np.exp(ls)
    k0, k1 = np.uint32(seed & 0xffffffff), np.uint32((seed >> 32) & 0xffffffff)
    ns = [int(n) for n in np.atleast_1d(np.asarray(n_samples))]
    out = np.empty((len(ns), B, L, D), dtype=mu.dtype)
    draws = np.zeros((len(ns), B, L, max(ns), D), dtype=mu.dtype) if return_draws else None
    row = np.arange(rows, dtype=np.uint32)[:, None, None]
    g = np.arange(G, dtype=np.uint32)[None, :, None]
    for i, n in enumerate(ns):
        h = np.uint32(h_offset + i)
        s = np.arange(n, dtype=np.uint32)[None, None, :]
        c1 = g | (s << np.uint32(8)) | np.uint32(head_id << 16)
        shape = (rows, G, n)
        x = [np.broadcast_to(v, shape) for v in philox4x32_10((row, c1, h, np.uint32(0)), (k0, k1))]
        gate = _u24(x[0]) < pi_r[:, :, None]                               # (rows, G, n)
        eps = []
        if f64:
            for j in range(1, 1 + (D + 1) // 2):
                y = [np.broadcast_to(v, shape) for v in philox4x32_10((row, c1, h, np.uint32(j)), (k0, k1))]
                eps += list(_box_muller_f64(_u53(y[0], y[1]), _u53(y[2], y[3])))
        else:
            eps += list(_box_muller_f32(_u24(x[1]), _u24(x[2])))
            if D > 2:
                y = [np.broadcast_to(v, shape) for v in philox4x32_10((row, c1, h, np.uint32(1)), (k0, k1))]
                eps += list(_box_muller_f32(_u24(y[0]), _u24(y[1])))
        for d in range(D):
            comp = mu[:, d].astype(mu.dtype)[None, :, None] + sigma[:, d].astype(mu.dtype)[None, :, None] * eps[d]
            gated = np.where(gate, comp.astype(np.float64), 0.0)
            if code == 0:
                tot = gated.sum(axis=(1, 2))
                out[i, :, :, d] = (tot / n).astype(mu.dtype).reshape(B, L)
            if code != 0 or return_draws:
                v = np.zeros((rows, n), dtype=np.float64)
                for gi in range(G):                                        # g ascending, one addition each
                    v = v + gated[:, gi, :]
                v = v.astype(mu.dtype)
                if code != 0:
                    out[i, :, :, d] = np.sort(v, axis=1)[:, (n - 1) // 2].reshape(B, L)
                if return_draws:
                    draws[i, :, :, :n, d] = v.reshape(B, L, n)
    return (out, draws) if return_draws else out
