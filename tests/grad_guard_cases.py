"""Case tables of the gradient guard (pose2room_amd/p2rnet/grad_guard.py, csrc/grad_guard.hip), shared by
test_grad_guard_cpu.py and test_grad_guard_gpu.py.  Everything here is CPU data made from seeds; the float64 contract the
cases are compared with is `grad_guard.grad_guard_reference`."""
import torch

CHUNK = 16384                   # P2R_GG_CHUNK: the elements of one partial sum
# every numel at which the kernel takes another path: nothing, less than one 16-byte group, around one wave (64 lanes x 1),
# around one pass of the 256 threads (256 elements = 64 groups of f32), around 1024 = one group per thread, several
# passes, and more than two chunks whatever the last one holds
NUMELS = (0, 1, 3, 63, 64, 65, 255, 256, 257, 1023, 4097, 70001)
assert NUMELS[-1] > 2 * CHUNK
OFFSETS = (0, 1, 2, 3)          # element offsets of the views: the 16-byte loads meet every misalignment

TWO_M22 = 2.0 ** -22            # one rounding of scale to f32, one of the quotient, one of the store: 3 * 2^-24 < 2^-22


def mixed_list(seed=0, numels=NUMELS, none_at=None, scale=1.0):
    """-> list of CPU gradients: numels in order, float64 and float32 alternating (the longest is float32, the one in
    front of it float64), one None slot in the middle (or at `none_at`)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(numels):
        dt = torch.float64 if i % 2 == 0 else torch.float32
        out.append((torch.randn(n, generator=g, dtype=torch.float64) * scale).to(dt))
    out.insert(len(out) // 2 if none_at is None else none_at, None)
    return out


def many_small(seed=1, count=700):
    """700 tensors of 1 to 3 elements (more than any per-launch table holds), every seventh float64, every 50th None"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(count):
        if i % 50 == 17:
            out.append(None)
            continue
        dt = torch.float64 if i % 7 == 3 else torch.float32
        out.append(torch.randn(1 + i % 3, generator=g, dtype=torch.float64).to(dt))
    return out


# (tensor index in `nonfinite_list`, position, value): first and last element and both sides of a chunk boundary
def nonfinite_list(seed=2):
    """-> (list, {index: [(position, value)]}): a float32 tensor of 70001 and a float64 tensor of 40000 elements with inf,
    -inf and NaN at the first element, the last element and on both sides of a chunk boundary, between clean tensors"""
    g = torch.Generator().manual_seed(seed)
    inf, nan = float('inf'), float('nan')
    f32 = torch.randn(70001, generator=g)
    f64 = torch.randn(40000, generator=g, dtype=torch.float64)
    clean = torch.randn(300, generator=g)
    spots = {1: [(0, inf), (70000, -inf), (CHUNK - 1, nan), (CHUNK, inf), (2 * CHUNK, -inf)],
             3: [(0, nan), (39999, inf), (CHUNK - 1, -inf), (CHUNK, nan)]}
    for pos, v in spots[1]:
        f32[pos] = v
    for pos, v in spots[3]:
        f64[pos] = v
    return [clean.clone(), f32, None, f64, clean.double()], spots


def magnitude_list():
    """4096 float32 entries of 1e30 (a float32 sum of squares is inf); float32 denormals, whose squares are exact in
    float64; float64 entries whose squares underflow to zero in float64; and the largest float32"""
    big = torch.full((4096,), 1e30, dtype=torch.float32)
    den32 = torch.tensor([1e-40, -3e-42, 1.4e-45, 1e-38, 0.0, -0.0], dtype=torch.float32)
    den64 = torch.tensor([1e-200, -1e-170, 4.9e-324, 1e-150], dtype=torch.float64)
    top = torch.tensor([torch.finfo(torch.float32).max, -torch.finfo(torch.float32).max], dtype=torch.float32)
    return [big, den32, den64, top]


CLIP_NUMELS = ((1, torch.float32), (65, torch.float32), (4097, torch.float32), (70001, torch.float32),
               (37, torch.float64))


def clip_problem(seed=3, steps=4, max_norm=1.0, times=13.0):
    """-> (params, [gradients of step s]): five parameters (CLIP_NUMELS) and per step gradients whose global norm is about
    `times` * max_norm"""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g, dtype=torch.float64).to(dt) for n, dt in CLIP_NUMELS]
    total = sum(n for n, _ in CLIP_NUMELS)
    grads = []
    for s in range(steps):
        k = times * max_norm / total ** 0.5 * (1.0 + 0.1 * s)
        grads.append([(torch.randn(n, generator=g, dtype=torch.float64) * k).to(dt) for n, dt in CLIP_NUMELS])
    return params, grads


def rel_close(got, want, rel):
    """|got - want| <= rel * |want| for two python floats (want == 0: got == 0)"""
    return abs(got - want) <= rel * abs(want)


def assert_measured(got_sumsq, got_bad, got_norm, ref, rel=1e-9):
    """device results (python lists / floats) against `grad_guard_reference`: every S_i and the norm within `rel`
    relative, the counts exact"""
    assert len(got_sumsq) == len(ref['sumsq']) and len(got_bad) == len(ref['nonfinite'])
    assert got_bad == ref['nonfinite'], [(i, a, b) for i, (a, b) in enumerate(zip(got_bad, ref['nonfinite'])) if a != b]
    for i, (a, b) in enumerate(zip(got_sumsq, ref['sumsq'])):
        assert rel_close(a, b, rel), (i, a, b)
    assert rel_close(got_norm, ref['norm'], rel), (got_norm, ref['norm'])


def assert_quotient(written, g, scale, rel=TWO_M22):
    """`written` (the gradient after the step) against g / scale in float64, element by element within `rel` relative"""
    want = g.detach().cpu().double() / scale
    got = written.detach().cpu().double()
    assert got.shape == want.shape
    err = (got - want).abs()
    bound = rel * want.abs()
    assert bool((err <= bound).all()), float((err - bound).max())
