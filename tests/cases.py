"""Seeded input builders shared by the CPU (oracle/golden) and GPU (parity) tests."""
import numpy as np
import torch


def cloud(b, n, seed, kind="uniform"):
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        return (torch.rand(b, n, 3, generator=g) * 4 - 2).contiguous()
    if kind == "lattice":      # exact ties everywhere: integer grid, small range
        return torch.randint(-3, 4, (b, n, 3), generator=g).float().contiguous()
    if kind == "halflattice":  # ties + exactly representable distances
        return (torch.randint(-8, 9, (b, n, 3), generator=g).float() * 0.25).contiguous()
    if kind == "near_origin":  # many points inside the |p|^2 <= 1e-3 skip ball
        x = torch.rand(b, n, 3, generator=g) * 4 - 2
        m = torch.rand(b, n, generator=g) < 0.3
        x[m] = x[m] * 0.01
        # a few exactly on the threshold neighbourhood
        x[:, 1 % n] = torch.tensor([0.031622776, 0.0, 0.0])
        return x.contiguous()
    if kind == "all_skipped":
        return (torch.rand(b, n, 3, generator=g) * 0.01).contiguous()
    if kind == "duplicates":
        base = torch.rand(b, max(n // 4, 1), 3, generator=g) * 4 - 2
        idx = torch.randint(0, base.shape[1], (b, n), generator=g)
        return torch.gather(base, 1, idx.unsqueeze(-1).expand(b, n, 3)).contiguous()
    if kind == "walk":         # P2RNet-like: random-walk trajectory (vote_xyz-like clusters)
        steps = torch.randn(b, n, 3, generator=g) * 0.05
        return (torch.cumsum(steps, 1) + torch.tensor([0.0, 0.9, 0.0])).contiguous()
    raise ValueError(kind)


FPS_CASES = [  # (b, n, m, kind, seed)
    (2, 512, 128, "uniform", 1), (4, 512, 128, "walk", 2), (3, 64, 16, "uniform", 3),
    (2, 100, 30, "uniform", 4), (2, 1, 1, "uniform", 5), (2, 5, 5, "lattice", 6),
    (2, 512, 128, "lattice", 7), (2, 300, 300, "halflattice", 8), (2, 512, 64, "near_origin", 9),
    (1, 128, 16, "all_skipped", 10), (2, 256, 100, "duplicates", 11), (1, 1000, 200, "uniform", 12),
    (1, 2048, 256, "lattice", 13), (1, 5000, 128, "uniform", 14), (1, 9000, 64, "uniform", 15),
    (1, 16384, 32, "lattice", 16), (1, 20000, 48, "uniform", 17), (2, 33, 7, "lattice", 18),
    (1, 700, 64, "lattice", 19), (1, 3000, 64, "halflattice", 20),
    # beyond one workgroup's register file: several workgroups per cloud
    (8, 54272, 40, "uniform", 21), (3, 17000, 33, "lattice", 22), (16, 16500, 20, "halflattice", 23),
    (40, 16400, 6, "uniform", 24), (2, 70000, 300, "duplicates", 25),
]

BALL_CASES = [  # (b, n, m, radius, nsample, kind, seed)
    (2, 512, 128, 0.3, 16, "walk", 1), (2, 512, 128, 0.3, 16, "uniform", 2),
    (3, 100, 17, 0.8, 8, "uniform", 3), (2, 64, 64, 1.0, 32, "lattice", 4),
    (2, 300, 50, 0.5, 16, "halflattice", 5), (1, 3000, 40, 0.4, 16, "uniform", 6),
    (1, 5000, 100, 0.25, 64, "halflattice", 7), (2, 10, 5, 0.01, 4, "uniform", 8),
    (1, 512, 128, 5.0, 100, "uniform", 9), (2, 1, 1, 1.0, 3, "uniform", 10),
]


def centres_from(xyz, m, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    b, n, _ = xyz.shape
    idx = torch.stack([torch.randperm(n, generator=g)[:m] if m <= n else torch.randint(0, n, (m,), generator=g)
                       for _ in range(b)])
    return torch.gather(xyz, 1, idx.unsqueeze(-1).expand(b, m, 3)).contiguous()


def random_boxes(K, seed, stride=8, ncls=3):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, (K, 3))
    s = rng.uniform(0.2, 2.0, (K, 3))
    score = (rng.permutation(K) + rng.uniform(0.1, 0.9, K)) / max(K, 1)   # distinct
    cls = rng.integers(0, ncls, (K, 1)).astype(np.float64)
    b = np.concatenate([c - s / 2, c + s / 2, score[:, None], cls], 1)
    return np.ascontiguousarray(b[:, :stride])


def boxes_xz(boxes):
    """(K,>=7) rows [x1,y1,z1,x2,y2,z2,score,...] -> (K,5) rows [x1,z1,x2,z2,score]: the 2-D boxes the reference's
    `use_3d_nms: False` branch builds (ap_helper.py:201-207)."""
    return np.ascontiguousarray(boxes[:, [0, 2, 3, 5, 6]])


def _hash_uniform(n, k):
    """n deterministic pseudo-random numbers in [-1, 1) from integer arithmetic only
    (exact on every platform / torch version): a multiply-xorshift hash of (index, key)."""
    M = (1 << 32) - 1
    h = (torch.arange(n, dtype=torch.int64) * 2654435761 + (k + 1) * 2246822519) & M
    h = h ^ (h >> 15)
    h = (h * 1540483477) & M
    h = h ^ (h >> 13)
    h = (h * 1103515245 + 12345) & M
    h = h ^ (h >> 16)
    return h.double() / float(1 << 31) - 1.0


def fill_weights(net):
    """Deterministic weight rule applied identically to the reference model (when the
    fixtures are generated) and to ours (when they are checked): every floating tensor of
    the state_dict is filled from an integer hash of (element index, key index), with
    He-style fan-in scaling for conv weights so the net behaves like a freshly initialised
    one (a first version used sines of the element index: those weights are orthogonal to
    the smooth pose signal, the convs cancel it, and train-mode BatchNorm then amplifies
    fp32 rounding differences ~4000x -- measured -- which made the fixtures ill-conditioned).
    The adjacency buffer `A` and integer buffers are left alone."""
    sd = net.state_dict()
    with torch.no_grad():
        for k, name in enumerate(sorted(sd.keys())):
            t = sd[name]
            if not t.is_floating_point() or name == 'backbone.A':
                continue
            u = _hash_uniform(t.numel(), k)          # uniform [-1,1): std 0.577
            if name.endswith('running_var'):
                v = 1.0 + 0.5 * u.abs()
            elif name.endswith('running_mean'):
                v = 0.1 * u
            elif 'batchnorm.weight' in name or name.endswith('tcn.0.weight') or name.endswith('tcn.3.weight'):
                v = 1.0 + 0.1 * u
            elif 'edge_importance' in name:
                v = 1.0 + 0.1 * u
            elif name.endswith('log_sigma'):
                v = 0.1 * u - 1.0
            elif name.endswith('mdn.mu'):
                v = 0.5 * u
            elif name.endswith('bias'):
                v = 0.1 * u
            elif t.dim() > 1:
                v = u * (2.4 / t[0].numel() ** 0.5)  # std = 1.39/sqrt(fan_in) ~ He init
            else:
                v = 0.1 * u
            t.copy_(v.view_as(t).to(t.dtype))
    return net


def state_checksum(net):
    sd = net.state_dict()
    return float(sum(v.double().abs().sum() for k, v in sd.items() if v.is_floating_point()))


def seam_cotangents(B, seed=77):
    """Seeded cotangents on (vote_xyz, vote_features) at the backbone -> detection seam: fixture g10c back-propagates
    these through the reference's backbone, the GPU test through ours."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 512, 3, generator=g), torch.randn(B, 512, 256, generator=g) * 0.1


def graph_conv_reference(x, weight, bias, Aeff):
    """the reference's ConvTemporalGraphical.forward in plain torch (conv1x1 + einsum), in the dtype of its arguments"""
    K = Aeff.shape[0]
    y = torch.nn.functional.conv2d(x, weight.view(K * 64, 64, 1, 1), bias)
    n, kc, t, v = y.shape
    return torch.einsum('nkctv,kvw->nctw', y.view(n, K, kc // K, t, v), Aeff)


def ring_adjacency(K, V, seed):
    """K planes over a V-joint ring skeleton: plane k links joints k hops apart (plus random extra links)."""
    rng = np.random.RandomState(seed)
    A = np.zeros((K, V, V), dtype=np.float32)
    for k in range(K):
        for v in range(V):
            A[k, v, (v + k) % V] = rng.uniform(0.2, 1.0)
            if rng.rand() < 0.3:
                A[k, v, rng.randint(V)] = rng.uniform(0.2, 1.0)
    return A


def graph_conv_inputs(N, T, A, seed):
    """(x, weight, bias, importance, cotangent) of one graph-conv call over the adjacency A (K, V, V), seeded on the CPU"""
    K, V = A.shape[0], A.shape[1]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 64, T, V, generator=g)
    w = torch.randn(K * 64, 64, generator=g) / 8
    b = torch.randn(K * 64, generator=g) * 0.1
    imp = 1 + 0.1 * torch.randn(K, V, V, generator=g)
    go = torch.randn(N, 64, T, V, generator=g)
    return x, w, b, imp, go


def bn_conv_pair(taps, seed, dims=2):
    """BatchNorm + 64 -> 64 convolution with `taps` temporal taps (dims=2: BatchNorm2d + Conv2d (taps,1); dims=1: BatchNorm1d
    + Conv1d(1)), affine parameters and running statistics away from their defaults, seeded on the CPU"""
    g = torch.Generator().manual_seed(seed)
    if dims == 2:
        bn, conv = torch.nn.BatchNorm2d(64), torch.nn.Conv2d(64, 64, (taps, 1), (1, 1), (taps // 2, 0))
    else:
        bn, conv = torch.nn.BatchNorm1d(64), torch.nn.Conv1d(64, 64, 1)
    with torch.no_grad():
        for t, lo, hi in ((bn.weight, 0.5, 1.5), (bn.bias, -0.5, 0.5), (bn.running_mean, -0.2, 0.2), (bn.running_var, 0.5, 2.0)):
            t.copy_(torch.rand(t.shape, generator=g) * (hi - lo) + lo)
        for t in (conv.weight, conv.bias):
            t.copy_((torch.rand(t.shape, generator=g) * 2 - 1) / (64 * taps) ** 0.5)
    return bn, conv


def det_loss_scene(B, S, K, T, seed, case):
    """(estimates, ground truth) of one detection-loss call; case: 'near' | 'random' | 'none' | 'ties' | 'single'"""
    g = torch.Generator().manual_seed(seed)
    J, G, NC = 53, 10, 22
    r = lambda *s: torch.randn(*s, generator=g)
    est = {
        'seed_skeleton': r(B, S, J, 3) * 0.4 + torch.tensor([0.0, 0.9, 0.0]),
        'vote_xyz': r(B, S, 3),
        'seed_inds': torch.sort(torch.randint(0, T, (B, S), generator=g), 1)[0],
        'aggregated_vote_xyz': r(B, K, 3),
        'center': r(B, K, 3),
        'size': r(B, K, 3) * 0.5,
        'heading': r(B, K, 2).double(),
        'objectness_scores': r(B, K, 2),
        'sem_cls_scores': r(B, K, NC),
    }
    n_obj = torch.randint(1, G + 1, (B,), generator=g)
    mask = (torch.arange(G)[None] < n_obj[:, None]).float()
    centre = r(B, G, 3)
    if case == 'near':          # GT centres next to aggregated votes: positives exist
        for b in range(B):
            for j in range(int(n_obj[b])):
                centre[b, j] = est['aggregated_vote_xyz'][b, (7 * j + 1) % K] + 0.05
    elif case == 'none':        # every proposal far from every GT box: no positive, n_pos = 1e-6
        centre = centre + 50.0
    elif case == 'ties':        # duplicated GT centres and proposals exactly on them: exact ties in every arg-min
        centre[:, 1] = centre[:, 0]
        est['aggregated_vote_xyz'][:, :4] = centre[:, :1]
        est['center'][:, 5] = est['center'][:, 4]
        n_obj = torch.clamp(n_obj, min=2)
        mask = (torch.arange(G)[None] < n_obj[:, None]).float()
    elif case == 'single':
        mask = torch.zeros(B, G); mask[:, 0] = 1
        centre[:, 0] = est['aggregated_vote_xyz'][:, 3]
    m3 = mask[..., None]
    gt = {
        'center_label': centre * m3, 'box_label_mask': mask, 'size': r(B, G, 3) * 0.5 * m3,
        'heading': r(B, G, 2) * m3, 'sem_cls_label': torch.randint(0, NC, (B, G), generator=g) * mask.long(),
        'vote_label': r(B, T, J, 9) * 0.5, 'vote_label_mask': (torch.rand(B, T, J, generator=g) < 0.6).long(),
    }
    if case == 'ties':          # equal GT votes: the first of the three must win, like torch.min / argmin
        gt['vote_label'][..., 3:6] = gt['vote_label'][..., 0:3]
    return est, gt


def seeded_randn(shape, seed, scale=1.0):
    """standard normal values of one seed on the CPU, times `scale`"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def pw_gemm_case(B, L, K, R, x_nlc, bias):
    """operands of one forward job of the point-wise GEMM: x (B,K,L) or (B,L,K), W (R,K), bias (R) or None, the input
    transform fin [4,K] = (mean, invstd, scale, shift)"""
    x = seeded_randn((B, L, K) if x_nlc else (B, K, L), 1)
    W = seeded_randn((R, K), 2, 0.1)
    bvec = seeded_randn((R,), 3) if bias else None
    fin = torch.stack([seeded_randn((K,), 4), seeded_randn((K,), 5).abs() + 0.5, seeded_randn((K,), 6),
                       seeded_randn((K,), 7)]).contiguous()
    return x, W, bvec, fin


def pw_data_gradient_case(B, L, K, R, x_nlc):
    """operands of one data-gradient job: g, z (B,K,L) or (B,L,K), the layer's weight W [out = K][in = R], the lazy
    BatchNorm-backward coefficients coef [3,K], the mask source mz (B,R,L) with its transform mfin [4,R]"""
    g = seeded_randn((B, L, K) if x_nlc else (B, K, L), 1)
    z = seeded_randn((B, L, K) if x_nlc else (B, K, L), 2)
    W = seeded_randn((K, R), 3, 0.1)
    coef = torch.stack([seeded_randn((K,), 4), seeded_randn((K,), 5), seeded_randn((K,), 6)]).contiguous()
    mz = seeded_randn((B, R, L), 7)
    mfin = torch.stack([seeded_randn((R,), 8), seeded_randn((R,), 9).abs() + 0.5, seeded_randn((R,), 10),
                        seeded_randn((R,), 11)]).contiguous()
    return g, z, W, coef, mz, mfin


def pw_wgrad_case(B, L, R, K, x_nlc, y_nlc):
    """operands of one weight-gradient job: g, z (B,R,L) or (B,L,R), y (B,K,L) or (B,L,K), coef [3,R], yfin [2,K]"""
    g = seeded_randn((B, L, R) if x_nlc else (B, R, L), 1)
    z = seeded_randn((B, L, R) if x_nlc else (B, R, L), 2)
    y = seeded_randn((B, L, K) if y_nlc else (B, K, L), 3)
    coef = torch.stack([seeded_randn((R,), 4), seeded_randn((R,), 5), seeded_randn((R,), 6)]).contiguous()
    yfin = torch.stack([seeded_randn((K,), 7), seeded_randn((K,), 8)]).contiguous()
    return g, z, y, coef, yfin


def seed_indices(B, T, S, kind, seed=5):
    """(B,S) int64 frame indices: 'sorted' distinct, 'dup' sorted with repeats, 'many' all within three frames, 'random'"""
    g = torch.Generator().manual_seed(seed)
    if kind == 'sorted':
        return torch.sort(torch.stack([torch.randperm(T, generator=g)[:S] for _ in range(B)]), dim=1)[0]
    if kind == 'many':        # far more seeds than frames: more hits per frame than the kernel's list holds
        return torch.randint(0, 3, (B, S), generator=g)
    inds = torch.randint(0, T, (B, S), generator=g)
    return torch.sort(inds, dim=1)[0] if kind == 'dup' else inds


def arc_length_case(B, T, S, g):
    """cumulative arc lengths (B,T) with plateaus and exactly representable steps (exact ties), drawn from generator g"""
    step = torch.rand(B, T - 1, generator=g)
    step[torch.rand(B, T - 1, generator=g) < 0.3] = 0.0              # plateaus
    step = (step * 8).round() / 8                                     # exactly representable: exact mid-point ties
    return torch.cumsum(torch.cat([torch.zeros(B, 1), step], 1).double(), 1).float()
