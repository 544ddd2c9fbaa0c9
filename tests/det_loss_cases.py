"""Scenes and a float64 reference for the detection loss (p2rnet/loss.py, csrc/det_loss.hip).  CPU only.

`scene` builds (estimates, ground truth) with the keys and dtypes of `cases.det_loss_scene` at any (B,S,K,T,J,G,NC);
`reference64` is the whole loss in float64 torch with autograd -- distances by broadcasting, `torch.min` for the first
minimum, masked ground-truth rows at the 1e18 sentinel, no nn_distance and no oracle -- plus the facts about a scene
that say whether a comparison against it is meaningful: how far every discrete decision of the loss (the two objectness
thresholds, the four arg-mins) is from flipping, and how many elements take each branch.  `SWEEP` lists the shapes the
fused kernel is tested at; each is the smallest that reaches the code it names.
"""
import collections
import functools

import numpy as np
import torch

NEAR, FAR = 0.3, 0.6                        # p2rnet/loss.py: NEAR_THRESHOLD, FAR_THRESHOLD
FAR_AWAY = 1.0e18                           # p2rnet/loss.py: _FAR_AWAY
TERMS = ('vote_loss', 'objectness_loss', 'center_loss', 'size_loss', 'heading_loss', 'sem_cls_loss')
WEIGHTS = (10.0, 5.0, 10.0, 10.0, 10.0, 1.0)
RATIOS = ('pos_ratio', 'neg_ratio', 'obj_acc')
DIFF = ('vote_xyz', 'objectness_scores', 'center', 'size', 'heading', 'sem_cls_scores')
KINDS = ('mixed', 'none', 'all', 'novotes', 'ties', 'holes')

Entry = collections.namedtuple('Entry', 'id dims kind mask j0 seed_inds_dtype seed')


def _entry(id, dims, kind, mask='prefix', j0=0, seed_inds_dtype=torch.int64, seed=0):
    return Entry(id, dims, kind, mask, j0, seed_inds_dtype, seed)


# dims = (B, S, K, T, J, G, NC)
SWEEP = [
    _entry('min', (1, 1, 1, 1, 1, 1, 1), 'all', seed=141),                  # every extent 1
    _entry('k257', (2, 300, 257, 40, 53, 32, 22), 'mixed', seed=2),         # second trip of the K loop, G = 32, S = 256 + 44
    _entry('lds', (3, 255, 361, 8, 17, 32, 5), 'mixed', 'holes', seed=3),   # LDS 65 516 B of 65 536, S = 255, J = 17
    _entry('b33', (33, 16, 16, 4, 5, 3, 2), 'mixed', seed=4),               # B > 32 in the serial finalise, NC = 2
    _entry('bwd', (2, 257, 1500, 16, 53, 1, 100), 'mixed', seed=15),        # B K NC = 300 000: backward grid-stride, G = 1
    _entry('j0', (2, 64, 37, 16, 53, 10, 22), 'holes', 'holes', 7, torch.int32, seed=6),
    _entry('none', (2, 64, 128, 32, 53, 10, 22), 'none', seed=7),
    _entry('all', (2, 64, 128, 32, 53, 10, 22), 'all', seed=18),
    _entry('novotes', (2, 64, 128, 32, 53, 10, 22), 'novotes', seed=9),
    _entry('ties', (2, 300, 257, 40, 53, 32, 22), 'ties', seed=10),         # first-minimum rule past the first stride
]
BY_ID = {e.id: e for e in SWEEP}


def _unit(g, *shape):
    v = torch.randn(*shape, 3, generator=g)
    return v / v.norm(dim=-1, keepdim=True)


def scene(B, S, K, T, J, G, NC, seed, kind, mask='prefix', seed_inds_dtype=torch.int64):
    """(estimates, ground truth) of one detection-loss call, seeded on the CPU.  kind:
      'mixed'   every valid GT centre gets one aggregated vote at 0.06 (positive; slot 0's is the LAST proposal) and one
                at 0.41 (between the thresholds: masked out); the other proposals are random
      'holes'   'mixed' with mask = 'holes'
      'none'    every GT centre 5 away on each axis: no positive proposal, nothing between the thresholds
      'all'     every proposal at 0.06 of a valid GT centre, every seed voted
      'novotes' 'mixed' with vote_label_mask all zero
      'ties'    duplicated rows in all four arg-mins (see `tie_counts`): exact ties in every precision
    mask: 'prefix' (ones, then zeros) or 'holes' (slot 0 masked, last slot valid, the others at random; G >= 2)."""
    assert kind in KINDS and mask in ('prefix', 'holes')
    if kind == 'holes':
        mask = 'holes'
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    est = {
        'seed_skeleton': r(B, S, J, 3) * 0.4 + torch.tensor([0.0, 0.9, 0.0]),
        'vote_xyz': r(B, S, 3),
        'seed_inds': torch.sort(torch.randint(0, T, (B, S), generator=g), 1)[0].to(seed_inds_dtype),
        'aggregated_vote_xyz': r(B, K, 3),
        'center': r(B, K, 3),
        'size': r(B, K, 3) * 0.5,
        'heading': r(B, K, 2).double(),
        'objectness_scores': r(B, K, 2),
        'sem_cls_scores': r(B, K, NC),
    }
    if mask == 'prefix':
        n_obj = torch.randint(1, G + 1, (B,), generator=g)
        if kind == 'ties':
            n_obj = torch.clamp(n_obj, min=2)
        m = (torch.arange(G)[None] < n_obj[:, None]).float()
    else:
        assert G >= 2
        m = (torch.rand(B, G, generator=g) < 0.6).float()
        m[:, 0], m[:, -1] = 0, 1
    centre = r(B, G, 3)
    agg, cen = est['aggregated_vote_xyz'], est['center']
    if kind in ('mixed', 'holes', 'novotes'):
        for b in range(B):
            slots = torch.nonzero(m[b] > 0)[:, 0].tolist()
            n = len(slots)
            assert K >= 2 * n, "a near and a band proposal per valid ground-truth box"
            where = [K - 1] + torch.randperm(K - 1, generator=g)[:2 * n - 1].tolist()
            for i, s in enumerate(slots):
                agg[b, where[i]] = centre[b, s] + 0.06 * _unit(g)
                cen[b, where[i]] = centre[b, s] + 0.2 * r(3)
                agg[b, where[n + i]] = centre[b, s] + 0.41 * _unit(g)
    elif kind == 'none':
        centre = centre + 5.0
    elif kind == 'all':
        for b in range(B):
            slots = torch.nonzero(m[b] > 0)[:, 0]
            agg[b] = centre[b, slots[torch.arange(K) % len(slots)]] + 0.06 * _unit(g, K)
    elif kind == 'ties':
        assert K >= 7 and G >= 2
        centre[:, 1] = centre[:, 0]                          # slots 0 and 1 are valid (n_obj >= 2) and equal
        agg[:, :3] = centre[:, :1]                           # proposals exactly on them, in the first stride ...
        agg[:, K - 1] = centre[:, 0]                         # ... and at the last index
        cen[:, 4] = centre[:, 0] + 0.01                      # the nearest proposal of slots 0 and 1, twice: 4 must win
        cen[:, K - 1] = cen[:, 4]
    m3 = m[..., None]
    gt = {
        'center_label': centre * m3, 'box_label_mask': m, 'size': r(B, G, 3) * 0.5 * m3,
        'heading': r(B, G, 2) * m3, 'sem_cls_label': torch.randint(0, NC, (B, G), generator=g) * m.long(),
        'vote_label': r(B, T, J, 9) * 0.5, 'vote_label_mask': (torch.rand(B, T, J, generator=g) < 0.6).long(),
    }
    if kind == 'ties':          # GT votes 0 and 1 equal at every seed: the first must win, like torch.min / argmin
        gt['vote_label'][..., 3:6] = gt['vote_label'][..., 0:3]
    elif kind == 'novotes':
        gt['vote_label_mask'].zero_()
    elif kind == 'all':
        gt['vote_label_mask'].fill_(1)
    return est, gt


def sweep_scene(entry):
    """(est, gt) of a `SWEEP` entry (or its id)"""
    e = BY_ID[entry] if isinstance(entry, str) else entry
    return scene(*e.dims, seed=e.seed, kind=e.kind, mask=e.mask, seed_inds_dtype=e.seed_inds_dtype)


def _huber(e):
    a = e.abs()
    q = torch.clamp(a, max=1.0)
    return 0.5 * q * q + (a - q)


def _gap(d, dim):
    """d: distances with the candidates along `dim` -> (smallest relative gap between the minimum and the nearest
    strictly larger candidate over the rows, number of rows whose minimum is attained more than once).  Candidates
    equal to the minimum are duplicates (identical coordinates give identical distances in every precision)."""
    d = d.detach().movedim(dim, -1)
    if d.shape[-1] < 2:
        return float('inf'), 0
    best = d.min(-1, keepdim=True)[0]
    tied = ((d == best).sum(-1) > 1)
    runner = torch.where(d > best, d, torch.full_like(d, float('inf'))).min(-1)[0]
    rel = (runner - best[..., 0]) / runner           # runner > best >= 0; inf / inf when all equal
    rel = torch.where(torch.isfinite(runner), rel, torch.full_like(rel, float('inf')))
    return rel.min().item(), int(tied.sum())


def reference64(est, gt, j0=0):
    """The detection loss of p2rnet/loss.py in float64 on the CPU -> (scalars, grads, facts).
    scalars: the six terms and `total` as Python floats (float64), the three ratios as np.float32 computed from the
    integer counts in the order of the finalise kernel; grads: d total / d input (float64) of the six differentiable
    inputs; facts: decision margins, branch counts, counts and the labels themselves (see the module docstring)."""
    d64 = lambda t: t.detach().cpu().double()
    x = {k: d64(est[k]).requires_grad_(True) for k in DIFF}
    sk, agg = d64(est['seed_skeleton']), d64(est['aggregated_vote_xyz'])
    inds = est['seed_inds'].detach().cpu().long()
    B, S, J = sk.shape[:3]
    K, G = agg.shape[1], gt['center_label'].shape[1]
    bmask = d64(gt['box_label_mask'])
    gt_centre = d64(gt['center_label'])

    # vote loss: of the three GT votes of the seed's frame, the one nearest to any joint of the seed skeleton
    bi = torch.arange(B)[:, None]
    smask = gt['vote_label_mask'].cpu()[bi, inds, j0].double()                    # (B,S)
    votes = sk[:, :, j0, None, :] + d64(gt['vote_label'])[bi, inds, j0].view(B, S, 3, 3)
    dv = ((votes[:, :, :, None, :] - sk[:, :, None, :, :]) ** 2).sum(-1)          # (B,S,3,J)
    per_joint, which = dv.min(2)                                                  # first vote on ties
    jmin = per_joint.argmin(-1)                                                   # first joint on ties
    chosen = which.gather(2, jmin[..., None])[..., 0]                             # (B,S)
    target = votes.gather(2, chosen[..., None, None].expand(B, S, 1, 3))[:, :, 0]
    e_vote = x['vote_xyz'] - target
    n_voted = smask.sum()
    vote = (_huber(e_vote).mean(-1) * smask).sum() / (n_voted + 1e-6)

    # correspondence: nearest VALID ground-truth centre of every aggregated vote, objectness label and mask
    valid = bmask > 0
    masked = torch.where(valid[..., None], gt_centre, torch.full_like(gt_centre, FAR_AWAY))
    da = ((agg[:, :, None, :] - masked[:, None, :, :]) ** 2).sum(-1)              # (B,K,G)
    d_as, assign = da.min(-1)
    eu = torch.sqrt(d_as + 1e-6)
    near, far = eu < NEAR, eu > FAR
    label, omask = near.double(), (near | far).double()
    w = torch.tensor([0.1, 0.9], dtype=torch.float32).double()                   # the class weights are f32 values
    so = x['objectness_scores']
    nll = torch.logsumexp(so, -1) - so.gather(2, near.long()[..., None])[..., 0]
    n_mask, n_pos_i = omask.sum(), label.sum()
    obj = (w[near.long()] * nll * omask).sum() / (n_mask + 1e-6)
    n_pos = n_pos_i + 1e-6

    # centre: chamfer against ALL slots (zero padding included), only the ground-truth side is masked
    dc = ((x['center'][:, :, None, :] - gt_centre[:, None, :, :]) ** 2).sum(-1)   # (B,K,G)
    dist1, i1 = dc.min(2)
    dist2, i2 = dc.min(1)
    n_box = bmask.sum()
    centre = ((dist1 * label).sum() / n_pos + (dist2 * bmask).sum() / (n_box + 1e-6)) / 2

    pick = lambda t: d64(t).gather(1, assign[..., None].expand(B, K, t.shape[-1]))
    e_size = x['size'] - pick(gt['size'])
    size = (_huber(e_size).mean(-1) * label).sum() / n_pos
    e_head = x['heading'] - pick(gt['heading'])
    head = (_huber(e_head).mean(-1) * label).sum() / n_pos
    cls = gt['sem_cls_label'].cpu().long().gather(1, assign)
    ss = x['sem_cls_scores']
    sem = ((torch.logsumexp(ss, -1) - ss.gather(2, cls[..., None])[..., 0]) * label).sum() / n_pos

    terms = (vote, obj, centre, size, head, sem)
    total = sum(wt * t for wt, t in zip(WEIGHTS, terms))
    grads = dict(zip(DIFF, torch.autograd.grad(total, [x[k] for k in DIFF])))

    pred = (so[..., 1] > so[..., 0]).detach()                                    # argmax: first maximum on ties
    counts = {'positives': int(n_pos_i), 'masked_in': int(n_mask), 'correct': int(((pred == near) & (omask > 0)).sum()),
              'valid_boxes': int(n_box), 'voted_seeds': int(n_voted)}
    f32 = np.float32
    total_n = f32(B) * f32(K)
    pos_ratio = f32(counts['positives']) / total_n
    scalars = {k: t.item() for k, t in zip(TERMS, terms)}
    scalars['total'] = total.item()
    scalars['pos_ratio'] = pos_ratio
    scalars['neg_ratio'] = f32(counts['masked_in']) / total_n - pos_ratio
    scalars['obj_acc'] = f32(counts['correct']) / (f32(counts['masked_in']) + f32(1e-6))

    per_vote = dv.min(3)[0]                          # (B,S,3): the decision is between the three votes
    gaps, ties = {}, {}
    for name, (d, dim) in {'assignment': (da, 2), 'center_dist1': (dc, 2), 'center_dist2': (dc, 1),
                           'vote': (per_vote, 2)}.items():
        gaps[name], ties[name] = _gap(d, dim)
    pos, voted = label > 0, smask > 0
    lin = lambda e, sel: int((e.detach().abs()[sel] > 1).sum())
    quad = lambda e, sel: int((e.detach().abs()[sel] <= 1).sum())
    facts = {
        'thr_near': (eu - NEAR).abs().min().item(), 'thr_far': (eu - FAR).abs().min().item(),
        'gaps': gaps, 'ties': ties, 'counts': counts,
        'branches': {'near': int(near.sum()), 'band': int((~near & ~far).sum()), 'far': int(far.sum()),
                     'vote_quadratic': quad(e_vote, voted), 'vote_linear': lin(e_vote, voted),
                     'size_quadratic': quad(e_size, pos), 'size_linear': lin(e_size, pos),
                     'heading_quadratic': quad(e_head, pos), 'heading_linear': lin(e_head, pos)},
        'objectness_label': near, 'objectness_mask': omask > 0, 'seed_mask': voted, 'object_assignment': assign,
        'center_index1': i1, 'center_index2': i2, 'vote_index': chosen,
        'center_extent': (x['center'].detach()[:, :, None, :] - gt_centre[:, None, :, :]).abs().max().item(),
    }
    return scalars, grads, facts


@functools.lru_cache(maxsize=None)
def sweep_reference(id):
    """(est, gt, scalars, grads, facts) of the `SWEEP` entry `id`, computed once per process; callers leave it unchanged"""
    e = BY_ID[id]
    est, gt = sweep_scene(e)
    return (est, gt) + reference64(est, gt, e.j0)


def tie_counts(est, gt, facts, j0=0):
    """The number of exactly tied decisions per arg-min that the duplicated rows of a scene account for: a decision is
    tied when the row it picks has a coordinate-for-coordinate duplicate among its candidates.  Found from the
    coordinates alone, so it can be held against `facts['ties']`, which is found from the float64 distances."""
    def dup(rows):                                   # (B,R,3) -> (B,R): another row of the sample equals this one
        same = (rows[:, :, None, :] == rows[:, None, :, :]).all(-1)
        return same.sum(-1) > 1
    valid = gt['box_label_mask'] > 0
    far = torch.full_like(gt['center_label'], FAR_AWAY)
    d_assign = dup(torch.where(valid[..., None], gt['center_label'], far))
    d_gt, d_est = dup(gt['center_label']), dup(est['center'])
    B, S = est['seed_inds'].shape
    votes = gt['vote_label'][torch.arange(B)[:, None], est['seed_inds'].long(), j0].view(B * S, 3, 3)
    d_vote = dup(votes).view(B, S, 3)                # vote i of the seed's frame has a twin
    return {'assignment': int(d_assign.gather(1, facts['object_assignment']).sum()),
            'center_dist1': int(d_gt.gather(1, facts['center_index1']).sum()),
            'center_dist2': int(d_est.gather(1, facts['center_index2']).sum()),
            'vote': int(d_vote.gather(2, facts['vote_index'][..., None]).sum())}
