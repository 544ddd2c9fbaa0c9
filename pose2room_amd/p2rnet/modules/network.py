"""P2RNet: backbone -> centre voting -> detection (mirror of the reference's
models/p2rnet/modules/network.py:10-106 and models/network.py:8-86)."""
import torch
import torch.nn as nn

from ..registers import METHODS, MODULES, LOSSES


def _multi_getattr(obj, dotted):
    for part in dotted.split("."):
        obj = getattr(obj, part)
    return obj


def _multi_hasattr(obj, dotted):
    for part in dotted.split("."):
        if not hasattr(obj, part):
            return False
        obj = getattr(obj, part)
    return True


class BaseNetwork(nn.Module):
    """Shared plumbing: per-phase optimiser spec, freezing, checkpoint key handling."""

    def freeze_modules(self, cfg):
        if cfg.config['mode'] == 'train':
            for layer in cfg.config['train']['freeze']:
                if not _multi_hasattr(self, layer):
                    continue
                for p in _multi_getattr(self, layer).parameters():
                    p.requires_grad = False
                cfg.log_string('The module: %s is fixed.' % layer)

    def set_mode(self):
        frozen = self.cfg.config['train']['freeze']
        for name, child in self.named_children():
            if name in frozen:
                child.train(False)

    def load_weight(self, pretrained_model):
        """Load a reference checkpoint's `net` dict: keys carry a leading 'module.'
        (DDP / DataParallel wrapper) which is dropped (models/network.py:59-67)."""
        own = self.state_dict()
        matched = {'.'.join(k.split('.')[1:]): v for k, v in pretrained_model.items()
                   if '.'.join(k.split('.')[1:]) in own}
        self.cfg.log_string(str({k.split('.')[0] for k in own if k not in matched}) + ' subnet missed.')
        own.update(matched)
        self.load_state_dict(own)

    def load_optim_spec(self, config, net_spec):
        if config['mode'] != 'train':
            return None
        if 'optimizer' in net_spec:
            spec = config['optimizer'].copy()
            for key in spec:
                spec[key] = net_spec['optimizer'].get(key, spec[key])
            return spec
        return config['optimizer']


@METHODS.register_module
class P2RNet(BaseNetwork):
    def __init__(self, cfg):
        nn.Module.__init__(self)
        self.cfg = cfg
        mode = cfg.config['mode']
        phase_names = ['backbone', 'centervoting', 'detection'] if cfg.config[mode]['phase'] in ['full'] else []
        if (not cfg.config['model']) or (not phase_names):
            cfg.log_string('No submodule found. Please check the phase name and model definition.')
            raise ModuleNotFoundError('No submodule found. Please check the phase name and model definition.')
        for phase_name, net_spec in cfg.config['model'].items():
            if phase_name not in phase_names:
                continue
            optim_spec = self.load_optim_spec(cfg.config, net_spec)
            self.add_module(phase_name, MODULES.get(net_spec['method'])(cfg, optim_spec))
            loss_cls = LOSSES.get(net_spec['loss'], 'Null')
            setattr(self, phase_name + '_loss',
                    loss_cls(net_spec.get('weight', 1), cfg.config['device']['gpu'], cfg))
        self.freeze_modules(cfg)

    def _votes(self, data):
        end_points = self.backbone(data['input_joints'], {})
        from .. import pw_op
        from . import vote_center
        if vote_center.USE_FUSED_HEAD and pw_op.votes_normalized_supported(self.centervoting, end_points['seed_skeleton'],
                                                                            end_points['seed_features']):
            # conv_input on the job-list kernels + offset / residual add / normalisation / re-layout in one launch
            xyz, features = pw_op.votes_normalized(self.centervoting, end_points['seed_skeleton'],
                                                   end_points['seed_features'])
        else:
            xyz, features = self.centervoting(end_points['seed_skeleton'], end_points['seed_features'])
            features = features.div(torch.norm(features, p=2, dim=2).unsqueeze(2))   # no epsilon, as the reference
        end_points['vote_xyz'] = xyz
        end_points['vote_features'] = features
        return xyz, features, end_points

    def forward(self, data, eps=None):
        """data['input_joints'] (B,T,J,3) -> end_points dict (network.py:75-96)."""
        xyz, features, end_points = self._votes(data)
        end_points, _ = self.detection(xyz, features, end_points, False, eps=eps)
        return end_points

    def generate_end_points(self, data):
        """The network part of `generate`: deterministic heads, no parsing / NMS."""
        xyz, features, end_points = self._votes(data)
        end_points, _ = self.detection.generate(xyz, features, end_points, False)
        return end_points

    def generate(self, data, eval=True):
        """Detection path with deterministic mixture means, prediction parsing and
        NMS (network.py:44-73)."""
        from ...net_utils.ap_helper import (parse_predictions, parse_groundtruths,
                                            assembly_pred_map_cls, assembly_gt_map_cls)
        end_points = self.generate_end_points(data)
        eval_dict, parsed_predictions = parse_predictions(end_points, data, self.cfg.eval_config)
        eval_dict = assembly_pred_map_cls(eval_dict, parsed_predictions, self.cfg.eval_config)
        if eval:
            parsed_gts = parse_groundtruths(data, self.cfg.eval_config)
            eval_dict['batch_gt_map_cls'] = assembly_gt_map_cls(parsed_gts)
        return end_points, eval_dict, parsed_predictions

    def generate_hypotheses(self, data, num_hypotheses, n_samples=None, seed=None, eval=True, central_tendency=None,
                            return_draws=False, return_device=False):
        """Multi-modal generation (the reference's `multi_mode`, proposal_net.py:56-59 / mdn.py:116-125): H hypotheses
        of the detection for one batch, each one `generate` whose mixture heads return the mean (or the median) of n_h
        Bernoulli-gated draws.  The trunk runs once; the draws of all heads and hypotheses are one kernel launch
        (mdn_sample_op) and the predictions of all hypotheses are parsed / NMS-ed as one H * B batch.
          n_samples: None -> each n_h uniform in 1..99 drawn from `seed`; an int or a length-H sequence fixes them.
          seed: None -> a 64-bit seed drawn from torch's default CPU generator (`torch.manual_seed` reproduces a call).
          central_tendency: None -> each head's own `hparams.central_tendency`; 'mean' or 'median' (the lower median,
          `torch.median`'s) overrides it for this call, the modules stay as they are.
          return_draws: each hypothesis' end_points gain 'draws' = {'center', 'size', 'heading'}, the heads' individual
          draws (B, K, n_h, D) (the centre's before the vote position is added).
        -> list of H (end_points, eval_dict, parsed_predictions) triples shaped like `generate`'s result; the
        deterministic end points (votes, aggregation, 'pi', objectness, class scores) are shared by all of them.
          return_device: no host lists (`eval` and `return_draws` do not apply); -> ONE dict of device tensors, what
          `parse_predictions(..., return_device=True)` gives for the H * B batch with the hypotheses as the leading
          axis: 'end_points' (the shared ones), 'center', 'size', 'heading' (H,B,K,.), 'pred_mask' (H,B,K),
          'pred_corners_3d' (H,B,K,8,3) f64, 'obj_prob' (H,B,K), 'pred_sem_cls' (H,B,K), 'sem_cls_scores' (H,B,K,C);
          net_utils/mm_device.py evaluates it without leaving the device."""
        from ...net_utils.ap_helper import (parse_predictions, parse_groundtruths,
                                            assembly_pred_map_cls, assembly_gt_map_cls)
        from .. import mdn_sample_op
        if return_device and return_draws:
            raise ValueError("generate_hypotheses: return_draws needs the host form (return_device=False)")
        seed, ns = mdn_sample_op.resolve_draws(num_hypotheses, n_samples, seed)
        H = len(ns)
        xyz, features, end_points = self._votes(data)
        end_points, stacked, _, *draws = self.detection.generate_hypotheses(
            xyz, features, end_points, H, ns, seed, central_tendency=central_tendency, return_draws=return_draws)
        B = end_points['aggregated_vote_xyz'].shape[0]
        joints = data['input_joints']
        if self.cfg.eval_config.get('parse_impl', 'torch') == 'kernel':
            # the kernel reads row n % B of the batch's joints for sample n of the stack: no H-fold copy
            gt_stacked, repeat = {'input_joints': joints}, {'joints_repeat': H}
        else:
            gt_stacked = {'input_joints': joints.unsqueeze(0).expand(H, *joints.shape).reshape(H * B, *joints.shape[1:])}
            repeat = {}
        if return_device:
            eval_all, parsed_all = parse_predictions(stacked, gt_stacked, self.cfg.eval_config, return_device=True,
                                                     **repeat)
            out = {'end_points': end_points, 'pred_mask': eval_all['pred_mask'], **parsed_all}
            out.update({k: stacked[k] for k in ('center', 'size', 'heading')})
            return {k: v if k == 'end_points' else v.reshape(H, B, *v.shape[1:]) for k, v in out.items()}
        eval_all, parsed_all = parse_predictions(stacked, gt_stacked, self.cfg.eval_config, **repeat)
        gt_map = assembly_gt_map_cls(parse_groundtruths(data, self.cfg.eval_config)) if eval else None
        out = []
        for h in range(H):
            sl = slice(h * B, (h + 1) * B)
            ep = dict(end_points)
            for k in ('center', 'size', 'heading'):
                ep[k] = stacked[k][sl]
            if return_draws:
                ep['draws'] = {k: d[h, :, :, :ns[h]] for k, d in zip(('center', 'size', 'heading'), draws[0])}
            eval_dict = assembly_pred_map_cls({'pred_mask': eval_all['pred_mask'][sl]},
                                              {k: v[sl] for k, v in parsed_all.items()}, self.cfg.eval_config)
            if eval:
                eval_dict['batch_gt_map_cls'] = gt_map
            out.append((ep, eval_dict, {k: v[sl] for k, v in parsed_all.items()}))
        return out

    @torch.no_grad()
    def predict_scenes(self, data, num_hypotheses=None, n_samples=None, seed=None, dump_threshold=None, contact=True,
                       unique=True):
        """What the reference's demo.py (`predict` + `visualize_step`, lines 204-266) gives the user of a trained model,
        for the whole batch and on the device: data['input_joints'] (B,T,J,3|4) -> net_utils.scene_device.SceneBatch --
        per sample the confident boxes as object nodes (centroid, R_mat, size, class), with `contact` the frame in which
        the body is closest to each node (`dist_node2bbox`), with `unique` the frames without duplicates (`np.unique`
        over the frames).  No ground truth is needed in `data`.
          num_hypotheses: None -> one scene per sample from the deterministic heads (`generate_end_points`); H -> the H
          hypotheses of `generate_hypotheses(return_device=True)` (n_samples, seed as there), an H * B stack that reads
          the B joints rows in place.
          dump_threshold: None -> cfg.config['generation']['dump_threshold'] when present, else 0.5.
        From the end points on nothing leaves the device except the one check `parse_predictions` inherits from the
        reference (`assert len(pick) > 0`); the SceneBatch crosses to the host when the caller asks it to."""
        from ...net_utils import scene_device
        from ...net_utils.ap_helper import parse_predictions
        if dump_threshold is None:
            dump_threshold = (self.cfg.config.get('generation') or {}).get('dump_threshold', 0.5)
        joints = data['input_joints']
        if num_hypotheses is None:
            end_points = self.generate_end_points(data)
            eval_dict, parsed = parse_predictions(end_points, data, self.cfg.eval_config, return_device=True)
            H, out = 1, {'pred_mask': eval_dict['pred_mask'], **parsed}
        else:
            out = self.generate_hypotheses(data, num_hypotheses, n_samples=n_samples, seed=seed, return_device=True)
            H = out['pred_mask'].shape[0]
            out = {k: out[k].reshape(H * out[k].shape[1], *out[k].shape[2:])
                   for k in ('pred_mask', 'pred_corners_3d', 'obj_prob', 'pred_sem_cls')}
        return scene_device.scenes_from_parsed(out['pred_corners_3d'], out['obj_prob'], out['pred_mask'],
                                               out['pred_sem_cls'], joints, dump_threshold, contact=contact,
                                               unique=unique, num_hypotheses=H)

    def predict_consensus(self, data, num_hypotheses, n_samples=None, seed=None, dump_threshold=None, iou_thresh=0.25,
                          class_aware=True, contact=True, unique=True):
        """One scene per sample out of `num_hypotheses` hypotheses: `predict_scenes(...)` with the same arguments, then
        `SceneBatch.consensus(iou_thresh, class_aware)` -- the objects the hypotheses agree on, in how many of them each
        appears and how far apart they put it (net_utils.consensus_device.ConsensusBatch; its `.scenes` is the
        SceneBatch).  Nothing more crosses to the host than in `predict_scenes`."""
        scenes = self.predict_scenes(data, num_hypotheses=num_hypotheses, n_samples=n_samples, seed=seed,
                                     dump_threshold=dump_threshold, contact=contact, unique=unique)
        return scenes.consensus(iou_thresh=iou_thresh, class_aware=class_aware)

    def predict_occupancy(self, data, grid, num_hypotheses=None, n_samples=None, seed=None, dump_threshold=None,
                          min_votes=None, owner=False, body=True, with_gt=False):
        """The predicted scenes as occupancy maps on `grid` (net_utils.occupancy_device.Grid): `predict_scenes(...)` with
        the same arguments, then `SceneBatch.occupancy(grid, ...)` -- per sample and hypothesis the voxels its boxes
        cover, per voxel the votes of the hypotheses, with `body` the voxels the input joints fall into and with
        `with_gt` (data must hold the labels) the ground-truth map and the scene IoU
        (net_utils.occupancy_device.OccupancyBatch; its `.scenes` is the SceneBatch).  Nothing more crosses to the host
        than in `predict_scenes`."""
        from ...net_utils import occupancy_device
        scenes = self.predict_scenes(data, num_hypotheses=num_hypotheses, n_samples=n_samples, seed=seed,
                                     dump_threshold=dump_threshold, contact=False, unique=False)
        gt = occupancy_device.scenes_from_labels(data, self.cfg) if with_gt else None
        return scenes.occupancy(grid, joints=data['input_joints'] if body else None, gt=gt, min_votes=min_votes,
                                owner=owner)

    def predict_interactions(self, data, num_hypotheses=None, n_samples=None, seed=None, dump_threshold=None,
                             contact_thresh=None, merge_gap=0, min_len=1, max_intervals=16):
        """When the body is in contact with which predicted object: `predict_scenes(...)` with the same arguments, then
        `SceneBatch.interactions(data['input_joints'], ...)` -- per node the contact frames as intervals, merged over
        gaps of at most `merge_gap` frames and at least `min_len` long, the joints that touch it, and per frame the node
        the body is most in contact with (net_utils.interaction_device.InteractionBatch; its `.scenes` is the
        SceneBatch).  Nothing more crosses to the host than in `predict_scenes`."""
        scenes = self.predict_scenes(data, num_hypotheses=num_hypotheses, n_samples=n_samples, seed=seed,
                                     dump_threshold=dump_threshold, contact=True, unique=False)
        return scenes.interactions(data['input_joints'], contact_thresh=contact_thresh, merge_gap=merge_gap,
                                   min_len=min_len, max_intervals=max_intervals)

    def loss(self, pred_data, gt_data):
        if isinstance(pred_data, tuple):
            pred_data = pred_data[0]
        return self.detection_loss(pred_data, gt_data, self.cfg.dataset_config)
