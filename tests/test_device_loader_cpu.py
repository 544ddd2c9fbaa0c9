"""CPU: the arithmetic contract of the device batch assembly (csrc/batch_assemble.hip, p2rnet/device_loader.py) against
the host loader, augment_sample + sample_to_tensors (dataloader.py), bit for bit; the store's input checks."""
import os

import numpy as np
import pytest

from pose2room_amd.p2rnet import dataloader as dl
from pose2room_amd.p2rnet import device_loader as dv
from pose2room_amd.p2rnet.synthetic import make_raw_sample

KEYS = ['input_joints', 'box_label_mask', 'sem_cls_label', 'center_label', 'size', 'heading', 'vote_label',
        'vote_label_mask']
VARIANTS = [(f, a) for f in (0, 1) for a in dv.ANGLES]


def _g8_sample():
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g8_loader_demo.npz'))
    inst = [{'class_id': int(g['s_class_id'][i]), 'centroid': g['s_centroid'][i], 'R_mat': g['s_R_mat'][i],
             'size': g['s_size'][i]} for i in range(len(g['s_class_id']))]
    return g['s_joints'].copy(), g['s_votes'].copy(), inst, 'g8'


def mirror_item(sample, num_frames, use_height, draw=None, max_num_obj=10):
    """The kernel's formula in NumPy: store tables + gather + per-frame transform."""
    joints, votes, inst, name = sample
    ids = dv.resample_reference(joints.shape[0], num_frames)
    floor = dv.floor_heights(joints)
    center, heading, size, mask, cls = dv.box_tables(inst, max_num_obj)
    if draw is None:
        j, v, m = dv.transform_reference(joints[ids], votes[ids], floor, False, use_height=use_height)
        c, h = center[dv.PLAIN].copy(), heading[dv.PLAIN]
    else:
        flip, angle, off = draw
        j, v, m = dv.transform_reference(joints[ids], votes[ids], floor, True, flip, dl.rot_y(angle), off, use_height)
        var = 4 * flip + dv.ANGLES.index(angle)
        c, h = center[var].copy(), heading[var]
        n = len(inst)
        c[:n] = c[:n] + np.array([1., 0., 1.]) * off
    return {'input_joints': j, 'box_label_mask': mask, 'sem_cls_label': cls, 'center_label': c.astype(np.float32),
            'size': size, 'heading': h, 'vote_label': v, 'vote_label_mask': m}


def host_item(sample, num_frames, use_height, draw=None, max_num_obj=10):
    joints, votes, inst, name = sample
    if draw is not None:
        joints, inst, votes = dl.augment_sample(joints, inst, votes, *draw)
    return dl.sample_to_tensors(joints, votes, inst, num_frames, max_num_obj, use_height, name)


def assert_bitwise(got, want):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), k          # bit patterns: signed zeros count


CASES = [(1, 768), (2, 2048), (37, 64), (37, 1), (341, 768), (700, 1024), (1024, 1024), (1500, 768), (5000, 2048),
         (5000, 1024)]


@pytest.mark.parametrize("T0,num_frames", CASES)
def test_mirror_equals_host_loader(T0, num_frames):
    sample = make_raw_sample(T0, n_boxes=6, seed=T0 + num_frames)
    for uh in (False, True):
        assert_bitwise(mirror_item(sample, num_frames, uh), host_item(sample, num_frames, uh))
    for i, (flip, angle) in enumerate(VARIANTS):
        draw = (flip, angle, (-0.83, 0.41, -0.0625, 0.97)[i % 4])
        uh = bool((i + T0) % 2)
        assert_bitwise(mirror_item(sample, num_frames, uh, draw), host_item(sample, num_frames, uh, draw))


def test_mirror_equals_host_loader_on_reference_sample():
    """The reference's own raw sample (tests/golden/g8_loader_demo.npz: f32 frames, three boxes)."""
    sample = _g8_sample()
    for num_frames in (1, 64, 768):
        for uh in (False, True):
            assert_bitwise(mirror_item(sample, num_frames, uh), host_item(sample, num_frames, uh))
            for flip, angle in VARIANTS:
                for off in (-0.3, 0.77):
                    draw = (flip, angle, off)
                    assert_bitwise(mirror_item(sample, num_frames, uh, draw), host_item(sample, num_frames, uh, draw))


def test_linspace_mirror():
    for T0 in list(range(1, 70)) + [127, 128, 341, 999, 1000, 1023, 1024, 1025, 4097, 5000, 65534, 65535]:
        for nf in [1, 2, 3, 5, 7, 16, 63, 64, 100, 768, 1000, 1024, 2048, 4099]:
            want = np.linspace(0, T0 - 1, nf).round().astype(np.uint16)
            got = dv.resample_reference(T0, nf)
            assert np.array_equal(got, want.astype(np.int64)), (T0, nf)


def test_box_table_plus_offset_equals_node_math():
    sample = make_raw_sample(8, n_boxes=7, seed=3)
    joints, votes, inst, _ = sample
    center, heading, size, mask, cls = dv.box_tables(inst, 10)
    for flip, angle in VARIANTS:
        var = 4 * flip + dv.ANGLES.index(angle)
        for off in (-0.999, -0.25, 0.0, 0.5):
            _, nodes, _ = dl.augment_sample(joints, inst, votes, flip, angle, off)
            for i, n in enumerate(nodes):
                c = center[var, i] + np.array([1., 0., 1.]) * off
                assert c.tobytes() == n['centroid'].tobytes()
                h = dl.rot2head(n['R_mat'])
                assert heading[var, i].tobytes() == np.array([np.sin(h), np.cos(h)], np.float32).tobytes()
    assert np.array_equal(mask, [1] * 7 + [0] * 3) and cls.dtype == np.int64 and (center[:, 7:] == 0).all()
    assert np.array_equal(cls[:7], [n['class_id'] for n in inst])
    with pytest.raises(ValueError):
        dv.box_tables(inst, 6)


def test_floor_height_is_augmentation_invariant():
    """use_height's floor once per sample: y is unchanged by every (flip, angle, offset), so the percentile of the
    augmented f64 joints equals that of the raw joints in f64; without augmentation it is the f32 percentile."""
    joints, votes, inst, _ = sample = make_raw_sample(300, seed=5)
    f64, f32 = dv.floor_heights(joints)
    assert f32 == float(np.percentile(joints[..., 1], 0.99)) and np.float32(f32) == np.percentile(joints[..., 1], 0.99)
    for flip, angle in VARIANTS:
        j, _, _ = dl.augment_sample(joints, inst, votes, flip, angle, -0.6)
        assert j.dtype == np.float64 and np.percentile(j[..., 1], 0.99) == f64


def test_store_rejects_bad_samples():
    ok = make_raw_sample(10, seed=1)
    long_j = np.zeros((dv.MAX_T0 + 1, 53, 3), np.float32)
    long_v = np.zeros((dv.MAX_T0 + 1, 53, 10), np.float32)
    with pytest.raises(ValueError, match='T0'):
        dv.DeviceSampleStore([ok, (long_j, long_v, [], 'long')], device='cuda:0')
    with pytest.raises(ValueError, match='joints'):
        dv.DeviceSampleStore([(ok[0][:, :52], ok[1][:, :52], [], 'j52')], device='cuda:0')
    with pytest.raises(ValueError, match='float32'):
        dv.DeviceSampleStore([(ok[0].astype(np.float64), ok[1], [], 'f64')], device='cuda:0')
    with pytest.raises(ValueError, match='max_num_obj'):
        dv.DeviceSampleStore([make_raw_sample(4, n_boxes=11, seed=2)], device='cuda:0')
    with pytest.raises(MemoryError, match='max_bytes'):
        dv.DeviceSampleStore([ok], device='cuda:0', max_bytes=1000)
    with pytest.raises(RuntimeError, match='GPU'):
        dv.DeviceSampleStore([ok], device='cpu')
