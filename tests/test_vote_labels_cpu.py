"""CPU: the vote-label contract (csrc/vote_labels.hip, net_utils/vote_labels.py) before any kernel is involved: the
NumPy mirror against the reference's own get_votes (G13), the slot rule on hand-made boxes, the checks of
contact_tables, the ABI of include/p2r_vote_labels.h / libp2r_vote_labels.so and the argument checks of its two entry
points, which return on the host before any launch."""
import ctypes
import subprocess

import numpy as np
import pytest

from pose2room_amd import _lib
from pose2room_amd.net_utils import vote_labels as vl
from pose2room_amd.p2rnet.synthetic import make_raw_sample
from tests import vote_cases
from tests.test_binding_cpu import _c_compiler

EINVAL = -22


# ---- 1. the mirror against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(9))
def test_mirror_equals_reference(i):
    case = vote_cases.g13()[i]
    got = vl.vote_labels_reference(case.joints, case.instances, case.contact_dist)
    assert got.dtype == np.float32 and got.shape == case.votes.shape
    assert np.array_equal(got[..., 0], case.votes[..., 0])                  # the mask
    assert got.tobytes() == case.votes.tobytes()                            # every bit, signed zeros included


def test_fixture_covers_what_it_claims():
    cases = vote_cases.g13()
    assert len(cases) == 9 and len(cases) >= 7
    assert sorted({c.joints.shape[0] for c in cases}) == [1, 5, 7, 19, 37]
    assert {len(c.instances) for c in cases} >= {0, 1, 2, 4, 10}
    assert [c.contact_dist for c in cases] == [1.0] * 8 + [0.5]
    total = np.sum([c.hist for c in cases], 0)
    assert all(total[:4] > 0) and total[4:].sum() > 0                       # 0, 1, 2, 3 and >= 4 hits all occur
    for c in cases:
        assert c.hist.sum() == c.joints.shape[0] * 53
        assert c.hist[0] == (c.votes[..., 0] == 0).sum()
        assert c.face_dist >= 1e-6, c.name                                 # no label hangs on a rounding of the hull test


# ---- 2. the slot rule ----------------------------------------------------------------------------------------------------
def _box(centre, size):
    return {'class_id': 0, 'centroid': np.array(centre, np.float64), 'R_mat': np.eye(3), 'size': np.array(size, np.float64)}


def test_slot_rule():
    # five nested boxes around joint 0, one box around joint 1 alone, nothing near joint 2
    nested = [_box((0.1 * k, 0.0, 0.0), (1.0 + k,) * 3) for k in range(5)]
    single = _box((50.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    joints = np.array([[[0.25, 0.5, -0.125], [50.5, 0.25, 0.0], [-100.0, 0.0, 0.0]]], np.float32)
    out = vl.vote_labels_reference(joints, nested + [single], 0.25)
    assert out.shape == (1, 3, 10)
    p = joints[0].astype(np.float64)
    vote = lambda box, j: (box['centroid'] - p[j]).astype(np.float32)       # noqa: E731
    assert out[0, 0, 0] == 1 and out[0, 1, 0] == 1
    assert np.array_equal(out[0, 0, 1:], np.concatenate([vote(nested[0], 0), vote(nested[1], 0), vote(nested[4], 0)]))
    assert np.array_equal(out[0, 1, 1:], np.tile(vote(single, 1), 3))
    assert out[0, 2].tobytes() == np.zeros(10, np.float32).tobytes()        # ten +0.0
    # the face itself is inside (<=), the next f32 beyond it is not
    edge = np.array([[[0.75, 0.0, 0.0], [np.nextafter(np.float32(0.75), np.float32(1)), 0.0, 0.0]]], np.float32)
    assert vl.vote_labels_reference(edge, [_box((0, 0, 0), (1, 1, 1))], 0.25)[0, :, 0].tolist() == [1.0, 0.0]


def test_contact_tables_rows_and_checks():
    _, _, inst, _ = make_raw_sample(3, n_boxes=4, seed=11)
    (c, R, h), n = vl.contact_tables(inst, 10, 1.0)
    assert n == 4 and c.shape == (10, 3) and R.shape == (10, 9) and h.shape == (10, 3)
    assert c.dtype == R.dtype == h.dtype == np.float64
    for i, node in enumerate(inst):
        assert np.array_equal(c[i], node['centroid']) and np.array_equal(R[i], node['R_mat'].reshape(9))
        assert h[i].tobytes() == (np.array(node['size']) / 2. + 1.0).tobytes()
    assert not c[4:].any() and not R[4:].any() and not h[4:].any()
    sheared = dict(inst[1], R_mat=inst[1]['R_mat'] + np.array([[0, 1e-3, 0], [0, 0, 0], [0, 0, 0]]))
    with pytest.raises(ValueError, match=r"sample 7 \(s7\), box 1.*orthonormal"):
        vl.contact_tables([inst[0], sheared], 10, 1.0, name="7 (s7)")
    with pytest.raises(ValueError, match="max_num_obj"):
        vl.contact_tables(make_raw_sample(2, n_boxes=11, seed=2)[2], 10, 1.0)
    with pytest.raises(ValueError, match="box 0.*not finite"):
        vl.contact_tables([dict(inst[0], size=np.array([1.0, np.nan, 1.0]))], 10, 1.0)
    with pytest.raises(ValueError, match="not finite"):
        vl.contact_tables([dict(inst[0], centroid=np.array([np.inf, 0.0, 0.0]))], 10, 1.0)
    with pytest.raises(ValueError, match="contact_dist"):
        vl.contact_tables(inst, 10, float('nan'))
    assert vl.default_contact_dist() == 1.0


# ---- 3. the ABI ----------------------------------------------------------------------------------------------------------
def test_header_binds_and_library_exports_exactly_it():
    from pose2room_amd.net_utils import ap_device, mm_device
    protos = _lib.prototypes(vl.HEADER_PATH)
    assert sorted(protos) == _lib.declared_symbols(vl.HEADER_PATH) == ['p2r_assemble_batch_lean', 'p2r_vote_labels']
    assert protos['p2r_vote_labels'].kinds == 'pppiiipp' and protos['p2r_vote_labels'].has_stream
    assert protos['p2r_vote_labels'].argtypes[5] is ctypes.c_longlong
    assert protos['p2r_assemble_batch_lean'].kinds == 'ppippiiip' and protos['p2r_assemble_batch_lean'].has_stream
    out = subprocess.run(["nm", "-D", "--defined-only", vl.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(protos)
    for other in (None, ap_device.HEADER_PATH, mm_device.HEADER_PATH):
        assert not set(protos) & set(_lib.declared_symbols(*([other] if other else [])))
    l = vl.lib()
    assert l.p2r_vote_labels.argtypes == protos['p2r_vote_labels'].argtypes and l.p2r_vote_labels.restype is ctypes.c_int


def test_libp2r_hip_still_exports_exactly_its_header():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(_lib.declared_symbols())
    assert 'p2r_assemble_batch' in exported and 'p2r_vote_labels' not in exported


def test_contact_boxes_layout_matches_the_compiler(tmp_path):
    import os
    cls = _lib.struct('p2r_contact_boxes', vl.HEADER_PATH)
    assert cls is not None and vl._Boxes._fields_ == cls._fields_
    assert [f for f, _ in cls._fields_] == ['centroid', 'R_mat', 'half', 'n_boxes', 'K']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "p2r_vote_labels.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(p2r_contact_boxes));']
    lines += [f'  printf("{f} %zu\\n", offsetof(p2r_contact_boxes, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_c_compiler(), "-std=c99", "-I", os.path.dirname(vl.HEADER_PATH), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    got = dict((ln.split()[0], int(ln.split()[1]))
               for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {'sizeof': ctypes.sizeof(cls)}
    want.update({f: getattr(cls, f).offset for f, _ in cls._fields_})
    assert got == want


# ---- 4. argument checks: on the host, before any launch ------------------------------------------------------------------
_Store, _Out = _lib.struct('p2r_sample_store'), _lib.struct('p2r_batch_out')
_BUF = ctypes.create_string_buffer(64)          # a non-NULL address; never read, every call below is refused first
_P = ctypes.addressof(_BUF)


def _boxes(**over):
    return vl._Boxes(**{**dict(centroid=_P, R_mat=_P, half=_P, n_boxes=_P, K=10), **over})


def _store(**over):
    ptrs = {f: _P for f, t in _Store._fields_ if t is ctypes.c_void_p}
    return _Store(**{**ptrs, 'votes': 0, 'n_frames_total': 8, 'n_samples': 2, 'J': 53, 'K': 10, **over})


def _out(**over):
    return _Out(**{**{f: _P for f, _ in _Out._fields_}, **over})


def test_vote_labels_refuses_bad_arguments():
    fn = vl.lib().p2r_vote_labels
    good = dict(joints=_P, frame_offset=_P, n_frames=_P, n_samples=2, J=53, F=8, boxes=_boxes(), votes=_P)

    def call(**over):
        a = {**good, **over}
        boxes = None if a['boxes'] is None else ctypes.byref(a['boxes'])
        return fn(a['joints'], a['frame_offset'], a['n_frames'], a['n_samples'], a['J'], a['F'], boxes, a['votes'], None)
    for bad in (dict(joints=None), dict(frame_offset=None), dict(n_frames=None), dict(votes=None), dict(boxes=None),
                dict(boxes=_boxes(K=-1)), dict(boxes=_boxes(K=257)), dict(boxes=_boxes(n_boxes=0)),
                dict(boxes=_boxes(centroid=0)), dict(boxes=_boxes(R_mat=0)), dict(boxes=_boxes(half=0)),
                dict(J=0), dict(J=-3), dict(n_samples=0), dict(n_samples=-1), dict(F=0), dict(F=-1),
                dict(F=1 << 40, J=1 << 20)):
        assert call(**bad) == EINVAL, bad


def test_assemble_batch_lean_refuses_bad_arguments():
    fn = vl.lib().p2r_assemble_batch_lean
    good = dict(store=_store(), boxes=_boxes(), B=4, sel=_P, aug=_P, augment=1, use_height=1, num_frames=16, out=_out())

    def call(**over):
        a = {**good, **over}
        ref = lambda s: None if s is None else ctypes.byref(s)      # noqa: E731
        return fn(ref(a['store']), ref(a['boxes']), a['B'], a['sel'], a['aug'], a['augment'], a['use_height'],
                  a['num_frames'], ref(a['out']), None)
    for bad in (dict(store=None), dict(boxes=None), dict(out=None), dict(store=_store(votes=_P)),
                dict(store=_store(joints=0)), dict(store=_store(frame_offset=0)), dict(store=_store(n_frames=0)),
                dict(store=_store(floor_height=0)), dict(store=_store(box_center=0)), dict(store=_store(J=0)),
                dict(store=_store(n_samples=0)), dict(store=_store(K=257)), dict(store=_store(n_frames_total=0)),
                dict(boxes=_boxes(K=-1)), dict(boxes=_boxes(K=257)), dict(boxes=_boxes(n_boxes=0)),
                dict(boxes=_boxes(half=0)), dict(B=-1), dict(B=65536), dict(num_frames=0), dict(num_frames=-5),
                dict(num_frames=1 << 30, store=_store(J=1 << 12)), dict(augment=2), dict(use_height=-1),
                dict(sel=None), dict(aug=None), dict(out=_out(vote_label=0)), dict(out=_out(vote_label_mask=0)),
                dict(out=_out(input_joints=0)), dict(out=_out(heading=0))):
        assert call(**bad) == EINVAL, bad
        if not {'B', 'sel', 'aug', 'out'} & set(bad) and bad.get('num_frames', 0) < 1:
            assert call(**bad, B=0) == EINVAL, bad              # an empty batch does not excuse a bad store
    # an empty batch is no error and launches nothing, whatever the per-batch pointers are
    assert call(B=0) == 0 and call(B=0, sel=None, aug=None, out=_out(vote_label=0)) == 0
    # the full store's entry point keeps refusing a store without votes
    assert _lib.lib().p2r_assemble_batch(ctypes.byref(_store()), 0, None, None, 0, 0, 16, ctypes.byref(_out()), None) == EINVAL
    assert _lib.lib().p2r_assemble_batch(ctypes.byref(_store(votes=_P)), 0, None, None, 0, 0, 16, ctypes.byref(_out()), None) == 0


def test_python_layer_refuses_cpu_tensors_and_bad_modes():
    import torch
    from pose2room_amd.p2rnet import device_loader as dv
    with pytest.raises(RuntimeError, match="GPU tensor"):
        vl.vote_labels(torch.zeros(2, 53, 3), torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int32), None)
    with pytest.raises(RuntimeError, match="GPU"):
        vl.generate_votes(np.zeros((2, 53, 3), np.float32), [], device='cpu')
    ok = make_raw_sample(4, seed=1)
    with pytest.raises(ValueError, match="'store' or 'derive'"):
        dv.DeviceSampleStore([ok], device='cuda:0', votes='lean')
    # a sample without votes goes through the same checks, and its boxes through contact_tables'
    with pytest.raises(ValueError, match='float32'):
        dv.DeviceSampleStore([(ok[0].astype(np.float64), None, [], 'f64')], device='cuda:0')
    with pytest.raises(ValueError, match='joints'):
        dv.DeviceSampleStore([(ok[0][:, :52], None, [], 'j52')], device='cuda:0', votes='derive')
    with pytest.raises(ValueError, match='max_num_obj'):
        dv.DeviceSampleStore([make_raw_sample(4, n_boxes=11, seed=2)], device='cuda:0', votes='derive')
    sheared = [dict(ok[2][0], R_mat=ok[2][0]['R_mat'] * 1.01)]
    for kw in (dict(votes='derive'), dict()):
        with pytest.raises(ValueError, match=r"sample 1 \(bad\), box 0.*orthonormal"):
            dv.DeviceSampleStore([ok, (ok[0], None, sheared, 'bad')], device='cuda:0', **kw)
    with pytest.raises(MemoryError, match='max_bytes'):
        dv.DeviceSampleStore([ok], device='cuda:0', max_bytes=1000, votes='derive')
    with pytest.raises(RuntimeError, match='GPU'):
        dv.DeviceSampleStore([(ok[0], None, ok[2], 'n')], device='cpu')
