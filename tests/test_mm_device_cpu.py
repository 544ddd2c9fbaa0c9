"""CPU: the device multi-modal evaluation's ABI (include/p2r_mm_eval.h, libp2r_mm_eval.so), the dense restatement of
the TMD against the host function and G11 (the reference's recorded output) before any kernel is involved, and the
argument checks of the Python layer."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from pose2room_amd import _lib
from tests import mm_cases

EINVAL = -22


def test_entry_points_declared_exported_and_shape_checked():
    """include/p2r_mm_eval.h declares the two entry points and libp2r_mm_eval.so exports exactly them; neither is
    declared by the other two headers"""
    from pose2room_amd.net_utils import ap_device, mm_device
    protos = _lib.prototypes(mm_device.HEADER_PATH)
    assert sorted(protos) == _lib.declared_symbols(mm_device.HEADER_PATH) == ['p2r_box_params', 'p2r_tmd']
    assert protos['p2r_box_params'].kinds == 'ipp' and protos['p2r_box_params'].has_stream
    assert protos['p2r_tmd'].kinds == 'iiippppp' and protos['p2r_tmd'].has_stream
    out = subprocess.run(["nm", "-D", "--defined-only", mm_device.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(protos)
    assert not set(protos) & set(_lib.declared_symbols())
    assert not set(protos) & set(_lib.declared_symbols(ap_device.HEADER_PATH))
    l = mm_device.lib()
    assert l.p2r_tmd.argtypes == protos['p2r_tmd'].argtypes and l.p2r_box_params.restype is ctypes.c_int
    n = None
    # refused before the device is touched: NULL operands, no GPU needed
    for H, B, K in [(0, 1, 1), (65, 1, 1), (1, 1, 1025), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (1, 1 << 22, 1024)]:
        assert l.p2r_tmd(H, B, K, n, n, n, n, n, n) == EINVAL, (H, B, K)
    assert l.p2r_box_params(-1, n, n, n) == EINVAL
    # empty problems are no error and launch nothing
    assert l.p2r_tmd(3, 0, 24, n, n, n, n, n, n) == 0 and l.p2r_tmd(3, 4, 0, n, n, n, n, n, n) == 0
    assert l.p2r_box_params(0, n, n, n) == 0


def test_dense_tmd_reproduces_host_tmd_and_g11():
    from pose2room_amd.net_utils.multi_modal_eval import tmd
    obbs, keep, cls = mm_cases.g11_dense()
    value, count = mm_cases.tmd_dense(obbs, keep, cls)
    present = count > 0
    # G11 alone exercises the entropy term and kept counts from 1 to all 10 hypotheses (mm_cases.edge_case has the rest)
    assert present.sum() == 64 and count[present].min() == 1 and count[present].max() == 10
    several = sum(len(set(cls[keep[:, b, k] != 0, b, k].tolist())) > 1 for b, k in zip(*np.nonzero(present)))
    assert several == 54
    assert (value[~present] == 0).all() and (value[present] >= 1).all()
    got = value.sum() / present.sum()
    assert got == pytest.approx(tmd(mm_cases.g11_records()), rel=0, abs=1e-9)
    assert got == pytest.approx(float(mm_cases.G11['b_tmd'][0]), rel=0, abs=1e-9)


@pytest.mark.parametrize("shape", mm_cases.EDGE_SHAPES)
def test_edge_cases_are_what_they_claim(shape):
    obbs, keep, cls, value, count, cells = mm_cases.edge_case(*shape)
    assert np.array_equal(count, keep.astype(bool).sum(0)) and (value[count == 0] == 0).all()
    if shape == (10, 3, 40):
        assert {'kept nowhere', 'kept once', 'identical boxes', 'classes 0 0 1 2'} <= set(cells)
        assert 0.4 < keep.mean() < 0.8 and len(np.unique(count)) > 5


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from pose2room_amd.net_utils import mm_device
    with pytest.raises(RuntimeError, match="GPU tensor"):
        mm_device.box_params(torch.zeros(2, 8, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        mm_device.tmd_values(torch.zeros(2, 1, 3, 7, dtype=torch.float64), torch.ones(2, 1, 3, dtype=torch.uint8),
                             torch.zeros(2, 1, 3, dtype=torch.long))
    ev = mm_device.DeviceMultiModalEvaluator(2, [0.25, 0.5], num_class=3)
    z = torch.zeros(2, 1, 2, 8, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ev.step_tensors(z, torch.ones(2, 1, 2), torch.ones(2, 1, 2), torch.zeros(2, 1, 2, 3),
                        torch.zeros(2, 1, 2, dtype=torch.long), z[0], torch.zeros(1, 2, dtype=torch.long), torch.ones(1, 2))
    for bad in (0, 65):
        with pytest.raises(ValueError):
            mm_device.DeviceMultiModalEvaluator(bad, [0.25])
    # nothing fed: empty metric dicts per hypothesis and threshold, NaN TMD (np.mean([]) of the host code), no records
    out = ev.compute()
    assert len(out['metrics']) == 2 and all(len(row) == 2 for row in out['metrics']) and np.isnan(out['tmd'])
    assert ev.records() == [[], []]


def test_multi_modal_loop_refuses_unknown_impl():
    from pose2room_amd.p2rnet import testing
    with pytest.raises(ValueError, match="impl"):
        testing.test_multi_modal(None, None, [], 3, impl='nonsense')
