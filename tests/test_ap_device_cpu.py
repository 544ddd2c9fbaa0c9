"""CPU: the device AP calculator's ABI, its dense re-formulation of the matching rule against G7 (the reference's
recorded outputs) before any kernel is involved, and the host calculator after the helper refactor."""
import ctypes

import numpy as np
import pytest
import torch

from pose2room_amd import _lib
from tests import ap_cases

EINVAL = -22


def test_entry_points_declared_exported_and_shape_checked():
    """include/p2r_ap_eval.h declares the two entry points and libp2r_ap_eval.so exports exactly them; libp2r_hip.so and
    its header are what they were (ABI version 3)"""
    import subprocess
    from pose2room_amd.net_utils import ap_device
    protos = _lib.prototypes(ap_device.HEADER_PATH)
    assert sorted(protos) == _lib.declared_symbols(ap_device.HEADER_PATH) == ['p2r_ap_match', 'p2r_obb_iou']
    assert protos['p2r_obb_iou'].kinds == 'iiipppp' and protos['p2r_obb_iou'].has_stream
    assert protos['p2r_ap_match'].kinds == 'iiiiipppppppp' and protos['p2r_ap_match'].has_stream
    out = subprocess.run(["nm", "-D", "--defined-only", ap_device.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(protos)
    assert _lib.lib().p2r_abi_version() == 3 and not set(protos) & set(_lib.declared_symbols())
    l = ap_device.lib()
    assert l.p2r_obb_iou.argtypes == protos['p2r_obb_iou'].argtypes and l.p2r_ap_match.restype is ctypes.c_int
    n = None
    # refused before the device is touched: NULL operands, no GPU needed
    assert l.p2r_obb_iou(1, 1025, 1, n, n, n, n, n) == EINVAL
    assert l.p2r_obb_iou(1, 1, 257, n, n, n, n, n) == EINVAL
    assert l.p2r_obb_iou(1 << 20, 1024, 256, n, n, n, n, n) == EINVAL          # B*K*G does not fit in int
    assert l.p2r_obb_iou(-1, 1, 1, n, n, n, n, n) == EINVAL
    for N, K, G, C, T in [(1, 1025, 1, 1, 1), (1, 1, 257, 1, 1), (1, 1, 1, 65, 1), (1, 1, 1, 1, 9), (1, -1, 1, 1, 1)]:
        assert l.p2r_ap_match(N, K, G, C, T, n, n, n, n, n, n, n, n, n) == EINVAL, (N, K, G, C, T)
    # empty problems are no error and launch nothing
    assert l.p2r_obb_iou(0, 4, 4, n, n, n, n, n) == 0 and l.p2r_obb_iou(2, 4, 0, n, n, n, n, n) == 0
    assert l.p2r_ap_match(0, 4, 4, 4, 2, n, n, n, n, n, n, n, n, n) == 0


def test_dense_formulation_reproduces_g7():
    """IoU of every (proposal, ground truth) pair of a scan once, the parallel 'first claimant' rule, one stable
    descending sort per class: G7's per-class ap / rec / prec for both thresholds, and the calculator's metric dict."""
    d = ap_cases.g7_dense()
    iou = ap_cases.dense_iou_cpu(d['det'], d['gt'])
    tp, npos = ap_cases.dense_match_numpy(iou, d['score'], d['valid'], d['gt_cls'], d['gt_mask'], ap_cases.THRESHOLDS)
    assert ((tp == 255) == (d['valid'] == 0)[None]).all()
    ap_cases.assert_matches_g7(ap_cases.finalize(d['score'], tp, npos))


def test_device_calculator_refuses_cpu_tensors():
    from pose2room_amd.net_utils import ap_device
    z = torch.zeros(1, 2, 8, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ap_device.obb_iou(z, z)
    calc = ap_device.DeviceAPCalculator([0.25, 0.5], num_class=3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        calc.step_tensors(z, torch.ones(1, 2), torch.ones(1, 2), torch.zeros(1, 2, 3), torch.zeros(1, 2, dtype=torch.long),
                          z, torch.zeros(1, 2, dtype=torch.long), torch.ones(1, 2))
    with pytest.raises(ValueError):
        ap_device.DeviceAPCalculator([0.1] * 9)
    assert isinstance(ap_device.DeviceAPCalculator(0.25, num_class=3).compute_metrics(), dict)
    assert len(calc.compute_metrics()) == 2


def test_host_calculator_unchanged_by_the_shared_helpers():
    """APCalculator on G7 through eval_det.curve_from_flags / ap_helper.metrics_from_curves"""
    from pose2room_amd.net_utils.ap_helper import APCalculator
    G7 = ap_cases.G7
    n_scan = int(G7['n_scan'])
    pred_all = {i: [] for i in range(n_scan)}
    gt_all = {i: [] for i in range(n_scan)}
    for row, c in zip(G7['det_rows'], G7['det_corners']):
        pred_all[int(row[0])].append((int(row[1]), c, float(row[2])))
    for row, c in zip(G7['gt_rows'], G7['gt_corners']):
        gt_all[int(row[0])].append((int(row[1]), c))
    for thr in ap_cases.THRESHOLDS:
        calc = APCalculator(thr, None, False)
        calc.step([pred_all[i] for i in range(n_scan)], [gt_all[i] for i in range(n_scan)])
        m = calc.compute_metrics()
        tag = 'thr%02d' % int(thr * 100)
        assert list(m.keys()) == list(G7[tag + '_metric_keys'])
        np.testing.assert_allclose(np.array([float(v) for v in m.values()]), G7[tag + '_metric_vals'], rtol=1e-12, equal_nan=True)


def test_test_loop_refuses_unknown_ap_impl():
    from pose2room_amd.p2rnet import testing
    with pytest.raises(ValueError, match="ap_impl"):
        testing.test_func(None, None, [], ap_impl='gpu')
