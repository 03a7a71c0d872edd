"""Host-side checks of the stage-2 (config/step2_axis.yaml) training path: the package's config against the reference's settings
(tests/golden/reference_step2_axis.yaml, a copy of the reference's config/step2_axis.yaml), the training-mode routing, and the float64
restatement of the axis loss that tests/test_gpu_axis_training.py holds the kernel to."""
import os
import types

import pytest
import torch
import torch.nn.functional as F
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ float64 restatement of axis_head.py:95-201
def double_angle(sc: torch.Tensor) -> torch.Tensor:
    s, c = sc[:, 0:1], sc[:, 1:2]
    return torch.cat((2 * s * c, c ** 2 - s ** 2), 1)


def smooth_l1(x: torch.Tensor, beta: float) -> torch.Tensor:
    """fvcore.nn.smooth_l1_loss(input, target, beta, reduction=None) of x = input - target."""
    if beta < 1e-5:
        return torch.abs(x)
    n = torch.abs(x)
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def masked_mean(loss: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
    """loss_weight-free torch.masked_select(loss, valid.ge(0.5)).mean(), valid [N,1] broadcast over the row."""
    return torch.masked_select(loss, valid.ge(0.5)).mean()


def axis_loss_ref(raw_rot, raw_tran, gt_rot, gt_tran, beta=0.0, loss_weight=1.0):
    """raw_rot [N,3] / raw_tran [N,2] (before F.normalize), gt_* [N,4] -> (loss_rot, loss_tran), as axis_head.py computes them (the
    early return of a valid column summing below 1 included).  Differentiable: backward gives the reference's gradients."""
    rot = torch.cat((F.normalize(raw_rot[:, :2], p=2, dim=1), raw_rot[:, 2:3]), 1)
    tran = F.normalize(raw_tran, p=2, dim=1)
    out = []
    for pred, gt, kind in ((rot, gt_rot, "rot"), (tran, gt_tran, "tran")):
        valid = gt[:, 3:4]
        if len(gt) == 0 or valid.sum() < 1:
            out.append(pred.sum() * 0.0)
            continue
        if kind == "rot":
            l = smooth_l1(pred - gt[:, :3], beta)
        else:
            l = smooth_l1(double_angle(pred) - double_angle(gt[:, :2]), beta)
        out.append(loss_weight * masked_mean(l, valid))
    return out[0], out[1]


def test_double_angle_and_masked_mean_known_answers():
    # angle 30 degrees -> 60 degrees
    sc = torch.tensor([[0.5, 3 ** 0.5 / 2], [0.0, 1.0], [1.0, 0.0]], dtype=torch.float64)
    want = torch.tensor([[3 ** 0.5 / 2, 0.5], [0.0, 1.0], [0.0, -1.0]], dtype=torch.float64)
    assert torch.allclose(double_angle(sc), want, atol=1e-15)
    l = torch.tensor([[1.0, 2.0, 3.0], [10.0, 20.0, 30.0], [4.0, 5.0, 6.0]], dtype=torch.float64)
    valid = torch.tensor([[1.0], [0.0], [0.5]], dtype=torch.float64)
    assert masked_mean(l, valid).item() == pytest.approx(21.0 / 6.0, abs=0)  # rows 0 and 2: (1+2+3+4+5+6) / 6
    assert smooth_l1(torch.tensor([-2.0, 0.0, 0.25]), 0.0).tolist() == [2.0, 0.0, 0.25]
    assert smooth_l1(torch.tensor([-2.0, 0.25]), 0.5).tolist() == [1.75, 0.0625]
    # a whole loss by hand: one valid row, raw (3, 4) -> (0.6, 0.8), offset 1; gt (0, 1, 0.5)
    raw_rot = torch.tensor([[3.0, 4.0, 1.0], [7.0, 7.0, 7.0]], dtype=torch.float64)
    raw_tran = torch.tensor([[0.0, 2.0], [1.0, 0.0]], dtype=torch.float64)
    gt_rot = torch.tensor([[0.0, 1.0, 0.5, 1.0], [0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    gt_tran = torch.tensor([[1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 1.0]], dtype=torch.float64)
    lr, lt = axis_loss_ref(raw_rot, raw_tran, gt_rot, gt_tran)
    assert lr.item() == pytest.approx((0.6 + 0.2 + 0.5) / 3, abs=1e-15)
    # tran row 0: (0, 1) -> double angle (0, 1) vs gt (1, 0) -> (0, -1): |0| + |2|; row 1: (1, 0) -> (0, -1) vs (0, 1): |0| + |-2|
    assert lt.item() == pytest.approx(4.0 / 4, abs=1e-15)
    lr0, lt0 = axis_loss_ref(raw_rot, raw_tran, gt_rot * torch.tensor([1, 1, 1, 0.0]), gt_tran * torch.tensor([1, 1, 1, 0.0]))
    assert lr0.item() == 0.0 and lt0.item() == 0.0


# ------------------------------------------------------------------------------------------ config
def _flat(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flat(v, prefix + k + "."))
        else:
            out[prefix + k] = v
    return out


def test_step2_axis_config_has_the_reference_keys_and_values():
    with open(os.path.join(ROOT, "configs", "step2_axis.yaml")) as f:
        mine = _flat(yaml.safe_load(f))
    with open(os.path.join(ROOT, "tests", "golden", "reference_step2_axis.yaml")) as f:
        ref = _flat(yaml.safe_load(f))
    assert mine.pop("MODEL.WEIGHTS") == "" and "MODEL.WEIGHTS" in ref
    ref.pop("MODEL.WEIGHTS")
    assert set(mine) == set(ref), set(mine) ^ set(ref)
    for k in ref:
        assert mine[k] == ref[k], (k, mine[k], ref[k])
    assert mine["MODEL.AXIS_ON"] is True and mine["MODEL.FREEZE"] == ["backbone", "proposal_generator", "roi_heads.box_head",
                                                                     "roi_heads.box_predictor"]
    # ... and it merges into the package's defaults
    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults

    cfg = get_cfg()
    get_planercnn_cfg_defaults(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "step2_axis.yaml"))
    assert cfg.MODEL.AXIS_ON and not cfg.MODEL.PLANE_ON and cfg.MODEL.ROI_AXIS_HEAD.SMOOTH_L1_BETA == 0.0


# ------------------------------------------------------------------------------------------ routing
def _stub(mask=False, plane=False, axis=False, depth=False, freeze=()):
    from articulation3d_amd.modeling.meta_arch import PlaneRCNN

    m = types.SimpleNamespace(depth_head_on=depth, roi_heads=types.SimpleNamespace(mask_on=mask, plane_on=plane, axis_on=axis),
                              _freeze=list(freeze), STAGE2_FREEZE=PlaneRCNN.STAGE2_FREEZE)
    return lambda: PlaneRCNN.training_stage(m)


def test_training_routing_accepts_stages_one_and_two_and_refuses_stage_three():
    f2 = ["backbone", "proposal_generator", "roi_heads.box_head", "roi_heads.box_predictor"]
    assert _stub()() == 1  # step1_bbox.yaml
    assert _stub(axis=True, freeze=f2)() == 2  # step2_axis.yaml
    for bad in (dict(axis=True),  # axis without the stage-2 freeze
                dict(axis=True, freeze=f2[:3]),
                dict(mask=True, plane=True, axis=True, depth=True, freeze=["backbone"]),  # step3_plane.yaml's flags
                dict(mask=True, plane=True, depth=True), dict(plane=True, axis=True, freeze=f2)):
        with pytest.raises(NotImplementedError) as e:
            _stub(**bad)()
        assert "step1_bbox" in str(e.value) and "step2_axis" in str(e.value)
