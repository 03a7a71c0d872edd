"""Host-side checks of the stage-4 (configs/step3_planehead.yaml, the plane share of the reference's step3_plane.yaml) training path: the
config and the training-mode routing, the flat layout of the plane head, the FC's column helpers, the refusal of malformed gt_planes,
and the float64 references that tests/test_gpu_plane_training.py holds the kernel and the step to (tests/plane_train_ref.py)."""
import os
import types

import pytest
import torch
import yaml

import plane_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F2 = ["backbone", "proposal_generator", "roi_heads.box_head", "roi_heads.box_predictor"]
REF_STEP3 = F2 + ["roi_heads.axis_head"]  # MODEL.FREEZE of the reference's step3_plane.yaml
F4 = REF_STEP3 + ["roi_heads.mask_head", "depth_head"]
F3 = F2 + ["roi_heads.axis_head", "roi_heads.plane_head", "depth_head"]  # configs/step3_mask.yaml


def _cfg():
    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults

    cfg = get_cfg()
    get_planercnn_cfg_defaults(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "step3_planehead.yaml"))
    return cfg


def _stage(mask=False, plane=False, axis=False, depth=False, freeze=()):
    from articulation3d_amd.modeling.meta_arch import PlaneRCNN

    m = types.SimpleNamespace(depth_head_on=depth, roi_heads=types.SimpleNamespace(mask_on=mask, plane_on=plane, axis_on=axis),
                              _freeze=list(freeze), STAGE2_FREEZE=PlaneRCNN.STAGE2_FREEZE)
    return PlaneRCNN.training_stage(m)


# ------------------------------------------------------------------------------------------ config and routing
def test_step3_planehead_config_is_step3_plane_with_two_more_frozen_heads():
    cfg = _cfg()
    assert cfg.MODEL.MASK_ON and cfg.MODEL.PLANE_ON and cfg.MODEL.AXIS_ON and cfg.MODEL.DEPTH_ON
    assert list(cfg.MODEL.FREEZE) == REF_STEP3 + ["roi_heads.mask_head", "depth_head"] == F4
    with open(os.path.join(ROOT, "configs", "step3_planehead.yaml")) as f:
        raw = yaml.safe_load(f)
    assert raw["MODEL"]["WEIGHTS"] == ""
    assert raw["MODEL"]["ROI_PLANE_HEAD"] == dict(NAME="PlaneRCNNConvFCHead", POOLER_RESOLUTION=14, POOLER_TYPE="ROIAlign", LOSS_WEIGHT=1.0,
                                                  NORMAL_ONLY=True)
    assert raw["SOLVER"]["IMS_PER_BATCH"] == 8 and "INPUT" not in raw  # (bitmask ground truth is the mask stage's addition)


def test_step3_planehead_config_routes_to_stage_four_and_only_the_plane_head_trains():
    from articulation3d_amd.modeling import build_model
    from articulation3d_amd.modeling.meta_arch import STAGE_TRAINER

    cfg = _cfg()
    cfg.MODEL.DEVICE = "cpu"
    model = build_model(cfg)
    assert model.training_stage() == 4 and STAGE_TRAINER[4] == ("..training_plane", "PlaneTrainer")
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert trainable and all(n.startswith(R.PH) for n in trainable)
    assert {n.split(".")[2] for n in trainable} == {"plane_conv1", "plane_conv2", "plane_conv3", "plane_conv4", "plane_fc1", "param_pred"}
    # the module-level call still has no training path, and says where the training path is
    model.roi_heads.plane_head.train()
    with pytest.raises(NotImplementedError) as e:
        model.roi_heads.plane_head(torch.zeros(1, 256, 14, 14), [])
    assert "PlaneTrainer" in str(e.value)


def test_stage_four_routing_rules():
    assert _stage(mask=True, plane=True, axis=True, depth=True, freeze=F4) == 4  # configs/step3_planehead.yaml
    assert _stage(plane=True, freeze=F2) == 4  # every other head off
    assert _stage(mask=True, plane=True, freeze=F2 + ["roi_heads.mask_head"]) == 4  # plane + frozen mask
    # the earlier stages keep their numbers
    assert _stage() == 1 and _stage(axis=True, freeze=F2) == 2
    assert _stage(mask=True, plane=True, axis=True, depth=True, freeze=F3) == 3 and _stage(mask=True, freeze=F2) == 3
    assert _stage(mask=True, axis=True, freeze=F2 + ["roi_heads.axis_head"]) == 3
    bad = [dict(mask=True, plane=True, axis=True, depth=True, freeze=[f for f in F3 if f != "roi_heads.plane_head"]),  # mask + plane jointly
           dict(mask=True, plane=True, axis=True, depth=True, freeze=["backbone"]),  # step3_plane.yaml's own flags
           dict(mask=True, plane=True, axis=True, depth=True, freeze=REF_STEP3),  # ... and its own FREEZE
           dict(plane=True, depth=True, freeze=F3),  # everything frozen
           dict(plane=True, axis=True, freeze=F2),  # unfrozen axis head
           dict(mask=True, plane=True, depth=True),  # nothing frozen
           dict(plane=True, depth=True, freeze=F2),  # unfrozen depth head
           dict(plane=True, freeze=F2[:3]),  # the detector not frozen
           dict(mask=True, plane=True, axis=True, depth=True, freeze=F4 + ["roi_heads.plane_head"])]  # nothing left to train
    for kw in bad:
        with pytest.raises(NotImplementedError) as e:
            _stage(**kw)
        msg = str(e.value)
        assert "step1_bbox" in msg and "step2_axis" in msg and "step3_mask" in msg and "step3_planehead" in msg and "plane and depth losses" in msg, msg


# ------------------------------------------------------------------------------------------ layout
def test_plane_layer_table_lays_out_the_checkpoint_format():
    from articulation3d_amd.training_head import flat_layout
    from articulation3d_amd.training_plane import plane_layer_table

    table = plane_layer_table()
    lay = flat_layout(**table)
    names = [R.PH + n for n in ("plane_conv1", "plane_conv2", "plane_conv3", "plane_conv4", "plane_fc1")]
    assert list(lay.layers) == names
    assert [lay.layers[n] for n in names] == [(0, 589824, 589824, 256), (590080, 589824, 1179904, 256), (1180160, 589824, 1769984, 256),
                                              (1770240, 589824, 2360064, 256), (2360320, 51380224, 53740544, 1024)]
    assert lay.tail == {"pred_w": (53741568, 3072), "pred_b": (53744640, 3)}
    assert lay.total == 53744644 and lay.total % 4 == 0
    assert lay.segments == [(0, 53744644)]  # one gradient-exchange segment
    assert all(v[0] % 4 == 0 for v in lay.layers.values()) and lay.tail["pred_w"][0] % 4 == 0  # 16-byte loads
    fc = table["layers"][-1]
    assert (fc.rows, fc.cin, fc.k) == (1024, 50176, 1) and [ly.k for ly in table["layers"][:4]] == [3] * 4


def test_fc_column_helpers_round_trip_and_index():
    from articulation3d_amd.training_head import fc_columns_to_chw, fc_columns_to_hwc

    C, S, rows = 5, 3, 4
    w = torch.arange(rows * C * S * S, dtype=torch.float32).reshape(rows, C * S * S)
    hwc = fc_columns_to_hwc(w, C, S)
    assert hwc.shape == w.shape and torch.equal(fc_columns_to_chw(hwc, C, S), w) and torch.equal(fc_columns_to_hwc(fc_columns_to_chw(w, C, S), C, S), w)
    r, c, y, x = 2, 3, 1, 2
    assert hwc[r, (y * S + x) * C + c] == w[r, (c * S + y) * S + x]
    # ... and it is the flattening of an NHWC activation: the same dot product
    act = torch.randn(2, C, S, S)
    assert torch.allclose(act.flatten(1) @ w.t(), act.permute(0, 2, 3, 1).flatten(1) @ hwc.t(), rtol=1e-5, atol=1e-3)


# ------------------------------------------------------------------------------------------ ground truth
def test_malformed_gt_planes_are_refused_before_a_trainer_is_built():
    from articulation3d_amd.modeling import build_model
    from articulation3d_amd.structures import Boxes, Instances
    from articulation3d_amd.training_plane import PlaneTrainer, check_gt_planes

    boxes = torch.tensor([[0.0, 0.0, 5.0, 5.0]])
    check_gt_planes([torch.zeros(1, 3)], [boxes])
    for bad in (torch.zeros(2, 3), torch.zeros(0, 3), torch.zeros(1, 4), torch.zeros(3)):
        with pytest.raises(AssertionError):
            check_gt_planes([bad], [boxes])
    # through the model's training-mode call
    cfg = _cfg()
    cfg.MODEL.DEVICE = "cpu"
    model = build_model(cfg).train()
    assert model._trainer_class() is PlaneTrainer
    inst = Instances((32, 32), gt_boxes=Boxes(boxes), gt_classes=torch.zeros(1, dtype=torch.long), gt_planes=torch.ones(1, 3))
    inst._fields["gt_planes"] = torch.ones(2, 3)  # (Instances itself refuses a field of another length)
    with pytest.raises(AssertionError) as e:
        model([{"image": torch.zeros(3, 32, 32, dtype=torch.uint8), "instances": inst}])
    assert "gt_planes" in str(e.value)
    assert getattr(model, "_trainer", None) is None


# ------------------------------------------------------------------------------------------ the references check themselves
def test_plane_loss_reference_known_answers():
    d = torch.float64
    h = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=d, requires_grad=True)
    w = torch.tensor([[3.0, 0.0], [0.0, 0.0], [4.0, 2.0]], dtype=d)
    b = torch.zeros(3, dtype=d, requires_grad=True)
    gt = torch.tensor([[[0.0, 0.0, 5.0], [0.0, -2.0, 0.0]]], dtype=d)
    img, g = torch.tensor([0, 0, 0]), torch.tensor([0, 1, 2])  # row 2: ground-truth index out of range
    # raw (3, 0, 4) -> (.6, 0, .8) against (0, 0, 1): .8;  raw (0, 0, 2) -> (0, 0, 1) against (0, -1, 0): 2;  row 2: nothing;  3 rows
    loss, raw = R.plane_loss_contract(h, w, b, img, g, gt, loss_weight=1.5)
    assert torch.equal(raw.detach(), torch.tensor([[3.0, 0.0, 4.0], [0.0, 0.0, 2.0], [3.0, 0.0, 6.0]], dtype=d))
    assert abs(loss.item() - 1.5 * 2.8 / 3) < 1e-15
    loss.backward()
    # db by hand (k = 1.5 / 3): row 0 sign (1, 0, -1) through the normalisation at (3, 0, 4), row 1 sign (0, 1, 1) at (0, 0, 2)
    want_db = 1.5 * torch.tensor([1 / 15 + 1 / 125, 1 / 6, -1 / 15 + 4 / 375], dtype=d)
    assert torch.allclose(b.grad, want_db, atol=1e-15)
    assert torch.equal(h.grad[2], torch.zeros(2, dtype=d))
    raw_loss, _ = R.plane_loss_contract(h.detach(), w, b.detach(), img, g, gt, normal_only=False)
    assert abs(raw_loss.item() - 8.0 / 3) < 1e-15  # |3| + |4 - 5| and |2| + |2|
    # plane_rcnn_loss on the same rows; no rows: pred.sum() * 0
    pred = torch.tensor([[0.6, 0.0, 0.8], [0.0, 0.0, 1.0]], dtype=d)
    assert abs(R.plane_rcnn_loss_ref(pred, gt[0], 1.0).item() - 1.4) < 1e-15
    assert R.plane_rcnn_loss_ref(pred[:0], gt[0, :0]).item() == 0.0 and R.plane_loss_contract(h[:0], w, b, img[:0], g[:0], gt)[0].item() == 0.0
    # a raw vector below the eps clamp: the prediction is raw / 1e-12 and only that term passes backward
    z = torch.zeros(1, 2, dtype=d, requires_grad=True)
    bz = torch.zeros(3, dtype=d, requires_grad=True)
    lz, _ = R.plane_loss_contract(z, w, bz, img[:1], g[:1], gt)
    lz.backward()
    assert abs(lz.item() - 1.0) < 1e-15 and torch.equal(bz.grad, torch.tensor([0.0, 0.0, -1e12], dtype=d))


def test_head_reference_and_kernel_contract_agree():
    """The reference head on pooled rows (CHW columns) and the kernel's contract on the FC's activation are the same loss."""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    P = {R.PH + "plane_conv1.weight": rn(2, 2, 3, 3), R.PH + "plane_conv1.bias": rn(2), R.PH + "plane_fc1.weight": rn(4, 18),
         R.PH + "plane_fc1.bias": rn(4), R.PH + "param_pred.weight": rn(3, 4), R.PH + "param_pred.bias": rn(3)}
    x, gt = rn(5, 2, 3, 3), rn(1, 5, 3)
    want = R.plane_loss_ref(x, P, gt[0], loss_weight=0.7)
    y = F.relu(F.conv2d(x, P[R.PH + "plane_conv1.weight"], P[R.PH + "plane_conv1.bias"], padding=1))
    h = F.relu(F.linear(y.flatten(1), P[R.PH + "plane_fc1.weight"], P[R.PH + "plane_fc1.bias"]))
    got, raw = R.plane_loss_contract(h, P[R.PH + "param_pred.weight"], P[R.PH + "param_pred.bias"], torch.zeros(5, dtype=torch.long),
                                     torch.arange(5), gt, loss_weight=0.7)
    assert abs(got.item() - want.item()) < 1e-14 and torch.allclose(raw, R.plane_head_raw(x, P), atol=1e-14)
    assert torch.allclose(R.plane_head_forward(x, P).norm(dim=1), torch.ones(5, dtype=torch.float64), atol=1e-14)
    # the gates argument: its own gates change nothing; the opposite gates matter only within GATE_MARGIN of a kink (none here)
    ties = []
    assert torch.equal(R.plane_head_raw(x, P, [y > 0], ties), R.plane_head_raw(x, P)) and ties == [0]
    assert torch.equal(R.plane_head_raw(x, P, [y <= 0]), R.plane_head_raw(x, P))
    Pk = dict(P)
    Pk[R.PH + "plane_conv1.bias"] = P[R.PH + "plane_conv1.bias"] - torch.tensor([y[0, 0, 0, 0].item() - 3e-6, 0.0], dtype=torch.float64)
    ties = []  # one pre-activation moved to 3e-6: the given gate decides whether it passes
    on, off = R.plane_head_raw(x, Pk, [torch.ones_like(y, dtype=torch.bool)], ties), R.plane_head_raw(x, Pk, [torch.zeros_like(y, dtype=torch.bool)])
    assert ties[0] >= 1 and torch.equal(on, R.plane_head_raw(x, Pk)) and (on - off).abs().max() < 1e-4


def test_loss_case_keeps_every_ordinary_residual_away_from_zero():
    """The shared case of the GPU test: outside the crafted rows no residual is near 0, so a wrong sign cannot hide behind a tolerance
    and fp32 rounding cannot flip an honest one; the crafted rows are what they claim to be."""
    for K in (1024, 256):
        for normal_only in (True, False):
            h, w, b, ri, rg, gt = R.loss_case(K=K)
            live = 23
            loss, dh, dw, db, raw, res = R.loss_case_ref(h, w, b, ri, rg, gt, live, normal_only=normal_only)
            ordinary = [r for r in range(live) if r not in R.CRAFTED.values()]
            assert res[ordinary].abs().min().item() > R.MIN_RESIDUAL, (K, normal_only, res[ordinary].abs().min().item())
            c = R.CRAFTED
            assert torch.equal(raw[c["eps"]], torch.zeros(3, dtype=torch.float64)) and torch.equal(raw[c["equal"]], torch.tensor([0.0, 3.0, 4.0], dtype=torch.float64))
            assert bool(res[c["bad_gt"]].isnan().all()) and bool(res[c["bad_img"]].isnan().all())
            assert bool((dh[c["bad_gt"]] == 0).all()) and bool((dh[c["bad_img"]] == 0).all())
            if normal_only:
                assert res[c["equal"]].tolist() == [0.0, 0.0, 0.0] and res[c["mirrored"]][:2].tolist() == [0.0, 0.0]
                assert abs(res[c["mirrored"]][2].item() - 1.6) < 1e-15 and bool((dh[c["equal"]] == 0).all())
                assert abs(res[c["zero_gt"]].norm().item() - 1.0) < 1e-12  # the unit prediction against a zero vector
            assert bool(torch.isfinite(loss)) and bool(h[live:].isnan().all())
