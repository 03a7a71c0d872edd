"""Host-side checks of the stage-3 (configs/step3_mask.yaml, the mask share of the reference's step3_plane.yaml) training path: the
config and the training-mode routing, the refusal of polygon ground truth, the deconv's packed layout, and the float64 references that
tests/test_gpu_mask_training.py holds the kernels to (tests/mask_train_ref.py)."""
import os
import types

import pytest
import torch
import torch.nn.functional as F
import yaml

import mask_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F2 = ["backbone", "proposal_generator", "roi_heads.box_head", "roi_heads.box_predictor"]
F3 = F2 + ["roi_heads.axis_head", "roi_heads.plane_head", "depth_head"]


def _cfg():
    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults

    cfg = get_cfg()
    get_planercnn_cfg_defaults(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "step3_mask.yaml"))
    return cfg


def _stage(mask=False, plane=False, axis=False, depth=False, freeze=()):
    from articulation3d_amd.modeling.meta_arch import PlaneRCNN

    m = types.SimpleNamespace(depth_head_on=depth, roi_heads=types.SimpleNamespace(mask_on=mask, plane_on=plane, axis_on=axis),
                              _freeze=list(freeze), STAGE2_FREEZE=PlaneRCNN.STAGE2_FREEZE)
    return PlaneRCNN.training_stage(m)


# ------------------------------------------------------------------------------------------ config and routing
def test_step3_mask_config_is_step3_plane_with_two_more_frozen_heads_and_bitmasks():
    cfg = _cfg()
    assert cfg.INPUT.MASK_FORMAT == "bitmask" and cfg.MODEL.MASK_ON and cfg.MODEL.PLANE_ON and cfg.MODEL.AXIS_ON and cfg.MODEL.DEPTH_ON
    assert list(cfg.MODEL.FREEZE) == F3
    with open(os.path.join(ROOT, "configs", "step3_mask.yaml")) as f:
        raw = yaml.safe_load(f)
    assert raw["MODEL"]["ROI_MASK_HEAD"] == dict(NAME="MaskRCNNConvUpsampleHead", NUM_CONV=4, POOLER_RESOLUTION=14, POOLER_SAMPLING_RATIO=2,
                                                 POOLER_TYPE="ROIAlign", CLS_AGNOSTIC_MASK=True)
    assert raw["SOLVER"]["IMS_PER_BATCH"] == 8 and raw["MODEL"]["ROI_PLANE_HEAD"]["NORMAL_ONLY"] is True


def test_step3_mask_config_routes_to_stage_three_and_only_the_mask_head_trains():
    from articulation3d_amd.modeling import build_model

    cfg = _cfg()
    cfg.MODEL.DEVICE = "cpu"
    model = build_model(cfg)
    assert model.training_stage() == 3
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert trainable and all(n.startswith(R.MH) for n in trainable)
    assert {n.split(".")[2] for n in trainable} == {"mask_fcn1", "mask_fcn2", "mask_fcn3", "mask_fcn4", "deconv", "predictor"}


def test_stage_three_routing_rules():
    assert _stage(mask=True, plane=True, axis=True, depth=True, freeze=F3) == 3  # configs/step3_mask.yaml
    assert _stage(mask=True, freeze=F2) == 3  # every other head off
    assert _stage(mask=True, axis=True, freeze=F2 + ["roi_heads.axis_head"]) == 3
    assert _stage() == 1 and _stage(axis=True, freeze=F2) == 2  # the earlier stages keep their numbers
    bad = [dict(mask=True, plane=True, axis=True, depth=True, freeze=F3 + ["roi_heads.mask_head"]),  # the mask head frozen
           dict(mask=True, plane=True, axis=True, depth=True, freeze=[f for f in F3 if f != "roi_heads.plane_head"]),  # unfrozen plane head
           dict(mask=True, plane=True, axis=True, depth=True, freeze=[f for f in F3 if f != "depth_head"]),  # unfrozen depth head
           dict(mask=True, axis=True, freeze=F2),  # unfrozen axis head
           dict(mask=True, plane=True, axis=True, depth=True, freeze=F3[1:]),  # the detector not frozen: backbone
           dict(mask=True, freeze=F2[:3]),  # ... box predictor
           dict(mask=True, plane=True, axis=True, depth=True, freeze=["backbone"]),  # step3_plane.yaml's own flags
           dict(plane=True, depth=True, freeze=F3)]  # no mask head at all
    for kw in bad:
        with pytest.raises(NotImplementedError) as e:
            _stage(**kw)
        msg = str(e.value)
        assert "step1_bbox" in msg and "step2_axis" in msg and "step3_mask" in msg and "plane and depth losses" in msg, msg


def test_polygon_ground_truth_is_refused_with_the_documented_reason():
    from articulation3d_amd.modeling import build_model
    from articulation3d_amd.structures import BitMasks, Boxes, Instances, gt_bitmasks

    poly = types.SimpleNamespace(polygons=[[torch.tensor([0.0, 0.0, 5.0, 0.0, 5.0, 5.0])]])
    with pytest.raises(NotImplementedError) as e:
        gt_bitmasks(poly)
    assert "INPUT.MASK_FORMAT: bitmask" in str(e.value) and "pycocotools" in str(e.value) and "proposal box" in str(e.value)
    t = torch.zeros(2, 8, 8, dtype=torch.bool)
    assert gt_bitmasks(t) is t and gt_bitmasks(BitMasks(t)) is t
    with pytest.raises(TypeError):
        gt_bitmasks(torch.zeros(2, 8, 8))  # float masks are not bitmasks
    bm = BitMasks(torch.ones(3, 4, 5, dtype=torch.uint8))
    assert len(bm) == 3 and len(bm[1]) == 1 and len(bm[torch.tensor([0, 2])]) == 2 and bm.image_size == (4, 5)
    assert bm.to("cpu").tensor.dtype == torch.uint8
    # through the model's training-mode call: refused before any trainer is built or anything runs
    cfg = _cfg()
    cfg.MODEL.DEVICE = "cpu"
    model = build_model(cfg).train()

    class Poly(list):  # (Instances fields need a length)
        polygons = [[0.0, 0.0, 5.0, 0.0, 5.0, 5.0]]

    inst = Instances((32, 32), gt_boxes=Boxes(torch.tensor([[0.0, 0.0, 5.0, 5.0]])), gt_classes=torch.zeros(1, dtype=torch.long), gt_masks=Poly([0]))
    with pytest.raises(NotImplementedError) as e:
        model([{"image": torch.zeros(3, 32, 32, dtype=torch.uint8), "instances": inst}])
    assert "INPUT.MASK_FORMAT: bitmask" in str(e.value)
    assert getattr(model, "_trainer", None) is None


# ------------------------------------------------------------------------------------------ deconv layout
def test_deconv_layout_round_trip_for_weights_and_gradients():
    from articulation3d_amd import ops
    from articulation3d_amd.training_mask import deconv_bias_fold, deconv_from_packed, deconv_to_packed

    torch.manual_seed(0)
    Cin, Cout, Rn, P = 6, 5, 3, 4
    w = torch.randn(Cin, Cout, 2, 2, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Cout, dtype=torch.float64, requires_grad=True)
    assert torch.equal(deconv_from_packed(deconv_to_packed(w.detach())), w.detach())
    p = deconv_to_packed(w.detach())
    assert torch.equal(deconv_to_packed(deconv_from_packed(p)), p)
    assert torch.equal(p.float(), ops.pack_deconv2x2(w.detach(), b.detach(), device="cpu").w)  # the inference pack's row order
    # the 1x1 layer in (dy, dx, co) order IS the deconv, unshuffled -- forward, weight gradient and bias gradient
    x = torch.randn(Rn, Cin, P, P, dtype=torch.float64)
    y = F.conv_transpose2d(x, w, b, stride=2)
    pk = deconv_to_packed(w.detach()).clone().requires_grad_(True)
    b4 = b.detach().repeat(4).requires_grad_(True)
    yu = F.conv2d(x, pk[:, :, None, None], b4).permute(0, 2, 3, 1)
    assert torch.allclose(R.unshuffle(y), yu, atol=1e-12) and torch.equal(R.shuffle(R.unshuffle(y)), y)
    gy = torch.randn_like(y)
    y.backward(gy)
    yu.backward(R.unshuffle(gy))
    assert torch.allclose(deconv_from_packed(pk.grad), w.grad, atol=1e-12)
    assert torch.allclose(deconv_bias_fold(b4.grad), b.grad, atol=1e-12)


# ------------------------------------------------------------------------------------------ the target reference checks itself
@pytest.mark.parametrize("hw", [(480, 640), (96, 128)])
def test_fp32_and_float64_targets_agree_outside_the_tie_margin(oracle, hw):
    masks, boxes, gt = R.target_case(hw[0], hw[1], seed=5)
    assert boxes.shape == (2, 120, 4)
    v64 = R.target_case_values(oracle, masks, boxes, gt, torch.float64)
    v32 = R.target_case_values(oracle, masks, boxes, gt, torch.float32)
    err = (v32.double() - v64).abs().max().item()
    print("max |fp32 - float64| of the ROIAlign values:", err)
    assert err < R.TIE_MARGIN  # the margin sits above the reference's own fp32 error
    R.check_targets(R.targets_from_values(v32), v64)
    # known answers: boxes without area give nothing, the rectangle's own box is all ones inside, the whole-image box has the 18 x 23 grid
    t = R.targets_from_values(v64).view(2, 120, 28, 28)
    assert not t[:, 2].any() and not t[:, 3].any()
    assert bool(t[:, 0, 1:-1, 1:-1].all())
    assert 0 < int(t[:, 1].sum()) < t[:, 1].numel()
    # ... and the slow pure-python statement of the operator agrees on one small box
    one = boxes[1, 6:7]
    flat = (masks[1] != 0).float()[:, None]
    py = oracle.roi_align_py(flat, torch.cat((gt[1, 6:7].float()[:, None], one), 1), 28, 1.0, 0, True)[:, 0]
    assert (py.double() - v64.view(2, 120, 28, 28)[1, 6]).abs().max() < 1e-5


def test_mask_loss_reference_known_answers():
    P = {R.MH + "deconv.weight": torch.zeros(2, 2, 2, 2, dtype=torch.float64), R.MH + "deconv.bias": torch.tensor([1.0, 2.0], dtype=torch.float64),
         R.MH + "predictor.weight": torch.tensor([[[[1.0]], [[-1.0]]]], dtype=torch.float64), R.MH + "predictor.bias": torch.tensor([3.0], dtype=torch.float64)}
    x = torch.zeros(1, 2, 1, 1, dtype=torch.float64)
    z = R.mask_head_logits(x, P)
    assert z.shape == (1, 2, 2) and torch.equal(z, torch.full((1, 2, 2), 2.0, dtype=torch.float64))  # 1 - 2 + 3
    t = torch.tensor([[[1, 0], [0, 1]]], dtype=torch.uint8)
    want = 0.5 * (torch.log1p(torch.exp(torch.tensor(-2.0, dtype=torch.float64))) + (2.0 + torch.log1p(torch.exp(torch.tensor(-2.0, dtype=torch.float64)))))
    assert abs(R.mask_loss_ref(x, P, t).item() - want.item()) < 1e-15
    assert R.mask_loss_ref(x[:0], P, t[:0]).item() == 0.0
