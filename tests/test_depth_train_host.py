"""Host-side checks of the stage-5 (configs/step3_depth.yaml, the depth share of the reference's step3_plane.yaml) training path: the
config and the training-mode routing, the flat layout of the depth head, the refusal of malformed depth maps, the solver's second
weight decay, and the float64 references that tests/test_gpu_depth_training.py holds the kernels and the step to
(tests/depth_train_ref.py) against torch's own modules."""
import os
import types

import pytest
import torch
import yaml

import depth_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F2 = ["backbone", "proposal_generator", "roi_heads.box_head", "roi_heads.box_predictor"]
REF_STEP3 = F2 + ["roi_heads.axis_head"]  # MODEL.FREEZE of the reference's step3_plane.yaml
F5 = REF_STEP3 + ["roi_heads.mask_head", "roi_heads.plane_head"]
F4 = REF_STEP3 + ["roi_heads.mask_head", "depth_head"]  # configs/step3_planehead.yaml
F3 = F2 + ["roi_heads.axis_head", "roi_heads.plane_head", "depth_head"]  # configs/step3_mask.yaml


def _cfg():
    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults

    cfg = get_cfg()
    get_planercnn_cfg_defaults(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "step3_depth.yaml"))
    return cfg


def _stage(mask=False, plane=False, axis=False, depth=False, freeze=()):
    from articulation3d_amd.modeling.meta_arch import PlaneRCNN

    m = types.SimpleNamespace(depth_head_on=depth, roi_heads=types.SimpleNamespace(mask_on=mask, plane_on=plane, axis_on=axis),
                              _freeze=list(freeze), STAGE2_FREEZE=PlaneRCNN.STAGE2_FREEZE)
    return PlaneRCNN.training_stage(m)


@pytest.fixture(scope="module")
def cpu_model():
    from articulation3d_amd.modeling import build_model

    cfg = _cfg()
    cfg.MODEL.DEVICE = "cpu"
    return build_model(cfg)


# ------------------------------------------------------------------------------------------ config and routing
def test_step3_depth_config_is_step3_plane_with_the_two_roi_heads_frozen():
    cfg = _cfg()
    assert cfg.MODEL.MASK_ON and cfg.MODEL.PLANE_ON and cfg.MODEL.AXIS_ON and cfg.MODEL.DEPTH_ON
    assert list(cfg.MODEL.FREEZE) == REF_STEP3 + ["roi_heads.mask_head", "roi_heads.plane_head"] == F5
    assert cfg.SOLVER.WEIGHT_DECAY == 1e-4 and cfg.SOLVER.WEIGHT_DECAY_NORM == 0.0
    with open(os.path.join(ROOT, "configs", "step3_depth.yaml")) as f:
        raw = yaml.safe_load(f)
    with open(os.path.join(ROOT, "configs", "step3_planehead.yaml")) as f:
        plane = yaml.safe_load(f)
    assert raw["MODEL"]["WEIGHTS"] == "" and raw["SOLVER"]["IMS_PER_BATCH"] == 8
    raw["MODEL"].pop("FREEZE"), plane["MODEL"].pop("FREEZE")
    assert raw == plane  # (both are step3_plane.yaml's keys and values but for the FREEZE list)


def test_step3_depth_config_routes_to_stage_five_and_only_the_depth_head_trains(cpu_model):
    from articulation3d_amd.modeling.meta_arch import STAGE_TRAINER
    from articulation3d_amd.training_depth import DepthTrainer

    model = cpu_model
    assert model.training_stage() == 5 and STAGE_TRAINER[5] == ("..training_depth", "DepthTrainer") and model._trainer_class() is DepthTrainer
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert trainable and all(n.startswith(R.DH) for n in trainable)
    assert sum(p.numel() for p in model.depth_head.parameters()) == R.NUM_PARAMS
    # the module-level call still has no training path, and says where the training path is
    model.depth_head.train()
    try:
        with pytest.raises(NotImplementedError) as e:
            model.depth_head({})
        assert "DepthTrainer" in str(e.value)
    finally:
        model.depth_head.eval()


def test_stage_five_routing_rules():
    assert _stage(mask=True, plane=True, axis=True, depth=True, freeze=F5) == 5  # configs/step3_depth.yaml
    assert _stage(depth=True, freeze=F2) == 5  # every other head off
    assert _stage(plane=True, depth=True, freeze=F2 + ["roi_heads.plane_head"]) == 5  # depth + a frozen plane head
    assert _stage(axis=True, depth=True, freeze=REF_STEP3) == 5
    # the earlier stages keep their numbers
    assert _stage() == 1 and _stage(axis=True, freeze=F2) == 2
    assert _stage(mask=True, plane=True, axis=True, depth=True, freeze=F3) == 3 and _stage(mask=True, freeze=F2) == 3
    assert _stage(mask=True, plane=True, axis=True, depth=True, freeze=F4) == 4 and _stage(plane=True, freeze=F2) == 4
    bad = [dict(mask=True, plane=True, axis=True, depth=True, freeze=[f for f in F5 if f != "roi_heads.plane_head"]),  # plane + depth jointly
           dict(mask=True, plane=True, axis=True, depth=True, freeze=[f for f in F5 if f != "roi_heads.mask_head"]),  # mask + depth jointly
           dict(mask=True, plane=True, axis=True, depth=True, freeze=["backbone"]),  # step3_plane.yaml's own flags
           dict(mask=True, plane=True, axis=True, depth=True, freeze=REF_STEP3),  # ... and its own FREEZE
           dict(mask=True, plane=True, axis=True, depth=True, freeze=F5 + ["depth_head"]),  # nothing left to train
           dict(depth=True, freeze=F2 + ["depth_head"]),
           dict(axis=True, depth=True, freeze=F2),  # unfrozen axis head
           dict(plane=True, depth=True, freeze=F2),  # unfrozen plane head
           dict(depth=True),  # nothing frozen
           dict(depth=True, freeze=F2[:3]),  # the detector not frozen
           dict(mask=True, plane=True, axis=True, depth=True, freeze=F5[1:])]
    for kw in bad:
        with pytest.raises(NotImplementedError) as e:
            _stage(**kw)
        msg = str(e.value)
        assert all(s in msg for s in ("step1_bbox", "step2_axis", "step3_mask", "step3_planehead", "step3_depth", "plane and depth losses")), msg


# ------------------------------------------------------------------------------------------ layout
def test_depth_layer_table_lays_out_the_checkpoint_format(cpu_model):
    from articulation3d_amd.training_depth import BLOCKS, depth_layer_table, norm_range
    from articulation3d_amd.training_head import flat_layout

    table = depth_layer_table()
    lay = flat_layout(**table)
    sd = {k: v for k, v in cpu_model.state_dict().items() if k.startswith(R.DH)}
    params = {k for k, _ in cpu_model.named_parameters() if k.startswith(R.DH)}
    # every trainable entry of the module, under its name, with its size
    sizes = {}
    for ly in table["layers"]:
        assert ly.k == 3 and (ly.stride, ly.pad) == (1, 1)
        assert tuple(sd[ly.name + ".weight"].shape) == (ly.rows, ly.cin, 3, 3) and tuple(sd[ly.name + ".bias"].shape) == (ly.rows,)
        _, nw, _, nb = lay.layers[ly.name]
        sizes[ly.name + ".weight"], sizes[ly.name + ".bias"] = nw, nb
    sizes[R.DH + "depth_pred.weight"], sizes[R.DH + "depth_pred.bias"] = lay.tail["pred_w"][1], lay.tail["pred_b"][1]
    for k, (_, n) in lay.tail.items():
        if k.startswith(R.DH):
            sizes[k] = n
    assert set(sizes) == params and all(sd[k].numel() == n for k, n in sizes.items())
    assert sum(sizes.values()) == R.NUM_PARAMS == lay.total - lay.tail["pad"][1]
    assert [b for b in BLOCKS] == R.BLOCKS and [BLOCKS[b][:2] for b in BLOCKS] == [R.entries(b)[:2] for b in R.BLOCKS]
    # the norm parameters: one 4-aligned tail range; everything in front of it, padding included, is the other SGD range
    begin, end = norm_range(lay)
    assert (begin, end) == (2656004, 2658436) and begin % 4 == 0 and end == lay.total and lay.total % 4 == 0
    norm_keys = [k for k in lay.tail if k.startswith(R.DH)]
    assert len(norm_keys) == 20 and all(".1." in k or ".2." in k for k in norm_keys)
    assert all(begin <= lay.tail[k][0] and lay.tail[k][0] + lay.tail[k][1] <= end and lay.tail[k][0] % 4 == 0 for k in norm_keys)
    assert all(o + nw <= begin and ob + nb <= begin and o % 4 == 0 for o, nw, ob, nb in lay.layers.values())
    assert lay.tail["pred_w"] == (2655424, 576) and lay.tail["pred_b"] == (2656000, 1) and lay.tail["pad"] == (2656001, 3)
    assert lay.segments == [(0, lay.total)]  # one gradient-exchange segment


def test_solver_carries_the_norm_weight_decay():
    from articulation3d_amd.engine import FlatSGD, solver_from_cfg
    from articulation3d_amd.training import SolverCfg

    s = solver_from_cfg(_cfg())
    assert s.weight_decay == 1e-4 and s.weight_decay_norm == 0.0 and SolverCfg().weight_decay_norm == 0.0
    # the optimiser reports one group per decay the trainer applies: two for the depth stage, one for every other
    one = FlatSGD(types.SimpleNamespace(iter=0, s=s))
    two = FlatSGD(types.SimpleNamespace(iter=0, s=s, weight_decays=[s.weight_decay, s.weight_decay_norm]))
    assert [g["weight_decay"] for g in one.param_groups] == [1e-4] and [g["weight_decay"] for g in two.param_groups] == [1e-4, 0.0]
    assert all(g["momentum"] == 0.9 for g in two.param_groups)


# ------------------------------------------------------------------------------------------ ground truth
def test_malformed_depth_maps_are_refused_before_a_trainer_is_built(cpu_model):
    from articulation3d_amd.structures import Boxes, Instances
    from articulation3d_amd.training_depth import DepthTrainer, check_gt_depth

    assert check_gt_depth(torch.zeros(2, 32, 64), (32, 64)).shape == (2, 32, 64)
    assert check_gt_depth([torch.zeros(32, 64, dtype=torch.float64)] * 3, (32, 64)).dtype == torch.float32
    for bad in (torch.zeros(2, 32, 32), torch.zeros(32, 64), torch.zeros(2, 1, 32, 64), [torch.zeros(32, 64), torch.zeros(16, 64)],
                [torch.zeros(1, 32, 64)], []):
        with pytest.raises(AssertionError):
            check_gt_depth(bad, (32, 64))
    # through the model's training-mode call
    model = cpu_model
    model.train()
    try:
        inst = Instances((32, 32), gt_boxes=Boxes(torch.tensor([[0.0, 0.0, 5.0, 5.0]])), gt_classes=torch.zeros(1, dtype=torch.long))
        x = {"image": torch.zeros(3, 32, 32, dtype=torch.uint8), "instances": inst}
        for depth in (torch.zeros(16, 32), torch.zeros(1, 32, 32), None):
            with pytest.raises(AssertionError) as e:
                model([dict(x, depth=depth) if depth is not None else x])
            assert "depth" in str(e.value)
        assert getattr(model, "_trainer", None) is None
        assert DepthTrainer.batch_extras([dict(x, depth=torch.ones(32, 32))])[0].shape == (1, 32, 32)
    finally:
        model.eval()


# ------------------------------------------------------------------------------------------ the references check themselves
def test_loss_reference_known_answers():
    d = torch.tensor([[[1.0, 3.0]]], dtype=torch.float64, requires_grad=True)  # upsampled: a 2 x 4 map with rows (1, 1.5, 2.5, 3)
    up = R.upsample2(d.detach())
    assert torch.equal(up, torch.tensor([[[1.0, 1.5, 2.5, 3.0]] * 2], dtype=torch.float64))
    gt = torch.tensor([[[2.0, 1.5, 0.0, 1e-4], [0.5, 0.0, 4.5, 3.0]]], dtype=torch.float64)
    # valid: (0,0) |1-2|, (0,1) tie, (1,0) |1-.5|, (1,2) |2.5-4.5|, (1,3) tie: 5 pixels, sum 3.5
    loss = R.depth_loss_ref(d, gt, 0.75)
    assert abs(loss.item() - 0.75 * 3.5 / 5) < 1e-15
    loss.backward()
    # signs: -1 at (0,0) [weight 1 on d0], +1 at (1,0) [d0], -1 at (1,2) [0.25 d0, 0.75 d1]; the ties give nothing
    assert torch.allclose(d.grad, 0.75 / 5 * torch.tensor([[[-1.0 + 1.0 - 0.25, -0.75]]], dtype=torch.float64), atol=1e-15)
    z = torch.zeros(1, 2, 3, dtype=torch.float64, requires_grad=True)
    lz = R.depth_loss_ref(z, torch.zeros(1, 4, 6, dtype=torch.float64))
    lz.backward()
    assert lz.item() == 0.0 and bool((z.grad == 0).all())  # everything masked out


def test_loss_cases_keep_every_unmasked_residual_away_from_zero():
    for B, h, w in ((2, 5, 7), (1, 1, 1), (1, 24, 32)):
        d, gt = R.loss_case(B, h, w)
        _, grad, res = R.loss_case_ref(d, gt, 0.75)
        ties = int((res == 0).sum())
        assert ties == (9 - int((gt[0, 1:4, 1:4] != 2.0).sum()) if h >= 3 else 0)
        assert res[res != 0].abs().min().item() > R.MIN_RESIDUAL * 0.99 if res.numel() > ties else True
        if h >= 3:
            assert 0.25 < float((gt == 0).float().mean()) < 0.42 and int((gt == R.VALID).sum()) > 0
            assert bool((gt[(gt != 0) & (gt != R.VALID)] > 10 * R.VALID).all()) and bool(grad.abs().sum() > 0)


def test_bn_reference_is_torchs_module_and_the_case_is_twenty_sigmas_off():
    z, gamma, beta, rm, rv, dy = R.bn_case((2, 5, 7, 64))
    r = R.bn_ref(z, gamma, beta, rm, rv, True, dy)
    assert bool(((r["mean"].abs() / r["var"].sqrt()) > 15).all())
    bn = torch.nn.BatchNorm2d(64, eps=0.001, momentum=0.01).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    y = torch.nn.functional.leaky_relu(bn(z.double().permute(0, 3, 1, 2).contiguous()))
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-14)
    assert close(y.detach().permute(0, 2, 3, 1), r["y"]) and close(bn.running_mean, r["running_mean"]) and close(bn.running_var, r["running_var"])
    N = 70
    want_rv = 0.99 * rv.double() + 0.01 * r["var"] * N / (N - 1)  # the running variance takes the unbiased estimate
    assert torch.allclose(r["running_var"], want_rv, rtol=1e-13) and int(bn.num_batches_tracked) == 1
    assert r["dbeta"].shape == (64,) and r["dz"].shape == z.shape and float(r["dz"].sum((0, 1, 2)).abs().max()) < 1e-10  # dz sums to 0 per channel


def test_decoder_reference_agrees_with_the_packages_modules_in_train_mode():
    """tests/depth_train_ref.decoder_pred against model.depth_head's own nn.Sequential blocks (real torch modules), float64, training
    mode: predictions, loss, every gradient, the running buffers; and its gates argument."""
    import copy

    import torch.nn.functional as F
    from articulation3d_amd.modeling.depth_head import PlaneRCNNDepthHead

    torch.manual_seed(3)
    dh = PlaneRCNNDepthHead(_cfg()).double().train()
    with torch.no_grad():
        for n, p in dh.named_parameters():
            if p.dim() == 1:
                p.add_(0.3 * torch.randn_like(p))  # (norm weights and every bias away from their 1 / 0 initial values)
    mod = copy.deepcopy(dh)
    feats = {k: v.double() for k, v in R.random_pyramid(2, 32, 96, seed=4).items()}  # p5 1 x 3, p6 1 x 2: deconv1's 2 x 4 is resized to 1 x 3
    x = mod.deconv1(mod.conv1(feats["p6"]))
    assert tuple(x.shape[-2:]) == (2, 4)
    x = F.interpolate(x, size=feats["p5"].shape[-2:], mode="bilinear", align_corners=False)
    for k, lvl in ((2, "p5"), (3, "p4"), (4, "p3"), (5, "p2")):
        x = getattr(mod, f"deconv{k}")(torch.cat([getattr(mod, f"conv{k}")(feats[lvl]), x], dim=1))
    x = mod.depth_pred(x)
    pred = F.interpolate(x, size=(32, 96), mode="bilinear", align_corners=False).view(-1, 32, 96)
    gt = R.craft_gt(pred).double()
    assert 0.3 < float((gt > R.VALID).double().mean()) < 0.9
    want = 0.75 * R.l1_loss_mask(pred, gt, (gt > 1e-4).double())
    want.backward()
    P = {R.DH + k: v.detach().clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in dh.state_dict().items()}
    running = {k: v for k, v in P.items() if "running" in k}
    keep = {}
    got = R.decoder_loss_ref(feats, P, gt, 0.75, running=running, keep=keep)
    got.backward()
    assert abs(got.item() - want.item()) < 1e-13 * abs(want.item())
    assert torch.allclose(R.upsample2(R.decoder_pred(feats, P)), pred, rtol=0, atol=1e-12)
    names = {R.DH + n for n, _ in mod.named_parameters()}
    front = {R.entries(b)[0][len(R.DH):] + ".bias" for b in R.BLOCKS}
    assert names == {k for k, v in P.items() if v.requires_grad} and sum(P[k].numel() for k in names) == R.NUM_PARAMS
    for n, p in mod.named_parameters():
        g = P[R.DH + n].grad
        if n in front:
            # a conv bias in front of a training-mode norm: zero gradient in exact arithmetic
            dz = keep[n.split(".")[0]][0].grad
            bound = 1e-12 * dz.abs().sum((0, 2, 3))  # (per channel; a dead channel has 0 against 0)
            assert bool((g.abs() <= bound).all()) and bool((p.grad.abs() <= bound).all()), n
        else:
            assert torch.allclose(g, p.grad, rtol=1e-9, atol=1e-14 * float(p.grad.abs().max()) + 1e-300), n
    for k, v in mod.state_dict().items():
        if "running" in k:
            assert torch.allclose(running[R.DH + k], v, rtol=1e-13, atol=0), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1
    # the gates argument: its own gates change nothing; the opposite gates matter only within GATE_MARGIN of a kink (none here)
    with torch.no_grad():
        Pd = {k: v.detach() for k, v in P.items()}
        own = {b: keep[b][1].detach() > 0 for b in R.BLOCKS}
        ties = []
        assert torch.equal(R.decoder_pred(feats, Pd, gates=own, ties=ties), R.decoder_pred(feats, Pd)) and len(ties) == 10
        assert sum(ties) <= R.GATE_FRACTION * sum(v.numel() for v in own.values()) + 1, ties
        flipped = R.decoder_pred(feats, Pd, gates={b: ~own[b] for b in R.BLOCKS})
        assert (flipped - R.decoder_pred(feats, Pd)).abs().max() < 1e-3 and (sum(ties) > 0 or torch.equal(flipped, R.decoder_pred(feats, Pd)))
