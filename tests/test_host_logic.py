"""CPU suite, part 2: host-side logic of the product (config, registries, containers, weight packing,
RLE codec, C-ABI surface).  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, make_cfg


def test_config_defaults_and_reference_yaml():
    cfg = make_cfg(0.7, "cpu")
    assert cfg.MODEL.META_ARCHITECTURE == "PlaneRCNN"
    assert cfg.MODEL.RPN.PRE_NMS_TOPK_TEST == 1000 and cfg.MODEL.ROI_HEADS.NUM_CLASSES == 2
    assert cfg.MODEL.ROI_PLANE_HEAD.POOLER_RESOLUTION == 14 and cfg.MODEL.ROI_AXIS_HEAD.FC_DIM == 1024
    cfg.merge_from_list(["MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.25", "MODEL.DEVICE", "cpu"])
    assert cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST == 0.25
    with pytest.raises(KeyError):
        cfg.merge_from_list(["MODEL.NOPE", 1])
    cfg.freeze()
    with pytest.raises(AttributeError):
        cfg.MODEL.DEVICE = "cuda"
    c2 = cfg.clone()
    c2.defrost()
    c2.MODEL.DEVICE = "cuda"
    assert cfg.MODEL.DEVICE == "cpu"
    # the reference's own YAML (its config/config.yaml, stored verbatim as a fixture) loads and agrees with ours on every shared key
    ref = os.path.join(ROOT, "tests", "golden", "reference_config.yaml")
    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults

    r = get_cfg()
    get_planercnn_cfg_defaults(r)
    r.merge_from_file(ref)
    import yaml

    ours = yaml.safe_load(open(os.path.join(ROOT, "configs", "planercnn_inference.yaml")))

    def walk(a, b, path=""):  # every key our inference YAML sets has the reference's value
        for k, v in a.items():
            assert k in b, path + k
            if isinstance(v, dict):
                walk(v, b[k], path + k + ".")
            else:
                assert (list(v) == list(b[k])) if isinstance(v, (list, tuple)) else (v == b[k]), path + k

    walk(ours, r)


def test_registries_resolve_reference_names():
    import articulation3d_amd.modeling  # noqa: F401  (registers everything)
    from articulation3d_amd import registry as R

    assert "PlaneRCNN" in R.META_ARCH_REGISTRY
    assert "PlaneRCNNROIHeads" in R.ROI_HEADS_REGISTRY
    assert "PlaneRCNNConvFCHead" in R.ROI_PLANE_HEAD_REGISTRY and "PlaneRCNNConvFCHead" in R.ROI_AXIS_HEAD_REGISTRY
    assert R.ROI_PLANE_HEAD_REGISTRY.get("PlaneRCNNConvFCHead") is not R.ROI_AXIS_HEAD_REGISTRY.get("PlaneRCNNConvFCHead")
    assert "PlaneRCNNDepthHead" in R.DEPTH_HEAD_REGISTRY
    for reg, name in ((R.BACKBONE_REGISTRY, "build_resnet_fpn_backbone"), (R.PROPOSAL_GENERATOR_REGISTRY, "RPN"),
                      (R.RPN_HEAD_REGISTRY, "StandardRPNHead"), (R.ANCHOR_GENERATOR_REGISTRY, "DefaultAnchorGenerator"),
                      (R.ROI_BOX_HEAD_REGISTRY, "FastRCNNConvFCHead"), (R.ROI_MASK_HEAD_REGISTRY, "MaskRCNNConvUpsampleHead")):
        assert name in reg
    with pytest.raises(KeyError):
        R.META_ARCH_REGISTRY.get("Nope")


def test_state_dict_names_match_checkpoint_format(oracle):
    """`exps/model_final.pth` uses detectron2 names; the oracle's init enumerates them."""
    from articulation3d_amd.modeling import build_model

    model = build_model(make_cfg(0.7, "cpu"))
    ours = {k for k in model.state_dict() if "num_batches_tracked" not in k}
    theirs = set(oracle.init_params(1, calibrate=False))
    assert ours == theirs
    for k in ("backbone.bottom_up.res2.0.conv1.weight", "backbone.fpn_lateral2.weight", "proposal_generator.rpn_head.conv.weight",
              "roi_heads.box_head.fc1.weight", "roi_heads.plane_head.plane_conv1.weight", "roi_heads.axis_head.axis_R_conv1.weight",
              "depth_head.conv1.0.weight", "depth_head.deconv5.2.running_var"):
        assert k in ours
    assert all(not p.requires_grad for p in model.backbone.parameters())  # MODEL.FREEZE honoured
    assert model.backbone.size_divisibility == 32
    shapes = model.backbone.output_shape()
    assert [shapes[f"p{i}"].stride for i in range(2, 7)] == [4, 8, 16, 32, 64] and shapes["p2"].channels == 256


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "articulation3d_amd")
    for dirpath, _d, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), f"{f} imports the oracle"


def test_boxes_instances_imagelist():
    from articulation3d_amd.structures import Boxes, ImageList, Instances, pairwise_iou

    b = Boxes(torch.tensor([[-5.0, 2, 50, 700], [10, 10, 10, 30]]))
    b.clip((480, 640))
    assert b.tensor.tolist() == [[0, 2, 50, 480], [10, 10, 10, 30]]
    assert b.nonempty().tolist() == [True, False] and len(b[b.nonempty()]) == 1
    inst = Instances((480, 640), pred_boxes=b, scores=torch.tensor([0.9, 0.2]))
    assert len(inst) == 2 and inst.has("scores") and len(inst[inst.scores > 0.5]) == 1
    with pytest.raises(AssertionError):
        inst.bad = torch.zeros(3)
    il = ImageList.from_tensors([torch.ones(3, 30, 40), torch.ones(3, 20, 50)], 32)
    assert il.tensor.shape == (2, 3, 32, 64) and il.image_sizes == [(30, 40), (20, 50)] and il.tensor[1, 0, 25, 10] == 0
    iou = pairwise_iou(Boxes(torch.tensor([[0.0, 0, 10, 10]])), Boxes(torch.tensor([[0.0, 0, 10, 10], [5, 5, 15, 15], [20, 20, 30, 30]])))
    np.testing.assert_allclose(iou.numpy(), [[1.0, 25 / 175, 0.0]], rtol=1e-6)
    cat = Instances.cat([inst, inst])
    assert len(cat) == 4


def test_rle_roundtrip_and_known_strings():
    from articulation3d_amd.utils import rle

    assert rle.encode(np.ones((3, 3), np.uint8))["counts"] == "09"
    assert rle.encode(np.zeros((3, 3), np.uint8))["counts"] == "9"
    rng = np.random.default_rng(3)
    for _ in range(10):
        m = (rng.random((37, 53)) > rng.random()).astype(np.uint8)
        assert (rle.decode(rle.encode(m)) == m).all()
    m = np.zeros((480, 640), np.uint8)
    m[100:300, 200:400] = 1
    r = rle.encode(m)
    assert r["size"] == [480, 640] and (rle.decode(r) == m).all()


def test_weight_packing_layouts():
    from articulation3d_amd import ops

    w = torch.randn(6, 32, 3, 3)
    p = ops.pack_conv(w, torch.randn(6), None, 1, 1, device="cpu")
    assert p.cols == 8 and p.w.shape == (8, 288) and p.Kpad == 288
    assert torch.equal(p.w[2, (1 * 3 + 2) * 32 + 5], w[2, 5, 1, 2]) and float(p.w[6:].abs().sum()) == 0
    bn = (torch.rand(6) + 0.5, torch.randn(6), torch.randn(6), torch.rand(6) + 0.5, 1e-3)
    p = ops.pack_conv(w, torch.randn(6), bn, 1, 1, device="cpu")
    np.testing.assert_allclose(p.scale[:6].numpy(), (bn[0] / torch.sqrt(bn[3] + 1e-3)).numpy(), rtol=1e-6)
    ws = torch.randn(64, 3, 7, 7)
    ps = ops.pack_stem(ws, (torch.ones(64), torch.zeros(64), torch.zeros(64), torch.ones(64), 1e-5), device="cpu")
    assert ps.w.shape == (64, 224) and ps.stem
    v = ps.w.view(64, 7, 8, 4)
    assert torch.equal(v[3, 2, 4, 1], ws[3, 1, 2, 4]) and float(v[:, :, 7].abs().sum()) == 0 and float(v[..., 3].abs().sum()) == 0
    wl = torch.randn(5, 2 * 3 * 16)
    pl = ops.pack_linear(wl, None, chw=(16, 2, 3), device="cpu")
    assert torch.equal(pl.w[1].view(2, 3, 16)[1, 2, 7], wl[1].view(16, 2, 3)[7, 1, 2])
    wd = torch.randn(32, 8, 2, 2)
    pd = ops.pack_deconv2x2(wd, torch.randn(8), device="cpu")
    assert pd.cols == 32 and torch.equal(pd.w[(1 * 2 + 0) * 8 + 3, 9], wd[9, 3, 1, 0])
    with pytest.raises(ValueError):
        ops.pack_conv(torch.randn(4, 3, 3, 3), device="cpu")
    assert ops.choose_splitk(124, 1024, 50176) == ops.choose_splitk(3200, 1024, 50176) > 1 and ops.choose_splitk(32000, 1024, 12544) == 1


def test_c_abi_library_exports_every_declared_symbol():
    """The .so loads and exports exactly what include/a3d.h declares (no compute calls without a GPU)."""
    from articulation3d_amd import _lib

    header = open(os.path.join(ROOT, "include", "a3d.h")).read()
    declared = set(re.findall(r"\b(a3d_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    if not os.path.exists(_lib.LIB_PATH):
        from articulation3d_amd import build

        build.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    lib = _lib.lib()
    assert lib.a3d_version() >= 1 and lib.a3d_record_floats(28) == 798
    assert lib.a3d_group_buffers_bytes(10) >= 10 * 1024 * 32
    # argument validation happens before any launch: bad descriptors are refused, not crashed on
    d = _lib.ConvDesc()
    assert lib.a3d_conv2d_nhwc_f32(ctypes.byref(d), None) == -1
    assert lib.a3d_conv_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.a3d_linear_small(None, None, None, None, 4, None, 1024, 3, 3, 0, None) == -1
    # struct layouts agree with the C side (a mismatch would shift every field)
    for sid, cls in _lib.STRUCT_IDS.items():
        assert lib.a3d_struct_size(sid) == ctypes.sizeof(cls), cls.__name__
    # 8 ptrs, 19 ints, pad, m_dev, tune + phase, w_wino, gate, precision + pad, w_wino_x3, w_wino_cm, w_x3, in_amax, in_amax2, y_amax, w_scale + pad,
    # wino_m, io_bf16 + pad, x_h2, x2_h2, dot_w, dot_y, wino_t_off + wino_t_total, w_bf16
    assert ctypes.sizeof(_lib.ConvDesc) == 8 * 8 + 19 * 4 + 4 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from articulation3d_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_ops_refuse_cpu_tensors():
    from articulation3d_amd import ops

    p = ops.pack_conv(torch.randn(4, 32, 1, 1), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv2d(torch.zeros(1, 2, 2, 32), p)


def test_anchor_generator_and_create_instances():
    from articulation3d_amd.modeling import build_model
    from articulation3d_amd.utils.arti_vis import create_instances, get_K_inv_dot_xy_1
    from articulation3d_amd.utils import rle
    from oracle import planercnn_oracle as O

    model = build_model(make_cfg(0.7, "cpu"))
    ca = model.proposal_generator.anchor_generator.cell_anchors
    for l, size in enumerate((32, 64, 128, 256, 512)):
        assert torch.equal(ca[l], O.cell_anchors(size, (0.5, 1.0, 2.0)))
    rays = get_K_inv_dot_xy_1()
    np.testing.assert_allclose(rays.astype(np.float32), O.k_inv_dot_xy1().numpy(), rtol=0, atol=0)
    m = np.zeros((480, 640), np.uint8)
    m[10:20, 30:50] = 1
    preds = [{"score": 0.9, "bbox": [30.0, 10.0, 20.0, 10.0], "category_id": 1, "segmentation": rle.encode(m)},
             {"score": 0.5, "bbox": [1.0, 1.0, 2.0, 2.0], "category_id": 0, "segmentation": rle.encode(m)}]
    inst = create_instances(preds, (480, 640), pred_planes=torch.tensor([[1.0, 2, 3], [4, 5, 6]]),
                            pred_rot_axis=torch.ones(2, 3), pred_tran_axis=torch.ones(2, 2), conf_threshold=0.7)
    assert len(inst) == 1 and inst.pred_boxes.tensor.tolist() == [[30.0, 10.0, 50.0, 20.0]]
    assert inst.pred_masks.shape == (1, 480, 640) and float(inst.pred_masks.sum()) == 200 and inst.pred_planes.tolist() == [[1.0, 2.0, 3.0]]


def test_track_planes_associates_by_iou_and_filters_short_tracks():
    from articulation3d_amd.structures import Boxes, Instances
    from articulation3d_amd.utils.opt_utils import track_planes

    preds = []
    for f in range(14):
        inst = Instances((480, 640))
        boxes, classes = [], []
        if f != 6:  # a one-frame gap is bridged (gap <= 5)
            boxes.append([100.0 + 3 * f, 100.0, 220.0 + 3 * f, 260.0])  # slowly drifting rotation plane
            classes.append(0)
        if f < 5:
            boxes.append([400.0, 300.0, 500.0, 420.0])  # short-lived translation plane: filtered (< 10 frames)
            classes.append(1)
        inst.pred_boxes = Boxes(torch.tensor(boxes).reshape(-1, 4))
        inst.pred_classes = np.asarray(classes, dtype=np.int64)
        preds.append(inst)
    planes = track_planes(preds)
    assert len(planes["rot"]) == 1 and planes["trans"] == []
    t = planes["rot"][0]
    assert sorted(t["ids"]) == [f for f in range(14) if f != 6] and t["latest_frame"] == 13
    # a jump breaks the association -> two short tracks, both filtered
    preds[7].pred_boxes = Boxes(torch.tensor([[300.0, 300.0, 400.0, 400.0]]))
    assert len(track_planes(preds[:9])["rot"]) == 0


def test_checkpoint_loading_is_never_silent(tmp_path):
    """a missing / unsupported MODEL.WEIGHTS raises; only load_weights=False gives random init."""
    import pytest
    import torch

    from articulation3d_amd.utils.arti_vis import load_checkpoint

    m = torch.nn.Linear(4, 2)
    with pytest.raises(FileNotFoundError):
        load_checkpoint(m, str(tmp_path / "model_final.pth"))
    with pytest.raises(ValueError):
        load_checkpoint(m, "detectron2://ImageNetPretrained/MSRA/R-50.pkl")
    pkl = tmp_path / "R-50.pkl"
    pkl.write_bytes(b"x")
    with pytest.raises(ValueError):
        load_checkpoint(m, str(pkl))
    good = tmp_path / "ok.pth"
    torch.save({"model": {"weight": torch.ones(2, 4), "bias": torch.zeros(2)}}, good)
    load_checkpoint(m, str(good))
    assert float(m.weight.sum()) == 8.0
    bad = tmp_path / "partial.pth"
    torch.save({"model": {"weight": torch.ones(2, 4)}}, bad)
    with pytest.raises(RuntimeError):
        load_checkpoint(m, str(bad))


def test_torch_ops_are_registered_without_a_cpu_kernel():
    """north_star: the kernels are PyTorch custom ops.  Schemas exist on import; there is no CPU implementation to fall back to."""
    import pytest
    import torch

    import articulation3d_amd  # noqa: F401
    from articulation3d_amd import torch_ops

    for name in torch_ops.OPS:
        assert hasattr(torch.ops.a3d, name), name
    schema = str(torch.ops.a3d.roi_align_fpn.default._schema)
    assert "Tensor[] feats" in schema and "bool aligned" in schema
    with pytest.raises((NotImplementedError, RuntimeError)) as e:
        torch.ops.a3d.group_nms(torch.zeros(1, 1024, 4), torch.zeros(1, 1024, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0.5)
    assert "CPU" in str(e.value)


def test_release_library_reads_no_environment_variable():
    """the C-ABI library is re-entrant and keeps no global state.  Round 5 moved every A/B switch of the kernels behind
    descriptor fields (a3d_conv_desc.tune, a3d_roialign_desc.serial) or compile-time constants that only a developer build
    (-DA3D_ABLATIONS) may override from the environment: the shipped library must not even import getenv, and the sources may call it
    in one place only (a3d_common.h's a3d_dev_knob, inside #ifdef A3D_ABLATIONS).  The one diagnostic exception is documented in
    include/a3d.h: a3d_last_conv_variant(), a per-THREAD label of the last conv launch."""
    import subprocess

    lib = os.path.join(ROOT, "articulation3d_amd", "liba3d_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    if os.environ.get("A3D_HIPCC_FLAGS", "").find("A3D_ABLATIONS") >= 0:
        pytest.skip("developer build")
    und = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\b(secure_)?getenv\b", und), [l for l in und.splitlines() if "getenv" in l]
    hits = []
    for f in sorted(os.listdir(os.path.join(ROOT, "articulation3d_amd", "csrc"))):
        if f.endswith((".hip", ".h")):
            for i, line in enumerate(open(os.path.join(ROOT, "articulation3d_amd", "csrc", f)), 1):
                if "getenv(" in line:
                    hits.append((f, i))
    assert [h[0] for h in hits] == ["a3d_common.h"], hits
    src = open(os.path.join(ROOT, "articulation3d_amd", "csrc", "a3d_common.h")).read()
    assert src.index("#ifdef A3D_ABLATIONS") < src.index("getenv(") < src.index("#else")


def test_bench_labels_map_onto_the_kernels_of_the_committed_profile():
    """The bench line names kernels by the dispatcher's labels; the rocprofv3 summary of the same command names template
    instantiations.  bench.rocprof_name is the bridge the roofline object's `traffic` and the per-kernel HBM figures go over: every
    conv label of the committed round-3 bench line must land on a kernel of the committed kernel trace, and the dominant kernel's
    average launch duration must agree between the two (the contract of profiles/)."""
    import csv
    import json
    import sys

    sys.path.insert(0, ROOT)
    import bench

    rnd = next(r for r in ("r06", "r05", "r04", "r03") if os.path.exists(os.path.join(ROOT, "profiles", f"{r}_bench.json")) and os.path.exists(os.path.join(ROOT, "profiles", f"{r}_kernel_stats.csv")))
    line = json.loads(open(os.path.join(ROOT, "profiles", f"{rnd}_bench.json")).read().strip().splitlines()[-1])
    rows = list(csv.DictReader(open(os.path.join(ROOT, "profiles", f"{rnd}_kernel_stats.csv"))))
    squeeze = lambda s: re.sub(r"\s+", "", s)
    if rnd == "r03":  # (round 3's wide direct kernel had two template arguments; round 4 added the third, "activations pre-split")
        squeeze = lambda s: re.sub(r"(conv_x3w_kernel<\w+,\w+),false>", r"\1>", re.sub(r"\s+", "", s))
    if rnd in ("r03", "r04"):  # (round 5 added the Winograd GEMM's fourth template argument, the ping-pong loop)
        base = squeeze
        squeeze = lambda s: re.sub(r"(wino_gemm_x3w_kernel<\d,\w+,\w+),[01]>", r"\1>", base(s))
    names = [squeeze(r["Name"]) for r in rows]
    for label in line["roofline"]["all_conv_kernels"]:
        if label.endswith("wino_fold_kernel") and rnd in ("r03", "r04"):  # (those rounds also launched the 64-tile form unsplit)
            label = label.split(" planes")[0]
        want = squeeze(bench.rocprof_name(label))
        assert any(want in n for n in names), (label, want)
    roof = line["roofline"]
    want = squeeze(bench.rocprof_name(roof["kernel"]))
    avg_us = next(float(r["AverageNs"]) / 1e3 for r, n in zip(rows, names) if want in n)
    # (the stats file averages over the WHOLE process -- warm-up and calibration launches included --, the bench line over the timed
    # region: they agree to the spread of launch sizes, not to the digit)
    assert 0.7 < avg_us / (roof["avg_launch_ms"] * 1e3) < 1.3, (avg_us, roof["avg_launch_ms"])
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-3)


def test_split_k_rule_of_the_bf16_conv_kernel_is_a_function_of_the_shape():
    """Round 4: ops._bf16_splitk (csrc/conv_bf16.hip's split-K, training step only).  Splits only where the 128 x 64 tiles leave most of the
    chip idle AND the reduction is long; never more splits than chunks allow; large grids and short reductions stay whole."""
    from articulation3d_amd import ops

    assert ops._bf16_splitk(2 * 30 * 40, 256, 9 * 256) == 3       # res4 conv2 at 2 images: 76 tiles x 72 chunks
    assert ops._bf16_splitk(2 * 15 * 20, 512, 9 * 512) == 6       # res5 conv2: 40 tiles x 144 chunks
    assert ops._bf16_splitk(2 * 30 * 40, 1024, 256) == 1          # a short reduction
    assert ops._bf16_splitk(16 * 120 * 160, 256, 9 * 256) == 1    # a grid that fills the chip
    for M, cols, K in ((100, 64, 32 * 24), (2400, 256, 32 * 1000), (1, 32, 32 * 24)):
        sk = ops._bf16_splitk(M, cols, K)
        assert 1 <= sk <= 8 and sk <= K // 32


def test_pack_cache_key_sees_slots_added_or_replaced_on_child_modules():
    """the pack cache looks its (dict, name) slots up once; a buffer registered on a CHILD later, or a child replaced, must
    still change the key (a stale packed filter would be served silently otherwise)."""
    import torch
    from articulation3d_amd.modeling.layers import Conv2d, FrozenBatchNorm2d

    m = Conv2d(8, 8, 1, bias=False, norm=FrozenBatchNorm2d(8))
    k0 = m._key()
    assert m._key() == k0
    m.norm.register_buffer("extra", torch.zeros(1))
    k1 = m._key()
    assert k1 != k0 and len(k1) == len(k0) + 1
    m._modules["norm"] = FrozenBatchNorm2d(8)  # (replaced without passing through this module's __setattr__)
    k2 = m._key()
    assert k2 != k1 and len(k2) == len(k0)
    with torch.no_grad():
        m.norm.weight.mul_(2.0)  # in-place edits are seen through the version counter, as before
    assert m._key() != k2


def test_design_kernel_table_names_kernels_of_the_committed_trace():
    """DESIGN.md section 3 answers "which kernel runs layer X in arithmetic Y" from ONE table, generated by
    tools/kernel_table.py out of the dispatcher's own record (profiles/r06_kernel_table.md).  Every label of its default-arithmetic
    column must be a kernel of the committed rocprofv3 trace of the same step (profiles/r06_kernel_stats.csv) through bench.rocprof_name,
    every layer of the detection path must have a row, and DESIGN.md must point at the table."""
    import csv
    import sys

    sys.path.insert(0, ROOT)
    import bench

    lines = open(os.path.join(ROOT, "profiles", "r06_kernel_table.md")).read().splitlines()
    rows = [[c.strip() for c in l.strip("|").split("|")] for l in lines if l.startswith("| `")]
    assert len(rows) >= 100, len(rows)
    names = {re.sub(r"\s+", "", r["Name"]) for r in csv.DictReader(open(os.path.join(ROOT, "profiles", "r06_kernel_stats.csv")))}
    layers = {r[0].strip("`") for r in rows}
    for want in ("backbone.bottom_up.res4.2.conv2", "backbone.fpn_output2", "proposal_generator.rpn_head.conv", "roi_heads.box_head.fc1",
                 "roi_heads.plane_head.plane_fc1", "roi_heads.axis_head.axis_R_conv1", "roi_heads.mask_head.deconv"):
        assert want in layers, want
    seen = set()
    for r in rows:
        for label in re.findall(r"`([^`]+)`", r[2]):  # the fp16x2 column
            label = re.sub(r" \((first|second|all) [^)]*\)$", "", label)
            label = re.sub(r" levels\d$", "", label)  # (the multi-level launch: the same kernel, a five-row table in its epilogue)
            want = re.sub(r"\s+", "", bench.rocprof_name(label))
            assert any(want in n for n in names), (r[0], label, want)
            seen.add(label.split("<")[0].split(" ")[0])
    assert {"conv_h2xs_b2b_kernel", "conv_h2xs_kernel", "wino_gemm_h2w_kernel", "conv_h2w_kernel", "conv_ph4p_kernel", "conv_c3p_kernel", "stem_pool_kernel"} <= seen, seen
    res42 = next(r for r in rows if r[0] == "`backbone.bottom_up.res4.2.conv2`")
    assert res42[3] == "`wino_gemm_x3_kernel`" and res42[2] == "`wino_gemm_h2w_kernel<4>`", res42  # (the verdict's own example: res4.2.conv2 in bf16x3)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "profiles/r06_kernel_table.md" in design and len(design) < 40 * 1024 and os.path.exists(os.path.join(ROOT, "MEASUREMENTS.md"))
