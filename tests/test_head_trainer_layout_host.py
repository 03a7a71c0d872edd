"""Host-side check of the flat parameter layout of the head trainers (articulation3d_amd/training_head.py: flat_layout over the axis and
the mask stage's layer tables).  The layout is the checkpoint format -- engine.FlatSGD.state_dict() saves the momentum buffer as it lies --
so it is held to numbers written out here, not to the code that computes it."""
import pytest

from articulation3d_amd.training_axis import AH, axis_layer_table
from articulation3d_amd.training_head import flat_layout
from articulation3d_amd.training_mask import MH, mask_layer_table

CONV = 256 * 3 * 3 * 256  # 589 824
FC = 1024 * 256 * 14 * 14
AXIS_TOTAL, AXIS_CUT = 107_548_736, 53_774_368
MASK_TOTAL, MASK_PRED = 2_622_980, 2_622_720


def _axis_expected():
    """name -> (weight offset, weights, bias offset, biases): the running sum, R tower then T."""
    want, off = {}, 0
    for t, last in (("R", "rot"), ("T", "tran")):
        sizes = [(f"{AH}axis_{t}_conv{k}", CONV, 256) for k in (1, 2, 3, 4)] + [(f"{AH}axis_{t}_fc1", FC, 1024), (AH + last, 32 * 1024, 32)]
        for name, nw, nb in sizes:
            want[name] = (off, nw, off + nw, nb)
            off += nw + nb
    return want, off


def _mask_expected():
    want, off = {}, 0
    for name, nw, nb in [(f"{MH}mask_fcn{k}", CONV, 256) for k in (1, 2, 3, 4)] + [(MH + "deconv", 4 * 256 * 256, 256)]:
        want[name] = (off, nw, off + nw, nb)
        off += nw + nb
    return want, off


def test_axis_layout_is_the_checkpoint_format():
    lay = flat_layout(**axis_layer_table())
    want, end = _axis_expected()
    assert list(lay.layers) == list(want) and lay.layers == want
    assert end == AXIS_TOTAL == lay.total and lay.tail == {}
    assert lay.layers[AH + "axis_T_conv1"][0] == AXIS_CUT == AXIS_TOTAL // 2
    assert lay.segments == [(0, AXIS_CUT), (AXIS_CUT, AXIS_TOTAL)]


def test_mask_layout_is_the_checkpoint_format():
    lay = flat_layout(**mask_layer_table())
    want, end = _mask_expected()
    assert list(lay.layers) == list(want) and lay.layers == want
    assert lay.layers[MH + "deconv"][1:] == (262_144, 4 * 590_080 + 262_144, 256)  # ONE bias per output channel
    assert end == MASK_PRED and lay.tail == {"pred_w": (MASK_PRED, 256), "pred_b": (MASK_PRED + 256, 1)}
    assert lay.total == MASK_TOTAL == (MASK_PRED + 257 + 3) // 4 * 4
    assert lay.segments == [(0, MASK_TOTAL)]


BU, RPN, BOX = "backbone.bottom_up.", "proposal_generator.rpn_head.", "roi_heads."
DET_TOTAL, DET_WEIGHTS, DET_WINOGRAD = 41_103_680, 41_099_264, 25_165_824
DET_FIRST = {BU + "res3.0.conv1": 0, BU + "res4.0.conv1": 1_212_416, BU + "res5.0.conv1": 8_290_304, "backbone.fpn_lateral2": 23_232_512,
             RPN + "conv": 26_576_896, BOX + "box_head.fc1": 27_175_200, BOX + "box_predictor.pred": 41_070_880}
DET_SEGMENTS = [(27_175_200, 41_103_680), (8_290_304, 27_175_200), (1_212_416, 8_290_304), (0, 1_212_416)]  # in exchange order


def _detector_sizes():
    """(name, weights, biases, 3x3) in flat-buffer order: res3-res5 with their FrozenBN folded (no bias entries), FPN, RPN head, box head."""
    sizes, cin = [], 256
    for stage, blocks, mid, out in (("res3", 4, 128, 512), ("res4", 6, 256, 1024), ("res5", 3, 512, 2048)):
        for i in range(blocks):
            p = f"{BU}{stage}.{i}."
            sizes += [(p + "conv1", mid * cin, 0, False), (p + "conv2", mid * 9 * mid, 0, True), (p + "conv3", out * mid, 0, False)]
            if i == 0:
                sizes.append((p + "shortcut", out * cin, 0, False))
            cin = out
    for level, c in ((2, 256), (3, 512), (4, 1024), (5, 2048)):
        sizes += [(f"backbone.fpn_lateral{level}", 256 * c, 256, False), (f"backbone.fpn_output{level}", CONV, 256, True)]
    return sizes + [(RPN + "conv", CONV, 256, True), (RPN + "pred", 32 * 256, 32, False), (BOX + "box_head.fc1", 1024 * 49 * 256, 1024, False),
                    (BOX + "box_head.fc2", 1024 * 1024, 1024, False), (BOX + "box_predictor.pred", 32 * 1024, 32, False)]


def test_detector_layout_is_the_checkpoint_format():
    """Stage 1's flat buffers (DetectorTrainer.params / grads / momentum): the larger half of the checkpoint format."""
    from articulation3d_amd.training import detector_layer_table

    table = detector_layer_table(2)
    lay = flat_layout(**table)
    want, off = {}, 0
    for name, nw, nb, _ in _detector_sizes():
        want[name] = (off, nw, off + nw, nb)
        off += nw + nb
    assert len(want) == 55 and list(lay.layers) == list(want) and lay.layers == want
    assert [ly.name for ly in table["layers"]] == list(want)
    assert off == DET_TOTAL == lay.total and off % 4 == 0 and lay.tail == {}
    assert {n: lay.layers[n][0] for n in DET_FIRST} == DET_FIRST
    assert all(lay.layers[n][3] == 0 for n in want if n.startswith(BU)) and all(lay.layers[n][3] > 0 for n in want if not n.startswith(BU))
    assert lay.segments[::-1] == DET_SEGMENTS
    assert all(a % 4 == 0 and b % 4 == 0 for a, b in lay.segments)
    assert all(w % 8 == 0 for w, _, _, _ in lay.layers.values())  # the bf16 filters' 16-byte rule (DetectorTrainer._p16)
    assert sum(nw for _, nw, _, _ in _detector_sizes()) == DET_WEIGHTS == sum(nw for _, nw, _, _ in lay.layers.values())
    assert sum(nw // 9 * 16 for _, nw, _, k3 in _detector_sizes() if k3) == DET_WINOGRAD
    assert sum(16 * ly.rows * ly.cin for ly in table["layers"] if ly.k == 3) == DET_WINOGRAD
    three = detector_layer_table(3)  # sensitivity: the class count moves nothing (the predictor is padded to 32 rows) but its sources
    assert flat_layout(**three).layers == want and three["layers"][-1].sources[1] == (BOX + "box_predictor.bbox_pred", 4, 12)


@pytest.mark.parametrize("table", [axis_layer_table, mask_layer_table])
def test_vector_reads_find_their_offsets_aligned(table):
    """16-byte reads: every layer's filter (the conv and transpose kernels), the predictor's weights (a3d_mask_loss), every segment bound
    of the gradient exchange and the padded total (a3d_sgd_momentum and the payload conversion run over float4)."""
    lay = flat_layout(**table())
    assert all(w % 4 == 0 for w, _, _, _ in lay.layers.values())
    assert all(a % 4 == 0 and b % 4 == 0 for a, b in lay.segments) and lay.total % 4 == 0
    if lay.tail:
        assert lay.tail["pred_w"][0] % 4 == 0


def test_layout_follows_the_table():
    """Sensitivity: the numbers above are the table's, not constants of the function."""
    t = mask_layer_table()
    full = flat_layout(t["layers"], tail=t["tail"])  # the deconv with a bias per ROW (4 x 256) instead of one per output channel
    assert full.tail["pred_w"][0] == MASK_PRED + 768 and full.total == MASK_TOTAL + 768
    assert full.layers[MH + "deconv"][3] == 1024
    a = axis_layer_table()
    ly = list(a["layers"])
    ly[4], ly[5] = ly[5], ly[4]  # the R tower's FC and its fused last layer swapped
    swapped, ref = flat_layout(ly, cuts=a["cuts"]), flat_layout(**a)
    assert swapped.total == ref.total and swapped.segments == ref.segments
    assert swapped.layers[AH + "rot"][0] == 4 * (CONV + 256) != ref.layers[AH + "rot"][0]
    assert swapped.layers[AH + "axis_R_fc1"] != ref.layers[AH + "axis_R_fc1"]
    ly[5], ly[6] = ly[6], ly[5]  # ... and the FC moved behind the cut: the segments move with it
    assert flat_layout(ly, cuts=a["cuts"]).segments != ref.segments
