"""CPU checks of tests/wgrad_ref64.py, the float64 reference tests/test_gpu_backward_ref64.py holds the weight-gradient kernels to.

(a) the tap-by-tap reference equals float64 autograd of F.conv2d on every case of the table (1e-12, relative, max norm);
(b) with a live count the images past it do not contribute (NaN in the dead part stays out);
(c) the one-hot gather helper agrees with the reference, exactly;
(d) the table's intended forms agree with the restated dispatch rule, and the slicing helpers leave the slices they promise;
(e) the three-tap loader's division by float reciprocal, restated in numpy float32, is exact for every padded pixel number below 2^21 at
    every row pitch and map height of the table -- and is NOT exact a little further up, which is why the guard carries weight."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref64 as R  # noqa: E402

ALL = R.CASES + [c for c, _ in R.LIVE]


def _autograd64(x, dy, c):
    w = torch.zeros(c["Cout"], c["Cin"], c["k"], c["k"], dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w, None, c["s"], c["p"]).backward(dy.double().permute(0, 3, 1, 2))
    return w.grad.permute(0, 2, 3, 1).reshape(c["Cout"], -1)


@pytest.mark.parametrize("c", ALL, ids=lambda c: c["name"])
def test_reference_equals_float64_autograd(c):
    x, dy = R.make_operands(c)
    for rb in (False, True):
        dw, S = R.wgrad_ref64(x, dy, c["k"], c["s"], c["p"], round_bf16=rb)
        xa, dya = (R.bf16_round(x), R.bf16_round(dy)) if rb else (x, dy)
        ref = _autograd64(xa, dya, c)
        assert dw.shape == ref.shape == S.shape
        assert float((dw - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
        assert bool((S >= dw.abs() * (1 - 1e-12)).all())
        if c["big"]:
            break  # (one pass over the 64 MB operands: the rounding is the same code on the same path)


@pytest.mark.parametrize("c", [c for c, _ in R.LIVE], ids=lambda c: c["name"])
def test_live_count_leaves_dead_images_out(c):
    x, dy = R.make_operands(c)
    Ho, Wo = R.out_hw(c)
    img = Ho * Wo
    full, _ = R.wgrad_ref64(x, dy, c["k"], c["s"], c["p"])
    for live, nb in ((0, 0), (img, 1), (c["B"] * img, c["B"]), ((c["B"] + 5) * img, c["B"]), (-7, 0)):
        xn, dyn = x.clone(), dy.clone()
        xn[nb:] = float("nan")
        dyn[nb:] = float("nan")
        dw, S = R.wgrad_ref64(xn, dyn, c["k"], c["s"], c["p"], live_pixels=live)
        want, _ = R.wgrad_ref64(x[:nb], dy[:nb], c["k"], c["s"], c["p"])
        assert torch.equal(dw, want) and bool(torch.isfinite(S).all())
        if nb == c["B"]:
            assert torch.equal(dw, full)
        if nb == 0:
            assert not dw.any() and not S.any()


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c["name"])
def test_one_hot_helper_agrees_with_reference(c):
    x, _ = R.make_operands(c)
    Ho, Wo = R.out_hw(c)
    for form in sorted({R.form_of(c, prec, io) for _, prec, io in R.runs([c])}):
        px = R.probe_pixels(c, form, c["probe_splitk"])
        assert len(px) == len(set(px)) and all(0 <= b < c["B"] and 0 <= oh < Ho and 0 <= ow < Wo for b, oh, ow in px)
        assert (0, 0, 0) in px and (c["B"] - 1, Ho - 1, Wo - 1) in px
        n, unit = R.reduction(c, form)
        lo, hi = R.boundary_pixels(c, form, c["probe_splitk"])
        if n > R.slice_len(n, c["probe_splitk"], unit):  # a sliced reduction is probed on both sides of a boundary, in different slices
            assert lo is not None and hi is not None and lo in px and hi in px, (c["name"], form)
            idx = {R.pixel_of(c, form, i): i for i in range(n)} if n < 4096 else None
            if idx is not None:
                L = R.slice_len(n, c["probe_splitk"], unit)
                assert idx[hi] // L == idx[lo] // L + 1 and idx[hi] - idx[lo] <= 4, (c["name"], form, lo, hi)
        else:
            assert (lo, hi) == (None, None)
        for i in range(0, len(px), c["Cout"]):
            grp = px[i:i + c["Cout"]]
            ch = [(5 * j + 3) % c["Cout"] for j in range(len(grp))] if c["Cout"] % 5 else list(range(len(grp)))
            dy = R.one_hot_dy((c["B"], Ho, Wo, c["Cout"]), grp, ch)
            dw, S = R.wgrad_ref64(x, dy, c["k"], c["s"], c["p"])
            want = R.one_hot_expected(x.double(), grp, ch, c["Cout"], c["k"], c["s"], c["p"])
            assert torch.equal(dw, want)  # one product per element: exact in any arithmetic
            assert torch.equal(S, want.abs())


def test_table_forms_follow_the_dispatch_rule_and_cover_every_label():
    labels = set()
    for c, prec, io in R.runs(R.CASES) + [(c, p, io) for c, pio in R.LIVE for p, io in pio]:
        form = R.form_of(c, prec, io)
        assert form == R.expected_form(c, prec, io), (c["name"], prec, io)
        assert c["Cin"] % 4 == 0 and c["Cout"] % 4 == 0
        if prec == 1 and form == 0:  # the first form loads channel pairs of a bf16-stored operand
            assert not ((io & 1) and c["Cin"] % 2) and not ((io & 2) and c["Cout"] % 2)
        labels.add(R.kernel_label(form, prec, io))
    assert labels == set(R.ALL_LABELS)
    by = {c["name"]: c for c in R.CASES}
    Ho, Wo = R.out_hw(by["guard_below"])
    assert by["guard_below"]["B"] * Ho * (Wo + 2) == 2097150
    Ho, Wo = R.out_hw(by["guard_at"])
    assert by["guard_at"]["B"] * Ho * (Wo + 2) == R.GUARD
    assert R.out_hw(by["k3s2_9x7_132to136"]) == (5, 4)


def test_slicing_helpers():
    assert R.slice_len(40, 3, 32) == 32 and R.splitk_with_empty_slice(40, 32) == 3  # the issue's P = 40, splitk = 3
    for n, unit in ((1, 32), (33, 32), (40, 32), (90, 32), (6, 64), (147, 64), (378, 64), (2097150, 64), (2095104, 32)):
        sk = R.splitk_with_empty_slice(n, unit)
        L = R.slice_len(n, sk, unit)
        assert L % unit == 0 and L * sk >= n and (sk - 1) * L >= n, (n, unit, sk)  # the last slice starts at or past the end
        assert sk < 65536
    c = next(c for c in R.CASES if c["name"] == "tr3_7x5_256to128")
    L = R.slice_len(*((R.reduction(c, 3)[0], 2, 64)))
    assert L == 128 and 0 < L % (c["W"] + 2) < c["W"]  # the boundary falls inside an image row
    px = R.probe_pixels(c, 3, 2)
    assert R.pixel_of(c, 3, 127) == (2, 4, 1) and R.pixel_of(c, 3, 128) == (2, 4, 2) and {(2, 4, 1), (2, 4, 2)} <= set(px)


def _float_div(kap, d):
    """q = (int)((kap + 0.5f) * (1.f / d)): the loader's division, in float32."""
    inv = np.float32(1.0) / np.float32(d)
    return ((kap.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


def test_float_reciprocal_division_is_exact_below_the_guard():
    kap = np.arange(R.GUARD, dtype=np.int32)
    three = [c for c in R.CASES + [c for c, _ in R.LIVE] if c["k"] == 3 and c["s"] == 1 and c["p"] == 1]
    pitches = sorted({c["W"] + 2 for c in three})
    heights = sorted({c["H"] for c in three})
    assert {3, 63, 64, 65, 2050}.issubset(pitches)
    for d in pitches + heights:
        assert np.array_equal(_float_div(kap, d), kap // d), d
    # ... and not beyond: some pitch of the table already divides wrongly below 2^24
    far = np.arange(R.GUARD, 1 << 24, dtype=np.int32)
    assert any(not np.array_equal(_float_div(far, d), far // d) for d in pitches)
