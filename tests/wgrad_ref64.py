"""Float64 host reference of the weight gradient and the case tables of tests/test_gpu_backward_ref64.py (read by the CPU check
tests/test_wgrad_ref64_host.py and by the GPU file alike).  torch only; every function runs on the device its tensors live on, so the two
2^21 cases (64 MB operands) evaluate the same code on the GPU in float64.

The definition is the one in the header of csrc/conv_wgrad.hip, NHWC operands, packed result [Cout][KH][KW][Cin]:

    dw[co][kh][kw][ci] = sum over b, oh, ow of  dy[b, oh, ow, co] * x[b, oh*s + kh - pad, ow*s + kw - pad, ci]     (x = 0 outside the image)

evaluated tap by tap: the padded x, sliced at (kh, kw) with step s, is the [P, Cin] operand of one float64 GEMM with dy [P, Cout].

The one-hot argument.  A dy that is 1.0 at a few (pixel, channel) pairs -- every channel used once -- leaves ONE non-zero product per output
element, so no summation order, split or accumulator width can hide behind a tolerance: dw[co] must equal x gathered at that pixel's
taps, bit for bit (fp32, bf16x3: 1.0 has no mid / lo term, the three dropped products of the split are zero, hi + mid + lo is x) or
bf16(x) bit for bit (bf16).  A wrong edge column, a dropped last pixel of a slice, a bad tap or a wrong division in a loader shows up
as a wrong or missing row.
"""
import math

import torch

U = 2.0 ** -22
GUARD = 1 << 21  # a3d_wgrad_tr_form: the three-tap loader's float divisions are exact for padded pixel numbers below this


def c_law(K):
    return 8.0 + math.sqrt(max(K, 0)) / 4.0


def out_hw(c):
    return (c["H"] + 2 * c["p"] - c["k"]) // c["s"] + 1, (c["W"] + 2 * c["p"] - c["k"]) // c["s"] + 1


def bf16_round(t):
    """Nearest-even rounding to bf16, widened back (torch's conversion is RNE)."""
    return t.to(torch.bfloat16).to(t.dtype)


def wgrad_ref64(x, dy, k, stride, pad, live_pixels=None, round_bf16=False):
    """x [B,H,W,Cin], dy [B,Ho,Wo,Cout] (fp32 or float64 torch tensors) -> (dw64, S), both [Cout, k*k*Cin] float64.
    S = sum_p |dy| |x_tap|.  live_pixels: output pixels that count (whole images); the images past them are never touched."""
    x, dy = torch.as_tensor(x), torch.as_tensor(dy)
    B, H, W, Cin = x.shape
    B2, Ho, Wo, Cout = dy.shape
    assert B == B2 and Ho == (H + 2 * pad - k) // stride + 1 and Wo == (W + 2 * pad - k) // stride + 1
    nb = B
    if live_pixels is not None:
        live = min(max(int(live_pixels), 0), B * Ho * Wo)
        assert live % (Ho * Wo) == 0, "whole images only"
        nb = live // (Ho * Wo)
    x, dy = x[:nb], dy[:nb]
    if round_bf16:
        x, dy = bf16_round(x.float()), bf16_round(dy.float())
    x, dy = x.double(), dy.double()
    xp = torch.zeros((nb, H + 2 * pad, W + 2 * pad, Cin), dtype=torch.float64, device=x.device)
    xp[:, pad:pad + H, pad:pad + W] = x
    dy2 = dy.reshape(nb * Ho * Wo, Cout)
    dw = torch.zeros((Cout, k, k, Cin), dtype=torch.float64, device=x.device)
    S = torch.zeros_like(dw)
    for kh in range(k):
        for kw in range(k):
            tap = xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride].reshape(nb * Ho * Wo, Cin)
            dw[:, kh, kw] = dy2.t() @ tap
            S[:, kh, kw] = dy2.abs().t() @ tap.abs()
    return dw.reshape(Cout, k * k * Cin), S.reshape(Cout, k * k * Cin)


def one_hot_dy(shape, pixels, channels):
    """dy [B,Ho,Wo,Cout] fp32: 1.0 at (b, oh, ow, co) for the paired pixels / channels, 0 elsewhere (channels distinct)."""
    assert len(pixels) == len(channels) == len(set(channels)) and len(set(pixels)) == len(pixels)
    dy = torch.zeros(shape, dtype=torch.float32)
    for (b, oh, ow), co in zip(pixels, channels):
        dy[b, oh, ow, co] = 1.0
    return dy


def one_hot_expected(x, pixels, channels, Cout, k, stride, pad):
    """What every arithmetic must return for one_hot_dy: row co = x gathered at the hot pixel's taps (0 outside the image), other rows 0.
    x [B,H,W,Cin] in the dtype to compare in (fp32, or the bf16-rounded values); -> [Cout, k*k*Cin] on x's device."""
    B, H, W, Cin = x.shape
    out = torch.zeros((Cout, k, k, Cin), dtype=x.dtype, device=x.device)
    for (b, oh, ow), co in zip(pixels, channels):
        for kh in range(k):
            for kw in range(k):
                iy, ix = oh * stride + kh - pad, ow * stride + kw - pad
                if 0 <= iy < H and 0 <= ix < W:
                    out[co, kh, kw] = x[b, iy, ix]
    return out.reshape(Cout, k * k * Cin)


# ------------------------------------------------------------------------------------------------------------ slicing, as documented
def expected_form(c, prec, io):
    """The dispatch rule of a3d_wgrad_tr_form restated: 3 / 1 = transposed-read form (taps per workgroup), 0 = first form."""
    Ho, Wo = out_hw(c)
    if prec != 1 or c["s"] != 1 or (Ho, Wo) != (c["H"], c["W"]):
        return 0
    if ((io & 1) and c["Cin"] % 8) or ((io & 2) and c["Cout"] % 8):
        return 0
    if c["k"] == 3 and c["p"] == 1:
        return 3 if c["B"] * Ho * (Wo + 2) < GUARD else 0
    if c["k"] == 1 and c["p"] == 0:
        return 1
    return 0


def reduction(c, form):
    """(length of the sliced reduction, its rounding unit): padded rows of W + 2 and 64-pixel chunks for the three-tap form, plain
    pixels and 64 for the one-tap form, plain pixels and 32 for the first form."""
    Ho, Wo = out_hw(c)
    if form == 3:
        return c["B"] * Ho * (Wo + 2), 64
    return c["B"] * Ho * Wo, (64 if form == 1 else 32)


def slice_len(n, splitk, unit):
    chunk = -(-n // splitk)
    return -(-chunk // unit) * unit


def splitk_with_empty_slice(n, unit):
    """The smallest slice count >= 2 that leaves at least one slice empty (ceil(n / splitk) rounded up to the unit covers n early)."""
    sk = 2
    while -(-n // slice_len(n, sk, unit)) >= sk:
        sk += 1
    return sk


def pixel_of(c, form, idx):
    """(b, oh, ow) of index `idx` in the form's numbering, or None where the padded numbering has no pixel."""
    Ho, Wo = out_hw(c)
    if form == 3:
        q, j = divmod(idx, Wo + 2)
        return (q // Ho, q % Ho, j) if j < Wo else None
    b, r = divmod(idx, Ho * Wo)
    return (b, r // Wo, r % Wo)


def boundary_pixels(c, form, splitk):
    """(last pixel of a slice, first pixel of the next) around the LAST slice boundary that has a pixel behind it -- in the padded
    numbering a short last slice may hold padding slots only -- or (None, None) where the reduction fits one slice."""
    n, unit = reduction(c, form)
    L = slice_len(n, splitk, unit)
    for edge in range((n - 1) // L * L, 0, -L):
        hi = next((p for p in (pixel_of(c, form, i) for i in range(edge, n)) if p is not None), None)
        lo = next((p for p in (pixel_of(c, form, i) for i in range(edge - 1, -1, -1)) if p is not None), None)
        if hi is not None and lo is not None:
            return lo, hi
    return None, None


def probe_pixels(c, form, splitk):
    """Hot pixels of a one-hot probe: the four corners of the first and the last image, a last-column pixel (ow = Wo - 1) off the
    corners where the map has one, and the two pixels of boundary_pixels."""
    Ho, Wo = out_hw(c)
    B = c["B"]
    px = []
    for b in sorted({0, B - 1}):
        for oh in sorted({0, Ho - 1}):
            for ow in sorted({0, Wo - 1}):
                px.append((b, oh, ow))
    px.append((B - 1, Ho // 2, Wo - 1))
    px += [p for p in boundary_pixels(c, form, splitk) if p is not None]
    seen, out = set(), []
    for p in px:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


# ------------------------------------------------------------------------------------------------------------------- the case tables
# precs: the arithmetics the case runs at; at precision 1 every storage combination `io` (bit 0: x, bit 1: dy stored as bf16) of IO.
# form1: the form the case is MEANT to run on at precision 1, per io where the storage decides (precision 0 and 2 always run the first
# form).  probe_splitk: slice count of the one-hot probes (a slice boundary inside the reduction wherever the reduction is long enough).
IO = (0, 1, 2, 3)


def _c(name, B, H, W, Cin, Cout, k, s, p, precs, form1, probe_splitk=2, big=False):
    return dict(name=name, B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, p=p, precs=tuple(precs), form1=form1, probe_splitk=probe_splitk, big=big)


FIRST_FORM = [
    _c("k3s2_9x7_132to136", 2, 9, 7, 132, 136, 3, 2, 1, (0, 1, 2), 0),     # odd map under stride 2 (5x4 out), ragged second 128-tile
    _c("k1s2_9x7_132to136", 2, 9, 7, 132, 136, 1, 2, 0, (0, 1, 2), 0),
    _c("k3s1_5x6_36to20", 3, 5, 6, 36, 20, 3, 1, 1, (0, 2), None, probe_splitk=3),  # (precision 1 would be the three-tap form)
    _c("p1_k1", 1, 1, 1, 12, 16, 1, 1, 0, (0, 2), None),                    # P = 1
    _c("p1_k1s2", 1, 1, 1, 12, 16, 1, 2, 0, (0, 1, 2), 0),                  # P = 1 on the first form at precision 1 too (stride 2)
    _c("p1_k3", 1, 1, 1, 12, 16, 3, 1, 1, (0, 2), None),                    # only the centre tap is non-zero
    _c("p1_k3s2", 1, 1, 1, 12, 16, 3, 2, 1, (0, 1, 2), 0),
    _c("p40_k3s2", 2, 7, 10, 8, 12, 3, 2, 1, (0, 1, 2), 0, probe_splitk=3),  # P = 40: splitk 3 -> slices of 32, the third is empty
    _c("p33_k1s2", 3, 1, 21, 8, 12, 1, 2, 0, (0, 1, 2), 0),                 # P = 33: one pixel past a 32-pixel chunk
]

# (1x63: Pp = 130, two slices of 128 would leave only padding slots in the second; three slices of 64 put pixels on both sides)
THREE_TAP = [_c(f"tr3_{H}x{W}", 2, H, W, 136, 72, 3, 1, 1, (1,), 3, probe_splitk=3 if (H, W) == (1, 63) else 2)
             for W in (1, 61, 62, 63) for H in (1, 3)] + [  # Wp = 3, 63, 64, 65
    _c("tr3_7x5_256to128", 3, 7, 5, 256, 128, 3, 1, 1, (1,), 3),            # Pp = 147, splitk 2 -> boundary 128 = row 18, column 2
    _c("tr3_cin132", 2, 5, 6, 132, 72, 3, 1, 1, (1,), {0: 3, 1: 0, 2: 3, 3: 0}),  # bf16-stored x, Cin & 7: back to the first form
    _c("guard_below", 1, 1023, 2048, 8, 8, 3, 1, 1, (1,), 3, probe_splitk=64, big=True),   # Pp = 2 097 150
    _c("guard_at", 1, 1024, 2046, 8, 8, 3, 1, 1, (1,), 0, probe_splitk=64, big=True),      # Pp = 2^21: the first form
]

ONE_TAP = [_c(f"tr1_rows{P}", P, 1, 1, 264, 72, 1, 1, 0, (1,), 1) for P in (1, 64, 65, 70)] + [  # ragged 256-wide ci tile
    _c("tr1_2x5x7", 2, 5, 7, 40, 24, 1, 1, 0, (1,), 1),
]

CASES = FIRST_FORM + THREE_TAP + ONE_TAP

# live-count cases, one per form family: (case, precision, io) -- p_dev in {0, one image, full, full + 5 images, -7}
LIVE = [
    (_c("live_first", 3, 9, 7, 12, 8, 3, 2, 1, (0, 1, 2), 0), [(0, 0), (1, 0), (1, 3), (2, 0)]),
    (_c("live_tr3", 3, 7, 5, 16, 8, 3, 1, 1, (1,), 3), [(1, 0), (1, 3)]),
    (_c("live_tr1", 3, 5, 7, 40, 24, 1, 1, 0, (1,), 1), [(1, 0), (1, 3)]),
]


def form_of(c, prec, io):
    """The intended form of a table row (data, not the rule)."""
    if prec != 1:
        return 0
    f = c["form1"]
    return f[io] if isinstance(f, dict) else f


def runs(cases):
    """(case, precision, io) of every launch configuration of `cases`."""
    out = []
    for c in cases:
        for prec in c["precs"]:
            for io in (IO if prec == 1 else (0,)):
                out.append((c, prec, io))
    return out


def run_id(r):
    c, prec, io = r
    return f"{c['name']}-p{prec}-io{io}"


def kernel_label(form, prec, io):
    """The kernel a launch runs, as train_ops.conv_wgrad names it for the timing records."""
    if form:
        return f"conv_wgrad_tr_kernel<{form}, {io}>"
    return {0: "conv_wgrad_kernel", 1: f"conv_wgrad_bf16_kernel<false, {io}>", 2: "conv_wgrad_bf16_kernel<true, 0>"}[prec]


ALL_LABELS = (["conv_wgrad_kernel", "conv_wgrad_bf16_kernel<true, 0>"] + [f"conv_wgrad_bf16_kernel<false, {io}>" for io in IO]
              + [f"conv_wgrad_tr_kernel<{f}, {io}>" for f in (3, 1) for io in IO])


def make_operands(c, seed=0):
    """fp32 x [B,H,W,Cin], dy [B,Ho,Wo,Cout] of a case (CPU, seeded; the storage variants are roundings of these)."""
    g = torch.Generator().manual_seed(1000 + seed)
    Ho, Wo = out_hw(c)
    x = torch.randn((c["B"], c["H"], c["W"], c["Cin"]), generator=g)
    dy = torch.randn((c["B"], Ho, Wo, c["Cout"]), generator=g)
    return x, dy
