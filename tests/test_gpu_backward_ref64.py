"""GPU suite (-m gpu): every weight-gradient form and every backward helper of the training step held to float64, element by element.

The weight gradient (csrc/conv_wgrad.hip, csrc/conv_wgrad_tr.hip) has fourteen kernels: the fp32 MFMA form, the bf16 first form at four
storage variants, its bf16x3 arithmetic, and the two transposed-read forms (three taps / one tap per workgroup) at four storage variants
each.  Every case of tests/wgrad_ref64.py runs on the form it names -- a3d_wgrad_tiles reports which form the library picks, and a case
that lands on another form fails by name -- and in every launch mode: plain, repeated (bit-identical), `scale` with `accumulate` on a
non-zero dw, an explicit `splitk` that leaves a slice empty (plain and accumulating), and `defer=` with a flush (the per-launch bits).

The law (tests/test_gpu_layer_ref64.py's), for every element, K = live pixels, dw_prev = prior content when accumulating (else 0):

    | dw - (dw_prev + scale dw64) |  <=  c(K) 2^-22 |scale| S  +  2^-22 (|dw_prev| + |scale dw64|),    S = sum_p |dy| |x_tap|,  c(K) = 8 + sqrt(K) / 4

fp32 accumulation of K terms costs sqrt(K) 2^-24; the bf16x3 split drops terms below 2^-24 of a product; bf16 x bf16 products are exact
in fp32, so precision 1 obeys the same law against float64 of the bf16-ROUNDED operands; the scale product and the accumulating add
round once each (the second term).  Where S = 0 (a tap that only ever sees padding) the result must be exactly 0.  No constant is
fitted; the worst err / bound per kernel label is printed, and the last test fails, by name, for any label the file did not exercise.

The form is asked of a3d_wgrad_tiles with a descriptor of the case's fields, the call train_ops.conv_wgrad itself makes to choose its slice
count: it shows what the dispatch picks for those fields, and a launch path that disagreed with it would show in the law and the exact
probes.  A developer build with -DA3D_ABLATIONS must leave A3D_WGRAD_TR unset, or every transposed-read case fails by name.

One-hot probes (wgrad_ref64's docstring has the argument): hot pixels at the corners of the first and last image, in the last column,
and on both sides of the last slice boundary, the boundary computed here from the documented slicing.  Exact in every arithmetic.

The helpers: colsum / colsum_bf16 / colsum_rows obey c(M) 2^-22 sum|dy| (+ 2^-22 |out_prev| when accumulating: the one rounding of that
add) against a float64 sum, and the scalar path (C % 4 != 0 or a pointer off 16 bytes) is additionally held to the BITS of its documented
summation order restated in numpy fp32 -- which also proves that path ran.  weight_transpose / TransposeBatch, zero_insert2,
sumpool2_add and the two SGD kernels are exact against op-by-op fp32 restatements (train_ops.hip is built with -ffp-contract=off);
wino_weight_transform obeys the law with K = 9 and S = |G| |g| |G^T|.
"""
import ctypes as C
import math
import os
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref64 as R  # noqa: E402

pytestmark = pytest.mark.gpu

U = R.U
WORST = defaultdict(float)  # kernel label -> worst err / bound over the file
SEEN = set()                # weight-gradient kernel labels whose form assertion held and whose launch was checked
_OPERANDS = {}              # case name -> operands and float64 references, built once


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from articulation3d_amd import train_ops

    return train_ops


def L():
    from articulation3d_amd import _lib

    return _lib


# ------------------------------------------------------------------------------------------------------------------------ plumbing
def ran_form(c, prec, io):
    """The form the library runs this layer on (a3d_wgrad_tiles: 3, 1 or 0)."""
    lib = L()
    d = lib.WgradDesc()
    Ho, Wo = R.out_hw(c)
    d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = c["B"], c["H"], c["W"], c["Cin"], Ho, Wo, c["Cout"]
    d.KH, d.KW, d.stride, d.pad = c["k"], c["k"], c["s"], c["p"]
    d.precision, d.io_bf16, d.splitk = prec, io, 1
    tiles, red = C.c_int(0), C.c_int(0)
    form = lib.lib().a3d_wgrad_tiles(C.byref(d), C.byref(tiles), C.byref(red))
    assert form in (0, 1, 3) and tiles.value > 0, (form, tiles.value)
    assert red.value == R.reduction(c, form)[0]
    return form


def check_form(c, prec, io):
    want, got = R.form_of(c, prec, io), ran_form(c, prec, io)
    assert got == want, f"{R.run_id((c, prec, io))}: meant for {R.kernel_label(want, prec, io)}, the library runs {R.kernel_label(got, prec, io)}"
    return got, R.kernel_label(got, prec, io)


def operands(c):
    """x, dy of a case on the GPU (fp32 and bf16 storage) and its float64 references: on the host, or on the GPU for the 64 MB cases."""
    o = _OPERANDS.get(c["name"])
    if o is None:
        x, dy = R.make_operands(c)
        xd, dyd = x.cuda(), dy.cuda()
        o = _OPERANDS[c["name"]] = dict(x={0: xd, 1: xd.bfloat16()}, dy={0: dyd, 1: dyd.bfloat16()}, host=(xd, dyd) if c["big"] else (x, dy), ref={})
    return o


def release(c, io):
    """The 64 MB cases give their operands and references back after their last storage variant (rebuilt, seeded, by the next test that
    needs them): nothing of that size stays resident on a shared GPU for the life of the module."""
    if c["big"] and io == R.IO[-1]:
        _OPERANDS.pop(c["name"], None)


def reference(c, prec):
    o = operands(c)
    rb = prec == 1
    if rb not in o["ref"]:
        o["ref"][rb] = R.wgrad_ref64(*o["host"], c["k"], c["s"], c["p"], round_bf16=rb)
    return o["ref"][rb]


def stored(c, io):
    o = operands(c)
    return o["x"][io & 1], o["dy"][(io >> 1) & 1]


def ratio_of(err, bound):
    """err / bound per element; an error where the bound is 0 is infinite (those elements must be exact)."""
    return torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))


def hold(label, what, got, want, bound):
    got = got.to(want.device).double()
    assert bool(torch.isfinite(got).all()), (label, what, "non-finite result")
    r = ratio_of((got - want).abs(), bound)
    worst = float(r.max())
    WORST[label] = max(WORST[label], worst)
    print(f"{label:38s} {what:34s} worst err/bound {worst:.4f}")
    if worst > 1.0:
        i = int(r.argmax())
        pytest.fail(f"{label} {what}: err/bound {worst:.3f} at flat element {i}: got {float(got.flatten()[i])!r}, float64 {float(want.flatten()[i])!r}")


def hold_wgrad(label, what, dw, ref, K, scale=None, prev=None):
    dw64, S = ref
    dev = dw64.device
    sc = scale.to(dev).double()[:, None] if scale is not None else torch.ones((), dtype=torch.float64, device=dev)
    pv = prev.to(dev).double() if prev is not None else torch.zeros((), dtype=torch.float64, device=dev)
    want = pv + sc * dw64
    bound = R.c_law(K) * U * sc.abs() * S + U * (pv.abs() + (sc * dw64).abs())
    hold(label, what, dw, want, bound)


def bits(t):
    return t.contiguous().view(torch.int32)


def wgrad(T, c, x, dy, dw=None, prec=0, **kw):
    if dw is None:
        dw = torch.full((c["Cout"], c["k"] * c["k"] * c["Cin"]), 7.0, device="cuda")
    return T.conv_wgrad(x, dy, dw, KH=c["k"], KW=c["k"], stride=c["s"], pad=c["p"], precision=prec, **kw)


# --------------------------------------------------------------------------------------------------- the law, in every launch mode
@pytest.mark.parametrize("run", R.runs(R.CASES), ids=R.run_id)
def test_wgrad_law_in_every_mode(T, run):
    c, prec, io = run
    form, label = check_form(c, prec, io)
    x, dy = stored(c, io)
    ref = reference(c, prec)
    Ho, Wo = R.out_hw(c)
    K = c["B"] * Ho * Wo
    g = torch.Generator().manual_seed(7)
    scale = (torch.rand(c["Cout"], generator=g) + 0.5) * (1 - 2 * (torch.arange(c["Cout"]) % 2))  # both signs
    prev = torch.randn((c["Cout"], c["k"] * c["k"] * c["Cin"]), generator=g)
    scale_d, prev_d = scale.cuda(), prev.cuda()

    plain = wgrad(T, c, x, dy, prec=prec)
    hold_wgrad(label, "plain", plain, ref, K)
    again = wgrad(T, c, x, dy, prec=prec)
    assert torch.equal(bits(plain), bits(again)), (label, "a second identical launch differs")

    acc = wgrad(T, c, x, dy, dw=prev_d.clone(), prec=prec, scale=scale_d, accumulate=True)
    hold_wgrad(label, "scale + accumulate", acc, ref, K, scale, prev)

    n, unit = R.reduction(c, form)
    sk = R.splitk_with_empty_slice(n, unit)
    assert (sk - 1) * R.slice_len(n, sk, unit) >= n  # the last slice is empty
    hold_wgrad(label, f"splitk {sk} (empty slice)", wgrad(T, c, x, dy, prec=prec, splitk=sk), ref, K)
    acc = wgrad(T, c, x, dy, dw=prev_d.clone(), prec=prec, scale=scale_d, accumulate=True, splitk=sk)
    hold_wgrad(label, f"splitk {sk} + scale + accumulate", acc, ref, K, scale, prev)

    defer = T.DeferredReduces(torch.device("cuda"))
    parked = wgrad(T, c, x, dy, prec=prec, defer=defer)
    assert len(defer.items) == 1
    defer.flush()
    assert torch.equal(bits(parked), bits(plain)), (label, "the deferred reduce differs from the per-launch reduce")
    SEEN.add(label)
    release(c, io)


# -------------------------------------------------------------------------------------------------------------------- one-hot probes
@pytest.mark.parametrize("run", R.runs(R.CASES), ids=R.run_id)
def test_wgrad_one_hot_probes(T, run):
    c, prec, io = run
    form, label = check_form(c, prec, io)
    o = operands(c)
    x, _ = stored(c, io)
    xcmp = o["x"][1].float() if prec == 1 else o["x"][0]  # bf16(x) for the bf16 arithmetic, x itself for fp32 and bf16x3
    Ho, Wo = R.out_hw(c)
    sk = c["probe_splitk"]
    px = R.probe_pixels(c, form, sk)
    n, unit = R.reduction(c, form)
    if n > R.slice_len(n, sk, unit):  # the reduction is sliced: both sides of a slice boundary are probed
        lo, hi = R.boundary_pixels(c, form, sk)
        assert lo is not None and hi is not None and lo in px and hi in px, (label, "no probe on both sides of a slice boundary")
    for i in range(0, len(px), c["Cout"]):
        grp = px[i:i + c["Cout"]]
        ch = [(j * 5 + 3) % c["Cout"] for j in range(len(grp))] if c["Cout"] % 5 else list(range(len(grp)))
        dy = R.one_hot_dy((c["B"], Ho, Wo, c["Cout"]), grp, ch).cuda()
        if io & 2:
            dy = dy.bfloat16()
        dw = wgrad(T, c, x, dy, prec=prec, splitk=sk)
        want = R.one_hot_expected(xcmp, grp, ch, c["Cout"], c["k"], c["s"], c["p"])
        if not torch.equal(dw, want):
            bad = (dw != want).nonzero()
            co, col = (int(v) for v in bad[0])
            pix = grp[ch.index(co)] if co in ch else None
            tap, ci = divmod(col, c["Cin"])
            pytest.fail(f"{label}: one-hot probe wrong in {len(bad)} elements, first at co {co} (hot pixel {pix}) tap {divmod(tap, c['k'])} ci {ci}: "
                        f"got {float(dw[co, col])!r}, want {float(want[co, col])!r}")
    SEEN.add(label)
    release(c, io)


# ----------------------------------------------------------------------------------------------------------------------- live count
@pytest.mark.parametrize("run", [(c, p, io) for c, pio in R.LIVE for p, io in pio], ids=R.run_id)
def test_wgrad_live_count_extremes(T, run):
    c, prec, io = run
    form, label = check_form(c, prec, io)
    x, dy = R.make_operands(c)
    Ho, Wo = R.out_hw(c)
    img, B = Ho * Wo, c["B"]
    cast = lambda t, bit: t.cuda().bfloat16() if bit else t.cuda()  # noqa: E731
    xs, dys = cast(x, io & 1), cast(dy, io & 2)
    full = wgrad(T, c, xs, dys, prec=prec, splitk=2)
    hold_wgrad(label, "full, no live count", full, R.wgrad_ref64(x, dy, c["k"], c["s"], c["p"], round_bf16=prec == 1), B * img)
    prev = torch.randn_like(full)
    scale = torch.rand(c["Cout"], device="cuda") + 0.5
    for count, nb in ((0, 0), (img, 1), (B * img, B), ((B + 5) * img, B), (-7, 0)):
        xn, dyn = x.clone(), dy.clone()
        xn[nb:] = float("nan")   # the dead images hold NaN in both operands: reading one of them poisons the sum
        dyn[nb:] = float("nan")
        xn, dyn = cast(xn, io & 1), cast(dyn, io & 2)
        p_dev = torch.tensor([count], dtype=torch.int32, device="cuda")
        dw = wgrad(T, c, xn, dyn, prec=prec, splitk=2, p_dev=p_dev)
        if nb == B:
            assert torch.equal(bits(dw), bits(full)), (label, count, "a full or clamped count must give the bits of the full launch")
        elif nb == 0:
            assert not bool(dw.any()) and bool(torch.isfinite(dw).all()), (label, count, "a live count of 0 must give exactly 0")
            acc = wgrad(T, c, xn, dyn, dw=prev.clone(), prec=prec, splitk=2, p_dev=p_dev, scale=scale, accumulate=True)
            assert torch.equal(bits(acc), bits(prev)), (label, count, "accumulating nothing must leave dw untouched")
        else:
            ref = R.wgrad_ref64(xn.float().cpu(), dyn.float().cpu(), c["k"], c["s"], c["p"], live_pixels=count, round_bf16=prec == 1)
            hold_wgrad(label, f"live count {count}", dw, ref, nb * img)
            acc = wgrad(T, c, xn, dyn, dw=prev.clone(), prec=prec, splitk=2, p_dev=p_dev, scale=scale, accumulate=True)
            hold_wgrad(label, f"live count {count} + accumulate", acc, ref, nb * img, scale.cpu(), prev.cpu())
    SEEN.add(label)


# --------------------------------------------------------------------------------------------------------------------- batched reduce
def test_wgrad_batched_reduce_of_four_layers(T):
    by = {c["name"]: c for c in R.CASES}
    layers = [("k3s2_9x7_132to136", 0, 0, 3, True), ("tr3_7x5_256to128", 1, 0, 2, False), ("tr1_rows70", 1, 3, None, True), ("k3s1_5x6_36to20", 2, 0, 5, False)]
    single, kws = [], []
    for name, prec, io, sk, scaled in layers:
        c = by[name]
        check_form(c, prec, io)
        x, dy = stored(c, io)
        kw = dict(prec=prec, splitk=sk, scale=(torch.rand(c["Cout"], device="cuda") + 0.5) if scaled else None)
        kws.append((c, x, dy, kw))
        single.append(wgrad(T, c, x, dy, **kw))
    defer = T.DeferredReduces(torch.device("cuda"))
    parked = [wgrad(T, c, x, dy, defer=defer, **kw) for c, x, dy, kw in kws]
    assert len(defer.items) == 4 and len({it.splitk for it in defer.items}) >= 3
    defer.flush()
    assert not defer.items
    for (name, *_), a, b in zip(layers, single, parked):
        assert torch.equal(bits(a), bits(b)), (name, "one flush of four parked layers differs from the per-launch reduce")


# ---------------------------------------------------------------------------------------------------------------------- column sums
def colsum_slicing(M):
    want = min(max(M // 512, 32), 256)
    rows_per = -(-M // want)
    return rows_per, -(-M // rows_per)


def colsum_scalar_bits(dy):
    """colsum_partial_kernel + colsum_final_kernel restated in numpy fp32: rows r0 + phase, step 4, per slice; the four phases as
    (p0 + p1) + (p2 + p3); the slices the same way."""
    M, Cc = dy.shape
    rows_per, slices = colsum_slicing(M)
    z = np.zeros(Cc, dtype=np.float32)

    def four(get, lo, hi):
        ph = []
        for sub in range(4):
            s = z.copy()
            for r in range(lo + sub, hi, 4):
                s = s + get(r)
            ph.append(s)
        return (ph[0] + ph[1]) + (ph[2] + ph[3])

    ws = np.stack([four(lambda r: dy[r], k * rows_per, min(M, (k + 1) * rows_per)) for k in range(slices)])
    return four(lambda k: ws[k], 0, slices)


def hold_colsum(label, what, out, dy64, M, prev=None):
    want = dy64.sum(0) + (prev.double() if prev is not None else 0.0)
    bound = R.c_law(M) * U * dy64.abs().sum(0) + (U * prev.double().abs() if prev is not None else 0.0)
    hold(label, what, out, want, bound)


@pytest.mark.parametrize("M", [1, 31, 33, 16383, 16385, 131585])
def test_colsum_law(T, M):
    assert colsum_slicing(131585) == (515, 256)  # past 256 * 512 rows the slice count stays at the workspace's 256
    g = torch.Generator(device="cuda").manual_seed(M)
    for Cc in ((4,) if M == 131585 else (3, 12, 15, 64, 260)):
        dy = torch.randn((M, Cc), device="cuda", generator=g)
        assert dy.data_ptr() % 16 == 0
        scalar = Cc % 4 != 0
        label = "colsum_partial_kernel" if scalar else "colsum_partial4_kernel<false>"
        out = torch.full((Cc,), 7.0, device="cuda")
        T.colsum(dy, out)
        hold_colsum(label, f"M {M} C {Cc}", out, dy.double(), M)
        if scalar:
            assert np.array_equal(out.cpu().numpy(), colsum_scalar_bits(dy.cpu().numpy())), (label, M, Cc, "not the documented summation order")
        prev = torch.randn(Cc, device="cuda", generator=g) * 100
        acc = prev.clone()
        T.colsum(dy, acc, accumulate=True)
        hold_colsum(label, f"M {M} C {Cc} accumulate", acc, dy.double(), M, prev)
        assert torch.equal(bits(acc), bits(prev + out))  # the same sum, one add
        if not scalar:
            d16 = dy.bfloat16()
            o16, o32 = torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
            T.colsum(d16, o16)
            hold_colsum("colsum_partial4_kernel<true>", f"M {M} C {Cc}", o16, d16.double(), M)
            T.colsum(d16.float(), o32)
            assert torch.equal(bits(o16), bits(o32)), ("colsum_bf16 differs from colsum on the widened values", M, Cc)


def test_colsum_off_alignment_takes_the_scalar_path(T):
    M, Cc = 16385, 8
    base = torch.randn(M * Cc + 1, device="cuda")
    dy = base[1:].view(M, Cc)  # a 4-byte offset: contiguous, C % 4 == 0, but no 16-byte loads
    assert dy.is_contiguous() and dy.data_ptr() % 16 == 4
    out = torch.empty(Cc, device="cuda")
    T.colsum(dy, out)
    hold_colsum("colsum_partial_kernel", f"M {M} C {Cc} +4 bytes", out, dy.double(), M)
    assert np.array_equal(out.cpu().numpy(), colsum_scalar_bits(dy.cpu().numpy())), "an unaligned pointer must take the scalar path's summation order"
    m_dev = torch.tensor([M], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        T.colsum_rows(dy, out, m_dev)
    with pytest.raises(RuntimeError):  # (colsum_rows has no scalar form at all)
        T.colsum_rows(torch.randn(33, 3, device="cuda"), torch.empty(3, device="cuda"), m_dev)


@pytest.mark.parametrize("M,Cc", [(1, 12), (33, 12), (16385, 12), (16385, 260)])
def test_colsum_rows_live_count(T, M, Cc):
    g = torch.Generator(device="cuda").manual_seed(M + Cc)
    dy = torch.randn((M, Cc), device="cuda", generator=g)
    full = torch.empty(Cc, device="cuda")
    T.colsum(dy, full)
    prev = torch.randn(Cc, device="cuda", generator=g)
    for count in (0, 1, M, M + 9, -3):
        live = min(max(count, 0), M)
        dyn = dy.clone()
        dyn[live:] = float("nan")
        m_dev = torch.tensor([count], dtype=torch.int32, device="cuda")
        out = torch.full((Cc,), 7.0, device="cuda")
        T.colsum_rows(dyn, out, m_dev)
        acc = prev.clone()
        T.colsum_rows(dyn, acc, m_dev, accumulate=True)
        if live == M:
            assert torch.equal(bits(out), bits(full)), (count, "the full count must give colsum's bits")
        elif live == 0:
            assert not bool(out.any()) and torch.equal(bits(acc), bits(prev)), count
        if live:
            hold_colsum("colsum_rows_partial4_kernel<false>", f"M {M} C {Cc} m_dev {count}", out, dy[:live].double(), live)
            hold_colsum("colsum_rows_partial4_kernel<false>", f"M {M} C {Cc} m_dev {count} accumulate", acc, dy[:live].double(), live, prev)
        d16 = dyn.bfloat16()
        o16, o32 = torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
        T.colsum_rows(d16, o16, m_dev)
        T.colsum_rows(d16.float(), o32, m_dev)
        assert torch.equal(bits(o16), bits(o32)), (count, "the bf16 form differs from the launch on the widened values")
        if live:
            hold_colsum("colsum_rows_partial4_kernel<true>", f"M {M} C {Cc} m_dev {count}", o16, d16[:live].double(), live)


# ------------------------------------------------------------------------------------------------------------------ filter transposes
def transposed(w, scale, Cout, k, Cin):
    """[Cout][k][k][Cin] -> [Cin][k][k][Cout], taps flipped, rows scaled: one fp32 product per element."""
    w4 = w.view(Cout, k, k, Cin)
    if scale is not None:
        w4 = w4 * scale[:, None, None, None]
    return w4.flip(1, 2).permute(3, 1, 2, 0).contiguous()


TRANSPOSE_SHAPES = [(20, 36, 3), (36, 20, 1), (132, 128, 3)]  # (Cout, Cin, k): 36 -> 20 k3, 20 -> 36 k1, 128 -> 132 k3


@pytest.mark.parametrize("shape", TRANSPOSE_SHAPES, ids=lambda s: f"{s[1]}to{s[0]}k{s[2]}")
@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
def test_weight_transpose_exact(T, shape, scaled):
    Cout, Cin, k = shape
    g = torch.Generator().manual_seed(Cout)
    w = torch.randn((Cout, k * k * Cin), generator=g)
    scale = (torch.rand(Cout, generator=g) + 0.5) if scaled else None
    out = torch.full((Cin * k * k * Cout,), 7.0, device="cuda")
    T.weight_transpose(w.cuda(), out, Cout, k, k, Cin, scale=None if scale is None else scale.cuda())
    assert torch.equal(out.cpu().view(Cin, k, k, Cout), transposed(w, scale, Cout, k, Cin))


def test_weight_transpose_batch_of_five(T):
    g = torch.Generator().manual_seed(5)
    shapes = [(12, 8, 1, True), (20, 36, 3, False), (36, 20, 1, True), (132, 128, 3, True), (16, 4, 1, False)]  # single-block items first and last
    assert all(((ci + 31) // 32) * ((co + 31) // 32) * k * k == 1 for co, ci, k, _ in (shapes[0], shapes[-1]))
    entries, singles = [], []
    for Cout, Cin, k, scaled in shapes:
        w = torch.randn((Cout, k * k * Cin), generator=g).cuda()
        sc = (torch.rand(Cout, generator=g) + 0.5).cuda() if scaled else None
        one = torch.full((Cin * k * k * Cout,), 7.0, device="cuda")
        T.weight_transpose(w, one, Cout, k, k, Cin, scale=sc)
        assert torch.equal(one.cpu().view(Cin, k, k, Cout), transposed(w.cpu(), None if sc is None else sc.cpu(), Cout, k, Cin))
        singles.append(one)
        entries.append((w, sc, torch.full_like(one, -3.0), Cout, k, k, Cin))
    tb = T.TransposeBatch(entries, torch.device("cuda"))
    assert tb.n == 5 and tb.blocks == sum(((ci + 31) // 32) * ((co + 31) // 32) * k * k for co, ci, k, _ in shapes)
    tb.run()
    for i, (one, e) in enumerate(zip(singles, entries)):
        assert torch.equal(bits(one), bits(e[2])), (i, shapes[i], "the batched transpose differs from the single launch")


@pytest.mark.parametrize("Cout,Cin", [(36, 20), (1024, 1028)])  # the second: more than 4096 x 256 filters, the grid stride is live
def test_wino_weight_transform_law(T, Cout, Cin):
    g = torch.Generator(device="cuda").manual_seed(Cout)
    w = torch.randn((Cout, 9 * Cin), device="cuda", generator=g)
    out = torch.full((16 * Cout * Cin,), 7.0, device="cuda")
    T.wino_weight_transform(w, out, Cout, Cin)
    G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64, device="cuda")
    g64 = w.double().view(Cout, 3, 3, Cin)
    want = torch.einsum("up,opqi,vq->uvoi", G, g64, G).reshape(16, Cout, Cin)
    S = torch.einsum("up,opqi,vq->uvoi", G.abs(), g64.abs(), G.abs()).reshape(16, Cout, Cin)
    hold("wino_weight_kernel", f"{Cout}x{Cin}", out.view(16, Cout, Cin), want, R.c_law(9) * U * S)


# ------------------------------------------------------------------------------------------------------------- spatial gradient plumbing
SPATIAL = [(2, 1, 1, 4), (2, 1, 2, 4), (2, 15, 20, 4), (2, 16, 21, 4), (1, 16, 21, 36), (2, 257, 256, 64)]  # the last: > 8192 x 256 float4s


@pytest.mark.parametrize("B,Ho,Wo,Cc", SPATIAL, ids=lambda v: str(v))
def test_zero_insert2_exact(T, B, Ho, Wo, Cc):
    if (Ho, Wo) == (257, 256):
        assert B * Ho * Wo * Cc // 4 > 8192 * 256
    g = torch.Generator(device="cuda").manual_seed(Ho * Wo)
    x = torch.randn((B, (Ho + 1) // 2, (Wo + 1) // 2, Cc), device="cuda", generator=g)
    want = torch.zeros((B, Ho, Wo, Cc), device="cuda")
    want[:, ::2, ::2] = x
    y = T.zero_insert2(x, Ho, Wo, out=torch.full((B, Ho, Wo, Cc), 7.0, device="cuda"))
    assert torch.equal(bits(y), bits(want))
    prev = torch.randn((B, Ho, Wo, Cc), device="cuda", generator=g)
    y = T.zero_insert2(x, Ho, Wo, out=prev.clone(), accumulate=True)
    assert torch.equal(bits(y), bits(prev + want))


@pytest.mark.parametrize("B,H,W,Cc", SPATIAL, ids=lambda v: str(v))
def test_sumpool2_add_exact(T, B, H, W, Cc):
    g = torch.Generator(device="cuda").manual_seed(H * W + 1)
    x = torch.randn((B, 2 * H, 2 * W, Cc), device="cuda", generator=g)
    y = torch.randn((B, H, W, Cc), device="cuda", generator=g)
    want = y + ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2]))  # the kernel's order, one fp32 add each
    T.sumpool2_add(x, y)
    assert torch.equal(bits(y), bits(want))


# ------------------------------------------------------------------------------------------------------------------------------ SGD
@pytest.mark.parametrize("n", [4, 1028, 8192 * 256 * 4 + 4])  # the last: one float4 past the grid of 8192 x 256 threads
def test_sgd_momentum_exact(T, n):
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731  (the kernel takes fp32 scalars)
    lr, mom, wd, gs = 0.02, 0.9, 1e-4, 0.5
    g = torch.Generator().manual_seed(n % 1000)
    p = torch.randn(n, generator=g)
    buf = torch.full((n,), float("nan"))  # `first` must not read it
    pd, bd = p.cuda(), buf.cuda()
    p16, b16 = p.cuda(), buf.cuda()   # the bf16-gradient kernel ...
    p32, b32 = p.cuda(), buf.cuda()   # ... against a3d_bf16_to_f32 + a3d_sgd_momentum
    pr, br = p.clone(), buf.clone()   # the same, restated on the host
    lib = L()
    for it in range(3):
        grad = torch.randn(n, generator=g)
        T.sgd_momentum(pd, grad.cuda(), bd, lr=lr, momentum=mom, weight_decay=wd, grad_scale=gs, first=it == 0)
        d = f32(gs) * grad + f32(wd) * p  # op by op, as -ffp-contract=off compiles it
        buf = d if it == 0 else f32(mom) * buf + d
        p = p - f32(lr) * buf
        assert torch.equal(bits(pd.cpu()), bits(p)) and torch.equal(bits(bd.cpu()), bits(buf)), (n, it, "a3d_sgd_momentum is not the op-by-op fp32 update")
        g16 = grad.cuda().bfloat16()
        T.sgd_momentum(p16, g16, b16, lr=lr, momentum=mom, weight_decay=wd, grad_scale=gs, first=it == 0)
        wide = torch.full((n,), 7.0, device="cuda")
        lib.check(lib.lib().a3d_bf16_to_f32(g16.data_ptr(), wide.data_ptr(), n, torch.cuda.current_stream().cuda_stream), "a3d_bf16_to_f32")
        assert torch.equal(bits(wide), bits(g16.float()))
        T.sgd_momentum(p32, wide, b32, lr=lr, momentum=mom, weight_decay=wd, grad_scale=gs, first=it == 0)
        assert torch.equal(bits(p16), bits(p32)) and torch.equal(bits(b16), bits(b32)), (n, it, "the bf16-gradient update differs from widen + update")
        d = f32(gs) * g16.float().cpu() + f32(wd) * pr
        br = d if it == 0 else f32(mom) * br + d
        pr = pr - f32(lr) * br
        assert torch.equal(bits(p16.cpu()), bits(pr)) and torch.equal(bits(b16.cpu()), bits(br)), (n, it)


def test_sgd_momentum_rejects_a_ragged_length(T):
    for dtype in (torch.float32, torch.bfloat16):
        p, buf = torch.zeros(6, device="cuda"), torch.zeros(6, device="cuda")
        with pytest.raises(RuntimeError):
            T.sgd_momentum(p, torch.ones(6, device="cuda", dtype=dtype), buf, lr=0.1, momentum=0.9, weight_decay=0.0)
        assert not bool(p.any())


# ------------------------------------------------------------------------------------------------------------------------- coverage
def test_every_weight_gradient_kernel_was_exercised():
    """Last in the file: every one of the fourteen weight-gradient kernels ran (form asserted, results checked) in the tests above.
    Meaningful after a run of the whole file in file order only (no -k selection, no reordering)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    print("\nworst err / bound per kernel label")
    for label in sorted(WORST):
        print(f"  {label:38s} {WORST[label]:.4f}")
    missing = [label for label in R.ALL_LABELS if label not in SEEN]
    assert not missing, "weight-gradient kernels not exercised by this file: " + ", ".join(missing)
    assert all(v <= 1.0 and math.isfinite(v) for v in WORST.values())
