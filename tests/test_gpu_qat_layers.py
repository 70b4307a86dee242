"""The per-layer QAT forward kernels (csrc/bnm_qat.hip: qat_bitlinear_fwd_kernel, qat_bitconv2d_fwd_kernel and their weight-quant /
batch-statistics launches) fuzzed over shapes, QuantTypes and NormTypes, and driven through their boundaries, every output judged
against the float64 evaluation of the reference's formulas (tests/qat_f64.py: check_bitlinear, check_bitconv2d).

BitLinear: the int8 matrix path on both sides of its LDS switch (d = 1018 is the widest it takes, 1019 the narrowest the float path
takes), 1 to 9 output tiles of 32 (the wave loop wraps at 5), batches across many workgroups, PerTensor and PerOutput clipping scalars,
all-zero / constant / one-hot / tied-maximum / non-finite rows.  BitConv2d: planes wider than a wavefront, RMS planes over 256 values,
strides that leave part of the padded plane unread, padding wider than a 1 x 1 kernel, the 160 KiB LDS limit from both sides,
thousands of workgroups, all-zero and constant planes.
"""
import pytest
import torch

import bitnetmcu_amd as b
from bitnetmcu_amd import qat
import qat_f64

pytestmark = pytest.mark.gpu
QUANTS = ["Binary", "BinarySym", "Ternary", "2bitsym", "4bit", "4bitsym", "FP130", "NF4", "5bitsym", "8bit", "None"]
NORMS = ["RMS", "Lin", "BatchNorm", "LayerNorm", "None"]
INT8 = ["Binary", "BinarySym", "Ternary", "2bitsym", "4bitsym", "5bitsym", "8bit"]      # qat_i8_factor != 0
SPECIALS = ["zero", "const", "onehot", "twomax", "+inf", "-inf", "nan"]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    """after the module: the largest error / allowance ratio each kernel and QuantType reached (run with -s to see the headroom)"""
    yield
    for key in sorted(WORST, key=str):
        print(f"\nworst within ratio {key}: {WORST[key]:.3g}", end="")


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def rows(n, d, g, scale_span=3.0):
    """n rows of d standard normals, each row scaled by 10^U(-span, span)"""
    x = torch.randn(n, d, generator=g)
    return (x * 10.0 ** ((torch.rand(n, 1, generator=g) * 2 - 1) * scale_span)).cuda()


def special_row(kind, d, g):
    r = torch.zeros(d)
    if kind == "const":
        r[:] = 0.75                     # (a dyadic constant: any order of summation is exact, so the row mean is too)
    elif kind == "onehot":
        r[int(torch.randint(d, (1,), generator=g))] = -3.0
    elif kind == "twomax":
        r = torch.randn(d, generator=g).clamp(-2, 2)
        r[int(torch.randint(d, (1,), generator=g))] = 5.0
        r[int(torch.randint(d, (1,), generator=g))] = -5.0
    elif kind in ("+inf", "-inf", "nan"):
        r = torch.randn(d, generator=g)
        r[int(torch.randint(d, (1,), generator=g))] = float(kind)
    return r.cuda()


def weights(k, d, g, per_output):
    w = (torch.randn(k, d, generator=g) * 0.05).cuda()
    s = w.abs().mean(dim=1) / 0.25 if per_output else w.abs().mean() / 0.25
    return w, s


def run_linear(x, w, s, qt, nt, what):
    if x.shape[0] == 0:
        y = qat.bitlinear_forward(x, w, s, qt, nt)
        assert y.shape == (0, w.shape[0])
        return
    _note(("linear", qt), qat_f64.check_bitlinear(x, w, s, qt, nt, what))


# ---- BitLinear -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 31, 33, 64, 65, 202, 511, 1017, 1018, 1019, 1024])
def test_bitlinear_widths_across_the_int8_switch(d, gpu_ok):
    """every QuantType at each width (every int8-eligible one on both sides of the int8 / float switch), output counts of 1 to 9
    tiles, batches of 1 to 33 rows, the NormTypes and both clipping-scalar kinds in rotation"""
    g = torch.Generator().manual_seed(1000 + d)
    ks = [1, 31, 32, 33, 129, 130, 257]
    ns = [1, 31, 32, 33]
    for i, qt in enumerate(QUANTS):
        k, n, nt = ks[(i + d) % len(ks)], ns[(i + d) % len(ns)], NORMS[(i + d) % len(NORMS)]
        w, s = weights(k, d, g, per_output=bool(i % 2))
        run_linear(rows(n, d, g), w, s, qt, nt, ("widths", d, k, n))
    if d >= 1017:       # the int8 path's widest tiles with 5 and 9 output tiles: the wave loop wraps
        for qt in INT8:
            for k in (130, 257):
                w, s = weights(k, d, g, per_output=True)
                run_linear(rows(40, d, g), w, s, qt, "RMS", ("wrap", d, k))


def test_bitlinear_every_quant_and_norm_type(gpu_ok):
    """all 11 QuantTypes x 5 NormTypes at one odd width with 5 output tiles and a partial last row tile"""
    g = torch.Generator().manual_seed(7)
    for qt in QUANTS:
        for j, nt in enumerate(NORMS):
            w, s = weights(130, 77, g, per_output=bool(j % 2))
            run_linear(rows(45, 77, g), w, s, qt, nt, ("grid",))


@pytest.mark.parametrize("seed", range(24))
def test_bitlinear_fuzz(seed, gpu_ok):
    g = torch.Generator().manual_seed(5000 + seed)
    pick = lambda seq: seq[int(torch.randint(len(seq), (1,), generator=g))]
    d = pick([1, 2, 31, 33, 64, 65, 202, 511, 1017, 1018, 1019, 1024, int(torch.randint(1, 1025, (1,), generator=g))])
    k = pick([1, 31, 32, 33, 129, 130, 257, int(torch.randint(1, 300, (1,), generator=g))])
    n = pick([0, 1, 31, 32, 33, 3000 + seed, int(torch.randint(1, 200, (1,), generator=g))])
    qt, nt = pick(QUANTS), pick(NORMS)
    w, s = weights(k, d, g, per_output=bool(seed % 2))
    x = rows(n, d, g)
    if n >= 8 and nt != "BatchNorm":         # (under BatchNorm a non-finite value spoils its whole column: see the test below)
        for i, kind in enumerate(SPECIALS):
            x[i] = special_row(kind, d, g)
    run_linear(x, w, s, qt, nt, ("fuzz", seed, d, k, n))


@pytest.mark.parametrize("nt", ["RMS", "Lin", "LayerNorm", "None"])
def test_bitlinear_special_rows(nt, gpu_ok):
    """all-zero, constant, one-hot, tied-maximum, +inf, -inf and NaN rows beside ordinary ones, on the int8 path (8bit, 2bitsym: d =
    202, 1018), the float path (8bit at d = 1019; 4bit, NF4, FP130) and QuantType None: NaN where the float64 evaluation has it - y,
    x_int, x_scale -, everything else to the usual bounds"""
    g = torch.Generator().manual_seed(11)
    for d, qts in ((202, ["8bit", "2bitsym", "4bit", "NF4", "FP130", "None"]), (1018, ["8bit"]), (1019, ["8bit", "Ternary"])):
        for qt in qts:
            x = rows(40, d, g)
            for i, kind in enumerate(SPECIALS):
                x[3 * i + 1] = special_row(kind, d, g)
            w, s = weights(70, d, g, per_output=qt in ("2bitsym", "8bit"))
            run_linear(x, w, s, qt, nt, ("special", d))


def test_bitlinear_batchnorm_edges(gpu_ok):
    """BatchNorm over one row (variance 0: every normalised value 0), with a constant column, and with a column holding an infinity
    or a NaN (every row's NaN, as the reference's batch statistics make it)"""
    g = torch.Generator().manual_seed(13)
    for qt in ("8bit", "4bitsym", "NF4", "None"):
        w, s = weights(33, 65, g, per_output=False)
        run_linear(rows(1, 65, g), w, s, qt, "BatchNorm", ("bn n=1",))
        x = rows(50, 65, g)
        x[:, 7] = 0.75
        run_linear(x, w, s, qt, "BatchNorm", ("bn const column",))
        for bad in (float("inf"), float("nan")):
            x = rows(5, 65, g)
            x[2, 40] = bad
            run_linear(x, w, s, qt, "BatchNorm", ("bn non-finite",))


# ---- BitConv2d ---------------------------------------------------------------------------------------------------------------------
# (n, cin, cout, groups, h, w, (kh, kw), stride, pad, QuantType, NormType)
CONV = [
    (2, 3, 6, 1, 70, 90, (3, 3), 1, 1, "8bit", "RMS"),            # a plane wider than 64 (two lane trips), 6300 values under RMS
    (3, 4, 8, 2, 20, 17, (3, 5), 2, 2, "4bitsym", "None"),         # (h + 2p - kh) not a multiple of the stride
    (4, 6, 6, 6, 23, 29, (5, 5), 3, 2, "Ternary", "RMS"),          # depthwise, stride 3
    (2, 2, 4, 1, 9, 9, (1, 1), 1, 2, "2bitsym", "None"),           # corner outputs read only padding
    (2, 6, 9, 3, 31, 33, (3, 3), 2, 0, "FP130", "RMS"),
    (2, 4, 4, 2, 16, 70, (3, 5), 1, 1, "None", "RMS"),             # QuantType None
    (1, 2, 4, 1, 40, 41, (5, 5), 3, 0, "NF4", "None"),
    (256, 16, 16, 16, 12, 12, (3, 3), 1, 1, "8bit", "RMS"),        # 4096 workgroups
    (1, 1, 16, 1, 202, 202, (3, 3), 1, 0, "8bit", "RMS"),          # 163,792 B of LDS: 48 B under the limit
]


def conv_weights(cout, cig, kh, kw, g):
    w = (torch.randn(cout, cig, kh, kw, generator=g) * 0.3).cuda()
    return w, w.abs().mean() / 0.25


def planes(n, c, h, w, g):
    x = torch.randn(n, c, h, w, generator=g)
    return (x * 10.0 ** ((torch.rand(n, c, 1, 1, generator=g) * 4 - 2))).cuda()


def run_conv(x, w, s, qt, nt, stride, pad, groups, what):
    _note(("conv", qt), qat_f64.check_bitconv2d(x, w, s, qt, nt, stride, pad, groups, what))


@pytest.mark.parametrize("case", CONV, ids=lambda c: "x".join(map(str, c[4:6])) + f"_{c[9]}_{c[10]}")
def test_bitconv2d_shapes(case, gpu_ok):
    n, cin, cout, groups, h, wd, (kh, kw), stride, pad, qt, nt = case
    g = torch.Generator().manual_seed(h * 1000 + wd)
    w, s = conv_weights(cout, cin // groups, kh, kw, g)
    run_conv(planes(n, cin, h, wd, g), w, s, qt, nt, stride, pad, groups, case)


def test_bitconv2d_lds_limit_is_refused_just_over(gpu_ok):
    """the LDS limit case above with two more output channels (163,864 B) is refused, not launched"""
    g = torch.Generator().manual_seed(3)
    w, s = conv_weights(18, 1, 3, 3, g)
    with pytest.raises(b.BnmError):
        qat.bitconv2d_forward(planes(1, 1, 202, 202, g), w, s, "8bit", "RMS", 1, (0, 0), 1)


@pytest.mark.parametrize("seed", range(12))
def test_bitconv2d_fuzz(seed, gpu_ok):
    g = torch.Generator().manual_seed(9000 + seed)
    pick = lambda seq: seq[int(torch.randint(len(seq), (1,), generator=g))]
    kh, kw = pick([(1, 1), (3, 3), (5, 5), (3, 5)])
    stride, pad = pick([1, 2, 3]), pick([0, 1, 2])
    groups = pick([1, 2, 3, 4])
    cig, cog = pick([1, 2, 3]), pick([1, 2, 3])
    if seed % 3 == 0:
        cig, cog = 1, 1                    # depthwise
    h = max(int(torch.randint(5, 41, (1,), generator=g)), kh)
    wd = max(int(torch.randint(5, 81, (1,), generator=g)), kw)
    n = int(torch.randint(1, 6, (1,), generator=g))
    qt, nt = pick(QUANTS), pick(["RMS", "None"])
    w, s = conv_weights(cog * groups, cig, kh, kw, g)
    run_conv(planes(n, cig * groups, h, wd, g), w, s, qt, nt, stride, pad, groups, ("fuzz", seed))


def test_bitconv2d_special_planes(gpu_ok):
    """an all-zero plane under RMS (0 / 0: NaN in every output that reads it, as in the reference), a constant plane, and under
    NormType None an image row holding an infinity (its activation_quant is 0 / 0) - on full, grouped and depthwise layers"""
    g = torch.Generator().manual_seed(17)
    for groups, cin, cout, qt in ((1, 3, 4, "8bit"), (2, 4, 6, "4bitsym"), (4, 4, 4, "Ternary")):
        for nt in ("RMS", "None"):
            x = planes(3, cin, 12, 70, g)
            x[0, 1] = 0.0
            x[1, 2] = 0.75
            if nt == "None":
                x[2, 0, 5, 33] = float("inf")
            w, s = conv_weights(cout, cin // groups, 3, 3, g)
            for pad in (0, 2):
                run_conv(x, w, s, qt, nt, 1, pad, groups, ("special", groups, nt, pad))
