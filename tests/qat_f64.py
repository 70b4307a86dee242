"""The reference's QAT forward formulas evaluated in float64, with every quantised value's distance from a rounding tie: the yardstick
the floating-point QAT kernels (csrc/bnm_qat.hip, csrc/bnm_qat_model.hip, csrc/bnm_qat_cnn.hip) are held to, shared by their GPU tests
and pinned to the reference module's own fixtures on CPU by tests/test_qat_cpu.py.  A plain helper module (torch tensors on any
device).

The formulas are qat.normalize / activation_quant / weight_quant / ste_formula / ste_conv_formula (BitNetMCU.py:119-177, 214-235,
284-305), rounded to float32 wherever the reference rounds - Normalize's denominator and quotient, activation_quant's scale and the
product it rounds to an integer (a float32 operation is a float64 one rounded once: exact for + - * / and sqrt) - and exact
elsewhere: the integer sums, the division by the two scales.

How a kernel output is judged (`within`): a kernel computes the same formula with float32 operations in another order, so a quantised
value whose float64 product lies within TIE of a rounding tie may land one step away in the kernel.  Per output:
  * every input of the output more than TIE from a tie: within `tight` of the reference (of the row's / plane's largest output);
  * otherwise, in addition, one quantisation step per near-tie input: |weight level| / (x_scale w_scale) for a linear layer,
    |tap| / x_scale for a convolution.
Weight levels (`kernel_levels`): the kernel's may differ from qat.weight_quant's only where perturbing w by a relative PERTURB changes
the reference quantiser's result (a rounding tie of a uniform grid, Binary's w == mean, FP130's powers of two, NF4's midpoints); the
layers are then evaluated with the kernel's own levels.
"""
import torch
import torch.nn.functional as F

from bitnetmcu_amd import qat

TIE = 5e-4
PERTURB = 1e-6
FC_TIGHT = 2e-5
CNN_TIGHT = 1e-5


def f32(t):
    """round a float64 tensor to float32 and back (one float32 rounding of an exact float64 result)"""
    return t.float().double()


# ---- weights -------------------------------------------------------------------------------------------------------------------
def _level(w, scale, mean, qt):
    """the per-weight part of qat.weight_quant (BitNetMCU.py:150-177) on float32 w with the tensor's scale and mean fixed"""
    v = w * scale
    if qt == "Ternary":
        return v.round().clamp(-1, 1)
    if qt == "Binary":
        return (w - mean).sign()
    if qt == "BinarySym":
        return w.sign()
    if qt == "2bitsym":
        return (v - 0.5).round().clamp(-2, 1) + 0.5
    if qt == "4bit":
        return (v - 0.01).round().clamp(-8, 7) + 0.01
    if qt == "4bitsym":
        return (v - 0.5).round().clamp(-8, 7) + 0.5
    if qt == "5bitsym":
        return (v - 0.5).round().clamp(-16, 15) + 0.5
    if qt == "8bit":
        return v.round().clamp(-128, 127)
    if qt == "FP130":
        return w.sign() * v.abs().log2().floor().clamp(0, 7).exp2()
    if qt == "NF4":
        levels = torch.tensor(qat.NF4_LEVELS, device=w.device)
        return levels[torch.argmin(torch.abs(v.unsqueeze(-1) - levels), dim=-1)]
    raise AssertionError(qt)


def reference_levels(w, s, qt):
    """qat.weight_quant in float32 -> (levels u, scale as a float64 tensor broadcastable against w, the levels of w (1 -+ PERTURB))"""
    w = w.float()
    s = torch.as_tensor(s, dtype=torch.float32, device=w.device)
    if s.numel() > 1:
        s = s.reshape(-1, *([1] * (w.dim() - 1)))
    else:
        s = s.reshape(())
    u, scale = qat.weight_quant(w, s, qt)
    scale = torch.as_tensor(scale, dtype=torch.float32, device=w.device)
    mean = w.mean()
    lo = _level(w * (1.0 - PERTURB), scale, mean, qt)
    hi = _level(w * (1.0 + PERTURB), scale, mean, qt)
    assert torch.equal(_level(w, scale, mean, qt), u), qt      # (the restatement above is weight_quant's own)
    return u, scale.double(), lo, hi


def kernel_levels(deq, w, s, qt):
    """The levels a kernel used, from its w_int / w_scale (`deq`, float32, w's shape): each must be the reference's level, or - where
    the perturbation rule allows it - the level of the perturbed weight.  No count allowance.  -> (levels f64, scale f64, changed)"""
    u, scale, lo, hi = reference_levels(w, s, qt)
    got = deq.double().reshape(w.shape) * scale
    cands = torch.stack([u, lo, hi]).double()
    dist = (got.unsqueeze(0) - cands).abs()
    best = dist.argmin(dim=0, keepdim=True)
    lev = cands.gather(0, best)[0]
    off = dist.gather(0, best)[0]
    assert bool((off <= 1e-4).all()), (qt, "a kernel level is neither the reference's nor a perturbed weight's",
                                        float(off.max()), int((off > 1e-4).sum()))
    return lev, scale, lev != u.double()


# ---- activation_quant ----------------------------------------------------------------------------------------------------------
def act_quant(xn):
    """activation_quant (BitNetMCU.py:119-128) per last-dimension row of float32 values held in float64 -> (x_int, scale, tie)"""
    with torch.no_grad():
        scale = f32(127.0 / xn.abs().amax(dim=-1, keepdim=True).clamp(min=1e-5))
        p = f32(xn * scale)
        xi = p.round().clamp(-128, 127)
        tie = (p - p.floor() - 0.5).abs()
    return xi, scale, tie


def normalize(x, nt):
    """BitLinear.Normalize (BitNetMCU.py:237-262) on float32 values held in float64: denominator and quotient rounded to float32.
    LayerNorm / BatchNorm: the row's / the batch's (per feature, dimension 0) statistics, the mean rounded to float32 before the
    float32 subtraction.  A NaN
    or an infinity reaches the result as it does in the reference's torch code (an all-zero row under RMS / Lin is 0 / 0 = NaN)."""
    if nt == "RMS":
        den = f32(torch.sqrt((x * x).mean(dim=1, keepdim=True)))
    elif nt == "Lin":
        den = f32(x.abs().mean(dim=1, keepdim=True))
    elif nt == "LayerNorm":
        mean = x.mean(dim=1, keepdim=True)
        den = f32(torch.sqrt(((x - mean) ** 2).mean(dim=1, keepdim=True) + 1e-5))
        x = f32(x - f32(mean))     # (the float32 mean: where the row's spread is far below its mean, its rounding is what counts)
    elif nt == "BatchNorm":
        mean = x.mean(dim=0, keepdim=True)
        den = f32(torch.sqrt(((x - mean) ** 2).mean(dim=0, keepdim=True) + 1e-5))
        x = f32(x - f32(mean))
    elif nt == "None":
        return x
    else:
        raise AssertionError(nt)
    return f32(x / den)


# ---- a BitLinear layer ---------------------------------------------------------------------------------------------------------
def fc_layer(x_in, levels, w_scale, nt, quant=True):
    """One BitLinear layer (BitNetMCU.py:214-235) from a float32 input [n, d] (any d: Normalize averages over the d values):
    levels [k, d] and w_scale (scalar, PerTensor, or [k, 1], PerOutput) float64 -> (y [n, k], tie [n, d], step [n, k]): y exact
    given the rounded quantities, tie the distance of every quantised product from a rounding tie, step the sum over the row's
    near-tie inputs of one quantisation step's effect on each output, |level| / (x_scale w_scale).  quant=False: QuantType 'None'
    (F.linear of the normalised input and the float32 weights `levels`; no tie, no step)."""
    x = x_in.double()
    with torch.no_grad():
        xn = normalize(x, nt)
        if not quant:
            return xn @ levels.t(), torch.full_like(xn, float("inf")), torch.zeros(x.shape[0], levels.shape[0], dtype=x.dtype,
                                                                                    device=x.device)
        xi, xs, tie = act_quant(xn)
        ws = w_scale.reshape(1, -1) if w_scale.numel() > 1 else w_scale.reshape(1, 1)
        y = (xi @ levels.t()) / xs / ws
        near = (tie <= TIE).double()
        step = (near @ levels.abs().t()) / xs / ws
    return y, tie, step


# ---- the convolution front (NormType 'None': activation_quant per image row) -----------------------------------------------------
def _conv3x3(xq, taps, step=None):
    """a 3x3 valid convolution of [n, C or 1, H, W] with per-channel taps [C, 9] as nine shifted multiply-adds in float64 (MIOpen has
    no float64 convolution); with `step` ([n, C or 1, H, W]: one quantisation step at near-tie inputs, else 0) also the bound term"""
    ho, wo = xq.shape[2] - 2, xq.shape[3] - 2
    t = taps.reshape(1, -1, 9, 1, 1)
    y = 0.0
    b = 0.0
    for k in range(9):
        dy, dx = divmod(k, 3)
        y = y + xq[:, :, dy:dy + ho, dx:dx + wo] * t[:, :, k]
        if step is not None:
            b = b + step[:, :, dy:dy + ho, dx:dx + wo] * t[:, :, k].abs()
    return y, b


def conv_layer(a, taps):
    """BitConv2d (BitNetMCU.py:284-305, NormType 'None', stride 1, no padding; conv1's single input plane or depthwise) on float32
    planes a [n, C or 1, H, W] held in float64: activation_quant per image row, taps [C, 9] = level / w_scale in float64
    -> (y [n, C, H-2, W-2], step [same]: one step per near-tie input times |tap|, tie [same as a])"""
    with torch.no_grad():
        xi, xs, tie = act_quant(a)
        near_step = (tie <= TIE).double() / xs
        y, step = _conv3x3(xi / xs, taps, near_step)
    return y, step, tie


def relu_pool(y):
    return F.max_pool2d(torch.relu(y), 2)


def cnn_taps(ws, ss, qts, kernel_taps=None):
    """[3][C, 9] float64 taps level / w_scale: the reference's levels, or the kernel's (its [3, C, 9] float32 taps w_int / w_scale)
    checked against the perturbation rule"""
    out = []
    for l in range(3):
        w = ws[l].float()
        if kernel_taps is None:
            u, scale, _, _ = reference_levels(w, ss[l], qts[l])
            lev = u.double()
        else:
            lev, scale, _ = kernel_levels(kernel_taps[l].reshape(w.shape), w, ss[l], qts[l])
        out.append((lev / scale).reshape(w.shape[0], 9))
    return out


def within(got, want, step, tight, what, cap=None, floor_rows=False, extra=None):
    """Per-output check of `got` against `want` (float64, rows = dimension 0): NaN exactly where `want` is NaN, an infinity exactly
    where `want` has the same one; elsewhere |got - want| <= tight x (the row's largest finite |want| + step) + step + extra - the
    kernel rounds at the size of what it computes, which is up to a step away from `want`; `extra` (optional, per output): a bound on
    the kernel's own float32 summation error where its terms do not sum exactly.  cap: every row's largest error within cap of its
    largest |want| (floor_rows: of max(that, a tenth of the median row maximum) - a row of one or two outputs can sit near zero).
    -> the largest ratio of error to allowance."""
    if want.shape[0] == 0:
        return 0.0
    got = got.double().reshape(want.shape[0], -1)
    want = want.reshape(want.shape[0], -1)
    step = step.reshape(want.shape[0], -1)
    nan_w, nan_g = torch.isnan(want), torch.isnan(got)
    assert torch.equal(nan_w, nan_g), (what, "NaN pattern", int((nan_w != nan_g).sum()))
    inf_w = torch.isinf(want)
    assert torch.equal(inf_w, torch.isinf(got)) and torch.equal(got[inf_w], want[inf_w]), (what, "infinities")
    fin = ~(nan_w | inf_w)      # (a row with a NaN is NaN throughout in a linear layer; a convolution plane may keep finite outputs)
    if not bool(fin.any()):
        return 0.0
    zero = torch.zeros_like(want)
    row_max = torch.where(fin, want, zero).abs().amax(dim=1, keepdim=True)
    err = torch.where(fin, (got - want).abs(), zero)
    s = torch.where(fin, step, zero)
    allowed = tight * (row_max + s) + s      # (a flipped step is |level| / (x_scale w_scale) in the kernel's own float32 scales)
    if extra is not None:
        allowed = allowed + torch.where(fin, extra.reshape(want.shape), zero)
    ratio = float((err / allowed.clamp(min=1e-300)).max())
    bad = err > allowed
    assert not bool(bad.any()), (what, "outside the derived bound", int(bad.any(dim=1).sum()), float((err - allowed).max()), ratio)
    if cap is not None:
        live = fin.any(dim=1, keepdim=True)
        scale = row_max
        if floor_rows:
            scale = torch.maximum(row_max, 0.1 * row_max[live].median())
        rel = err.amax(dim=1, keepdim=True) / scale.clamp(min=1e-30)
        assert bool((rel[live] <= cap).all()), (what, "above the cap", float(rel[live].max()))
    return ratio


# ---- a general BitConv2d --------------------------------------------------------------------------------------------------------
def conv2d_layer(x, taps, stride=1, pad=0, groups=1, nt="None", quant=True):
    """BitConv2d (BitNetMCU.py:284-322) of float32 planes x [n, cin, h, w] held in float64, with taps [cout, cin / groups, kh, kw]
    float64 = level / w_scale (quant=False, QuantType 'None': the float32 weights), any groups, square stride, symmetric zero padding:
    Normalize ('RMS' over each plane, :306-308, or 'None'), activation_quant per image row BEFORE padding, zero padding after it,
    then the convolution as im2col (F.unfold) and a float64 product (MIOpen has no float64 convolution)
    -> (y [n, cout, ho, wo], step [same]: one quantisation step per near-tie input times |tap|, absum [same]: sum |x_q tap|)."""
    a = x.double()
    cout, cig, kh, kw = taps.shape
    with torch.no_grad():
        if nt == "RMS":
            a = f32(a / f32(torch.sqrt((a * a).mean(dim=(2, 3), keepdim=True))))
        elif nt != "None":
            raise AssertionError(nt)
        if quant:
            xi, xs, tie = act_quant(a)
            xq, near = xi / xs, (tie <= TIE).double() / xs
        else:
            xq, near = a, torch.zeros_like(a)
        n, cin, h, wd = a.shape
        ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
        t = taps.double().reshape(groups, cout // groups, cig * kh * kw)

        def conv(v, tt):
            cols = F.unfold(F.pad(v, (pad, pad, pad, pad)), (kh, kw), stride=stride).reshape(n, groups, cig * kh * kw, ho * wo)
            return torch.einsum("gok,ngkl->ngol", tt, cols).reshape(n, cout, ho, wo)

        y = conv(xq, t)
        step = conv(near, t.abs())
        absum = conv(xq.abs(), t.abs())
    return y, step, absum


def conv_allowance(absum, taps):
    """The kernel's own float32 error on top of CNN_TIGHT: it keeps x_int / x_scale and level / w_scale as rounded floats and
    accumulates d = cig kh kw products with fmaf, so (d + 2) roundings of at most 2^-24 of sum |x_q tap| per output"""
    d = taps.shape[1] * taps.shape[2] * taps.shape[3]
    return (d + 2) * 2.0 ** -24 * absum


def plane_rows(t):
    """[n, c, ho, wo] -> [n c, ho wo]: one row per (image, channel) plane, the unit `within` scales CNN_TIGHT by"""
    return t.reshape(t.shape[0] * t.shape[1], -1)


# ---- whole forward passes --------------------------------------------------------------------------------------------------------
def fc_chain(x, levels, w_scales, nt):
    """FCMNIST's forward (models.py:70-90) from x [n, d] in float64, every layer's output rounded to float32 as F.linear's is
    -> (outputs per layer - hidden ones after ReLU -, rows whose quantised products are all more than TIE from a tie in every layer)"""
    h = x.double()
    outs = []
    clean = torch.ones(h.shape[0], dtype=torch.bool, device=h.device)
    for l, (lev, sc) in enumerate(zip(levels, w_scales)):
        y, tie, _ = fc_layer(h, lev, sc, nt)
        clean &= (tie > TIE).all(dim=1)
        y = f32(y if l + 1 == len(levels) else torch.relu(y))
        outs.append(y)
        h = y
    return outs, clean


def _any3x3(m):
    ho, wo = m.shape[2] - 2, m.shape[3] - 2
    out = torch.zeros_like(m[:, :, :ho, :wo])
    for k in range(9):
        dy, dx = divmod(k, 3)
        out |= m[:, :, dy:dy + ho, dx:dx + wo]
    return out


def _any2x2(m):
    return m[:, :, 0::2, 0::2] | m[:, :, 0::2, 1::2] | m[:, :, 1::2, 0::2] | m[:, :, 1::2, 1::2]


def front_chain(x, taps):
    """CNNMNIST's convolution front (models.py:109-119) from images [n, 1, 16, 16] in float64, every convolution's output rounded to
    float32 -> (y1, y2, y3, features [n, 4 C], clean [n, 4 C]).  A feature is clean when no quantised value it depends on lies within
    TIE of a tie: none in the 3x3 windows behind it, and - since a changed value can be its row's maximum, which scales the whole
    row's quantisation - none anywhere in an image row that one of those windows reads."""
    a = x.double().reshape(-1, 1, 16, 16)
    dirty = torch.zeros(a.shape, dtype=torch.bool, device=a.device)
    ys = []
    for l in range(3):
        y, _, tie = conv_layer(a, taps[l])
        dirty = _any3x3(dirty.any(dim=3, keepdim=True).expand_as(dirty) | (tie <= TIE))
        y = f32(y)
        ys.append(y)
        if l == 0:
            a = torch.relu(y)
        else:
            a, dirty = relu_pool(y), _any2x2(dirty)
    return ys[0], ys[1], ys[2], a.flatten(1), ~dirty.flatten(1)


# ---- the per-layer GPU op (csrc/bnm_qat.hip) judged output by output ---------------------------------------------------------------
# QuantTypes whose products x_int * level sum exactly in float32 (integers or half-integers, |sum| <= 2^24): the kernel's y is its exact
# sum divided by its two scales, two float32 roundings
EXACT_SUM = ("Binary", "BinarySym", "Ternary", "2bitsym", "4bitsym", "5bitsym", "8bit", "FP130")
U = 2.0 ** -24          # the unit roundoff of float32
XSCALE_ULPS = 8         # x_scale: the kernel sums the row's squares / absolute values in another order than the reference


def _ulp32(v):
    """the spacing of float32 at |v| (float64 tensor in, float64 tensor out)"""
    a = v.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def workspace_levels(device, d, k):
    """the levels uT [dpad][kpad] -> [k, d] and w_scale [k] the last per-layer call of shape (d, k) on this stream used (float32)"""
    ws = qat._workspaces[(device.index, torch.cuda.current_stream(device).cuda_stream, d, k)]
    dpad, kpad = (d + 1) & ~1, (k + 31) & ~31
    return ws[:dpad * kpad].reshape(dpad, kpad)[:d, :k].t().contiguous(), ws[dpad * kpad:dpad * kpad + k].clone()


def _check_weights(w, s, qt, wdq, u_ws, wsc_ws):
    """the kernel's levels (workspace) and w_int / w_scale (return_w_deq, what the backward consumes) per weight -> (levels, scale) f64"""
    if qt == "None":
        assert torch.equal(wdq, w) and torch.equal(u_ws, w.reshape(u_ws.shape)), "QuantType None: the weights themselves"
        return w.double(), torch.ones((), dtype=torch.float64, device=w.device)
    lev, scale, _ = kernel_levels(wdq, w, s, qt)
    lev2 = lev.reshape(u_ws.shape)
    assert torch.equal(u_ws.double(), lev2), (qt, "workspace levels differ from w_int / w_scale's", int((u_ws.double() != lev2).sum()))
    want_sc = scale.reshape(-1).expand(u_ws.shape[0])
    tol = 2 * _ulp32(want_sc) if qt == "Ternary" else 0.0      # (Ternary: mean|w| summed in another order)
    assert bool(((wsc_ws.double() - want_sc).abs() <= tol).all()), (qt, "w_scale")
    deq = (u_ws.double() / wsc_ws.double()[:, None]).float()       # (53 >= 2 x 24 + 2 bits: the float32 quotient, correctly rounded)
    assert torch.equal(wdq.reshape(deq.shape), deq), (qt, "w_deq is not level / w_scale in float32", int((wdq.reshape(deq.shape) != deq).sum()))
    return lev, scale


def check_bitlinear(x, w, s, qt, nt, what=""):
    """qat.bitlinear_forward on x [n, d], w [k, d], s (scalar or [k]) against the float64 layer, every element:
      * weights: the workspace's levels and w_scale and return_w_deq (= level / w_scale in float32), per weight (`kernel_levels`);
      * activations: x_int equals the float64 act_quant value, or lies +-1 from it where that value is within TIE of a tie; x_scale
        within XSCALE_ULPS float32 ulps; NaN exactly where the float64 evaluation has it;
      * self-consistency: y against the exact value of the kernel's OWN x_int, x_scale, levels and w_scale - within 4 U of it for the
        exactly summed types (an exact 0 gives 0), plus (d + 1) U sum |x_int level| / (x_scale w_scale) for '4bit' / 'NF4';
      * end to end: y within FC_TIGHT of the float64 layer (with the kernel's levels) on every row, plus a step per near-tie input.
    -> the largest ratio of error to allowance of the end-to-end check"""
    n, d = x.shape
    k = w.shape[0]
    quant = qt != "None"
    out = qat.bitlinear_forward(x, w, s, qt, nt, return_int=quant, return_w_deq=True)
    y, wdq = out[0], out[-1]
    torch.cuda.synchronize()
    u_ws, wsc_ws = workspace_levels(x.device, d, k)
    lev, scale = _check_weights(w, s, qt, wdq, u_ws, wsc_ws)
    lev = lev.reshape(k, d)
    y64, tie, step = fc_layer(x, lev, scale, nt, quant)
    y = y.double()
    if not quant:
        xn = normalize(x.double(), nt)
        extra = (d + 8) * U * (xn.abs() @ lev.abs().t())        # (the kernel's normalised values carry a few roundings of their own)
        return within(y, y64, step, FC_TIGHT, (what, qt, nt), extra=extra)
    xi, xs = out[1].double(), out[2].double()
    xi64, xs64, tie = act_quant(normalize(x.double(), nt))
    xs64 = xs64.reshape(-1)
    assert torch.equal(torch.isnan(xs), torch.isnan(xs64)), (what, qt, nt, "x_scale NaN pattern")
    assert torch.equal(torch.isnan(xi), torch.isnan(xi64)), (what, qt, nt, "x_int NaN pattern")
    f = ~torch.isnan(xs64)
    assert bool(((xs[f] - xs64[f]).abs() <= XSCALE_ULPS * _ulp32(xs64[f])).all()), (what, qt, nt, "x_scale",
                                                                                    float(((xs[f] - xs64[f]).abs() / _ulp32(xs64[f])).max()))
    fi = ~torch.isnan(xi64)
    dx = (xi - xi64).abs()
    assert bool((dx[fi & (tie > TIE)] == 0).all()) and bool((dx[fi] <= 1).all()), (what, qt, nt, "x_int", int((dx[fi] != 0).sum()))
    # self-consistency on the rows the kernel computed finitely
    rows = torch.isfinite(xs) & (xs != 0) & torch.isfinite(xi).all(dim=1)
    ws = wsc_ws.double()[None, :] if scale.numel() > 1 else wsc_ws.double()[:1][None, :]
    exact = (xi[rows] @ u_ws.double().t()) / xs[rows, None] / ws
    allowed = 4 * U * exact.abs()
    if qt not in EXACT_SUM:
        allowed = allowed + (d + 1) * U * (xi[rows].abs() @ u_ws.double().abs().t()) / xs[rows, None] / ws
    err = (y[rows] - exact).abs()
    assert bool((err <= allowed).all()), (what, qt, nt, "y against the kernel's own operands", int((err > allowed).sum()),
                                          float((err / allowed.clamp(min=1e-300)).max()))
    ws64 = scale.reshape(1, -1) if scale.numel() > 1 else scale.reshape(1, 1)
    extra = None if qt in EXACT_SUM else (d + 1) * U * (xi64.abs() @ lev.abs().t()) / xs64[:, None] / ws64
    return within(y, y64, step, FC_TIGHT, (what, qt, nt), extra=extra)


def check_bitconv2d(x, w, s, qt, nt, stride=1, pad=0, groups=1, what=""):
    """qat.bitconv2d_forward against the float64 convolution with the kernel's own levels (workspace, `kernel_levels`), every output,
    per (image, channel) plane: CNN_TIGHT of the plane's largest |y| + (d + 2) U sum |x_q tap| + one step per near-tie input;
    NaN exactly where the float64 evaluation has it.  -> the largest ratio of error to allowance"""
    y = qat.bitconv2d_forward(x, w, s, qt, nt, stride, (pad, pad), groups)
    torch.cuda.synchronize()
    cout, cig, kh, kw = w.shape
    u_ws, wsc_ws = workspace_levels(x.device, cig * kh * kw, cout)
    if qt == "None":
        assert torch.equal(u_ws, w.reshape(cout, -1))
        taps = w.double()
    else:
        lev, scale, _ = kernel_levels((u_ws.double() / wsc_ws.double()[:, None]).float(), w, s, qt)
        taps = lev / scale
    y64, step, absum = conv2d_layer(x, taps, stride, pad, groups, nt, qt != "None")
    assert y.shape == y64.shape, (what, tuple(y.shape), tuple(y64.shape))
    return within(plane_rows(y), plane_rows(y64), plane_rows(step), CNN_TIGHT, (what, qt, nt),
                  extra=plane_rows(conv_allowance(absum, taps)))
