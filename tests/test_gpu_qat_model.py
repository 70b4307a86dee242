"""Whole-model QAT forward on the GPU: csrc/bnm_qat_model.hip through the C ABI against
fixtures generated from the reference's own FCMNIST module (tests/golden/make_qat_model_golden.py).

This is a FLOATING-POINT kernel, so parity is within tolerance, and the tolerances are:
  * w_int / w_scale per layer: equal to the reference's, except at most 0.2 % of the weights where the value being rounded lies at a
    rounding tie (an ulp of the scale);
  * LAYER BY LAYER, each layer fed with the KERNEL'S OWN input of that layer (so that one flipped activation step cannot cascade):
    the layer's outputs equal a float64 evaluation of the reference's formula - Normalize, activation_quant, the exact integer
    product, / x_scale / w_scale, ReLU - within 2e-5 of the row's largest output, on every row all of whose quantised activations sit
    more than 5e-4 away from a rounding tie (at least half of the rows: a row has up to 256 activations), and within one activation
    step of one input (3e-2) on the rest;
  * END TO END against the reference module's float32 logits and hidden activations: at least 90 % of the rows within 5e-4 of the
    row's largest value, every row within 6e-2 (a flipped activation step somewhere in four layers);
  * the all-zero row: NaN logits, as the reference's 0 / 0 produces;
  * gradients through the module: median error 2e-3 of the largest entry, every entry within 0.15 (a flipped step or a ReLU mask
    that flipped at an exact zero moves one row's contribution by a discrete amount).
The random-shape fuzzes and the dynamic-batch test judge every output, not a count of rows (`check_derived`, tests/qat_f64.py): a
bound derived per output from the float64 evaluation's distances to rounding ties - 2e-5 of the row's largest output plus one
activation step for each input that lies within 5e-4 of a tie - on the kernel's own input of every layer, and 2e-5 end to end on every
row that is tie-clean through the whole chain.
"""
import os

import numpy as np
import pytest
import torch

import bitnetmcu_amd as b
from bitnetmcu_amd import qat
import qat_f64
import util

pytestmark = pytest.mark.gpu
GM = util.qat_model_golden()
CONFIGS = {"a": ("4bitsym", "RMS"), "b": ("4bitsym", "RMS"), "c": ("Ternary", "Lin"), "d": ("8bit", "RMS"), "e": ("2bitsym", "RMS"),
           "f": ("Binary", "RMS"), "g": ("4bitsym", "LayerNorm"), "h": ("8bit", "LayerNorm"),
           "i": ("Binary", "RMS"), "j": ("4bitsym", "Lin"), "k": ("8bit", "LayerNorm")}      # i - k: hidden widths 129 .. 192 (six tiles)
ZERO_ROW = 5
TIE = qat_f64.TIE


def case(tag):
    w1, w2, w3, ncls = (int(v) for v in GM[f"{tag}/cfg"])
    nl = 4 if w3 else 3
    ws = [torch.from_numpy(GM[f"{tag}/w{l}"]).cuda() for l in range(nl)]
    ss = [torch.from_numpy(GM[f"{tag}/s{l}"]).cuda() for l in range(nl)]
    widths = [256, w1, w2] + ([w3] if w3 else []) + [ncls]
    return torch.from_numpy(GM[f"{tag}/x"]).cuda(), ws, ss, widths


def check(tag, n_rows=None):
    qt, nt = CONFIGS[tag]
    x, ws, ss, widths = case(tag)
    if n_rows is not None:
        x = x[:n_rows]
    n = x.shape[0]
    nl = len(ws)
    assert qat.fc_model_supported(widths, [qt] * nl, nt)
    logits, hidden, wdq = qat.fc_model_forward(x.reshape(n, 1, 16, 16), ws, ss, [qt] * nl, nt, return_hidden=True, return_w_deq=True)
    plain = qat.fc_model_forward(x, ws, ss, [qt] * nl, nt)          # without the optional outputs: the same logits
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(plain, nan=-7.0), torch.nan_to_num(logits, nan=-7.0))
    logits, hidden = logits.cpu().numpy(), hidden.cpu().numpy()
    rows = np.ones(n, bool)
    if n > ZERO_ROW and nt != "LayerNorm":      # (LayerNorm's epsilon keeps the all-zero row finite: it is checked like any other)
        rows[ZERO_ROW] = False
        assert np.isnan(logits[ZERO_ROW]).all(), tag
    assert not np.isnan(logits[rows]).any() and not np.isnan(hidden[rows]).any(), tag
    # ---- weights ----
    levels, wscales = [], []
    for l in range(nl):
        ref_u, ref_sc = GM[f"{tag}/w_int{l}"].astype(np.float64), GM[f"{tag}/w_scale{l}"].astype(np.float64)
        sc = ref_sc if ref_sc.size > 1 else np.full(ref_u.shape[0], ref_sc[0])
        got = wdq[l].cpu().numpy().astype(np.float64) * sc[:, None]
        bad = np.abs(got - ref_u) > 1e-4
        assert bad.mean() <= 2e-3, (tag, l, bad.mean())
        lev, wsc, _ = qat_f64.kernel_levels(wdq[l], ws[l], ss[l], qt)      # the kernel's own levels where a tie flipped
        levels.append(lev)
        wscales.append(wsc)
    # ---- layer by layer on the kernel's own inputs ----
    offs = np.concatenate([[0], np.cumsum(widths[1:-1])])
    xin = x
    for l in range(nl):
        y, tie, _ = qat_f64.fc_layer(xin, levels[l], wscales[l], nt)
        y, tie = y.cpu().numpy(), tie.cpu().numpy()
        last = l == nl - 1
        got = logits if last else hidden[:, offs[l]:offs[l + 1]]
        want = y if last else np.maximum(y, 0.0)
        err = np.abs(got - want)[rows].max(axis=1) / np.maximum(np.abs(want)[rows].max(axis=1), 1e-30)
        clean = (tie[rows] > TIE).all(axis=1)
        assert clean.mean() >= 0.5 or n < 40, (tag, l, clean.mean())
        assert (err[clean] <= 2e-5).all(), (tag, l, err[clean].max())
        assert (err <= 3e-2).all(), (tag, l, err.max())
        xin = torch.from_numpy(got).to(x.device)
    # ---- end to end against the reference module ----
    for got, ref in ((logits, GM[f"{tag}/logits"][:n]), (hidden, GM[f"{tag}/hidden"][:n])):
        scale = np.maximum(np.abs(ref[rows]).max(axis=1), 1e-30)
        err = np.abs(got - ref)[rows].max(axis=1) / scale
        assert (err <= 5e-4).mean() >= 0.9 and err.max() <= 6e-2, (tag, (err <= 5e-4).mean(), err.max())


def check_derived(x, ws, ss, qts, nt, cap, eval_logits=None):
    """The fuzzes' criterion (tests/qat_f64.py), nothing counted:
      * both forms (HID true / false instantiations) give the same logits, bit for bit, NaN-aware;
      * every weight level is the reference's, or a perturbed weight's where the perturbation rule allows (qat_f64.kernel_levels);
      * layer by layer on the kernel's OWN hidden outputs: NaN exactly where the float64 evaluation is NaN (a row whose input is all
        zero: exact integer sums decide that in both), every output within the derived bound - 2e-5 of the row's largest plus one
        activation step per near-tie input -, every row within `cap` of its largest output (not less than a tenth of the median row's);
      * end to end: every row that is tie-clean through the whole float64 chain from x equals the chain within 2e-5 of its largest
        output (logits and hidden activations).
    Returns (logits, hidden, the largest ratio of an error to its derived bound)."""
    logits, hidden, wdq = qat.fc_model_forward(x, ws, ss, qts, nt, return_hidden=True, return_w_deq=True)
    plain = qat.fc_model_forward(x, ws, ss, qts, nt) if eval_logits is None else eval_logits
    assert torch.equal(torch.isnan(plain), torch.isnan(logits)) and torch.equal(torch.nan_to_num(plain), torch.nan_to_num(logits))
    nl = len(ws)
    levels, scales = [], []
    for l in range(nl):
        lev, sc, _ = qat_f64.kernel_levels(wdq[l], ws[l], ss[l], qts[l])
        levels.append(lev)
        scales.append(sc)
    offs = [0]
    for w in ws[:-1]:
        offs.append(offs[-1] + w.shape[0])
    outs = [hidden[:, offs[l]:offs[l + 1]] for l in range(nl - 1)] + [logits]
    worst = 0.0
    xin = x.flatten(1)
    for l in range(nl):
        y, _, step = qat_f64.fc_layer(xin, levels[l], scales[l], nt)
        want = y if l + 1 == nl else torch.relu(y)
        # (a layer of fewer than 8 outputs - the logits of a 1..7-class model - has rows whose largest output is the largest of a few
        # numbers that can all sit near zero, where one activation step of a Binary / Ternary layer is most of it: 0.2 there, as below
        # 32 inputs; such rows are within their derived bound like every other)
        c = cap if want.shape[1] >= 8 else max(cap, 0.2)
        worst = max(worst, qat_f64.within(outs[l], want, step, qat_f64.FC_TIGHT, ("layer", l), cap=c, floor_rows=True))
        xin = outs[l]
    chain, clean = qat_f64.fc_chain(x.flatten(1), levels, scales, nt)
    for l in range(nl):
        qat_f64.within(outs[l][clean], chain[l][clean], torch.zeros_like(chain[l][clean]), qat_f64.FC_TIGHT, ("end to end", l))
    return logits, hidden, worst


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_whole_model_forward_against_the_reference_module(tag, gpu_ok):
    check(tag)


def test_batch_sizes_ragged_tiles_and_empty(gpu_ok):
    """n = 0, 1, one row short of a tile, a tile, a tile + 1, and a batch that leaves some waves without work."""
    for n in (1, 31, 32, 33, 200):
        check("a", n)
    x, ws, ss, widths = case("a")
    out = qat.fc_model_forward(x[:0], ws, ss, ["4bitsym"] * 4, "RMS")
    assert out.shape == (0, 10)


def test_large_batch_rows_do_not_depend_on_the_batch(gpu_ok):
    """300,000 rows (more tiles than the launch has waves: the work counter hands them out): every row's logits equal the logits
    the same row gets in a 64-row batch, bit for bit - rows are independent and the arithmetic per row is fixed."""
    x, ws, ss, widths = case("a")
    g = torch.Generator(device="cuda").manual_seed(3)
    big = torch.randn(300_000, 256, device="cuda", generator=g) * (torch.rand(300_000, 1, device="cuda", generator=g) * 2 + 0.01)
    full = qat.fc_model_forward(big, ws, ss, ["4bitsym"] * 4, "RMS")
    for first in (0, 12_345, 299_936):
        part = qat.fc_model_forward(big[first:first + 64].clone(), ws, ss, ["4bitsym"] * 4, "RMS")
        assert torch.equal(part, full[first:first + 64]), first
    # ... and equal the restated formula (torch's own GPU kernels as the fp32 reference) on nearly every row
    want, _ = qat.fc_model_reference(big[:20_000], ws, [s[0] for s in ss], ["4bitsym"] * 4, "RMS")
    err = (full[:20_000] - want).abs().max(dim=1).values / want.abs().max(dim=1).values
    assert (err <= 5e-4).float().mean() >= 0.9 and err.max() <= 6e-2


def test_unsupported_configurations_are_refused_not_emulated(gpu_ok):
    x, ws, ss, widths = case("a")
    assert not qat.fc_model_supported(widths, ["4bit"] * 4, "RMS")              # levels carry + 0.01: not int8
    assert not qat.fc_model_supported(widths, ["FP130"] * 4, "RMS")             # + 128 does not fit int8
    assert not qat.fc_model_supported(widths, ["4bitsym"] * 4, "BatchNorm")     # needs the whole batch per layer
    assert qat.fc_model_supported(widths, ["4bitsym"] * 4, "LayerNorm")
    assert not qat.fc_model_supported([256, 200, 64, 64, 10], ["4bitsym"] * 4, "RMS")
    assert qat.fc_model_supported([256, 160, 160, 160, 10], ["Binary"] * 4, "RMS") and qat.fc_model_supported([256, 192, 192, 10], ["8bit"] * 3, "Lin")
    assert qat.fc_model_supported([256, 192, 192, 192, 64], ["4bitsym"] * 4, "RMS")      # (two waves per workgroup: the image is 135 KiB)
    assert qat.fc_model_supported([128, 64, 64, 64, 10], ["4bitsym"] * 4, "RMS")               # fewer inputs: rows padded with zeros
    assert not qat.fc_model_supported([128, 64, 64, 64, 10], ["4bitsym"] * 4, "LayerNorm")    # (its mean would reach the padding)
    assert not qat.fc_model_supported([260, 64, 64, 64, 10], ["4bitsym"] * 4, "RMS")
    with pytest.raises(NotImplementedError):
        qat.fc_model_forward(x, ws, ss, ["NF4"] * 4, "RMS")
    lib = b.load()      # return codes: include/bitnetmcu_hip.h BNM_OK 0, BNM_EINVAL -1, BNM_EUNSUPPORTED -3
    import ctypes as C
    wa = (C.c_uint32 * 5)(*widths)
    assert lib.bnm_qat_model_workspace_bytes(4, wa) > 0 and lib.bnm_qat_model_workspace_bytes(5, wa) == 0
    qa = (C.c_int * 4)(6, 6, 6, 6)
    sc = (C.c_uint32 * 4)(1, 1, 1, 1)
    wp = (C.c_void_p * 4)(*[w.data_ptr() for w in ws])
    sp = (C.c_void_p * 4)(*[s.data_ptr() for s in ss])
    y = torch.empty((x.shape[0], 10), device="cuda")
    wsp = torch.empty(1 << 16, device="cuda")
    args = lambda **k: [C.c_void_p(x.data_ptr()), x.shape[0], 4, wa, wp, sp, sc, qa, k.get("nt", 0), C.c_void_p(k.get("y", y.data_ptr())), None, None,
                        C.c_void_p(wsp.data_ptr()), k.get("wsb", wsp.numel() * 4), None]
    assert lib.bnm_qat_model_forward_device(*args()) == 0
    assert lib.bnm_qat_model_forward_device(*args(wsb=64)) == -1              # workspace too small
    assert lib.bnm_qat_model_forward_device(*args(y=y.data_ptr() + 4)) == -1  # logits not 16-byte aligned
    assert lib.bnm_qat_model_forward_device(*args(nt=2)) == -3          # BatchNorm
    torch.cuda.synchronize()


def test_fcmnist_module_forward_backward(gpu_ok):
    """qat.FCMNIST (the reference module's mirror) with the reference's weights: forward = the one-kernel op; backward from the
    tensors it saved equals the reference's autograd gradients."""
    x, ws, ss, widths = case("a")
    m = qat.FCMNIST(64, 64, 64, QuantType="4bitsym", NormType="RMS", WScale="PerTensor").cuda()
    layers = m.bitlinear_layers()
    with torch.no_grad():
        for l, layer in enumerate(layers):
            layer.weight.copy_(ws[l])
            layer.s = torch.nn.Parameter(ss[l].reshape(()).clone(), requires_grad=False)
    keep = torch.ones(x.shape[0], dtype=torch.bool, device="cuda")
    keep[ZERO_ROW] = False
    xk = x[keep].reshape(-1, 1, 16, 16).clone().requires_grad_(True)
    assert m.fused(xk)
    y = m(xk)
    (y * torch.from_numpy(GM["a/gy"]).cuda()).sum().backward()
    ref = GM["a/logits"][keep.cpu().numpy()]
    err = np.abs(y.detach().cpu().numpy() - ref).max(axis=1) / np.abs(ref).max(axis=1)
    assert (err <= 5e-4).mean() >= 0.9 and err.max() <= 6e-2
    # gradients: an activation that flipped one step in the forward pass (or a hidden unit whose exact-zero sum became +-1: ReLU's
    # mask) moves that ROW's contribution by a discrete amount - and a weight gradient sums over the rows, so one such row shifts
    # every entry a little: median error within 2e-3 of the largest entry, all within 0.15 (the algebra itself is pinned exactly:
    # tests/test_qat_cpu.py feeds the same backward with the reference's own tensors and gets the reference's gradients to 1e-4)
    def grad_close(got, ref, what):
        err = np.abs(got - ref) / np.abs(ref).max()
        assert np.median(err) <= 2e-3 and err.max() <= 0.15, (what, np.median(err), err.max())
    grad_close(xk.grad.reshape(-1, 256).cpu().numpy(), GM["a/gx"], "gx")
    for l, layer in enumerate(layers):
        grad_close(layer.weight.grad.cpu().numpy(), GM[f"a/gw{l}"], f"gw{l}")
    # ... and exactly the reference's algebra where nothing can flip: the backward fed with the forward's OWN saved tensors equals
    # torch autograd through the restated formula evaluated layer by layer on those same tensors
    with torch.no_grad():
        _, hidden, wdq = qat.fc_model_forward(xk.detach(), ws, ss, ["4bitsym"] * 4, "RMS", return_hidden=True, return_w_deq=True)
    gy = torch.from_numpy(GM["a/gy"]).cuda()
    gx2, gws2 = qat.fc_model_backward(xk.detach(), hidden, wdq, gy, "RMS", [64, 64, 64, 10])
    assert torch.equal(gx2, xk.grad) and all(torch.equal(g, layer.weight.grad) for g, layer in zip(gws2, layers))
    # a configuration the fused op does not serve runs layer by layer through BitLinear's op - same module, same result shape
    m2 = qat.FCMNIST(64, 64, 64, QuantType="4bitsym", NormType="BatchNorm").cuda()
    assert not m2.fused(xk) and m2(xk.detach()).shape == (x.shape[0] - 1, 10)


def fuzz_model_case(seed):
    """seed -> (x, weights, scalars, QuantTypes, NormType, cap) of test_fuzz_random_model_shapes"""
    rng = np.random.default_rng(1000 + seed)
    n_hidden = int(rng.integers(2, 4))
    hidden_w = [int(rng.integers(8, 129)) for _ in range(n_hidden)]
    if seed % 5 == 0:
        hidden_w = [int(rng.choice([32, 64, 96, 128])) for _ in range(n_hidden)]
    if seed >= 24 and seed % 3:      # the six-tile class: at least one hidden layer of 129 .. 192 units, the others anything up to 176
        hidden_w = [int(rng.integers(8, 177)) for _ in range(n_hidden)]
        hidden_w[int(rng.integers(0, n_hidden))] = int(rng.integers(129, 193))
    widths = [256] + hidden_w + [int(rng.integers(1, 65))]
    qt = ["Binary", "BinarySym", "Ternary", "2bitsym", "4bitsym", "5bitsym", "8bit"][seed % 7]
    nt = ("RMS", "Lin", "LayerNorm")[seed % 3]
    perout = seed % 4 == 1
    n = int(rng.choice([1, 7, 32, 33, 257, 1000, 4097]))
    g = torch.Generator(device="cuda").manual_seed(seed)
    ws = [torch.randn(widths[l + 1], widths[l], device="cuda", generator=g) * 0.1 for l in range(len(widths) - 1)]
    if perout:
        ss = [w.abs().max(dim=-1).values.clamp(min=1e-5) / 0.25 * (0.5 + torch.rand(w.shape[0], device="cuda", generator=g)) for w in ws]
    else:
        ss = [(w.abs().mean() / 0.25).reshape(1) for w in ws]
    x = torch.randn(n, 256, device="cuda", generator=g) * (torch.rand(n, 1, device="cuda", generator=g) * 3 + 0.02)
    qts = [qt] * len(ws)
    assert qat.fc_model_supported(widths, qts, nt), (widths, qt, nt)
    return x, ws, ss, qts, nt, 6e-2


@pytest.mark.parametrize("seed", range(36))
def test_fuzz_random_model_shapes(seed, gpu_ok):
    """Random stacks the kernel serves - 3 or 4 layers, hidden widths 8..128 (seeds 24+: up to 192; any, not only multiples of 32), 1..64 classes, every
    int8-level QuantType, both norms, per-tensor and per-output clipping scalars, ragged batch sizes - against the float64 reference
    (tests/qat_f64.py, pinned to the reference module on CPU by tests/test_qat_cpu.py) by `check_derived`: both forms' logits the same
    bits, every layer on the kernel's own input within its derived per-output bound, tie-clean rows end to end within 2e-5."""
    check_derived(*fuzz_model_case(seed))


def test_cnnmnist_module_forward_backward(gpu_ok):
    """qat.CNNMNIST (the reference module's mirror; the model trainingparameters.yaml names) with the reference's weights: the
    convolution front layer by layer through BitConv2d's op, the FC stack behind Flatten (256-96-64-10, 2bitsym then 4bitsym) as the
    ONE-kernel op.  Against the reference module's own features, logits and autograd gradients (fixture), floating point: a conv
    activation that flips one quantisation step moves its image row's outputs a little: features - 85 % of the rows within 1e-4 of the
    row's largest value, all within 5e-3; logits - the FC model's tolerances (90 % within 5e-4, all within 6e-2); gradients - median
    error 2e-3 of the largest entry, all within 5e-2."""
    m = qat.CNNMNIST(96, 64, 0, cnn_width=64, QuantType="4bitsym", WScale="PerTensor", NormType="RMS", num_classes=10).cuda()
    layers = [x for x in list(m.model) + [m.classifier] if hasattr(x, "weight_quant")]
    with torch.no_grad():
        for l, layer in enumerate(layers):
            layer.weight.copy_(torch.from_numpy(GM[f"cnn/w{l}"]))
            layer.s = torch.nn.Parameter(torch.from_numpy(GM[f"cnn/s{l}"]).reshape(()).cuda(), requires_grad=False)
    x = torch.from_numpy(GM["cnn/x"]).cuda().reshape(-1, 1, 16, 16).requires_grad_(True)
    assert m.fused(x)
    with torch.no_grad():
        feats = m.front(x.detach())
    ref_f = GM["cnn/features"]
    ef = np.abs(feats.cpu().numpy() - ref_f).max(axis=1) / np.abs(ref_f).max(axis=1)
    assert (ef <= 1e-4).mean() >= 0.85 and ef.max() <= 5e-3, ((ef <= 1e-4).mean(), ef.max())      # (measured: 96 % within 1e-5, max 6e-4)
    y = m(x)
    ref = GM["cnn/logits"]
    err = np.abs(y.detach().cpu().numpy() - ref).max(axis=1) / np.abs(ref).max(axis=1)
    assert (err <= 5e-4).mean() >= 0.9 and err.max() <= 6e-2, ((err <= 5e-4).mean(), err.max())      # (measured: 98 %, max 9e-3)
    (y * torch.from_numpy(GM["cnn/gy"]).cuda()).sum().backward()

    def grad_close(got, want, what):
        e = np.abs(got - want) / np.abs(want).max()
        assert np.median(e) <= 2e-3 and e.max() <= 5e-2, (what, np.median(e), e.max())      # (measured: medians <= 2.5e-4, max 1e-2)
    grad_close(x.grad.reshape(-1, 256).cpu().numpy(), GM["cnn/gx"].reshape(-1, 256), "gx")
    for l, layer in enumerate(layers):
        grad_close(layer.weight.grad.cpu().numpy(), GM[f"cnn/gw{l}"], f"gw{l}")
    # more than 64 channels: the FC stack's input is wider than 256 - layer by layer, same module (fewer: test below)
    m80 = qat.CNNMNIST(64, 64, 0, cnn_width=80, QuantType="4bitsym").cuda()
    with torch.no_grad():
        assert not m80.fused(x) and m80.front_fused(x.detach()) and m80(x.detach()).shape == (x.shape[0], 10)


@pytest.mark.parametrize("tag", ["a", "c", "g"])
def test_c_host_runs_the_model_forward(tag, tmp_path):
    """examples/qat_forward.c: a gcc-only host that reads a model and float rows from files and calls the whole-model forward through
    include/bitnetmcu_hip.h - the logits it prints are the BITS the Python binding returns for the same tensors (same kernel, same
    launch geometry) and pass the end-to-end tolerance against the reference module's."""
    import subprocess
    import util
    x, ws, ss, widths = case(tag)
    qt, nt = CONFIGS[tag]
    nl = len(ws)
    head = np.array([nl] + widths + [qat.QUANT_TYPES[qt]] * nl + [qat.NORM_TYPES[nt]], dtype=np.int32)
    with open(tmp_path / "model.f32", "wb") as f:
        f.write(head.tobytes())
        for w, s in zip(ws, ss):
            f.write(s.cpu().numpy().astype(np.float32).reshape(-1)[:1].tobytes())
            f.write(w.cpu().numpy().astype(np.float32).tobytes())
    (tmp_path / "rows.f32").write_bytes(x.cpu().numpy().astype(np.float32).tobytes())
    exe = util.compile_c_host("qat_forward.c", tmp_path)
    out = subprocess.run([exe, str(tmp_path / "model.f32"), str(tmp_path / "rows.f32")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = np.array([[float(v) for v in line.split()] for line in out.stdout.splitlines()], dtype=np.float32)
    want = qat.fc_model_forward(x, ws, ss, [qt] * nl, nt).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or np.array_equal(np.isnan(got), np.isnan(want)) and \
        np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    ref = GM[f"{tag}/logits"]
    rows = [i for i in range(len(ref)) if i != ZERO_ROW]
    err = np.abs(got[rows] - ref[rows]).max(axis=1) / np.abs(ref[rows]).max(axis=1)
    assert (err <= 5e-4).mean() >= 0.9 and err.max() <= 6e-2, ((err <= 5e-4).mean(), err.max())


def test_widest_stack_two_waves_per_workgroup(gpu_ok):
    """256-192-192-192-64: the weight image is 135 KiB, a workgroup is two waves; 40,000 rows are more tiles than the capped grid
    has waves (the counter hands them out).  Every row equals its 64-row-batch result bit for bit and the restated formula within
    the end-to-end tolerances."""
    widths = [256, 192, 192, 192, 64]
    g = torch.Generator(device="cuda").manual_seed(77)
    ws = [torch.randn(widths[l + 1], widths[l], device="cuda", generator=g) * 0.1 for l in range(4)]
    ss = [(w.abs().mean() / 0.25).reshape(1) for w in ws]
    x = torch.randn(40_000, 256, device="cuda", generator=g) * (torch.rand(40_000, 1, device="cuda", generator=g) * 3 + 0.02)
    qts = ["4bitsym"] * 4
    assert qat.fc_model_supported(widths, qts, "RMS")
    full, hid = qat.fc_model_forward(x, ws, ss, qts, "RMS", return_hidden=True)
    assert hid.shape == (40_000, 576)
    for first in (0, 20_001, 39_936):
        part = qat.fc_model_forward(x[first:first + 64].clone(), ws, ss, qts, "RMS")
        assert torch.equal(part, full[first:first + 64]), first
    want, want_h = qat.fc_model_reference(x, ws, [s[0] for s in ss], qts, "RMS")
    for got, ref in ((full, want), (hid, want_h)):
        err = (got - ref).abs().max(dim=1).values / ref.abs().max(dim=1).values
        assert (err <= 5e-4).float().mean() >= 0.9 and err.max() <= 6e-2, (float((err <= 5e-4).float().mean()), float(err.max()))


@pytest.mark.parametrize("tag,nt", [("cnn32", "Lin"), ("cnn48", "RMS")])
def test_cnnmnist_with_fewer_than_256_features(tag, nt, gpu_ok):
    """CNNMNIST at 32 / 48 channels: the FC stack has 128 / 192 inputs - the kernel reads rows zero-padded to 256 floats and the
    preparation folds Normalize's other denominator (mean over 128 values, not 256) into layer 1's weight scales.  The reference
    module's own logits and gradients (fixtures), the end-to-end tolerances of this file; both halves of the model are one kernel each."""
    cw, w1, w2, ncls = (int(v) for v in GM[f"{tag}/cfg"])
    m = qat.CNNMNIST(w1, w2, 0, cnn_width=cw, QuantType="4bitsym", WScale="PerTensor", NormType=nt, num_classes=ncls).cuda()
    layers = [x for x in list(m.model) + [m.classifier] if hasattr(x, "weight_quant")]
    with torch.no_grad():
        for l, layer in enumerate(layers):
            layer.weight.copy_(torch.from_numpy(GM[f"{tag}/w{l}"]))
            layer.s = torch.nn.Parameter(torch.from_numpy(GM[f"{tag}/s{l}"]).reshape(()).cuda(), requires_grad=False)
    x = torch.from_numpy(GM[f"{tag}/x"]).cuda().reshape(-1, 1, 16, 16).requires_grad_(True)
    with torch.no_grad():
        assert m.fused(x) and m.front_fused(x.detach())
        y0 = m(x.detach())
    ref = GM[f"{tag}/logits"]
    err = np.abs(y0.cpu().numpy() - ref).max(axis=1) / np.abs(ref).max(axis=1)
    assert (err <= 5e-4).mean() >= 0.9 and err.max() <= 6e-2, ((err <= 5e-4).mean(), err.max())
    y = m(x)      # with gradients: the front layer by layer, the FC stack the kernel in its training form
    err = np.abs(y.detach().cpu().numpy() - ref).max(axis=1) / np.abs(ref).max(axis=1)
    assert (err <= 5e-4).mean() >= 0.9 and err.max() <= 6e-2, ((err <= 5e-4).mean(), err.max())
    (y * torch.from_numpy(GM[f"{tag}/gy"]).cuda()).sum().backward()

    def grad_close(got, want, what):
        # (40 images: ONE flipped activation step in one image's convolution front moves every entry of the 288-entry convolution
        # weight gradients - cnn32 has one, medians 2e-3; the layer-by-layer path sits at the same distances to two digits:
        # profiles/probes/cnnmnist_grad_distances.py)
        e = np.abs(got - want) / np.abs(want).max()
        assert np.median(e) <= 5e-3 and e.max() <= 0.15, (what, np.median(e), e.max())
    grad_close(x.grad.reshape(-1, 256).cpu().numpy(), GM[f"{tag}/gx"].reshape(-1, 256), "gx")
    for l, layer in enumerate(layers):
        grad_close(layer.weight.grad.cpu().numpy(), GM[f"{tag}/gw{l}"], f"gw{l}")


def fuzz_width_case(seed):
    """seed -> (x, weights, scalars, QuantTypes, NormType, cap) of test_fuzz_input_widths_below_256"""
    rng = np.random.default_rng(7000 + seed)
    d = int(rng.integers(4, 256)) if seed % 2 else int(rng.choice([64, 128, 192]))
    widths = [d, int(rng.integers(16, 129)), int(rng.integers(16, 129)), int(rng.integers(2, 48))]
    qt = ["4bitsym", "8bit", "Ternary", "2bitsym", "Binary"][seed % 5]
    nt = ("RMS", "Lin")[seed % 2]
    n = int(rng.choice([5, 64, 999]))
    g = torch.Generator(device="cuda").manual_seed(seed)
    ws = [torch.randn(widths[l + 1], widths[l], device="cuda", generator=g) * 0.1 for l in range(3)]
    ss = [(w.abs().mean() / 0.25).reshape(1) for w in ws]
    x = torch.randn(n, d, device="cuda", generator=g) * (torch.rand(n, 1, device="cuda", generator=g) * 3 + 0.02)
    assert qat.fc_model_supported(widths, [qt] * 3, nt)
    # (below 32 inputs a row's largest output can rest on a handful of quantised activations, one step of which is most of it)
    return x, ws, ss, [qt] * 3, nt, 0.2 if d < 32 else 6e-2


@pytest.mark.parametrize("seed", range(10))
def test_fuzz_input_widths_below_256(seed, gpu_ok):
    """Any number of inputs up to 256 (the binding pads the rows; the float64 reference normalises over the d real ones): logits and
    hidden activations by `check_derived`."""
    check_derived(*fuzz_width_case(seed))


def test_dynamically_taken_batches_of_tiles(gpu_ok):
    """Calls large enough that the launcher hands out `batch` = 2 and 4 consecutive 32-row tiles per take from the work counter
    (bnm_qat_model.hip:629-634: batch = units / (CUs x workgroups per CU x waves per workgroup x 8), at most 4) - the static first batch
    of every wave, `next_left` and `batch_first()` -, in three launch classes:
      * 64-64-64 4bitsym RMS, the evaluation form: 8 waves per workgroup, one workgroup per CU;
      * 64-64-64 4bitsym LayerNorm with the hidden activations written: one wave per SIMD, two workgroups of 4 waves per CU;
      * 256-192-192-192-64 with the hidden activations: six tiles, 2 waves per workgroup, one per CU.
    Batch 4 is asked for with twice the rows the formula needs (it stays 4 if the formula changes by a factor of 2), batch 2 with the
    formula's own count; both ragged (a partial last tile, a last batch shorter than `batch`).  Every row's logits and hidden outputs
    equal, bit for bit, those of calls of 65,536 rows (batch 1: the static / one-tile path), and the last 4,096 rows pass the fuzzes'
    derived float64 criterion (check_derived)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    a_x, a_ws, a_ss, _ = case("a")
    g_x, g_ws, g_ss, _ = case("g")
    gen = torch.Generator(device="cuda").manual_seed(91)
    wide = [256, 192, 192, 192, 64]
    w_ws = [torch.randn(wide[l + 1], wide[l], device="cuda", generator=gen) * 0.1 for l in range(4)]
    w_ss = [(w.abs().mean() / 0.25).reshape(1) for w in w_ws]
    # (class, weights, scalars, NormType, hidden written, units per batch step = CUs x workgroups per CU x waves x 8)
    classes = [("flagship eval", a_ws, a_ss, "RMS", False, cus * 1 * 8 * 8),
               ("LayerNorm, hidden", g_ws, g_ss, "LayerNorm", True, cus * 2 * 4 * 8),
               ("six tiles, hidden", w_ws, w_ss, "RMS", True, cus * 1 * 2 * 8)]
    n_max = max(32 * 8 * step + 17 for *_, step in classes)
    x = torch.randn(n_max, 256, device="cuda", generator=gen) * (torch.rand(n_max, 1, device="cuda", generator=gen) * 3 + 0.02)
    bits = lambda t: t.contiguous().view(torch.int32)
    for what, ws, ss, nt, hid, step in classes:
        qts = ["4bitsym"] * len(ws)
        for n in (32 * (2 * step + 2) + 5, 32 * 8 * step + 17):      # batch 2 (the last batch one tile), batch 4 (the last batch one tile)
            units = (n + 31) // 32
            assert units // step in (2, 8) and units % 2 == 1
            xs = x[:n]
            out = qat.fc_model_forward(xs, ws, ss, qts, nt, return_hidden=hid)
            logits, hidden = out if hid else (out, None)
            for first in range(0, n, 65_536):
                part = qat.fc_model_forward(xs[first:first + 65_536], ws, ss, qts, nt, return_hidden=hid)
                pl, ph = part if hid else (part, None)
                assert torch.equal(bits(pl), bits(logits[first:first + 65_536])), (what, n, first)
                if hid:
                    assert torch.equal(bits(ph), bits(hidden[first:first + 65_536])), (what, n, first)
            tail_l, tail_h, _ = check_derived(xs[n - 4096:], ws, ss, qts, nt, 6e-2)
            assert torch.equal(bits(tail_l), bits(logits[n - 4096:])), (what, n)
            if hid:
                assert torch.equal(bits(tail_h), bits(hidden[n - 4096:])), (what, n)
            del out, logits, hidden
