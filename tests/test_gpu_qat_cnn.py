"""The convolution front of the reference's CNNMNIST in one kernel (csrc/bnm_qat_cnn.hip) on the GPU, through
the C ABI, against fixtures generated from the reference's own module (tests/golden/make_qat_model_golden.py: "cnn/*") and against
the layer-by-layer path (qat.BitConv2d's op per layer, pinned to the reference's BitConv2d by tests/test_gpu_qat.py).

FLOATING POINT: parity is within tolerance.  The kernel's float32 operations are the reference's one by one up to the order of the
nine products of a convolution sum, so an output differs from the reference's by a rounding of that sum (~1e-7 relative) - unless
that rounding moves a value that sits at a tie of the NEXT layer's activation_quant: then one input of nine is a quantisation step
(1 / 127 of its row's maximum) off.  The tolerances, relative to the image's largest feature:
  * at least 90 % of the images within 1e-5 (no flipped step anywhere in 14,000 quantised values; measured: 96-100 %);
  * every image within 1e-2 (measured: 4e-3);
  * the layer-by-layer path, which sums in yet another order, sits at the same distances from the reference.
Those are the fixture checks.  Random fronts, channel counts and QuantTypes are judged per output instead (`check_derived`,
tests/qat_f64.py): each of the three planes against the float64 convolution of the kernel's own previous plane, within 1e-5 of the
image's largest value plus one quantisation step for each input of the 3x3 window that lies within 5e-4 of a rounding tie.
"""
import ctypes as C
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


def golden_module():
    m = qat.CNNMNIST(96, 64, 0, cnn_width=64, QuantType="4bitsym", WScale="PerTensor", NormType="RMS", num_classes=10).cuda()
    layers = [x for x in list(m.model) + [m.classifier] if hasattr(x, "weight_quant")]
    with torch.no_grad():
        for l, layer in enumerate(layers):
            layer.weight.copy_(torch.from_numpy(GM[f"cnn/w{l}"]))
            layer.s = torch.nn.Parameter(torch.from_numpy(GM[f"cnn/s{l}"]).reshape(()).cuda(), requires_grad=False)
    return m


def layer_by_layer(m, x):
    with torch.no_grad():
        for k in list(m.model)[:9]:
            x = k(x)
    return x


def distances(got, want):
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy() if torch.is_tensor(want) else want
    return np.abs(got - want).max(axis=1) / np.maximum(np.abs(want).max(axis=1), 1e-30)


def close(got, want, what):
    e = distances(got, want)
    n = len(e)
    assert (e <= 1e-5).sum() >= n - max(2, n // 10) and e.max() <= 1e-2, (what, float((e <= 1e-5).mean()), float(e.max()))


def check_derived(x, ws, ss, qts, features=None, cap=2e-2):
    """The per-output criterion of tests/qat_f64.py, nothing counted: the training form's features are the evaluation form's (or
    `features`) bit for bit and exactly maxpool(relu(y3)) - an image whose y3 is all negative has all-zero features, as it must -;
    the taps are the reference's levels up to the perturbation rule (read from the workspace, [layer][channel][9] w_int / w_scale);
    y1, y2, y3 each against the float64 convolution of the quantised ReLU / pool of the KERNEL'S previous plane: within 1e-5 of the
    image's largest value of that plane plus |tap| / x_scale for every near-tie input of the output's window, every image within
    `cap`.  -> (features, the largest ratio of an error to its derived bound)"""
    if features is None:
        features = qat.cnn_front_forward(x, ws, ss, qts)
    f, y1, y2, y3 = qat.cnn_front_forward(x, ws, ss, qts, return_planes=True)
    channels = ws[0].shape[0]
    taps = qat._front_workspaces[(x.device.index, torch.cuda.current_stream().cuda_stream, channels)][:27 * channels].reshape(3, channels, 9).clone()
    assert torch.equal(f, features)
    assert torch.equal(f, torch.nn.functional.max_pool2d(torch.relu(y3), 2).flatten(1))
    taps = qat_f64.cnn_taps(ws, ss, qts, taps)
    worst = 0.0
    n = x.shape[0]
    for first in range(0, n, 512):
        xs = x[first:first + 512].reshape(-1, 1, 16, 16).double()
        p1, p2, p3 = (y[first:first + 512].double() for y in (y1, y2, y3))
        for got, a, l in ((p1, xs, 0), (p2, torch.relu(p1), 1), (p3, qat_f64.relu_pool(p2), 2)):
            want, step, _ = qat_f64.conv_layer(a, taps[l])
            worst = max(worst, qat_f64.within(got, want, step, qat_f64.CNN_TIGHT, (f"y{l + 1}", first), cap=cap))
    return f, worst


def test_front_and_model_against_the_reference_module(gpu_ok):
    """The reference's own CNNMNIST (96-64, 64 channels): features behind Flatten, then the logits with the FC stack's one-kernel op
    behind the front's - two launches + two preparation launches for the whole model."""
    m = golden_module()
    x = torch.from_numpy(GM["cnn/x"]).cuda().reshape(-1, 1, 16, 16)
    with torch.no_grad():
        assert m.front_fused(x) and m.fused(x)
        f = m.front(x)
        y = m(x)
    assert f.shape == (x.shape[0], 256)
    close(f, GM["cnn/features"], "features")
    ref = GM["cnn/logits"]
    err = distances(y, ref)
    assert (err <= 5e-4).mean() >= 0.9 and err.max() <= 6e-2, ((err <= 5e-4).mean(), err.max())
    # the per-layer path (what configurations outside the kernel take): same answers, same distances
    close(layer_by_layer(m, x), GM["cnn/features"], "layer by layer")


@pytest.mark.parametrize("channels", [16, 34, 64, 128])
def test_training_form_writes_the_planes_the_backward_needs(channels, gpu_ok):
    """The training form's features are the evaluation form's bit for bit; its planes y1 / y2 / y3 (the convolutions' outputs before
    their ReLU, channels-last) pass the per-output float64 criterion (check_derived); ragged batches; the features are the pooled ReLU
    of y3 exactly."""
    torch.manual_seed(channels + 1)
    m = qat.CNNMNIST(64, 64, 0, cnn_width=channels, QuantType="4bitsym").cuda()
    convs = [c for c in m.model if isinstance(c, qat.BitConv2d)]
    ws, ss, qts = [c.weight.detach() for c in convs], [c.s for c in convs], [c.QuantType for c in convs]
    for n in (1, 3, 130, 1001):
        x = torch.randn(n, 1, 16, 16, device="cuda") * (torch.rand(n, 1, 1, 1, device="cuda") * 2 + 0.05)
        f, y1, y2, y3 = qat.cnn_front_forward(x, ws, ss, qts, return_planes=True)
        assert torch.equal(f, qat.cnn_front_forward(x, ws, ss, qts))
        assert y1.shape == (n, channels, 14, 14) and y2.shape == (n, channels, 12, 12) and y3.shape == (n, channels, 4, 4)
        assert all(t.is_contiguous(memory_format=torch.channels_last) for t in (y1, y2, y3))
        check_derived(x, ws, ss, qts, f)


def test_module_trains_through_the_fused_front(gpu_ok):
    """With a gradient asked for, CNNMNIST's front runs in its training form and the backward works from the saved planes: the
    gradients of the input and of all six weight tensors equal the per-layer path's (the layers called one by one) within the gradient
    tolerances of tests/test_gpu_qat_model.py; images that want no gradient get none computed.  (The reference's own gradients:
    test_cnnmnist_module_forward_backward there, through this same path.)"""
    m = golden_module()
    x = torch.from_numpy(GM["cnn/x"]).cuda().reshape(-1, 1, 16, 16)
    gy = torch.from_numpy(GM["cnn/gy"]).cuda()
    xa = x.clone().requires_grad_(True)
    assert m.front_fused(xa)
    (m(xa) * gy).sum().backward()
    got = [xa.grad.clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None]
    m.zero_grad()
    xb = x.clone().requires_grad_(True)
    y = xb
    for k in list(m.model):
        y = k(y)
    (m.classifier(y) * gy).sum().backward()
    want = [xb.grad] + [p.grad.clone() for p in m.parameters() if p.grad is not None]
    assert len(got) == len(want) == 7
    for a, b_ in zip(got, want):
        e = (a - b_).abs() / b_.abs().max()
        assert e.median() <= 2e-3 and e.max() <= 0.15, (tuple(a.shape), float(e.median()), float(e.max()))
    m.zero_grad()
    (m(x) * gy).sum().backward()      # the usual case: data without a gradient
    again = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(again) == 6 and all(torch.equal(a, b_) for a, b_ in zip(again, got[1:]))


@pytest.mark.parametrize("channels", [16, 18, 32, 48, 64, 100, 128])
def test_channel_counts_and_batch_sizes_against_the_layer_by_layer_path(channels, gpu_ok):
    """8 .. 64 channel pairs per image (8, 4, 2 images or one per wave; lanes idle where the pairs do not divide 64), ragged batches,
    random weights: the per-output float64 criterion (check_derived)."""
    torch.manual_seed(channels)
    m = qat.CNNMNIST(64, 64, 0, cnn_width=channels, QuantType="4bitsym").cuda()
    for n in (1, 2, 3, 7, 64, 1001):
        x = torch.randn(n, 1, 16, 16, device="cuda") * (torch.rand(n, 1, 1, 1, device="cuda") * 2 + 0.05)
        with torch.no_grad():
            assert m.front_fused(x)
            got = m.front(x)
        assert got.shape == (n, 4 * channels)
        convs = [c for c in m.model if isinstance(c, qat.BitConv2d)]
        check_derived(x, [c.weight.detach() for c in convs], [c.s for c in convs], [c.QuantType for c in convs], got)
    with torch.no_grad():
        assert m.front(torch.empty(0, 1, 16, 16, device="cuda")).shape == (0, 4 * channels)


@pytest.mark.parametrize("qt", ["8bit", "4bitsym", "4bit", "Ternary", "Binary", "BinarySym", "2bitsym", "5bitsym", "FP130", "NF4"])
def test_quant_types(qt, gpu_ok):
    """The taps are w_int / w_scale as floats: every QuantType of the reference's weight_quant ('None', which skips activation_quant
    as well, is refused): the kernel's taps against the perturbation rule, the planes against the per-output float64 criterion."""
    torch.manual_seed(5)
    m = qat.CNNMNIST(64, 64, 0, cnn_width=32).cuda()
    convs = [c for c in m.model if isinstance(c, qat.BitConv2d)]
    x = torch.randn(300, 1, 16, 16, device="cuda")
    ws, ss = [c.weight.detach() for c in convs], [c.s for c in convs]
    check_derived(x, ws, ss, [qt] * 3)


def fuzz_front_case(seed):
    """seed -> (images, weights, scalars, QuantTypes) of test_fuzz_random_fronts"""
    rng = np.random.default_rng(5000 + seed)
    channels = 2 * int(rng.integers(8, 65))
    qts = [str(rng.choice(["8bit", "4bitsym", "Ternary", "Binary", "2bitsym", "5bitsym", "FP130", "4bit", "NF4", "BinarySym"])) for _ in range(3)]
    if seed % 3 == 0:
        qts = ["8bit"] * 3      # (CNNMNIST's own)
    n = int(rng.choice([1, 2, 5, 31, 64, 257, 1000, 4099]))
    g = torch.Generator(device="cuda").manual_seed(seed)
    ws = [torch.randn(channels, 1, 3, 3, device="cuda", generator=g) * float(rng.choice([0.05, 0.3, 1.0])) for _ in range(3)]
    ss = [(w.abs().mean() / 0.25 * float(rng.choice([0.5, 1.0, 3.0]))).reshape(1) for w in ws]
    x = torch.randn(n, 1, 16, 16, device="cuda", generator=g) * (torch.rand(n, 1, 1, 1, device="cuda", generator=g) * 2 + 0.05) * float(rng.choice([0.1, 1.0, 10.0]))
    assert qat.cnn_front_supported(channels, ss, qts), (channels, qts)
    return x, ws, ss, qts


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_random_fronts(seed, gpu_ok):
    """Random fronts the kernel serves - an even channel count of 16 .. 128, a QuantType per layer, weights and clipping scalars of
    random magnitude (weights past the clipping range included), images from a tenth to ten times the usual brightness, ragged
    batches - both forms, every plane by the per-output float64 criterion (check_derived)."""
    check_derived(*fuzz_front_case(seed))


def test_rows_do_not_depend_on_the_batch_and_special_images(gpu_ok):
    """200,000 images (more groups than the launch has waves): every image's features equal the features it gets in a small batch,
    bit for bit.  An all-zero image and an image with one non-zero pixel: finite features (NormType 'None': no 0 / 0), equal to the
    per-layer path's; a huge image: scale-invariant up to rounding; a tiny one: as the per-layer path (the 1e-5 clamp acts)."""
    m = golden_module()
    g = torch.Generator(device="cuda").manual_seed(11)
    big = torch.randn(200_000, 1, 16, 16, device="cuda", generator=g) * (torch.rand(200_000, 1, 1, 1, device="cuda", generator=g) * 2 + 0.01)
    big[7] = 0.0
    big[8] = 0.0
    big[8, 0, 5, 9] = 1.5
    big[9] = big[10] * 1e4
    big[11] = big[10] * 1e-4
    with torch.no_grad():
        full = m.front(big)
        for first in (0, 100_001, 199_990):
            assert torch.equal(m.front(big[first:first + 10].clone()), full[first:first + 10]), first
    assert torch.isfinite(full).all()
    assert torch.equal(full[7], torch.zeros(256, device="cuda"))
    close(full[:2000], layer_by_layer(m, big[:2000]), "first 2000")
    assert torch.allclose(full[9] * 1e-4, full[10], rtol=1e-4, atol=1e-6 * float(full[10].abs().max()))
    # (the tiny image is NOT a scaled copy: activation_quant's clamp of a row maximum at 1e-5 acts on it - here as in the reference)


def test_unsupported_configurations_are_refused_not_emulated(gpu_ok):
    lib = b.load()
    one = (C.c_uint32 * 3)(1, 1, 1)
    q8 = (C.c_int * 3)(10, 10, 10)
    assert lib.bnm_qat_cnn_front_supported(64, one, q8) == 1 and lib.bnm_qat_cnn_front_supported(16, one, q8) == 1
    for ch in (0, 8, 14, 17, 63, 130, 256):
        assert lib.bnm_qat_cnn_front_supported(ch, one, q8) == 0, ch
    assert lib.bnm_qat_cnn_front_supported(64, (C.c_uint32 * 3)(1, 64, 1), q8) == 0      # per-output clipping scalars
    assert lib.bnm_qat_cnn_front_supported(64, one, (C.c_int * 3)(10, 0, 10)) == 0          # QuantType 'None': no activation_quant either
    m = qat.CNNMNIST(64, 64, 0, cnn_width=8).cuda()
    x = torch.randn(5, 1, 16, 16, device="cuda")
    with torch.no_grad():
        assert not m.front_fused(x) and m.front(x).shape == (5, 32)      # layer by layer, same module
    convs = [c for c in m.model if isinstance(c, qat.BitConv2d)]
    with pytest.raises(NotImplementedError):
        qat.cnn_front_forward(x, [c.weight for c in convs], [c.s for c in convs])
    with pytest.raises(RuntimeError):
        qat.cnn_front_forward(x.cpu(), [c.weight for c in convs], [c.s for c in convs])
    # return codes: BNM_OK 0, BNM_EINVAL -1, BNM_EUNSUPPORTED -3
    m64 = golden_module()
    convs = [c for c in m64.model if isinstance(c, qat.BitConv2d)]
    ws = [c.weight.detach().contiguous() for c in convs]
    ss = [c.s.detach().reshape(1).contiguous() for c in convs]
    wp = (C.c_void_p * 3)(*[w.data_ptr() for w in ws])
    sp = (C.c_void_p * 3)(*[s.data_ptr() for s in ss])
    qa = (C.c_int * 3)(10, 10, 10)
    x = torch.randn(6, 256, device="cuda")
    f = torch.empty(6, 256, device="cuda")
    wsp = torch.empty(4096, device="cuda")
    args = lambda **k: [C.c_void_p(k.get("x", x.data_ptr())), 6, k.get("ch", 64), wp, sp, k.get("sc", one), k.get("qa", qa), C.c_void_p(f.data_ptr()),
                        C.c_void_p(wsp.data_ptr()), k.get("wsb", wsp.numel() * 4), None]
    assert lib.bnm_qat_cnn_front_forward_device(*args()) == 0
    assert lib.bnm_qat_cnn_front_forward_device(*args(wsb=64)) == -1
    assert lib.bnm_qat_cnn_front_forward_device(*args(x=x.data_ptr() + 4)) == -1
    assert lib.bnm_qat_cnn_front_forward_device(*args(qa=(C.c_int * 3)(10, 99, 10))) == -1
    assert lib.bnm_qat_cnn_front_forward_device(*args(ch=12)) == -3
    assert lib.bnm_qat_cnn_front_forward_device(*args(qa=(C.c_int * 3)(10, 0, 10))) == -3
    assert int(lib.bnm_qat_cnn_front_workspace_bytes(64)) == 3 * 64 * 9 * 4
    torch.cuda.synchronize()


def test_c_host_runs_the_whole_cnnmnist_forward(tmp_path, gpu_ok):
    """examples/qat_cnn_forward.c: a gcc-only host that chains the two kernels (convolution front, FC stack) on the reference's own
    CNNMNIST fixture - the logits it prints are the bits the Python module returns under torch.no_grad() and pass the end-to-end
    tolerance against the reference module's."""
    import subprocess
    m = golden_module()
    convs = [c for c in m.model if isinstance(c, qat.BitConv2d)]
    fcs = m.bitlinear_layers()
    head = np.array([64, len(fcs)] + [f.out_features for f in fcs] + [qat.QUANT_TYPES[c.QuantType] for c in convs] +
                    [qat.QUANT_TYPES[f.QuantType] for f in fcs] + [qat.NORM_TYPES[fcs[0].NormType]], dtype=np.int32)
    with open(tmp_path / "model.f32", "wb") as f:
        f.write(head.tobytes())
        for layer in convs + fcs:
            f.write(layer.s.detach().cpu().numpy().astype(np.float32).reshape(-1)[:1].tobytes())
            f.write(layer.weight.detach().cpu().numpy().astype(np.float32).tobytes())
    x = torch.from_numpy(GM["cnn/x"]).cuda().reshape(-1, 1, 16, 16)
    (tmp_path / "images.f32").write_bytes(GM["cnn/x"].astype(np.float32).tobytes())
    exe = util.compile_c_host("qat_cnn_forward.c", tmp_path)
    out = subprocess.run([exe, str(tmp_path / "model.f32"), str(tmp_path / "images.f32")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = np.array([[float(v) for v in line.split()] for line in out.stdout.splitlines()], dtype=np.float32)
    with torch.no_grad():
        want = m(x).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ref = GM["cnn/logits"]
    err = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
    assert (err <= 5e-4).mean() >= 0.9 and err.max() <= 6e-2, ((err <= 5e-4).mean(), err.max())


def test_two_streams_and_two_threads_do_not_share_scratch(gpu_ok):
    """The taps / weight images of a call live in a workspace per (device, stream): the whole CNNMNIST forward on two side streams from
    two host threads at once, different models and batches, gives each thread exactly what it gets alone."""
    import threading
    m1, m2 = golden_module(), qat.CNNMNIST(64, 48, 0, cnn_width=32, QuantType="8bit", NormType="Lin").cuda()
    g = torch.Generator(device="cuda").manual_seed(21)
    x1 = torch.randn(20_000, 1, 16, 16, device="cuda", generator=g)
    x2 = torch.randn(33_333, 1, 16, 16, device="cuda", generator=g) * 3.0
    with torch.no_grad():
        alone = [m1(x1).clone(), m2(x2).clone()]
    torch.cuda.synchronize()
    got, errors = [None, None], []

    def work(k, m, x):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s), torch.no_grad():
                for _ in range(5):
                    y = m(x)
                s.synchronize()
            got[k] = y
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(0, m1, x1)), threading.Thread(target=work, args=(1, m2, x2))]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    assert torch.equal(got[0], alone[0]) and torch.equal(got[1], alone[1])
