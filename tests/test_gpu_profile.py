"""Activation profiles on the GPU (-m gpu): bnm_infer_device_profiled / bnm_infer_float_device_profiled against the oracle port's
activation rows reduced in numpy (tests/profile_ref.py).  Integer statistics: every counter must be equal."""
import numpy as np
import pytest

import util
from util import MODEL_NAMES
import bitnetmcu_amd as b
from bitnetmcu_amd import synth, evaluate, DIST_U, DIST_M
from bitnetmcu_amd.profile import ActivationProfile
import profile_ref

pytestmark = pytest.mark.gpu

SIZES = [1, 31, 32, 33, 4097, 20011]
# FC models the profiling variant of the generic kernel serves (tile classes 2 and 4, 256-byte rows); the rest profile by tap + reduce
FUSED_MODELS = {"fc_4bitsym_64", "mcu_12k", "mcu_12k_fp130", "mcu_1k", "tern_96", "tern_96_sparse", "doc12k_ternary", "doc12k_2bit",
                "doc12k_8bit"}


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _modes(ctx):
    """The profile modes the context accepts (mode 1: only where a fused profiling kernel serves the model)."""
    modes = [0, 2]
    try:
        ctx.set_profile_mode(1)
        modes.append(1)
    except b.BnmError:
        pass
    return modes


def _labels(rng, n, nc):
    """labels in [0, nc) with a few out of range (-1, nc, a large value)"""
    lab = rng.integers(0, nc, n).astype(np.int32)
    bad = rng.random(n) < 0.05
    lab[bad] = rng.choice(np.array([-1, nc, 1 << 30], np.int32), int(bad.sum()))
    return lab


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_profile_equals_the_oracle(name, gpu_ok, orc):
    """Every zoo model, both image distributions, ragged sizes around a 32-image tile and the 2,048-image reduction block:
    every counter equals numpy's reduction of the oracle's activation rows, in every accepted mode; the class ids equal
    bnm_infer_device's; labelled calls give numpy's confusion matrix, out-of-range labels included."""
    import torch
    model = util.load_golden_model(name)
    om = util.OracleModel(model, orc)
    ctx = b.Context(model)
    words = ctx.profile_words()
    nc = model.num_classes
    rng = np.random.default_rng(7)
    nmax = max(SIZES)
    for dist in (DIST_U, DIST_M):
        x = synth.images(11 if dist == DIST_U else 5_000_011, nmax, dist)
        want_cls, acts = profile_ref.oracle_acts(om, x)
        labels = _labels(rng, nmax, nc)
        xd = torch.from_numpy(x).cuda()
        ld = torch.from_numpy(labels).cuda()
        plain = torch.empty(nmax, dtype=torch.int32, device="cuda")
        ctx.set_profile_mode(0)
        ctx.infer_device(xd, plain)
        for mode in _modes(ctx):
            ctx.set_profile_mode(mode)
            for k, n in enumerate(SIZES):
                lab = labels[:n] if k % 2 else None
                want = profile_ref.profile_counters(model, acts[:n], want_cls[:n], lab)
                ctr = torch.zeros(words + 8, dtype=torch.int64, device="cuda")
                cls = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                ctx.profile_device(xd[:n], ctr, labels=ld[:n] if lab is not None else None, cls=cls)
                got = _u64(ctr)
                assert np.array_equal(got[:words], want), (name, dist, mode, n)
                assert not got[words:].any(), (name, dist, mode, n)          # nothing past the layout
                assert torch.equal(cls, plain[:n]), (name, dist, mode, n)
                assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want_cls[:n])
                fused = mode != 2 and name in FUSED_MODELS
                assert ctx.last_kernel == "fused_fc_generic_prof_kernel" if fused else "profile_reduce_kernel" in ctx.last_kernel
    ctx.close()


@pytest.mark.parametrize("name", ["fc_4bitsym_64", "mcu_1k", "mcu_12k_fp130", "tern_96", "doc12k_binary", "cnn_64", "mcu_cnn_letters"])
def test_float_profile_equals_the_oracle_on_quantised_images(name, gpu_ok, orc):
    """Float images, NaN / +-inf rows among them: the counters are the oracle's on checker.quantize_input(x), and the non-finite
    count grows by what bnm_infer_float_device counts for the same images."""
    import torch
    from checker import quantize_input
    model = util.load_golden_model(name)
    om = util.OracleModel(model, orc)
    rng = np.random.default_rng(3)
    n = 6001
    x = rng.normal(size=(n, 256)).astype(np.float32)
    x[5, 3] = np.nan
    x[77, 0] = np.inf
    x[78, 255] = -np.inf
    x[4000:4003, 100] = np.nan
    x[17] = 0.0
    want_cls, acts = profile_ref.oracle_acts(om, quantize_input(x))
    labels = _labels(rng, n, model.num_classes)
    want = profile_ref.profile_counters(model, acts, want_cls, labels)
    xd = torch.from_numpy(x).cuda()
    ref = b.Context(model)
    ref.infer_float_device(xd, torch.empty(n, dtype=torch.int32, device="cuda"))
    want_bad = ref.float_nonfinite
    assert want_bad == 6
    ctx = b.Context(model)
    for mode in _modes(ctx):
        ctx.set_profile_mode(mode)
        before = ctx.float_nonfinite
        ctr = torch.zeros(ctx.profile_words(), dtype=torch.int64, device="cuda")
        cls = torch.empty(n, dtype=torch.int32, device="cuda")
        ctx.profile_device(xd, ctr, labels=torch.from_numpy(labels).cuda(), cls=cls)
        assert np.array_equal(_u64(ctr), want), (name, mode)
        assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want_cls), (name, mode)
        assert ctx.float_nonfinite - before == want_bad
        assert ctx.last_kernel.startswith("quantize_input_kernel+")
    # the host form and evaluate.profile give the same statistics
    p = ctx.profile(x, labels)
    q = evaluate.profile(model, x, labels, batch=2500)
    for pr in (p, q):
        assert pr.images == n and pr.labelled == n
        assert np.array_equal(pr.confusion.reshape(-1), want[len(want) - 3 - model.num_classes ** 2:len(want) - 3])
        assert pr.accuracy() == pytest.approx(float((want_cls == labels).sum()) / n)
        for l, ll in zip(pr.layers, ActivationProfile(model, want).layers):
            assert np.array_equal(l.active, ll.active) and np.array_equal(l.sum, ll.sum) and np.array_equal(l.hist, ll.hist)
    ctx.close()
    ref.close()


@pytest.mark.parametrize("name", ["fc_4bitsym_64", "tern_96", "mcu_cnn_16small"])
def test_profiles_accumulate_across_calls_streams_and_graph_replays(name, gpu_ok):
    """Calls add to the counters: two calls into one buffer equal one call on the concatenation - on one stream, on two streams,
    and for a call captured in a HIP graph (single stream) and replayed twice."""
    import torch
    model = util.load_golden_model(name)
    ctx = b.Context(model)
    words = ctx.profile_words()
    n1, n2 = 70_001, 33_333
    x = torch.empty((n1 + n2, 256), dtype=torch.int8, device="cuda")
    synth.fill_device(x, first=123, dist=DIST_M)
    lab = torch.from_numpy(_labels(np.random.default_rng(5), n1 + n2, model.num_classes)).cuda()
    one = torch.zeros(words, dtype=torch.int64, device="cuda")
    ctx.profile_device(x, one, labels=lab)
    two = torch.zeros(words, dtype=torch.int64, device="cuda")
    ctx.profile_device(x[:n1], two, labels=lab[:n1])
    ctx.profile_device(x[n1:], two, labels=lab[n1:])
    torch.cuda.synchronize()
    assert torch.equal(one, two)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    par = torch.zeros(words, dtype=torch.int64, device="cuda")
    with torch.cuda.stream(streams[0]):
        ctx.profile_device(x[:n1], par, labels=lab[:n1])
    with torch.cuda.stream(streams[1]):
        ctx.profile_device(x[n1:], par, labels=lab[n1:])
    torch.cuda.synchronize()
    assert torch.equal(one, par)
    # graph: one eager call on the capturing stream first (scratch is allocated there, never under capture)
    n = 4097
    xs = x[:n]
    single = torch.zeros(words, dtype=torch.int64, device="cuda")
    ctx.profile_device(xs, single, labels=lab[:n])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    warm = torch.zeros(words, dtype=torch.int64, device="cuda")
    with torch.cuda.stream(side):
        ctx.profile_device(xs, warm, labels=lab[:n])
    side.synchronize()
    g_ctr = torch.zeros(words, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.profile_device(xs, g_ctr, labels=lab[:n])
    torch.cuda.synchronize()
    assert not g_ctr.any()                          # capture enqueues nothing
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_ctr, 2 * single) and torch.equal(warm, single)
    ctx.close()


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_fused_profiling_kernel_serves_exactly_the_documented_models(name, gpu_ok):
    """Mode 1 is accepted exactly where the profiling variant of the generic kernel serves the model; mode 0 then runs it, mode 2
    runs tap + reduce."""
    import torch
    ctx = b.Context(util.load_golden_model(name))
    assert (1 in _modes(ctx)) == (name in FUSED_MODELS)
    x = torch.empty((100, 256), dtype=torch.int8, device="cuda")
    synth.fill_device(x, first=1, dist=DIST_U)
    ctr = torch.zeros(ctx.profile_words(), dtype=torch.int64, device="cuda")
    ctx.set_profile_mode(0)
    ctx.profile_device(x, ctr)
    assert (ctx.last_kernel == "fused_fc_generic_prof_kernel") == (name in FUSED_MODELS)
    ctx.set_profile_mode(2)
    ctx.profile_device(x, ctr)
    assert ctx.last_kernel.endswith("+profile_reduce_kernel")
    torch.cuda.synchronize()
    ctx.close()


def test_profile_mode_and_arguments(gpu_ok):
    import torch
    model = util.load_golden_model("fc_4bitsym_64")
    ctx = b.Context(model)
    for bad in (-1, 3):
        with pytest.raises(b.BnmError):
            ctx.set_profile_mode(bad)
    lib = ctx._lib
    x = torch.zeros((64, 256), dtype=torch.int8, device="cuda")
    ctr = torch.zeros(ctx.profile_words() + 1, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert lib.bnm_infer_device_profiled(ctx._h, x.data_ptr(), 64, None, None, None, s) == -1                   # no counters
    assert lib.bnm_infer_device_profiled(ctx._h, x.data_ptr(), 64, None, None, ctr.data_ptr() + 4, s) == -1     # misaligned
    assert lib.bnm_infer_device_profiled(ctx._h, x.data_ptr(), 0, None, None, ctr.data_ptr(), s) == 0           # nothing to do
    assert lib.bnm_infer_device_profiled(ctx._h, x.data_ptr(), 64, None, None, ctr.data_ptr(), s) == 0          # ids not kept
    torch.cuda.synchronize()
    p = ActivationProfile(model, ctr[:-1].cpu().numpy())
    assert p.images == 64 and p.labelled == 0 and int(p.pred.sum()) == 64 and not ctr[-1].item()
    ctx.close()


def test_profile_at_scale_counters_pass_32_bits(gpu_ok, orc):
    """5 x 10^7 images resident on the device: 16 images, chosen from 4,000 synthetic ones so that one neuron's activation is above
    86 in every one of them, repeated (its sum then passes 2^32).  Every hist row sums to images x width exactly, pred is the
    bincount of the ids the call wrote, and every counter is exactly n / 16 times one period's plus the rest; on the first 10^7
    images modes 0 and 2 agree."""
    import torch
    model = util.load_golden_model("mcu_1k")
    ctx = b.Context(model)
    words = ctx.profile_words()
    period = 16
    n = 50_331_648 + 5            # 12 * 2^22 + 5
    pool = synth.images(99, 4000, DIST_U)
    _, acts = profile_ref.oracle_acts(util.OracleModel(model, orc), pool)
    cols = profile_ref.profiled_columns(model, acts).astype(np.int64)
    j = int(np.argmax(np.sort(cols, axis=0)[-period]))          # the column whose 16th largest value is largest
    pick = np.argsort(cols[:, j])[-period:]
    assert int(cols[pick, j].sum()) * (n // period) > 1 << 32
    base = torch.from_numpy(pool[pick]).cuda()
    x = base.repeat(-(-n // period), 1)[:n].contiguous()
    cls = torch.empty(n, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(words, dtype=torch.int64, device="cuda")
    ctx.set_profile_mode(0)
    ctx.profile_device(x, ctr, cls=cls)
    per = torch.zeros(words, dtype=torch.int64, device="cuda")
    ctx.profile_device(base, per)
    rest = torch.zeros(words, dtype=torch.int64, device="cuda")
    ctx.profile_device(base[:n % period], rest)
    torch.cuda.synchronize()
    p = ActivationProfile(model, _u64(ctr))
    assert p.images == n
    for l in p.layers:
        assert int(l.hist.sum()) == n * l.width
    assert np.array_equal(p.pred, torch.bincount(cls.long(), minlength=model.num_classes).cpu().numpy())
    want = _u64(per).astype(object) * (n // period) + _u64(rest).astype(object)
    assert np.array_equal(_u64(ctr).astype(object), want)
    assert int(_u64(ctr).max()) > 1 << 32
    m = 10_000_000
    a = torch.zeros(words, dtype=torch.int64, device="cuda")
    c = torch.zeros(words, dtype=torch.int64, device="cuda")
    ctx.set_profile_mode(0)
    ctx.profile_device(x[:m], a)
    ctx.set_profile_mode(2)
    ctx.profile_device(x[:m], c)
    torch.cuda.synchronize()
    assert torch.equal(a, c)
    ctx.close()
