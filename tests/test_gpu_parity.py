"""GPU parity tests (-m gpu): everything goes through the C ABI of libbitnetmcu_hip.so and is compared bit-exactly
with (i) the committed golden vectors produced by the compiled reference and (ii) the oracle port on seeded
synthetic inputs.  Integer work: the bar is bit-exact, class ids AND all logits AND all int8 activations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import util
from util import GOLDEN, MODEL_NAMES
import bitnetmcu_amd as b
from bitnetmcu_amd import synth, DIST_U, DIST_M

pytestmark = pytest.mark.gpu


def paths_for(ctx):
    """(label, setup) for every kernel path this model can run."""
    out = [("auto", lambda c: c.set_path(b.PATH_AUTO))]
    out.append(("layerwise", lambda c: c.set_path(b.PATH_LAYERWISE_ALU)))
    try:        # one int8 GEMM kernel per layer on the matrix cores (every codec the C engine decodes)
        ctx.set_path(b.PATH_LAYERWISE_MFMA)
        out.append(("layerwise_mfma", lambda c: c.set_path(b.PATH_LAYERWISE_MFMA)))
    except b.BnmError:
        pass
    # 4 = the generic kernel (run-time widths, weights in LDS; 7 / 8 = the same with one / two image tiles per wave forced),
    # 5 / 6 = dual-tile loop with a CU-shared / device-wide work counter
    for v in (0, 1, 2, 3, 4, 5, 6, 7, 8):
        def fused(c, v=v):
            c.set_path(b.PATH_FUSED_MFMA)
            c.set_tuning(variant=v)
        try:
            fused(ctx)
            out.append((f"fused_v{v}", fused))
        except b.BnmError:
            pass
    if any(l == "fused_v6" for l, _ in out):
        # small batches of variant 6 run the fixed-stride kernel (one dispatch); a grid of 1 workgroup = 4 resident waves keeps the
        # work-counter kernel itself in the small-size tests
        def fused6_small_grid(c):
            c.set_path(b.PATH_FUSED_MFMA)
            c.set_tuning(variant=6, grid_blocks=1)
        out.append(("fused_v6_grid1", fused6_small_grid))
    # streamed weights (two / one image per lane; work counter / fixed stride: 96-96-96 only), the plain ALU kernel (every shape of
    # the ALU table)
    for tv in (2, 1, 12, 11, 0):
        def tern(c, tv=tv):
            c.set_path(b.PATH_TERNARY_ALU)
            c.set_ternary_variant(tv)
        try:
            tern(ctx)
            out.append((f"ternary_alu_v{tv}", tern))
        except b.BnmError:
            pass
    ctx.set_path(b.PATH_AUTO)
    return out


def test_device_generator_equals_host_generator(gpu_ok):
    import torch
    for dist in (DIST_U, DIST_M):
        for first, count in ((0, 1000), (10**8 - 77, 77), (2**40 + 5, 33)):
            t = torch.empty((count, 256), dtype=torch.int8, device="cuda")
            synth.fill_device(t, first=first, dist=dist)
            assert np.array_equal(t.cpu().numpy(), synth.images(first, count, dist))


def test_class_digest_kernel(gpu_ok):
    import torch
    cls = np.random.default_rng(5).integers(0, 10, 100003).astype(np.uint32)
    d = synth.digest_device(torch.from_numpy(cls.view(np.int32)).cuda(), first=12345, n_bins=10).cpu().numpy()
    assert int(d[0].astype(np.uint64)) == synth.class_digest(cls, 12345)
    assert d[1:].tolist() == np.bincount(cls, minlength=10).tolist()


def test_gpu_unpack_kernels_all_codecs(gpu_ok, bnm, orc):
    """packed words -> int8 rows on the GPU == orc_weight_at for every (row, k)."""
    k = np.load(os.path.join(GOLDEN, "kat_codecs.npz"))
    for c in range(int(k["n_cases"])):
        bpw, n_in, n_out = (int(v) for v in k[f"c{c}_meta"])
        w = np.ascontiguousarray(k[f"c{c}_w"])
        stride = (n_in + 31) // 32 * 32
        lo = np.zeros((n_out, stride), np.int8)
        hi = np.zeros((n_out, stride), np.int8)
        if bpw not in (1, 2, 4, 12, 16, 20, 64):
            continue
        b._lib.check(bnm, bnm.bnm_unpack_layer_host(w.ctypes.data, bpw, n_in, n_out, lo.ctypes.data, hi.ctypes.data, stride), "unpack")
        want = np.array([[orc.orc_weight_at(w.ctypes.data, bpw, n_in, r, kk) for kk in range(n_in)] for r in range(n_out)])
        assert np.array_equal(lo[:, :n_in].astype(np.int32) + hi[:, :n_in].astype(np.int32), want), (bpw, n_in, n_out)
        assert not lo[:, n_in:].any() and not hi[:, n_in:].any()


def test_reference_symbols_against_golden(gpu_ok, bnm):
    """The drop-in per-function symbols (host pointers) on the reference-generated KATs."""
    f = util.Funcs(bnm)
    k = np.load(os.path.join(GOLDEN, "kat_codecs.npz"))
    for c in range(int(k["n_cases"])):
        bpw, n_in, n_out = (int(v) for v in k[f"c{c}_meta"])
        for tag in "sux":
            out = f.processfclayer(k[f"c{c}{tag}_act"], k[f"c{c}_w"], bpw, n_in, n_out)
            assert np.array_equal(out, k[f"c{c}{tag}_out"]), (bpw, n_in, n_out, tag)
    k = np.load(os.path.join(GOLDEN, "kat_relunorm.npz"))
    for c in range(int(k["n_cases"])):
        out, pos = f.relunorm(k[f"in{c}"])
        assert np.array_equal(out, k[f"out{c}"]) and pos == int(k[f"pos{c}"]), c
        out, pos = f.relunorm_inplace(k[f"in{c}"])
        assert np.array_equal(out, k[f"out{c}"]) and pos == int(k[f"pos{c}"]), ("inplace", c)
    k = np.load(os.path.join(GOLDEN, "kat_convpool.npz"))
    for c in range(int(k["n_conv"])):
        xy, shift = (int(v) for v in k[f"conv{c}_meta"])
        for inplace in (True, False):
            assert np.array_equal(f.conv33(k[f"conv{c}_in"], k[f"conv{c}_w"], xy, shift, inplace), k[f"conv{c}_out"])
    for c in range(int(k["n_pool"])):
        xy = int(k[f"pool{c}_meta"][0])
        for inplace in (True, False):
            assert np.array_equal(f.maxpool22(k[f"pool{c}_in"], xy, inplace), k[f"pool{c}_out"])


def test_reference_symbols_any_size(gpu_ok, bnm, orc):
    """The reference's four functions take any size; so do the drop-in symbols: rows longer than one LDS pass (960 inputs), vectors
    longer than a wave's registers (1024), planes wider than the LDS plane (64) - against the oracle port, incl. in-place use."""
    f, o = util.Funcs(bnm), util.Funcs(orc, "orc_")
    rng = np.random.default_rng(77)
    for bpw, n_in, n_out in ((4, 2048, 9), (2, 1968, 5), (1, 4096, 3), (16, 1000, 6), (12, 1024, 4), (20, 3000, 2), (64, 2000, 7), (64, 970, 3)):
        act = rng.integers(-128, 128, n_in).astype(np.int8)
        if bpw == 64:
            w = rng.integers(0, 59049, size=n_out * (n_in // 10)).astype(np.uint16)
        else:
            fb = {1: 1, 2: 2, 4: 4, 12: 4, 20: 4, 16: 8}[bpw]
            w = rng.integers(0, 2**32, size=n_out * ((n_in * fb + 31) // 32), dtype=np.uint32)
        assert np.array_equal(f.processfclayer(act, w, bpw, n_in, n_out), o.processfclayer(act, w, bpw, n_in, n_out)), (bpw, n_in, n_out)
    for n in (1025, 3000, 70001):
        x = rng.integers(-200000, 200000, n).astype(np.int32)
        x[n // 3] = x[n // 2] = x.max() + 5           # two equal maxima: the first position wins
        for fn in ("relunorm", "relunorm_inplace"):
            got, want = getattr(f, fn)(x), getattr(o, fn)(x)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], (n, fn)
    for xy in (65, 100, 257):
        plane = rng.integers(-3000, 3000, xy * xy).astype(np.int32)
        w = rng.integers(-128, 128, 9).astype(np.int8)
        for inplace in (True, False):
            assert np.array_equal(f.conv33(plane, w, xy, 5, inplace), o.conv33(plane, w, xy, 5, inplace)), xy
            assert np.array_equal(f.maxpool22(plane, xy, inplace), o.maxpool22(plane, xy, inplace)), xy


@pytest.mark.parametrize("name", ["fc_4bitsym_64", "mcu_cnn_16small"])
def test_reference_symbols_full_schedule(name, gpu_ok, bnm):
    """BitMnistInference's schedule executed call by call through OUR processfclayer/ReLUNorm/conv/pool symbols."""
    model = util.load_golden_model(name)
    k = np.load(os.path.join(GOLDEN, f"kat_{name}.npz"))
    f = util.Funcs(bnm)
    for i in (0, 13, 80):
        c, lg, acts = util.run_schedule(f, model, k["images"][i])
        assert c == k["cls"][i] and np.array_equal(lg, k["logits"][i]) and np.array_equal(acts, k["acts"][i])


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_model_golden_all_paths(name, gpu_ok):
    model = util.load_golden_model(name)
    k = np.load(os.path.join(GOLDEN, f"kat_{name}.npz"))
    x, tn = k["images"], int(k["trace_n"])
    ctx = b.Context(model)
    seen = []
    for label, setup in paths_for(ctx):
        setup(ctx)
        cls, lg = ctx.infer(x, logits=True)
        assert np.array_equal(cls, k["cls"]), (name, label)
        assert np.array_equal(lg[:tn], k["logits"]), (name, label)
        seen.append(label)
    assert np.array_equal(ctx.activations(x[:tn]), k["acts"]), name
    assert "layerwise" in seen and len(seen) >= 2
    ctx.close()


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_model_vs_oracle_synthetic(name, gpu_ok, orc):
    model = util.load_golden_model(name)
    om = util.OracleModel(model, orc)
    n = 150000 if model.kind == b.KIND_FC else 3000
    x = np.concatenate([synth.images(7_000_000, n, DIST_U), synth.images(3_000_000, n, DIST_M)])
    want_cls, want_lg = om.infer(x, logits=True)
    ctx = b.Context(model)
    for label, setup in paths_for(ctx):
        setup(ctx)
        cls, lg = ctx.infer(x, logits=True)
        assert np.array_equal(cls, want_cls), (name, label)
        assert np.array_equal(lg, want_lg), (name, label)
    ctx.close()


@pytest.mark.parametrize("name", [n for n in MODEL_NAMES if "cnn" in n])
def test_cnn_front_end_both_kernels(name, gpu_ok, orc):
    """The lane = image kernel (3: all three convolutions on the matrix cores; 302: two tiles per take), conv1 on the matrix cores
    with a lane per channel (1) and the all-VALU front end of round 1 (0): ids and logits equal the oracle's on synthetic images
    of both distributions, odd batch sizes, ragged 32-image tiles and the extreme images."""
    model = util.load_golden_model(name)
    om = util.OracleModel(model, orc)
    ctx = b.Context(model)
    x = np.concatenate([synth.images(123, 1501, DIST_U), synth.images(9, 1502, DIST_M), np.zeros((2, 256), np.int8),
                        np.full((2, 256), -128, np.int8), np.full((2, 256), 127, np.int8)])
    want = om.infer(x, logits=True)
    assert ctx.cnn_tail_fused        # every CNN of the zoo: the FC tail runs inside the lane = image kernel's wave (one kernel)
    for variant in (3, 302, 5, 6, 4, 402, 1, 0):   # 4 / 402: the tail as its own launch; 5: conv3's third plane kept (the zoo's weights rule it out); 6: the four-wave form
        ctx.set_cnn_variant(variant)
        assert ctx.cnn_tail_fused == (variant in (3, 302, 5, 6)) and ctx.cnn_planes == (3 if variant == 5 else 2)
        assert ctx.cnn_pipelined == (variant in (3, 302, 5))
        # (<= 16 channels: two images per item, the last one or two images through the single-image instantiation)
        for n in (len(x), 1, 5, 2, 3, 4, 1000, 31, 32, 33, 65):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (name, variant, n)
    ctx.close()


@pytest.mark.parametrize("name,variant,n", [("fc_4bitsym_64", 6, 2_000_077), ("fc_4bitsym_64", 4, 2_000_077), ("fc_4bitsym_64", 3, 2_000_077),
                                            ("tern_96", -1, 1_000_033), ("cnn_64", -1, 200_011), ("mcu_cnn_16small", -1, 100_003)])
def test_context_on_two_streams(name, variant, n, gpu_ok):
    """Launches of ONE context queued on two streams at once (counter blocks and the CNN / layer-wise scratch are kept per
    stream): every result equals the single-stream result."""
    import torch
    model = util.load_golden_model(name)
    ctx = b.Context(model)
    if variant >= 0:
        ctx.set_tuning(variant=variant)
    sets = []
    for k in range(6):
        x = torch.empty((n, 256), dtype=torch.int8, device="cuda")
        synth.fill_device(x, first=k * 10_000_019, dist=DIST_U)
        want = torch.empty(n, dtype=torch.int32, device="cuda")
        ctx.infer_device(x, want)
        sets.append((x, want, torch.full((n,), -1, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for k, (x, _, got) in enumerate(sets):
        with torch.cuda.stream(streams[k & 1]):
            ctx.infer_device(x, got)
    torch.cuda.synchronize()
    for k, (_, want, got) in enumerate(sets):
        assert torch.equal(want, got), (name, variant, k)
    ctx.close()


def _setup(ctx, path, variant):
    if path:
        ctx.set_path(path)
    if variant >= 0:
        ctx.set_tuning(variant=variant)


@pytest.mark.parametrize("name,path,variant,n", [("fc_4bitsym_64", 0, 6, 300_007), ("fc_4bitsym_64", 0, 4, 300_007),
                                                 ("tern_96", 3, -1, 150_001), ("tern_96", 1, -1, 150_001), ("cnn_64", 0, -1, 60_013)])
def test_many_launches_on_three_streams(name, path, variant, n, gpu_ok):
    """360 launches of ONE context queued on three streams at once, far more than any ring could hold: every stream owns its counter
    block, and every kernel leaves it zeroed for the stream's next launch (no memset between launches).  A launch that found a dirty
    or shared counter would skip or repeat tiles; every result must equal the single-stream result."""
    import torch
    model = util.load_golden_model(name)
    ctx = b.Context(model)
    _setup(ctx, path, variant)
    inputs = []
    for k in range(4):
        x = torch.empty((n - 1000 * k, 256), dtype=torch.int8, device="cuda")
        synth.fill_device(x, first=k * 10_000_019, dist=DIST_U)
        want = torch.empty(len(x), dtype=torch.int32, device="cuda")
        ctx.infer_device(x, want)
        inputs.append((x, want))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    launches = 360
    outs = [(inputs[(k * 7) % 4][1], torch.full((len(inputs[(k * 7) % 4][0]),), -1, dtype=torch.int32, device="cuda")) for k in range(launches)]
    torch.cuda.synchronize()          # the fills ran on the default stream, which the side streams do not wait for
    for k in range(launches):
        with torch.cuda.stream(streams[k % 3]):
            ctx.infer_device(inputs[(k * 7) % 4][0], outs[k][1])
    torch.cuda.synchronize()
    for k, (want, got) in enumerate(outs):
        assert torch.equal(want, got), (name, path, variant, k)
    # a released stream's block returns to the pool; the context keeps working on that stream afterwards
    ctx.release_stream(streams[0])
    x, want = inputs[0]
    got = torch.full((len(x),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[0]):
        ctx.infer_device(x, got)
    torch.cuda.synchronize()
    assert torch.equal(want, got)
    ctx.close()


@pytest.mark.parametrize("name,path,variant,n", [("fc_4bitsym_64", 0, 6, 300_007), ("fc_4bitsym_64", 0, 4, 100_003), ("cnn_64", 0, -1, 30_011),
                                                 ("mcu_cnn_16", 0, -1, 30_011), ("mcu_cnn_48", 0, -1, 30_012)])   # two images per front-end item
def test_graph_replays_next_to_eager_launches(name, path, variant, n, gpu_ok):
    """A captured launch keeps a counter block of its own: the graph replayed on one stream while eager launches of the same
    context run on the CAPTURING stream and on a third one - 30 rounds, every result equal to the single-stream result.
    (CNN model: its captured launches use the capturing stream's SCRATCH rows, which cannot be allocated under capture, so the
    documented contract there is: no eager launches on the capturing stream while its graph replays elsewhere - the eager launches
    of that case run on two other streams.)"""
    import torch
    model = util.load_golden_model(name)
    ctx = b.Context(model)
    _setup(ctx, path, variant)
    xg = torch.empty((n, 256), dtype=torch.int8, device="cuda")
    xe = torch.empty((n + 777, 256), dtype=torch.int8, device="cuda")
    synth.fill_device(xg, first=5, dist=DIST_U)
    synth.fill_device(xe, first=77_000_000, dist=DIST_U)
    want_g = torch.empty(n, dtype=torch.int32, device="cuda")
    want_e = torch.empty(n + 777, dtype=torch.int32, device="cuda")
    ctx.infer_device(xg, want_g)
    ctx.infer_device(xe, want_e)
    cap, other, third = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    eager_a = torch.cuda.Stream() if model.kind == b.KIND_CNN else cap
    got_g = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with torch.cuda.stream(cap):
        ctx.infer_device(xg, got_g)              # first use on the capturing stream: scratch is allocated here, not under capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        ctx.infer_device(xg, got_g)
    torch.cuda.synchronize()
    for k in range(30):
        got_g.fill_(-1)
        e1 = torch.full((n + 777,), -1, dtype=torch.int32, device="cuda")
        e2 = torch.full((n + 777,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(other):
            g.replay()
        with torch.cuda.stream(eager_a):
            ctx.infer_device(xe, e1)
        with torch.cuda.stream(third):
            ctx.infer_device(xe, e2)
        torch.cuda.synchronize()
        assert torch.equal(got_g, want_g) and torch.equal(e1, want_e) and torch.equal(e2, want_e), (name, variant, k)
    ctx.close()


@pytest.mark.parametrize("name", ["fc_4bitsym_64", "tern_96", "cnn_64", "mcu_cnn_16small", "mcu_cnn_48"])
def test_infer_device_under_graph_capture(name, gpu_ok, orc):
    """bnm_infer_device enqueues only stream work (kernels; scratch is allocated per stream on first use), so a
    launch-bound small-batch loop can be captured into a HIP graph once and replayed: warm up on the capture stream, capture,
    replay on three different inputs, ids and logits against the oracle."""
    import torch
    model = util.load_golden_model(name)
    om = util.OracleModel(model, orc)
    ctx = b.Context(model)
    n = 1000
    x = torch.empty((n, 256), dtype=torch.int8, device="cuda")
    cls = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    lg = torch.empty((n, model.num_classes), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        synth.fill_device(x, first=0, dist=DIST_U)
        ctx.infer_device(x, cls, lg)             # first use on this stream: allocations happen here, not under capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.infer_device(x, cls, lg)
    for k in range(3):
        xin = synth.images(31 + 4099 * k, n, DIST_M if k == 1 else DIST_U)
        x.copy_(torch.from_numpy(xin).cuda())
        cls.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_cls, want_lg = om.infer(xin, logits=True)
        assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want_cls) and np.array_equal(lg.cpu().numpy(), want_lg), (name, k)
    ctx.close()


def test_one_kernel_calls_capture_without_a_warm_up(gpu_ok, orc):
    """The fused float-input call and the one-kernel CNN call are ONE dispatch each and use no scratch (a captured launch takes a
    preallocated counter block): they can be captured into a HIP graph on a stream the context has never seen - no eager call first -
    and replayed on new inputs; ids (and the CNN's logits) against numpy quantisation / the oracle."""
    import torch
    from bitnetmcu_amd import harness
    # float images -> class ids
    model = util.load_golden_model("fc_4bitsym_64")
    ctx = b.Context(model)
    n = 5000
    xf = torch.zeros((n, 256), dtype=torch.float32, device="cuda")
    cls = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.infer_float_device(xf, cls)
    assert ctx.last_kernel == "fused_fc_f32_kernel"
    rng = np.random.default_rng(3)
    for k in range(3):
        x = (rng.normal(size=(n, 256)) * (10.0 ** (k - 1))).astype(np.float32)
        xf.copy_(torch.from_numpy(x).cuda())
        cls.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(cls.cpu().numpy().astype(np.uint32), util.OracleModel(model, orc).infer(harness.quantize_input(x))), k
    ctx.close()
    # CNN, one kernel (named, so that the call's size does not send it to the channel kernel)
    model = util.load_golden_model("mcu_cnn_48")
    ctx = b.Context(model)
    ctx.set_cnn_variant(3)
    n = 777
    x8 = torch.zeros((n, 256), dtype=torch.int8, device="cuda")
    cls = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    lg = torch.empty((n, model.num_classes), dtype=torch.int32, device="cuda")
    side2 = torch.cuda.Stream()
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side2):
        ctx.infer_device(x8, cls, lg)
    assert ctx.last_kernel == "cnn_li_fused_pipe_kernel"
    for k in range(3):
        xin = synth.images(1000 * k, n, DIST_U)
        x8.copy_(torch.from_numpy(xin).cuda())
        cls.fill_(-1)
        torch.cuda.synchronize()
        g2.replay()
        torch.cuda.synchronize()
        want_cls, want_lg = util.OracleModel(model, orc).infer(xin, logits=True)
        assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want_cls) and np.array_equal(lg.cpu().numpy(), want_lg), k
    ctx.close()


@pytest.mark.parametrize("name", ["fc_4bitsym_64", "tern_96", "cnn_64"])
def test_ragged_and_empty_batches(name, gpu_ok, orc):
    model = util.load_golden_model(name)
    om = util.OracleModel(model, orc)
    ctx = b.Context(model)
    x = synth.images(42, 4200, DIST_M)
    want_cls, want_lg = om.infer(x, logits=True)
    for label, setup in paths_for(ctx):
        setup(ctx)
        for n in (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 1000, 4099):
            cls, lg = ctx.infer(x[:n], logits=True)
            assert cls.shape == (n,) and np.array_equal(cls, want_cls[:n]), (name, label, n)
            assert np.array_equal(lg, want_lg[:n]), (name, label, n)
            assert np.array_equal(ctx.infer(x[:n]), want_cls[:n])          # class ids only (no logits buffer)
    ctx.close()


@pytest.mark.parametrize("name", ["fc_4bitsym_64", "tern_96"])
def test_latency_path_words_written_once(name, gpu_ok, orc):
    """n <= 64 host images, class ids only: bnm_infer_host polls the page-locked class words and takes the first change of a word as
    the result, so no kernel may write a word twice (a placeholder store in the dual kernel's first iteration once did).  Different
    images on every call, so a stale buffer cannot pass for a result."""
    model = util.load_golden_model(name)
    om = util.OracleModel(model, orc)
    ctx = b.Context(model)
    for k in range(12):
        n = (64, 64, 33, 64, 1, 64)[k % 6]
        x = synth.images(7000 + 977 * k, n, DIST_U if k & 1 else DIST_M)
        want = om.infer(x)
        for _ in range(3):
            assert np.array_equal(ctx.infer(x), want), (name, k, n)
    ctx.close()


def test_device_pointer_api_does_not_touch_neighbours(gpu_ok, orc):
    """Ragged n on device buffers: nothing is written past cls[n] / logits[n]."""
    import torch
    model = util.load_golden_model("fc_4bitsym_64")
    ctx = b.Context(model)
    for variant in (0, 1, 2, 3):
        ctx.set_tuning(variant=variant)
        for n in (1, 33, 63, 64, 65, 1000, 70000):
            imgs = torch.empty((n, 256), dtype=torch.int8, device="cuda")
            synth.fill_device(imgs, first=9, dist=DIST_U)
            cls = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda")
            lg = torch.full((n + 64, 10), -7, dtype=torch.int32, device="cuda")
            ctx.infer_device(imgs, cls, lg)
            torch.cuda.synchronize()
            want_cls, want_lg = util.OracleModel(model, orc).infer(imgs.cpu().numpy(), logits=True)
            assert np.array_equal(cls[:n].cpu().numpy().astype(np.uint32), want_cls)
            assert np.array_equal(lg[:n].cpu().numpy(), want_lg)
            assert (cls[n:] == -7).all() and (lg[n:] == -7).all()
    ctx.close()


def test_relunorm_extremes_through_model_path(gpu_ok, orc):
    """Images engineered to hit ReLUNorm's corners inside the fused kernel: all-zero input (every layer all zero,
    argmax tie -> index 0), saturated inputs, and single-pixel inputs."""
    x = np.zeros((70, 256), np.int8)
    x[1] = 127
    x[2] = -128
    for i in range(3, 67):
        x[i, (i * 37) % 256] = 127 if i % 2 else -128
    x[67, ::2], x[67, 1::2] = 127, -128
    x[68] = np.arange(256).astype(np.int8)
    x[69] = -1
    for name in ("fc_4bitsym_64", "mcu_1k", "mcu_12k_fp130", "tern_96", "cnn_64"):
        model = util.load_golden_model(name)
        want = util.OracleModel(model, orc).infer(x, logits=True)
        ctx = b.Context(model)
        for label, setup in paths_for(ctx):
            setup(ctx)
            got = ctx.infer(x, logits=True)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, label)
        ctx.close()


def test_input_quantisation_matches_numpy_float32(gpu_ok):
    """the Python-side quantisation step (test_inference.py:140-141) on the GPU."""
    import torch
    from bitnetmcu_amd import harness
    rng = np.random.default_rng(11)
    x = rng.normal(size=(5000, 256)).astype(np.float32)
    x[0] = 0.0                                   # max|x| below the 1e-5 floor
    x[1] = np.linspace(-1, 1, 256, dtype=np.float32) * 127 / 127   # many exact .5 ties after scaling
    x[2, :] = 0.5; x[2, 0] = 127.0               # x*scale = 0.5 exactly -> rounds to even (0)
    x[3, :] = -1.5; x[3, 0] = 127.0              # -1.5 -> -2
    x[4] = rng.integers(-300, 300, 256).astype(np.float32) / 2.0
    x[4, 0] = 150.0
    x[5] = x[5] * 1e-7                           # tiny values, scale hits the floor
    x[6] = x[6] * 1e20
    ctx = b.Context(util.load_golden_model("mcu_1k"))
    q = ctx.quantize_device(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.array_equal(q, harness.quantize_input(x))
    # and the two steps chained on device == the reference's per-image Python flow
    cls = torch.empty(len(x), dtype=torch.int32, device="cuda")
    ctx.infer_device(ctx.quantize_device(torch.from_numpy(x).cuda()), cls)
    want_cls, want_lg = util.OracleModel(ctx.model).infer(harness.quantize_input(x), logits=True)
    assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want_cls)
    # ... and as ONE call (bnm_infer_float_device), on a side stream, with logits
    side = torch.cuda.Stream()
    xd = torch.from_numpy(x).cuda()
    cls2 = torch.full((len(x),), -1, dtype=torch.int32, device="cuda")
    lg2 = torch.empty((len(x), ctx.model.num_classes), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ctx.infer_float_device(xd, cls2, lg2)
    side.synchronize()
    assert np.array_equal(cls2.cpu().numpy().astype(np.uint32), want_cls) and np.array_equal(lg2.cpu().numpy(), want_lg)
    ctx.close()
    # a CNN model through the same call
    cctx = b.Context(util.load_golden_model("mcu_cnn_16"))
    cls3 = torch.empty(len(x), dtype=torch.int32, device="cuda")
    cctx.infer_float_device(xd, cls3)
    torch.cuda.synchronize()
    assert np.array_equal(cls3.cpu().numpy().astype(np.uint32), util.OracleModel(cctx.model).infer(harness.quantize_input(x)))
    cctx.close()


def _float_edge_rows(rng, n):
    """Float images with the quantisation's edge cases in the first rows (test_inference.py:140-141)."""
    x = rng.normal(size=(n, 256)).astype(np.float32)
    k = min(n, 12)
    e = np.array(x[:12])
    e[0] = 0.0                                    # max|x| below the 1e-5 floor: scale 127 / 1e-5, every value 0
    e[1] = np.linspace(-1, 1, 256, dtype=np.float32)
    e[2, :] = 0.5; e[2, 0] = 127.0               # x * scale = 0.5 exactly -> rounds to even (0)
    e[3, :] = -1.5; e[3, 0] = 127.0              # -1.5 -> -2
    e[4] = rng.integers(-300, 300, 256).astype(np.float32) / 2.0      # many exact .5 ties
    e[4, 0] = 150.0
    e[5] = e[5] * 1e-7                           # tiny values, scale hits the floor
    e[6] = e[6] * 1e20
    e[7, :] = 2.5; e[7, 17] = -127.0             # the maximum is a negative value
    e[8] = rng.integers(-127, 128, 256).astype(np.float32); e[8, 255] = 127.0   # integers: quantise to themselves
    e[9] = -e[8]
    e[10] = 1e-5 * np.sign(e[10])                # exactly the floor
    e[11] = np.float32(3.0e38) * np.sign(e[11])  # near FLT_MAX: the scale is subnormal-free but tiny
    x[:k] = e[:k]
    return x


FLOAT_MODELS = ["fc_4bitsym_64", "mcu_1k", "mcu_12k", "mcu_12k_fp130", "tern_96", "tern_96_sparse", "doc12k_ternary", "doc12k_2bit",
                "doc12k_8bit", "doc12k_binary"]


@pytest.mark.parametrize("name", FLOAT_MODELS)
def test_fused_float_input_kernel_equals_quantise_then_oracle(name, gpu_ok, orc):
    """SURVEY.md 8(f) row 1, fused: float32 images -> class ids (and logits) in ONE kernel (bnm_fused_f32_kernel.hpp) must equal
    numpy's float32 quantisation (harness.quantize_input = test_inference.py:140-141) followed by the oracle: every FC model of the
    zoo, both landing depths, ragged sizes (tiles, 8-image groups, one image), a one-workgroup grid (many units and work-counter
    takes per wave), batches of one unit (a take per unit), a side stream; and the two-kernel path of the same call."""
    import torch
    from bitnetmcu_amd import harness
    model = util.load_golden_model(name)
    ctx = b.Context(model)
    om = util.OracleModel(model, orc)
    rng = np.random.default_rng(1234)
    x = _float_edge_rows(rng, 70001)
    q = harness.quantize_input(x)
    want_cls, want_lg = om.infer(q, logits=True)
    xd = torch.from_numpy(x).cuda()
    ncls = model.num_classes
    expect_fused = True                           # (every FC model of the zoo: tile classes 2, 4 and - 160-160-160 - 6)
    assert ctx.float_fused == expect_fused, name
    modes = [(0, 0), (2, 0)]
    try:
        ctx.set_float_mode(1, 2)
        modes.append((1, 2))
    except b.BnmError:
        assert name == "doc12k_binary"             # (the 6-tile class holds one group only)
    try:
        ctx.set_float_mode(1, 4)
        modes.append((1, 4))
    except b.BnmError:
        pass                                       # (the 4-tile class holds two groups only)
    side = torch.cuda.Stream()
    for mode, groups in modes:
        ctx.set_float_mode(mode, groups)
        assert ctx.float_fused == (expect_fused and mode != 2)
        for n in (70001, 4099, 1000, 255, 33, 32, 31, 9, 8, 7, 1):
            for grid, batch, logits in ((0, 0, True), (1, 1, False), (1, 3, True)):
                if n < 4099 and grid:
                    continue
                ctx.set_tuning(grid_blocks=grid)
                ctx.set_work_batch(batch)
                cls = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                lg = torch.full((n, ncls), -1, dtype=torch.int32, device="cuda") if logits else None
                torch.cuda.synchronize()
                with torch.cuda.stream(side):
                    ctx.infer_float_device(xd[:n], cls, lg)
                side.synchronize()
                assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want_cls[:n]), (name, mode, groups, n, grid, batch)
                if logits:
                    assert np.array_equal(lg.cpu().numpy(), want_lg[:n]), (name, mode, groups, n, grid, batch)
        ctx.set_tuning(grid_blocks=0)
        ctx.set_work_batch(0)
    # an input that is not at the start of an allocation (16-byte aligned, not 1 KiB aligned to a tile)
    ctx.set_float_mode(0)
    cls = torch.empty(5000, dtype=torch.int32, device="cuda")
    ctx.infer_float_device(xd[37:5037], cls)
    torch.cuda.synchronize()
    assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want_cls[37:5037])
    ctx.close()


@pytest.mark.parametrize("name", [n for n in MODEL_NAMES if "cnn" in n])
def test_float_input_cnn_in_one_kernel(name, gpu_ok, orc):
    """SURVEY 8(f) row 1 for the CNN models: float images -> class ids (+ logits) in ONE kernel - the one-kernel CNN form with the
    input quantisation in front of its convolution operands (cnn_li_fused_kernel<., true>) - against numpy's float32 quantisation +
    the oracle: every CNN of the zoo, the front end named (every call size runs it) and left to the context (small calls: two
    kernels on the channel path), ragged tiles, edge rows, logits, the two-kernel form of the same call."""
    import torch
    from bitnetmcu_amd import harness
    model = util.load_golden_model(name)
    om = util.OracleModel(model, orc)
    C = model.layer(0).out_channels
    rng = np.random.default_rng(77)
    n_all = max(3000, 2 * C * C + 70)
    x = _float_edge_rows(rng, n_all)
    want_cls, want_lg = om.infer(harness.quantize_input(x), logits=True)
    xd = torch.from_numpy(x).cuda()
    for named in (True, False):
        ctx = b.Context(model)
        assert ctx.float_fused and ctx.cnn_tail_fused, name
        if named:
            ctx.set_cnn_variant(3)
        for mode in (0, 2):
            ctx.set_float_mode(mode)
            for n in (n_all, 1000, 33, 32, 31, 1):
                cls = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                lg = torch.full((n, model.num_classes), -1, dtype=torch.int32, device="cuda")
                ctx.infer_float_device(xd[:n], cls, lg)
                torch.cuda.synchronize()
                one = mode == 0 and (named or n >= 2 * C * C)
                if one:
                    assert ctx.last_kernel == "cnn_li_fused_pipe_kernel<float>", (name, named, mode, n, ctx.last_kernel)      # (zoo models: conv1 sums < 2^16)
                else:
                    assert ctx.last_kernel.startswith("quantize_input_kernel+"), (name, named, mode, n, ctx.last_kernel)
                assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want_cls[:n]), (name, named, mode, n)
                assert np.array_equal(lg.cpu().numpy(), want_lg[:n]), (name, named, mode, n)
        ctx.close()


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_fused_float_input_kernel_on_random_models(seed, gpu_ok, orc):
    """Random FC models (a codec per layer out of all seven - FP1.3.0's +128 second weight plane among them -, widths up to 192:
    the 2-, 4- and 6-tile classes of the kernel -, 2 to 64 classes) through the float-input kernel vs numpy quantisation + oracle."""
    import torch
    from bitnetmcu_amd import harness
    rng = np.random.default_rng(4400 + seed)
    n_layers = int(rng.choice([3, 4]))
    codecs = tuple(int(c) for c in rng.choice([1, 2, 4, 12, 16, 20, 64], size=n_layers))
    need = {1: 32, 2: 16, 4: 8, 12: 8, 20: 8, 16: 4, 64: 8}
    widths = []
    for k in range(1, n_layers):
        g = need[codecs[k]]
        hi = int(rng.choice([32, 64, 128, 192]))
        widths.append(int(rng.integers(1, hi // g + 1)) * g)
    n_classes = int(rng.integers(2, 65))
    model = b.Model.from_header_text(_random_model_text(rng, codecs, tuple(widths), n_classes))
    ctx = b.Context(model)
    # (a model whose weights - two planes for FP1.3.0's +128 - leave LDS for fewer than four waves runs the two-kernel path)
    x = _float_edge_rows(rng, 3001)
    x[11] /= np.float32(64.0)                     # (the near-FLT_MAX row stays finite under the scale below: inputs are finite by contract)
    x = x * np.float32(rng.choice([1e-3, 1.0, 37.5]))
    assert np.isfinite(x).all()
    want_cls, want_lg = util.OracleModel(model, orc).infer(harness.quantize_input(x), logits=True)
    xd = torch.from_numpy(x).cuda()
    for n in (3001, 64, 5):
        cls = torch.empty(n, dtype=torch.int32, device="cuda")
        lg = torch.empty((n, n_classes), dtype=torch.int32, device="cuda")
        ctx.infer_float_device(xd[:n], cls, lg)
        torch.cuda.synchronize()
        assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want_cls[:n]), (codecs, widths, n_classes, n)
        assert np.array_equal(lg.cpu().numpy(), want_lg[:n]), (codecs, widths, n_classes, n)
    ctx.close()


def test_processfclayer_same_array_two_geometries(gpu_ok, bnm, orc):
    """the symbols' device-side weight cache is keyed by the layer geometry too.  One host array presented as 64 -> 32
    and as 32 -> 64 four-bit weights (both 1024 bytes), and one ternary array as 40 -> 8 and 20 -> 16: every call equals the oracle,
    and the activation buffer of the narrower call is exactly as long as that call says (a stale wider n_act would read past it)."""
    f, o = util.Funcs(bnm), util.Funcs(orc, "orc_")
    rng = np.random.default_rng(99)
    w4 = rng.integers(0, 2**32, size=256, dtype=np.uint64).astype(np.uint32)           # 1024 bytes
    for n_in, n_out in ((64, 32), (32, 64), (64, 32), (32, 64)):
        act = rng.integers(-128, 128, n_in).astype(np.int8)
        assert np.array_equal(f.processfclayer(act, w4, 4, n_in, n_out), o.processfclayer(act, w4, 4, n_in, n_out)), (n_in, n_out)
    trits = rng.integers(0, 3, size=(32, 10))
    w16 = np.array([int(np.ceil(int("".join(map(str, t)), 3) * 65536 / 59049)) for t in trits], dtype=np.uint16)   # exportquant.py:139-157
    for n_in, n_out in ((40, 8), (20, 16), (40, 8)):
        act = rng.integers(-128, 128, n_in).astype(np.int8)
        assert np.array_equal(f.processfclayer(act, w16, 64, n_in, n_out), o.processfclayer(act, w16, 64, n_in, n_out)), (n_in, n_out)


def test_last_kernel_names_what_the_call_ran(gpu_ok):
    """bnm_ctx_get_cnn_variant is the SETTING; bnm_ctx_last_kernel names what the last call really launched -
    on both sides of an AUTO context's 2 C^2 small-call threshold, for a named front end, for the FC remainders and for the float
    paths - and bench.py's kernel_name() (the key of the replayed counters) agrees with it."""
    import torch
    sys.path.insert(0, util.REPO)
    import bench
    x = torch.empty((20000, 256), dtype=torch.int8, device="cuda")
    synth.fill_device(x, first=0, dist=DIST_U)
    cls = torch.empty(20000, dtype=torch.int32, device="cuda")

    def ran(ctx, n):
        ctx.infer_device(x[:n], cls[:n])
        torch.cuda.synchronize()
        return ctx.last_kernel

    model = util.load_golden_model("cnn_64")
    ctx = b.Context(model)
    assert ctx.last_kernel == ""
    C = model.layer(0).out_channels
    assert C == 64 and ctx.cnn_variant == 3
    for n, front in ((2 * C * C - 1, "cnn_front_mfma_kernel"), (2 * C * C, "cnn_li_fused_pipe_kernel"), (1, "cnn_front_mfma_kernel")):
        got = ran(ctx, n)
        assert got.split("+")[0] == front, (n, got)
        assert ctx._lib.bnm_ctx_get_cnn_variant(ctx._h) == 3             # the setting does not move
        assert set(bench.kernel_name(b, ctx, model, n, False).split("+")) == set(got.split("+")), (n, got)
    ctx.set_cnn_variant(3)                                               # named: holds for every call size
    assert ran(ctx, 7) == "cnn_li_fused_pipe_kernel"                     # (front end + FC tail: the call's only launch; the pipelined form)
    assert ctx.cnn_pipelined
    ctx.set_cnn_variant(6)                                               # the four-waves-per-SIMD form of the same
    assert ran(ctx, 7) == "cnn_li_fused_kernel" and not ctx.cnn_pipelined
    assert bench.kernel_name(b, ctx, model, 7, True) == "cnn_li_fused_kernel"
    ctx.set_cnn_variant(4)                                               # the tail as its own launch
    assert ran(ctx, 7) == "cnn_li_kernel+fused_fc_kernel"
    ctx.set_cnn_variant(1)
    assert ran(ctx, 20000).split("+")[0] == "cnn_front_mfma_kernel"
    ctx.set_cnn_variant(0)
    assert ran(ctx, 100).split("+")[0] == "cnn_front_kernel"
    ctx.close()

    model = util.load_golden_model("fc_4bitsym_64")
    ctx = b.Context(model)
    assert ran(ctx, 1000) == "fused_fc_dual_kernel+fused_fc_kernel"       # 15 pairs + 40 images
    assert ran(ctx, 960) == "fused_fc_dual_kernel"
    assert ran(ctx, 5) == "fused_fc_kernel"
    ctx.set_tuning(variant=4)
    assert ran(ctx, 1000) == "fused_fc_generic_kernel"
    ctx.set_tuning(variant=6)
    ctx.set_path(b.PATH_LAYERWISE_MFMA)
    assert ran(ctx, 100) == "fc_layer_mfma_kernel+relunorm_kernel"
    ctx.set_path(b.PATH_AUTO)
    xf = synth.float_images_device(x[:1000])
    ctx.infer_float_device(xf, cls[:1000])
    torch.cuda.synchronize()
    assert ctx.last_kernel == "fused_fc_f32_kernel" and ctx.float_fused
    ctx.set_float_mode(2)
    ctx.infer_float_device(xf, cls[:1000])
    torch.cuda.synchronize()
    assert ctx.last_kernel == "quantize_input_kernel+fused_fc_dual_kernel+fused_fc_kernel" and not ctx.float_fused
    ctx.close()
    ctx = b.Context(util.load_golden_model("tern_96"))
    ctx.set_path(b.PATH_TERNARY_ALU)
    assert ran(ctx, 100) == "ternary_stream_kernel"
    ctx.set_ternary_variant(0)
    assert ran(ctx, 100) == "ternary_alu_kernel"
    ctx.close()


def test_mixed_stream_probe_writes_the_fold_of_what_it_read(gpu_ok):
    """bnm_stream_rw_device (bench.py's yardstick for the ids + logits row): every 32-row tile's 32 x 44 output bytes are the XOR
    fold of the tile's eight 1 KiB slices, 16-byte unit i of the output = unit i mod 64 of the fold; rows beyond the last whole
    tile are left alone."""
    import torch
    n = 32 * 37 + 5
    x = torch.from_numpy(synth.images(4, n, DIST_U)).cuda()
    tiles = n // 32
    src = x.cpu().numpy().view(np.uint32)[:tiles * 32].reshape(tiles, 8, 64, 4)      # [tile][slice][lane][dword]
    fold = np.bitwise_xor.reduce(src, axis=1)                                           # [tile][lane][dword]
    units = 32 * 44 // 16
    want = np.stack([fold[:, i % 64] for i in range(units)], axis=1).reshape(-1)
    for mode in (0, 1, 4 + 16, 8 + 32 * 4):      # tiles per batch (37 tiles: ragged batches), plain stores, six waves per SIMD
        out = torch.full((n * 44 // 4 + 16,), -1, dtype=torch.int32, device="cuda")
        synth.stream_rw_device(x, out, 44, mode)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:tiles * units * 4], want) and (got[tiles * units * 4:] == 0xFFFFFFFF).all(), mode


BENCH_CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                       "dtype", "data", "config", "roofline")


def _check_bench_stdout(stdout):
    """The LAST stdout line is the one the driver parses: the only line that starts with '{', under 4 KB,
    the contract's keys in it."""
    import json
    lines = stdout.splitlines()
    js = [l for l in lines if l.startswith("{")]
    assert len(js) == 1 and lines[-1] == js[0], "ONE JSON line, the last of stdout, from rank 0"
    assert len(js[0]) < 4096, len(js[0])
    c = json.loads(js[0])
    for k in BENCH_CONTRACT_KEYS:
        assert k in c, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms", "algorithmic_bytes_per_launch"):
        assert k in c["roofline"], k
    assert "workload" in c["config"]
    return c


def test_bench_dump_outputs_are_the_last_timed_step(gpu_ok, orc, tmp_path):
    """bench.py --dump-outputs DIR: the class ids and logits the timed call returned, every image of a small run, equal the oracle's;
    --steps sets the number of timed steps the line reports."""
    import json
    import subprocess
    import sys
    d = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(util.REPO, "bench.py"), "--images", "20000", "--steps", "2", "--warmup", "1",
                          "--logits", "--no-cpu", "--no-extra", "--full-json", str(tmp_path / "full.json"), "--dump-outputs", str(d)],
                         capture_output=True, text=True, timeout=900)
    c = _check_bench_stdout(out.stdout)
    assert c["steps"] == 2 and c["warmup"] == 1 and c["verified_vs_oracle"] is True
    assert np.array_equal(np.load(d / "image_index.npy"), np.arange(20000))
    want_cls, want_logits = util.OracleModel(util.load_golden_model("fc_4bitsym_64"), orc).infer(synth.images(0, 20000, DIST_U), logits=True)
    cls, logits = np.load(d / "class_ids.npy"), np.load(d / "logits.npy")
    assert cls.dtype == np.float32 and logits.dtype == np.float64
    assert np.array_equal(cls, want_cls) and np.array_equal(logits, want_logits)
    assert json.load(open(tmp_path / "full.json"))["steps"] == 2


def test_bench_json_contract(gpu_ok, tmp_path):
    """bench.py on a small N: ONE short JSON line with the contract's keys as the last stdout line, every detail in the full record
    (--full-json), verified against the oracle."""
    import json
    import subprocess
    import sys
    full = str(tmp_path / "full.json")
    out = subprocess.run([sys.executable, os.path.join(util.REPO, "bench.py"), "--images", "300000", "--steps", "3", "--warmup", "1",
                          "--cpu-seconds", "1", "--full-json", full], capture_output=True, text=True, timeout=900)
    c = _check_bench_stdout(out.stdout)
    d = json.load(open(full))
    # the compact line against the full record
    assert c["n_gpus"] == 1 and c["steps"] == 3 and c["warmup"] == 1 and c["dtype"] == "i8" and c["vs_baseline"] is None
    assert abs(c["value"] - d["value"]) <= 1e-4 * d["value"] and abs(c["ms_per_step"] - d["ms_per_step"]) <= 1e-4 * d["ms_per_step"]
    assert abs(c["roofline"]["frac"] - d["roofline"]["frac"]) < 1e-4 and c["roofline"]["kernel"] == d["roofline"]["kernel"]
    assert c["verified_vs_oracle"] is True and c["cpu_baseline"]["value"] > 0 and c["cpu_baseline"]["kind"] in ("reference", "port")
    assert c["roofline"]["stream_read"]["GB/s"] > 0 and 0 < c["roofline"]["mfma"]["frac"] < 1 and 0 < c["roofline"]["mfma"]["busy_frac"] < 1
    assert set(c["rows"]) == set(k for k in d["extra_configs"] if "roofline" in d["extra_configs"][k])
    assert all(v[3] is True and v[0] > 0 and 0 < v[2] <= 1 for v in c["rows"].values()), c["rows"]
    assert c["rows_cpu"]["cnn_64"] > 0 and c["rows_cpu"]["ternary_alu"] > 0
    # ... and the '# ' lines carry the same detail on stdout
    assert any(l.startswith("# row cnn_64 {") for l in out.stdout.splitlines()) and any(l.startswith("# full {") for l in out.stdout.splitlines())
    for k in BENCH_CONTRACT_KEYS + ("cpu_baseline",):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["dtype"] == "i8" and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["verified_vs_oracle"] is True and "workload" in d["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "stream_read", "time_vs_stream_read", "median_launch_ms"):
        assert k in d["roofline"]
    assert 0 < d["roofline"]["frac"] <= 1 and d["roofline"]["stream_read"]["GB/s"] > 0
    # north_star: int8 MFMA utilisation vs the gfx950 peak on the MFMA path - static count x measured rate, busy share replayed from
    # a counter pass of the SAME kernel binary (code hash checked by bench.load_counters)
    mf = d["roofline"]["mfma"]
    assert mf["per_image"] == 26 / 32 and mf["peak_per_s"] == 1024 * 2.4e9 / 32
    assert abs(mf["achieved_per_s"] - d["value"] * 26 / 32) < 1e-6 * mf["achieved_per_s"] and 0 < mf["frac"] < 1
    assert 0 < mf["busy_frac"] < 1 and "code_sha1" in mf["busy_frac_source"]
    assert d["roofline"]["traffic"] is None      # (replayed for the headline workload - 1e8 images - only)
    # the headline row parses the REFERENCE'S OWN header bytes (a staged byte-identical copy of
    # BitNetMCU_model_fc.h: tests/golden/_ref_headers/, oracle/build_oracle.py), and so does the CNN row
    assert d["digest"].startswith("0x") and "the reference's own BitNetMCU_model_fc.h" in d["config"]["model_source"], d["config"]["model_source"]
    assert d["roofline"]["launched"] == "fused_fc_dual_kernel+fused_fc_kernel"      # 300,000 = 4,687 pairs + 32 images
    ex = d["extra_configs"]
    assert "the reference's own BitNetMCU_model_cnn.h" in ex["cnn_64"]["model_source"]
    # float images -> class ids in ONE kernel, its own HBM roofline on 1,028 bytes per inference
    fl = ex["fc_float_input"]
    assert fl["verified_vs_oracle"] is True and fl["kernel"] == "fused_fc_f32_kernel" and fl["launches_per_step"] == 1
    assert fl["roofline"]["algorithmic_bytes_per_inference"] == 1028 and 0 < fl["roofline"]["frac"] <= 1
    assert ex["fc_float_input_two_kernels"]["kernel"].startswith("quantize_input_kernel+") and ex["fc_float_input_two_kernels"]["verified_vs_oracle"] is True
    # the CNN is one launch per call; its row says what binds it in the kernel's own terms
    assert ex["cnn_64"]["launched"] in ("cnn_li_fused_pipe_kernel", "cnn_front_mfma_kernel+fused_fc_kernel")
    assert "int8_ops_algorithmic" in ex["cnn_64"]["roofline"] and ex["cnn_64"]["roofline"]["int8_ops_algorithmic"]["per_image"] == 2 * 236416
    # the whole-model QAT forward has a row of its own (HBM roofline on 1,024 + 40 bytes per row)
    qf = ex["qat_fc_forward"]
    assert qf["verified_vs_oracle"] is True and qf["rows"] == 300000 and qf["roofline"]["algorithmic_bytes_per_row"] == 1064 and 0 < qf["roofline"]["frac"] <= 1
    # the CNN row's MFMA count is the kernel's own (bnm_ctx_cnn_planes): 14 + 24 + 2 x 2 per channel and tile x 64 channels / 32 + the tail's 5
    assert ex["cnn_64"]["roofline"]["mfma"]["per_channel_tile"] == 42 and ex["cnn_64"]["roofline"]["mfma"]["per_image"] == 85.0
    assert ex["cnn_64"]["steps"] >= 10 and ex["cnn_64"]["warmup"] >= 2
    for k in ("ternary_alu", "ternary_mfma_generic", "cnn_64", "fc_generic_kernel", "fc_logits", "fc_dist_m", "doc12k_binary",
              "doc12k_ternary", "doc12k_2bit", "doc12k_8bit"):
        assert ex[k]["verified_vs_oracle"] is True and ex[k]["value"] > 0 and "roofline" in ex[k], k
        assert 0 < ex[k]["roofline"]["frac"] <= 1, k
    assert ex["ternary_alu"]["roofline"]["bound"] == "valu" and ex["cnn_64"]["roofline"]["bound"] == "valu"
    # the ids + logits row next to what its bytes cost with no arithmetic on this box (bnm_stream_rw_device)
    assert ex["fc_logits"]["roofline"]["stream_read_write"]["GB/s"] > 0 and ex["fc_logits"]["roofline"]["time_vs_stream_read_write"] > 0.5
    assert ex["ternary_alu"]["path"] == b.PATH_TERNARY_ALU and ex["ternary_mfma_generic"]["path"] == b.PATH_FUSED_MFMA
    # the VALU-bound configs quote the ALGORITHMIC fraction (MACs at 4 per dot4 lane), which can only be below the pipe's utilisation
    assert ex["ternary_alu"]["roofline"]["macs_per_image"] == 43968 and ex["cnn_64"]["roofline"]["macs_per_image"] == 236416
    if "pipe_utilisation" in ex["ternary_alu"]["roofline"]:
        assert ex["ternary_alu"]["roofline"]["frac"] <= ex["ternary_alu"]["roofline"]["pipe_utilisation"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"]
    for row in ("ternary_alu", "cnn_64"):          # configs[2] / configs[3] carry the reference's CPU rate as well
        assert ex[row]["cpu_baseline"]["value"] > 0 and ex[row]["cpu_baseline"]["kind"] in ("reference", "port")


def _fc_layer_lines(rng, k, bpw, n_in, n_out, trit_digits=None):
    """One FC layer of an exporter-dialect header with RANDOM packed weights.  Ternary layers get the exporter's padding to a
    multiple of 10 (pad trits = 0); trit_digits(layer, n_out, n_in) -> base-3 digits (0: +1, 1: -1, 2: 0) replaces the random trits."""
    if bpw == 64:
        padded = (n_in + 9) // 10 * 10
        trits = rng.integers(0, 3, size=(n_out, padded))
        if trit_digits is not None:
            trits[:, :n_in] = trit_digits(k, n_out, n_in)
        trits[:, n_in:] = 2                                   # pad = zero weight (exportquant.py:132-137)
        # base-3, most significant trit first, per 10-trit group (exportquant.py:146-156)
        g = trits.reshape(n_out, padded // 10, 10)
        v = np.zeros((n_out, padded // 10), np.int64)
        for t in range(10):
            v = v * 3 + g[:, :, t]
        w = ((v * 65536 + 59048) // 59049).astype(np.uint16).ravel()
        decl, n_decl = "uint16_t", padded
    else:
        fb = {1: 1, 2: 2, 4: 4, 12: 4, 20: 4, 16: 8}.get(bpw, 4)
        w = rng.integers(0, 2**32, size=n_out * (n_in * fb // 32), dtype=np.uint32)
        decl, n_decl = "uint32_t", n_in
    return [f"#define L{k}_active", f"#define L{k}_bitperweight {bpw}", f"#define L{k}_incoming_weights {n_decl}",
            f"#define L{k}_outgoing_weights {n_out}", f"const {decl} L{k}_weights[] = {{" + ",".join(hex(int(x)) for x in w) + "};"]


def _random_model_text(rng, codecs, widths, n_classes=10, trit_digits=None):
    """Header text of an FC model with RANDOM packed weights: every codec id through the whole-model kernels, in
    shapes of the fused table."""
    lines = ["#include <stdint.h>", "#define MODEL_FCMNIST", "#define NUM_LAYERS %d" % len(codecs), "#define MAX_N_ACTIVATIONS 256"]
    n_in = 256
    outs = list(widths) + [n_classes]
    for k, (bpw, n_out) in enumerate(zip(codecs, outs), start=1):
        lines += _fc_layer_lines(rng, k, bpw, n_in, n_out, trit_digits)
        n_in = n_out
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("codecs,widths", [
    ((1, 1, 1, 1), (64, 64, 64)),          # binary
    ((2, 2, 2, 2), (64, 64, 64)),
    ((12, 12, 12, 12), (64, 64, 64)),      # 4-bit two's complement
    ((16, 16, 16, 16), (64, 64, 64)),      # 8-bit: weights cannot be doubled -> DBL = false kernels
    ((16, 4, 1, 12), (64, 64, 64)),        # mixed
    ((20, 20, 20, 20), (64, 64, 64)),      # FP1.3.0 split path
    ((20, 4, 4, 4), (64, 64, 64)),
    ((64, 64, 64, 64), (96, 96, 96)),      # ternary, random trits (dense), exporter padding
    ((64, 4, 2, 4), (64, 64, 64)),         # ternary first layer + others (fused table shape)
    ((4, 4, 4), (16, 16)),                 # three-layer model
    ((36, 4, 4, 4), (64, 64, 64)),         # unknown codec (NF4 id): layer outputs zeros -> layer-wise path only
])
def test_random_models_every_codec_through_model_kernels(codecs, widths, gpu_ok, orc):
    rng = np.random.default_rng(hash((codecs, widths)) % 2**32)
    model = b.Model.from_header_text(_random_model_text(rng, codecs, widths))
    om = util.OracleModel(model, orc)
    x = np.concatenate([synth.images(5, 3000, DIST_U), synth.images(5, 3000, DIST_M), np.zeros((3, 256), np.int8),
                        np.full((3, 256), -128, np.int8), np.full((3, 256), 127, np.int8)])
    want = om.infer(x, logits=True)
    ctx = b.Context(model)
    labels = []
    for label, setup in paths_for(ctx):
        setup(ctx)
        got = ctx.infer(x, logits=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (codecs, label)
        labels.append(label)
    if 36 not in codecs:
        assert any(l.startswith("fused") for l in labels), (codecs, labels)
    ctx.close()


@pytest.mark.parametrize("n_classes", [1, 2, 7, 9, 16, 17, 32])
def test_dual_kernel_logits_for_other_class_counts(n_classes, gpu_ok, orc):
    """The dual-tile kernel stores a tile's logits through an LDS staging area when n_classes <= 16 (odd counts: rows that are only
    dword-aligned) and piecewise above; every fused variant, whole pairs + ragged remainders, ids and logits against the oracle."""
    rng = np.random.default_rng(9000 + n_classes)
    model = b.Model.from_header_text(_random_model_text(rng, (4, 4, 4, 4), (64, 64, 64), n_classes))
    om = util.OracleModel(model, orc)
    x = np.concatenate([synth.images(21, 4000, DIST_U), synth.images(21, 300, DIST_M)])
    want = om.infer(x, logits=True)
    ctx = b.Context(model)
    ran = []
    for label, setup in paths_for(ctx):
        if not label.startswith("fused"):
            continue
        setup(ctx)
        for n in (len(x), 4096, 193, 128, 64, 63):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (n_classes, label, n)
        ran.append(label)
    assert "fused_v6" in ran and "fused_v3" in ran, ran
    ctx.close()


@pytest.mark.parametrize("signs", ["-+-+", "+-+-", "----", "++++", "dense"])
def test_ternary_alu_kernels_extreme_sums(signs, gpu_ok, orc):
    """Ternary 256-96-96-96-10 models whose layers are all +1, all -1 or zero-free random trits, on all -128 / 127 / 0 / random
    images: layer sums reach -32768 .. +32768 (the streamed kernels park sums as saturated int16 pairs: +32768 is the one value
    that saturates) and every ReLUNorm shift from 0 to 9 occurs.  All three ALU kernels, ids and logits vs the oracle."""
    rng = np.random.default_rng(len(signs) * 131 + ord(signs[0]))

    def digits(k, n_out, n_in):
        if signs == "dense":
            return rng.integers(0, 2, size=(n_out, n_in))
        d = np.full((n_out, n_in), 0 if signs[k - 1] == "+" else 1)
        if k > 1:      # a few neurons of the other sign so that later layers see a mix
            d[::7] = 1 - d[::7]
        return d
    model = b.Model.from_header_text(_random_model_text(rng, (64, 64, 64, 64), (96, 96, 96), trit_digits=digits))
    om = util.OracleModel(model, orc)
    x = np.concatenate([np.full((70, 256), -128, np.int8), np.full((70, 256), 127, np.int8), np.zeros((5, 256), np.int8),
                        synth.images(11, 700, DIST_U), synth.images(11, 700, DIST_M),
                        np.where(np.arange(256) % 2 == 0, -128, 127).astype(np.int8)[None].repeat(3, 0)])
    want = om.infer(x, logits=True)
    ctx = b.Context(model)
    ctx.set_path(b.PATH_TERNARY_ALU)
    for tv in (2, 1, 12, 11, 0):
        ctx.set_ternary_variant(tv)
        for n in (len(x), 129, 128, 127, 65, 1):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (signs, tv, n)
    ctx.close()


@pytest.mark.parametrize("widths", [(128, 128, 112), (64, 64, 64), (128, 128, 128),
                                    # the streamed kernel's family beyond round 3's four-entry table: H1, H2 in {32, 64, 96, 128}, H3 = 16 k
                                    (32, 32, 16), (64, 96, 48), (128, 32, 80), (96, 128, 112), (32, 128, 128), (128, 64, 16), (96, 64, 32)])
@pytest.mark.parametrize("signs", ["-+-+", "++++", "dense"])
def test_ternary_alu_kernel_other_widths(widths, signs, gpu_ok, orc):
    """The no-MFMA path for the other ternary shapes of its table - among them the reference's documented 12 KB ternary model,
    128-128-112 (docs/documentation.md:169-183; padded input counts 260 / 130 / 130 / 120 as the exporter writes them): all +1 /
    mixed / zero-free random trits on extreme and synthetic images, ids and logits against the oracle; the MFMA path on the same
    model must agree as well."""
    rng = np.random.default_rng(sum(widths) * 7 + len(signs) + ord(signs[0]))

    def digits(k, n_out, n_in):
        if signs == "dense":
            return rng.integers(0, 2, size=(n_out, n_in))
        d = np.full((n_out, n_in), 0 if signs[k - 1] == "+" else 1)
        if k > 1:
            d[::7] = 1 - d[::7]
        return d
    model = b.Model.from_header_text(_random_model_text(rng, (64, 64, 64, 64), widths, trit_digits=digits))
    om = util.OracleModel(model, orc)
    x = np.concatenate([np.full((70, 256), -128, np.int8), np.full((70, 256), 127, np.int8), np.zeros((5, 256), np.int8),
                        synth.images(11, 700, DIST_U), synth.images(11, 700, DIST_M)])
    want = om.infer(x, logits=True)
    ctx = b.Context(model)
    assert ctx.path == b.PATH_FUSED_MFMA          # AUTO: the fastest bit-exact kernel
    got = ctx.infer(x, logits=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ctx.set_path(b.PATH_TERNARY_ALU)
    with pytest.raises(b.BnmError):
        ctx.set_ternary_variant(2)                # two images per lane: 96-96-96 only
    # 1: streamed weights, one image per lane, work counter (the default for these shapes); 11: fixed stride; 0: round 1's plain
    # kernel, which exists for the four shapes of its table only
    plain = widths in ((128, 128, 112), (64, 64, 64), (128, 128, 128))
    if not plain:
        with pytest.raises(b.BnmError):
            ctx.set_ternary_variant(0)
    for variant in (None, 1, 11) + ((0,) if plain else ()):
        if variant is not None:
            ctx.set_ternary_variant(variant)
        for n in (len(x), 129, 64, 1):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (widths, signs, variant, n)
            got = ctx.infer(x[:n])
            assert np.array_equal(got, want[0][:n]), (widths, signs, variant, n)
    ctx.close()


@pytest.mark.parametrize("widths,n_classes", [((96, 80, 32), 10),      # H2 is not a multiple of 32
                                               ((96, 64, 40), 10),      # H3 is not a multiple of 16
                                               ((160, 64, 32), 10),     # H1 beyond 128
                                               ((96, 96, 96), 70)])     # more than 64 classes
def test_ternary_alu_path_refuses_shapes_outside_its_family(widths, n_classes, gpu_ok):
    rng = np.random.default_rng(3)
    model = b.Model.from_header_text(_random_model_text(rng, (64, 64, 64, 64), widths, n_classes))
    ctx = b.Context(model)
    assert ctx.path == b.PATH_FUSED_MFMA
    with pytest.raises(b.BnmError):
        ctx.set_path(b.PATH_TERNARY_ALU)
    ctx.close()


def _random_cnn_text(rng, C, codecs, widths, n_classes=10, conv_weights=None):
    """Header text of a CNN model in the reference's topology (conv, conv, pool, conv, pool, 3 x FC;
    BitNetMCU_MNIST_dll.c:48-91) with C channels and RANDOM weights."""
    lines = ["#include <stdint.h>", "#define MODEL_CNNMNIST", "#define NUM_LAYERS 8", "#define MAX_N_ACTIVATIONS 256"]

    def conv(k, cin, xin):
        w = conv_weights(k) if conv_weights else rng.integers(-6, 7, size=9 * C)
        lines.extend([f"#define L{k}_active", f"#define L{k}_type BitConv2d", f"#define L{k}_in_channels {cin}", f"#define L{k}_out_channels {C}",
                      f"#define L{k}_incoming_x {xin}", f"#define L{k}_incoming_y {xin}", f"#define L{k}_outgoing_x {xin - 2}",
                      f"#define L{k}_outgoing_y {xin - 2}", f"#define L{k}_kernel_size 3", f"#define L{k}_stride 1", f"#define L{k}_padding 0",
                      f"#define L{k}_groups {1 if cin == 1 else C}", f"#define L{k}_bitperweight 8",
                      f"const int8_t L{k}_weights[] = {{" + ",".join(str(int(v)) for v in w) + "};"])

    def pool(k, xin):
        lines.extend([f"#define L{k}_active", f"#define L{k}_type MaxPool2d", f"#define L{k}_pool_size 2", f"#define L{k}_incoming_x {xin}",
                      f"#define L{k}_incoming_y {xin}", f"#define L{k}_outgoing_x {xin // 2}", f"#define L{k}_outgoing_y {xin // 2}"])
    conv(2, 1, 16)
    conv(4, C, 14)
    pool(6, 12)
    conv(7, C, 6)
    pool(9, 4)
    n_in = 4 * C
    for k, bpw, n_out in zip((11, 13, 15), codecs, list(widths) + [n_classes]):
        lines.extend(_fc_layer_lines(rng, k, bpw, n_in, n_out))
        n_in = n_out
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("codecs,widths,n_classes", [
    ((4, 4, 4, 4), (32, 32, 32), 10),           # one tile per layer
    ((4, 4, 4, 4), (128, 64, 64), 47),          # EMNIST-balanced head (models.py:83), 4-tile class
    ((4, 4, 4), (96, 64), 10),                  # three layers, 3-tile first layer
    ((4, 2, 4, 4), (48, 80, 24), 26),           # widths that are not multiples of 32
    ((16, 16, 16, 16), (128, 128, 96), 37),     # 8-bit: not doubled
    ((20, 20, 20, 20), (64, 64, 64), 10),       # FP1.3.0 with +128 present: second weight plane
    ((20, 20, 20, 20), (96, 128, 40), 12),      # the same in the 4-tile class
    ((4, 4, 4, 4), (200, 104, 56), 10),         # 8-tile class (one wave per SIMD)
    ((2, 4, 1, 4), (256, 32, 64), 62),          # 8-tile class, narrow tail, 62 classes
    ((64, 64, 64, 64), (64, 128, 32), 10),      # ternary through MFMA, exporter padding
])
def test_random_shapes_through_the_generic_fused_kernel(codecs, widths, n_classes, gpu_ok, orc):
    """VERDICT r01 missing #1: widths are free parameters of the reference's models (models.py:62-84); every shape must
    run through a fused kernel, bit-exact in class ids and logits, ragged batch sizes included."""
    rng = np.random.default_rng(hash((codecs, widths, n_classes)) % 2**32)
    text = _random_model_text(rng, codecs, widths, n_classes)
    if 20 in codecs:
        assert "7" in text     # random nibbles: +128 weights are present
    model = b.Model.from_header_text(text)
    om = util.OracleModel(model, orc)
    ctx = b.Context(model)
    assert ctx.path == b.PATH_FUSED_MFMA, "shape fell off the fused kernels"
    ctx.set_tuning(variant=4)
    for n in (1, 31, 33, 1000, 4097):
        x = np.concatenate([synth.images(11, n, DIST_U)[: (n + 1) // 2], synth.images(11, n, DIST_M)[: n // 2]])
        want = om.infer(x, logits=True)
        got = ctx.infer(x, logits=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (widths, n)
        assert np.array_equal(ctx.infer(x), want[0])          # class ids only (no logits buffer)
    edge = np.concatenate([np.zeros((3, 256), np.int8), np.full((3, 256), -128, np.int8), np.full((3, 256), 127, np.int8)])
    got, want = ctx.infer(edge, logits=True), om.infer(edge, logits=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ctx.close()


@pytest.mark.parametrize("name", ["tern_96", "tern_96_sparse", "doc12k_2bit", "doc12k_ternary"])
def test_register_resident_weight_kernel(name, gpu_ok, orc):
    """Variant 9 (bnm_fused_regw.hip: weight fragments in AccVGPRs at one wave per SIMD, hand-pipelined dual-tile loop with asm
    MFMAs; opt-in) on the shapes it is instantiated for - all fragments in registers (96-96-96, 112-96-96) and the hybrid with the
    classifier's fragments in LDS (128-128-112): class ids and logits == oracle on device-resident images, ragged ends
    (the last < 64 images go to the generic kernel), calls too small for the kernel (all of it goes there), ids-only calls,
    the ReLUNorm extremes; == the generic kernel on every one of a million images."""
    model = b.Model.from_zoo(name)
    om = util.OracleModel(model, orc)
    ctx = b.Context(model)
    ctx.set_tuning(variant=9)
    assert ctx.variant == 9 and ctx.path == b.PATH_FUSED_MFMA
    for n in (1, 63, 64, 65, 4097, 65536 + 37, 3 * 65536 + 64 * 5 + 1):
        x = np.concatenate([synth.images(7, n, DIST_U)[: (n + 1) // 2], synth.images(7, n, DIST_M)[: n // 2]])
        m = min(n, 70_000)
        want = om.infer(x[:m], logits=True)
        got = ctx.infer(x, logits=True)
        assert np.array_equal(got[0][:m], want[0]) and np.array_equal(got[1][:m], want[1]), (name, n)
        assert np.array_equal(ctx.infer(x), got[0])           # class ids only (no logits buffer)
        if n > m:                                             # the tail of the big batches: head of the reversed batch
            xr = np.ascontiguousarray(x[::-1])
            gr = ctx.infer(xr, logits=True)
            assert np.array_equal(gr[0][::-1], got[0]) and np.array_equal(gr[1][::-1], got[1]), (name, n, "order dependence")
            wt = om.infer(x[-20_000:], logits=True)
            assert np.array_equal(got[0][-20_000:], wt[0]) and np.array_equal(got[1][-20_000:], wt[1]), (name, n, "tail")
    edge = np.concatenate([np.zeros((64, 256), np.int8), np.full((64, 256), -128, np.int8), np.full((64, 256), 127, np.int8)] * 400)
    got, want = ctx.infer(edge, logits=True), om.infer(edge[:192], logits=True)
    assert np.array_equal(got[0][:192], want[0]) and np.array_equal(got[1][:192], want[1])
    assert np.array_equal(got[0].reshape(400, 192), np.tile(want[0], (400, 1)))
    # against the generic kernel on a million images
    import torch
    n = 1_000_000 + 77
    x = torch.empty((n, 256), dtype=torch.int8, device="cuda")
    b.synth.fill_device(x, first=5, dist=DIST_U)
    out = {}
    for variant in (9, 4):
        ctx.set_tuning(variant=variant)
        cls = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        lg = torch.full((n, model.num_classes), -7, dtype=torch.int32, device="cuda")
        ctx.infer_device(x, cls, lg)
        torch.cuda.synchronize()
        out[variant] = (cls.cpu().numpy(), lg.cpu().numpy())
    assert np.array_equal(out[9][0], out[4][0]) and np.array_equal(out[9][1], out[4][1])
    ctx.close()


def test_register_resident_weight_kernel_is_refused_for_other_shapes(gpu_ok):
    for name in ("fc_4bitsym_64", "doc12k_binary", "cnn_64"):
        ctx = b.Context(b.Model.from_zoo(name))
        before = ctx.variant
        with pytest.raises(b.BnmError):
            ctx.set_tuning(variant=9)
        assert ctx.variant == before
        ctx.close()


@pytest.mark.parametrize("C,codecs,widths,n_classes", [
    (24, (2, 4, 4), (96, 64), 10),      # 96-byte act rows -> padded to 128
    (40, (4, 4, 4), (64, 32), 10),      # 160 -> 256
    (80, (2, 4, 4), (96, 64), 10),      # the 80-wide CNN of docs/documentation.md:898: 320 -> 512, two channel groups
    (8, (4, 4, 4), (32, 32), 37),       # 32 -> 64; <= 16 channels: two images per front-end item
    (12, (16, 4, 4), (32, 32), 10),     # 48 -> 64
    (44, (4, 4, 4), (64, 32), 10),      # 32 channels one image per item + 12 channels two images per item, separate ReLUNorm
    (48, (2, 4, 4), (96, 64), 10),
    (72, (2, 4, 4), (96, 64), 10),      # 64 + 8
    (112, (4, 4, 4), (64, 64), 10),     # 64 + 32 + 16: all three kinds of segment
    (100, (16, 4, 4), (64, 64), 10),    # 64 + 32 + 4
    # the wide CNNs of docs/documentation_cnn.md:186-191: ternary first FC layer (padded input counts 320 / 390 / 520)
    (80, (64, 4, 4), (96, 64), 10),
    (96, (64, 4, 4), (96, 64), 10),
    (128, (64, 4, 4), (96, 64), 10),
    (64, (64, 4, 4), (96, 64), 10),     # ... and the same tail behind the fused 64-channel front end
    # odd channel counts (8-bit first FC layer: 4 C inputs need no padding): partly filled pair segments and blocks
    (5, (16, 4, 4), (32, 32), 10),
    (21, (16, 4, 4), (32, 32), 10),
    (37, (16, 4, 4), (64, 32), 10),
    (69, (16, 4, 4), (64, 32), 10),
    (127, (16, 4, 4), (64, 32), 10),
])
def test_random_cnn_channel_counts_through_the_generic_tail(C, codecs, widths, n_classes, gpu_ok, orc):
    rng = np.random.default_rng(C * 1000 + n_classes)
    model = b.Model.from_header_text(_random_cnn_text(rng, C, codecs, widths, n_classes))
    om = util.OracleModel(model, orc)
    ctx = b.Context(model)
    assert ctx.path == b.PATH_FUSED_MFMA
    x = np.concatenate([synth.images(3, 700, DIST_U), synth.images(3, 701, DIST_M), np.full((1, 256), -128, np.int8)])
    want = om.infer(x, logits=True)
    # front end: fixed shares, round 1's kernel, the default (dynamic batches)
    taps = {}
    for cv in (2, 0, 1):
        ctx.set_cnn_variant(cv)
        for n in (len(x), 1, 2, 3, 4, 7):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (C, cv, n)
        taps[cv] = ctx.activations(x[:301])       # the int8 activations after every ReLUNorm (the front end's 4 C bytes first)
    # the MFMA front end (pairs of images per item, fused ReLUNorm) against round 1's all-VALU kernel, an independent implementation
    assert np.array_equal(taps[1], taps[0]) and np.array_equal(taps[2], taps[0]), C
    ctx.set_path(b.PATH_LAYERWISE_ALU)
    got = ctx.infer(x, logits=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ctx.close()


@pytest.mark.parametrize("codecs,widths,n_classes", [
    ((4, 4, 4, 4), (320, 64, 64), 10),          # one layer wider than 256
    ((4, 2, 1, 4), (512, 512, 512), 10),        # everything wide: 16 tiles per layer, binary / 2-bit / 4-bit
    ((16, 16, 16, 16), (300, 200, 100), 26),    # 8-bit, widths that are not multiples of 32
    ((20, 20, 20, 20), (288, 96, 64), 10),      # FP1.3.0 with +128 present: second weight plane
    ((64, 64, 64, 64), (384, 120, 96), 10),     # ternary, exporter padding (260 / 390 / 120 / 100 declared inputs)
    ((4, 4, 4), (272, 40), 47),                 # three layers
])
def test_models_outside_the_fused_kernels_run_layerwise_on_the_matrix_cores(codecs, widths, n_classes, gpu_ok, orc, capfd, monkeypatch):
    """Shapes beyond the fused kernels (a layer wider than 256 outputs) used to fall to the bit-serial layer-wise kernels, a
    500x cliff.  They now run one int8 GEMM kernel per layer on the matrix cores (any widths) - loudly (a warning names the
    reason), bit-exact in class ids and logits against the oracle, and equal to the bit-serial path."""
    monkeypatch.delenv("BNM_QUIET", raising=False)          # the warning is part of what is tested
    rng = np.random.default_rng(hash((codecs, widths, n_classes)) % 2**32)
    model = b.Model.from_header_text(_random_model_text(rng, codecs, widths, n_classes))
    ctx = b.Context(model)
    assert ctx.path == b.PATH_LAYERWISE_MFMA
    err = capfd.readouterr().err
    assert "layer-wise MFMA path" in err and "wider than 256" in err
    om = util.OracleModel(model, orc)
    for n in (1, 31, 33, 127, 1000, 4097):
        x = np.concatenate([synth.images(11, n, DIST_U)[: (n + 1) // 2], synth.images(11, n, DIST_M)[: n // 2]])
        want = om.infer(x, logits=True)
        got = ctx.infer(x, logits=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (widths, n)
        assert np.array_equal(ctx.infer(x), want[0])
    edge = np.concatenate([np.zeros((3, 256), np.int8), np.full((3, 256), -128, np.int8), np.full((3, 256), 127, np.int8)])
    want = om.infer(edge, logits=True)
    got = ctx.infer(edge, logits=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ctx.set_path(b.PATH_LAYERWISE_ALU)
    got = ctx.infer(edge, logits=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(b.BnmError):
        ctx.set_path(b.PATH_FUSED_MFMA)
    ctx.close()


@pytest.mark.parametrize("seed", range(48))
def test_fuzz_random_models_every_available_path(seed, gpu_ok, orc):
    """Seeded fuzz over what the exporter can produce: 3 or 4 layers, a codec per layer out of all seven, widths from 8 to 320
    (whatever the next layer's packing allows: n_in x bits a multiple of 32, exportquant.py:97-98), 2 to 64 classes.  The library's
    own choice of kernel (fused specialised / generic - uniform or general path, any tile class - or layer-wise MFMA) and every
    other path the model can run must reproduce the oracle's class ids and logits on synthetic + extreme images, ragged sizes."""
    rng = np.random.default_rng(7000 + seed)
    n_layers = int(rng.choice([3, 4]))
    codecs = tuple(int(c) for c in rng.choice([1, 2, 4, 12, 16, 20, 64], size=n_layers))
    need = {1: 32, 2: 16, 4: 8, 12: 8, 20: 8, 16: 4, 64: 8}       # input count granularity of a layer with this codec
    widths = []
    for k in range(1, n_layers):
        g = need[codecs[k]]
        hi = int(rng.choice([64, 128, 200, 320]))
        widths.append(int(rng.integers(1, hi // g + 1)) * g)
    n_classes = int(rng.integers(2, 65))
    os.environ["BNM_QUIET"] = "1"
    try:
        model = b.Model.from_header_text(_random_model_text(rng, codecs, tuple(widths), n_classes))
        ctx = b.Context(model)
    finally:
        os.environ.pop("BNM_QUIET", None)
    om = util.OracleModel(model, orc)
    x = np.concatenate([synth.images(seed, 333, DIST_U), synth.images(seed, 334, DIST_M), np.zeros((2, 256), np.int8),
                        np.full((2, 256), -128, np.int8), np.full((2, 256), 127, np.int8)])
    want = om.infer(x, logits=True)
    assert ctx.path in (b.PATH_FUSED_MFMA, b.PATH_LAYERWISE_MFMA), (codecs, widths)
    tried = []
    for label, setup in paths_for(ctx):
        setup(ctx)
        for n in (len(x), 65, 1):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (codecs, widths, n_classes, label, n)
        tried.append(label)
    assert "auto" in tried and "layerwise" in tried and "layerwise_mfma" in tried, tried
    ctx.close()


@pytest.mark.parametrize("seed", range(28))
def test_fuzz_random_cnn_models(seed, gpu_ok, orc):
    """The CNN topology (BitNetMCU_MNIST_dll.c:48-91) with 4 to 96 channels (seeds from 12 on: 4 to 256, ternary FC layers among
    the codecs), random conv weights, a random codec per FC layer and random tail widths: front end (MFMA - one, two or 1.5 .. 8.5
    items per image - and round 1's VALU kernel) + whichever tail the model gets, ids and logits vs the oracle."""
    rng = np.random.default_rng(9100 + seed)
    wide = seed >= 12
    C = 4 * int(rng.integers(1, 65 if wide else 25))
    codecs = tuple(int(c) for c in rng.choice([1, 2, 4, 12, 16, 64] if wide else [1, 2, 4, 12, 16], size=3))
    need = {1: 32, 2: 16, 4: 8, 12: 8, 16: 4, 64: 4}
    if seed % 4 == 3:                        # any channel count, not only multiples of 4 (8-bit first FC layer: 4 C inputs always fit)
        C = max(1, C - int(rng.integers(1, 4)))
        codecs = (16,) + codecs[1:]
    if (4 * C) % need[codecs[0]]:
        codecs = (16,) + codecs[1:]          # 4 C act bytes are a multiple of 16: any codec but binary / 2-bit fits every C
    widths = tuple(int(rng.integers(1, 128 // need[codecs[k]] + 1)) * need[codecs[k]] for k in (1, 2))
    n_classes = int(rng.integers(2, 41))
    # odd seeds: conv kernels over the whole int8 range (the zoo's do: -128 .. 127), seeds 0 mod 4: small ones; seeds 2 mod 4: conv1
    # kernels up to +-56 - conv1 sums up to 64,512: the pipelined one-kernel form (sums below 2^16) over its whole range - the others full range
    conv_weights = ((lambda k: rng.integers(-128, 128, size=9 * C)) if seed % 2 else
                    (lambda k: rng.integers(-56, 57, size=9 * C) if k == 2 else rng.integers(-128, 128, size=9 * C)) if seed % 4 == 2 else None)
    model = b.Model.from_header_text(_random_cnn_text(rng, C, codecs, widths, n_classes, conv_weights))
    om = util.OracleModel(model, orc)
    x = np.concatenate([synth.images(seed, 120, DIST_U), synth.images(seed, 121, DIST_M), np.full((2, 256), -128, np.int8),
                        np.full((2, 256), 127, np.int8)])
    want = om.infer(x, logits=True)
    ctx = b.Context(model)
    for variant in (3, 4, 1, 0):     # (3: the one-kernel form where the tail fits it - C <= 64, layers <= 96 wide -, else as 4)
        try:
            ctx.set_cnn_variant(variant)
        except b.BnmError:
            assert variant in (3, 4) and C > 170      # the lane = image kernel's records must fit the LDS beside six waves
            continue
        for n in (len(x), 5, 6):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (C, codecs, widths, n_classes, variant, n)
    ctx.close()


@pytest.mark.parametrize("seed", [11, 12])
def test_fuzz_kernel_symbols(seed, gpu_ok, orc):
    """The reference's four kernel symbols as the library exports them against the oracle's on random arguments far beyond the
    model shapes (profiles/fuzz_symbols.py): every codec id incl. unknown ones, rows of up to 3,000 inputs, ReLUNorm over 1..6,000
    values of every magnitude up to INT32_MAX (where the C engine's rounding add wraps), planes up to 96 x 96, in place and not."""
    sys.path.insert(0, os.path.join(util.REPO, "profiles"))
    import fuzz_symbols
    counts, bad = fuzz_symbols.fuzz(seed, 150)
    assert not bad and counts["fc"] == 150, bad[:5]


def test_unknown_codec_keeps_the_bit_serial_path(gpu_ok, orc, capfd, monkeypatch):
    """A codec the C engine does not decode (NF4's id 36: every sum is 0, BitNetMCU_inference.c:202) has no int8 rows: such a model
    stays on the bit-serial layer-wise kernels, which restate the C branches one by one."""
    monkeypatch.delenv("BNM_QUIET", raising=False)
    rng = np.random.default_rng(36)
    model = b.Model.from_header_text(_random_model_text(rng, (4, 36, 4, 4), (64, 64, 64)))
    ctx = b.Context(model)
    assert ctx.path == b.PATH_LAYERWISE_ALU and "layer-wise ALU" in capfd.readouterr().err
    with pytest.raises(b.BnmError):
        ctx.set_path(b.PATH_LAYERWISE_MFMA)
    x = synth.images(0, 300, DIST_U)
    want = util.OracleModel(model, orc).infer(x, logits=True)
    got = ctx.infer(x, logits=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ctx.close()


@pytest.mark.parametrize("C,codecs", [(160, (2, 4, 4)), (144, (2, 4, 4)), (200, (2, 4, 4)), (256, (2, 4, 4)),
                                      (256, (64, 4, 4))])     # 1,024 real inputs, declared 1,030 (ternary padding)
def test_wide_cnn_tail_runs_layerwise_on_the_matrix_cores(C, codecs, gpu_ok, orc):
    """More than 128 channels: act rows longer than the fused FC kernels' 512 bytes - the front end (one fused launch over image
    pairs: five whole blocks per image; 4 + a pair item; 6 + a pair item; 8, the maximum) feeds the layer-wise MFMA tail."""
    rng = np.random.default_rng(C)
    model = b.Model.from_header_text(_random_cnn_text(rng, C, codecs, (96, 64), 10))
    ctx = b.Context(model)
    assert ctx.path == b.PATH_LAYERWISE_MFMA
    x = np.concatenate([synth.images(3, 150, DIST_U), synth.images(3, 151, DIST_M)])
    want = util.OracleModel(model, orc).infer(x, logits=True)
    taps = {}
    for cv in (0, 2, 1):
        ctx.set_cnn_variant(cv)
        for n in (len(x), 1, 2, 3):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (C, cv, n)
        taps[cv] = ctx.activations(x[:100])
    assert np.array_equal(taps[1], taps[0]) and np.array_equal(taps[2], taps[0])
    ctx.close()


@pytest.mark.parametrize("C", [5, 24, 64, 100])
def test_cnn_kernels_with_full_range_conv_weights(C, gpu_ok, orc):
    """The zoo's conv kernels use the whole int8 range (-128 .. 127), the random models above only -6 .. 6.  Full-range random
    kernels plus channels whose nine taps are ALL -128 / ALL 127 / all zero (the extreme sums: conv1 outputs of 14 bits, pooled
    conv2 outputs of 20, features of 26 - what the lane = image kernel's int8 planes and compressed ReLUNorm records must hold),
    on extreme and synthetic images; every front end against the oracle."""
    rng = np.random.default_rng(C)

    def conv_weights(k):
        w = rng.integers(-128, 128, size=(C, 9))
        w[0], w[1], w[2] = -128, 127, 0
        if C > 4:
            w[3] = {2: 127, 4: -128, 7: 127}[k]                    # all-positive first stage into an all-negative second one
            w[4] = np.array([127, -128] * 4 + [127])
        return w.reshape(-1)
    model = b.Model.from_header_text(_random_cnn_text(rng, C, (16, 4, 4), (64, 32), 10, conv_weights))
    om = util.OracleModel(model, orc)
    x = np.concatenate([np.full((3, 256), -128, np.int8), np.full((3, 256), 127, np.int8), np.zeros((2, 256), np.int8),
                        synth.images(C, 300, DIST_U), synth.images(C, 300, DIST_M)])
    want = om.infer(x, logits=True)
    ctx = b.Context(model)
    for variant in (3, 4, 1, 0):
        ctx.set_cnn_variant(variant)
        for n in (len(x), 33, 1):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (C, variant, n)
    ctx.close()


def test_cnn_third_plane_is_dropped_exactly_when_the_weights_rule_it_out(gpu_ok, orc):
    """The lane = image kernels carry conv3's third operand plane (bits 16..23 of the pooled conv2 values) only for models whose
    weights can reach it (bnm_cnn_li_tables' bound: m1 = (127 sum(w1+) + 128 sum|w1-|) >> 4, m2 = (m1 sum(w2+)) >> 4 < 2^16).  Every
    CNN of the zoo is below the bound; two crafted models sit right at it - all-positive kernels whose bound IS attained by the
    all-127 image: pooled conv2 outputs of 65,205 (two planes, at their maximum) and 65,772 (needs the third) - and every form of
    the kernel (one kernel, two launches, float input) must equal the oracle on them."""
    import torch
    from bitnetmcu_amd import harness
    for name in [n for n in MODEL_NAMES if "cnn" in n]:
        ctx = b.Context(util.load_golden_model(name))
        assert ctx.cnn_planes == 2, name
        ctx.close()
    C = 8
    for w2sum, planes in ((115, 2), (116, 3)):
        w2 = [13] * 8 + [w2sum - 104]
        rng = np.random.default_rng(w2sum)

        def conv_weights(k):
            return np.array(([127] * 9 if k == 2 else w2 if k == 4 else list(rng.integers(-128, 128, size=9))) * C)
        model = b.Model.from_header_text(_random_cnn_text(rng, C, (16, 4, 4), (64, 32), 10, conv_weights))
        om = util.OracleModel(model, orc)
        x = np.concatenate([np.full((40, 256), 127, np.int8), np.full((3, 256), -128, np.int8), synth.images(5, 500, DIST_U),
                            np.clip(synth.images(6, 500, DIST_M).astype(np.int16) + 100, -128, 127).astype(np.int8)])
        want = om.infer(x, logits=True)
        for variant in (3, 4, 1):
            ctx = b.Context(model)
            assert ctx.cnn_planes == planes, (w2sum, ctx.cnn_planes)
            ctx.set_cnn_variant(variant)
            for n in (len(x), 33):
                got = ctx.infer(x[:n], logits=True)
                assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (w2sum, variant, n)
            ctx.close()
        # float input: images that quantise to exactly these bytes
        xf = x.astype(np.float32)
        xf[:, 0] = np.where(np.abs(xf).max(axis=1) < 127, 127.0, xf[:, 0])      # (every image's max|x| = 127 or 128: scale 1 or 127/128)
        q = harness.quantize_input(xf)
        wantf = om.infer(q, logits=True)
        ctx = b.Context(model)
        ctx.set_cnn_variant(3)
        cls = torch.empty(len(xf), dtype=torch.int32, device="cuda")
        lg = torch.empty((len(xf), 10), dtype=torch.int32, device="cuda")
        ctx.infer_float_device(torch.from_numpy(xf).cuda(), cls, lg)
        torch.cuda.synchronize()
        assert ctx.last_kernel == "cnn_li_fused_kernel<float>"
        assert np.array_equal(cls.cpu().numpy().astype(np.uint32), wantf[0]) and np.array_equal(lg.cpu().numpy(), wantf[1]), w2sum
        ctx.close()


def test_cnn_pipelined_form_runs_exactly_when_conv1_sums_fit_16_bits(gpu_ok, orc):
    """cnn_li_fused_pipe_kernel starts conv1's accumulators at -32768 and lets v_cvt_pk_i16_i32 be the ReLU and the int16 packing:
    right only while no conv1 sum exceeds 65535 (bnm_cnn_li_tables' sums16: 127 sum(w1+) + 128 sum|w1-| per channel).  Every CNN of
    the zoo is below the bound.  Crafted models AT it, whose bound is attained by an image of the test: positive kernels summing to
    516 (all-127 image: 65,532 - pipelined, conv1 outputs at the top of their 12 bits) and 517 (65,659: the four-wave form);
    negative kernels summing to -511 (all -128 image: 65,408 - pipelined) and -512 (65,536: not).  Every form equals the oracle."""
    import torch
    from bitnetmcu_amd import harness
    for name in [n for n in MODEL_NAMES if "cnn" in n]:
        ctx = b.Context(util.load_golden_model(name))
        ctx.set_cnn_variant(3)
        assert ctx.cnn_pipelined, name
        ctx.close()
    C = 8
    for w1, piped in (([58] * 8 + [52], True), ([58] * 8 + [53], False), ([-57] * 8 + [-55], True), ([-57] * 8 + [-56], False)):
        for small_w2 in (False, True):
            rng = np.random.default_rng(abs(sum(w1)) + small_w2)

            def conv_weights(k):
                if k == 2:
                    return np.array(w1 * C)
                if k == 4 and small_w2:
                    return np.array(list(rng.integers(-128, 20, size=9)) * C)      # (pooled conv2 outputs below 2^16: two conv3 planes)
                return np.array(list(rng.integers(-128, 128, size=9)) * C)
            model = b.Model.from_header_text(_random_cnn_text(rng, C, (16, 4, 4), (64, 32), 10, conv_weights))
            om = util.OracleModel(model, orc)
            x = np.concatenate([np.full((40, 256), 127, np.int8), np.full((40, 256), -128, np.int8), synth.images(5, 500, DIST_U),
                                np.clip(synth.images(6, 500, DIST_M).astype(np.int16) + 100, -128, 127).astype(np.int8)])
            want = om.infer(x, logits=True)
            for variant in (3, 6, 4, 1):
                ctx = b.Context(model)
                ctx.set_cnn_variant(variant)
                assert ctx.cnn_pipelined == (piped and variant == 3), (w1, variant)
                assert not small_w2 or ctx.cnn_planes == 2, (w1, ctx.cnn_planes)
                for n in (len(x), 33):
                    got = ctx.infer(x[:n], logits=True)
                    assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (w1, small_w2, variant, n)
                if variant in (3, 6):
                    assert ctx.last_kernel == ("cnn_li_fused_pipe_kernel" if piped and variant == 3 else "cnn_li_fused_kernel")
                ctx.close()
            xf = x.astype(np.float32)
            xf[:, 0] = np.where(np.abs(xf).max(axis=1) < 127, 127.0, xf[:, 0])
            wantf = om.infer(harness.quantize_input(xf), logits=True)
            ctx = b.Context(model)
            ctx.set_cnn_variant(3)
            cls = torch.empty(len(xf), dtype=torch.int32, device="cuda")
            lg = torch.empty((len(xf), 10), dtype=torch.int32, device="cuda")
            ctx.infer_float_device(torch.from_numpy(xf).cuda(), cls, lg)
            torch.cuda.synchronize()
            assert ctx.last_kernel == ("cnn_li_fused_pipe_kernel<float>" if piped else "cnn_li_fused_kernel<float>")
            assert np.array_equal(cls.cpu().numpy().astype(np.uint32), wantf[0]) and np.array_equal(lg.cpu().numpy(), wantf[1]), (w1, small_w2)
            ctx.close()


@pytest.mark.parametrize("name", ["mcu_cnn_16", "cnn_64"])
def test_cnn_default_front_end_on_both_sides_of_the_small_call_rule(name, gpu_ok, orc):
    """A context left to itself gives calls of fewer than 2 C^2 images to the channel kernel and larger ones to the lane = image
    kernel (bnm_capi_infer.cpp: a wave of the latter walks all channels, 2 us each, however few images there are): ids and logits on
    both sides of the threshold, and with each kernel chosen explicitly, equal the oracle's."""
    model = util.load_golden_model(name)
    C = model.layer(0).out_channels
    n0 = 2 * C * C
    x = synth.images(11, n0 + 40, DIST_U)
    want = util.OracleModel(model, orc).infer(x, logits=True)
    for variant in (None, 3, 4, 1):
        ctx = b.Context(model)
        if variant is not None:
            ctx.set_cnn_variant(variant)
        for n in (1, 31, n0 - 1, n0, n0 + 33):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (name, variant, n)
        ctx.close()


@pytest.mark.parametrize("C", [48, 56])
def test_cnn_lane_image_kernel_on_a_large_sample(C, gpu_ok, orc):
    """Events of one image in 50,000: round 4's kernel lost a plane-2 operand dword to the late write-back of an MFMA whose dead
    result rows the allocator had handed to an inline-asm output (tests/test_kernel_static.py has the static check) - only with
    full-range weights, only where the pooled conv2 values pass 2^16, and not reproducibly.  300,000 images: the front end's act
    bytes against the channel kernel (an independent implementation), twice (run-to-run identical), ids and logits of the
    no-tap path against it as well, and the first 3,000 images against the oracle."""
    rng = np.random.default_rng(C)
    model = b.Model.from_header_text(_random_cnn_text(rng, C, (16, 4, 4), (96, 64), 10, lambda k: rng.integers(-128, 128, size=9 * C)))
    n = 300_000
    x = synth.images(3, n, DIST_U)
    acts, outs = {}, {}
    # ("li": ids and logits from the one-kernel form - the FC tail inside the front end's wave -, act bytes from cnn_li_kernel, which
    # the tap always runs; "li unfused": ids and logits from cnn_li_kernel + the tail's own launch)
    for key, variant in (("channel", 1), ("li", 3), ("li again", 3), ("li unfused", 4)):
        ctx = b.Context(model)
        ctx.set_cnn_variant(variant)
        assert ctx.cnn_variant == min(variant, 3) and ctx.cnn_tail_fused == (variant == 3)
        acts[key] = ctx.activations(x)[:, :4 * C]
        outs[key] = ctx.infer(x, logits=True)
        ctx.close()
    for key in ("li", "li again", "li unfused"):
        assert np.array_equal(acts[key], acts["channel"]), (C, key, int((acts[key] != acts["channel"]).sum()))
        assert np.array_equal(outs[key][0], outs["channel"][0]) and np.array_equal(outs[key][1], outs["channel"][1]), (C, key)
    want = util.OracleModel(model, orc).infer(x[:3000], logits=True)
    assert np.array_equal(outs["li"][0][:3000], want[0]) and np.array_equal(outs["li"][1][:3000], want[1])


@pytest.mark.parametrize("C,codecs,widths", [(18, (16, 4, 4), (96, 64)),      # 72 act bytes: not a multiple of 16
                                              (150, (16, 4, 4), (96, 64)),     # 600 act bytes: beyond the fused kernels, C % 4 = 2
                                              (130, (16, 16, 4), (64, 32)),    # 520
                                              (7, (16, 4, 4), (304, 64))])     # a 304-wide layer: beyond the fused kernels, 28 act bytes
def test_cnn_channel_counts_that_are_not_multiples_of_four_on_every_tail(C, codecs, widths, gpu_ok, orc):
    """the parser accepts any channel count 1..256 (an 8-bit first FC layer makes 4 C = 72 inputs exportable), and the
    layer-wise MFMA tail reads act rows in 32-byte K-steps with 16-byte loads - its rows are padded to a multiple of 32 bytes now.
    Every path the model can take, ids and logits vs the oracle."""
    rng = np.random.default_rng(1000 + C)
    model = b.Model.from_header_text(_random_cnn_text(rng, C, codecs, widths, 10))
    om = util.OracleModel(model, orc)
    x = np.concatenate([synth.images(C, 130, DIST_U), synth.images(C, 131, DIST_M)])
    want = om.infer(x, logits=True)
    ctx = b.Context(model)
    auto = ctx.path
    ran = []
    for path in (b.PATH_AUTO, b.PATH_FUSED_MFMA, b.PATH_LAYERWISE_MFMA, b.PATH_LAYERWISE_ALU):
        try:
            ctx.set_path(path)
        except b.BnmError:
            continue
        ran.append(ctx.path)
        for n in (len(x), 1, 3):
            got = ctx.infer(x[:n], logits=True)
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (C, path, n)
    assert b.PATH_LAYERWISE_MFMA in ran and b.PATH_LAYERWISE_ALU in ran and auto in ran
    ctx.close()


def test_evaluate_binding_and_latency_numbers(gpu_ok, orc, capsys):
    """float dataset -> class ids with the C engine's arithmetic, in two launches."""
    from bitnetmcu_amd import harness, evaluate
    r = np.load(os.path.join(GOLDEN, "real_images.npz"))
    model = util.load_golden_model("fc_4bitsym_64")
    ctx = b.Context(model)
    # the 13 real images, de-quantised to floats whose maximum magnitude is 127 -> quantise back to themselves
    xf = r["images"].astype(np.float32) / 127.0 * 3.0
    assert np.array_equal(harness.quantize_input(xf), r["images"])
    acc, pred = evaluate.accuracy(ctx, xf, r["labels"])
    assert acc == 1.0 and np.array_equal(pred, r["labels"])
    rng = np.random.default_rng(2)
    xr = rng.normal(size=(20000, 256)).astype(np.float32)
    assert np.array_equal(evaluate.predict(ctx, xr), util.OracleModel(model, orc).infer(harness.quantize_input(xr)))
    ctx.close()


def test_bench_under_torchrun_single_rank(gpu_ok, tmp_path):
    """The N>1 launch contract with one rank: torch.distributed.run -> RCCL process group, model broadcast, barriers,
    MAX-reduced time, all-reduced digest (the driver runs the same command with 2/4/8 ranks)."""
    import json
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    full = str(tmp_path / "full.json")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), os.path.join(util.REPO, "bench.py"), "--gpus", "1", "--steps", "2",
                          "--warmup", "1", "--images", "1000000", "--no-cpu", "--scaling", "strong", "--full-json", full], capture_output=True, text=True,
                         timeout=900, env=env)
    assert "{" in out.stdout, out.stderr[-2000:]
    c = _check_bench_stdout(out.stdout)
    assert c["config"]["rccl_ranks"] == 1 and c["config"]["dist_backend"] == "nccl" and c["scaling"] == "strong"
    d = json.load(open(full))
    assert d["n_gpus"] == 1 and d["verified_vs_oracle"] is True and sum(d["class_histogram"]) == 1000000
    assert d["scaling"] == "strong" and d["config"]["global_images"] == 1000000 and "extra_configs" in d
    assert d["config"]["rccl_ranks"] == 1 and d["config"]["dist_backend"] == "nccl"


def _bench_json(args, timeout=900):
    """-> (the full record, the compact last line)"""
    import json
    import subprocess
    import sys
    import tempfile
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    with tempfile.TemporaryDirectory() as td:
        full = os.path.join(td, "full.json")
        out = subprocess.run([sys.executable, os.path.join(util.REPO, "bench.py")] + args + ["--full-json", full], capture_output=True, text=True,
                             timeout=timeout, env=env)
        assert "{" in out.stdout, (out.returncode, out.stdout[-1500:], out.stderr[-3000:])
        c = _check_bench_stdout(out.stdout)
        return json.load(open(full)), c


def test_bench_launches_its_own_ranks_two_ranks_share_the_gpu(gpu_ok):
    """`python bench.py --gpus 2` WITHOUT a launcher starts two ranks itself.  On the one-GPU test box they share GPU 0 over gloo:
    the strong split of BASELINE configs[4] - 10^8 images as 2 x 5 x 10^7 contiguous shards generated on their owner, model
    blob broadcast from rank 0, barriers, MAX-reduced time - and the ALL-REDUCED digest of the two shards' class ids must be the
    oracle's digest of all 10^8 images."""
    n = int(os.environ.get("BNM_FULL_N", "100000000"))
    d, c = _bench_json(["--gpus", "2", "--dist-backend", "gloo", "--ranks-share-device", "--scaling", "strong", "--images", str(n),
                        "--steps", "3", "--warmup", "1", "--no-cpu"])
    assert c["n_gpus"] == 2 and c["config"]["ranks_share_device"] is True and len(c["per_rank_ms_per_step"]) == 2 and "rows" not in c
    assert c["verified_vs_oracle"] is True and c["config"]["global_images"] == n
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["global_images"] == n
    assert d["config"]["images_per_gpu"] == n // 2 and d["config"]["dist_backend"] == "gloo" and d["config"]["ranks_share_device"] is True
    assert d["config"]["rccl_ranks"] is None and "extra_configs" not in d
    assert d["verified_vs_oracle"] is True and sum(d["class_histogram"]) == n
    # every rank's own time is in the line; the reported time is the slowest rank's
    assert len(d["per_rank_ms_per_step"]) == 2 and abs(max(d["per_rank_ms_per_step"]) - d["ms_per_step"]) < 1e-9
    assert len(d["per_rank_kernel_ms"]) == 2 and all(0 < k <= t * 1.001 for k, t in zip(d["per_rank_kernel_ms"], d["per_rank_ms_per_step"]))
    if n == 100_000_000:
        assert int(d["digest"], 16) == 0x81b56c9fafee6636 == int(d["digest_expected"], 16)


def test_bench_gpus_flag_must_match_the_world_size(gpu_ok):
    """An 8-GPU command may never print a 1-GPU number: bench.py --gpus 2 started as ONE rank by a launcher refuses to run, and
    --gpus 2 on a box with one visible GPU (RCCL, one rank per GPU) fails loudly instead of printing n_gpus: 1."""
    import subprocess
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29517")
    out = subprocess.run([sys.executable, os.path.join(util.REPO, "bench.py"), "--gpus", "2", "--images", "100000", "--steps", "1",
                          "--warmup", "0", "--no-cpu", "--no-extra"], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode != 0 and "WORLD_SIZE=1" in (out.stderr + out.stdout) and "{" not in out.stdout
    import torch
    if torch.cuda.device_count() == 1:
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        out = subprocess.run([sys.executable, os.path.join(util.REPO, "bench.py"), "--gpus", "2", "--images", "100000", "--steps", "1",
                              "--warmup", "0", "--no-cpu", "--no-extra"], capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode != 0 and "{" not in out.stdout
        assert "only 1 visible" in (out.stderr + out.stdout)


def test_c_abi_multi_gpu_entry_point(gpu_ok, bnm, orc):
    """bnm_run_synth_multi_gpu on however many GPUs are visible (1 on the test box): digest + histogram equal the oracle's."""
    import ctypes as C
    model = util.load_golden_model("fc_4bitsym_64")
    n = 300_001
    out = (C.c_uint64 * 11)()
    secs = C.c_double()
    used = bnm.bnm_run_synth_multi_gpu(model._h, n, 0, DIST_U, b.SEED_DIST_U, out, 10, C.byref(secs))
    assert used >= 1 and secs.value > 0
    cls = util.OracleModel(model, orc).infer(synth.images(0, n, DIST_U))
    assert out[0] == synth.class_digest(cls, 0)
    assert list(out)[1:] == np.bincount(cls, minlength=10).tolist()
    # the model went through ncclBroadcast (rank 0's BNMBLOB -> every rank's context is built from the received bytes) and the
    # digests through ncclAllReduce: RCCL is loadable on the box, one rank = one communicator
    assert bnm.bnm_multi_gpu_transport() == b"rccl"
    # ... and without RCCL (BNM_NO_RCCL: the library never opens it) the host is the transport: same digest
    import subprocess
    import sys
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); import bitnetmcu_amd as b; L = b.load(); m = b.Model.from_zoo('fc_4bitsym_64');"
            "out = (C.c_uint64 * 11)(); used = L.bnm_run_synth_multi_gpu(m._h, %d, 0, 0, b.SEED_DIST_U, out, 10, None);"
            "print(used, L.bnm_multi_gpu_transport().decode(), out[0], sum(list(out)[1:]))" % (util.REPO, n))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, BNM_NO_RCCL="1"))
    assert r.stdout.split() == [str(used), "host", str(out[0]), str(n)], (r.stdout, r.stderr[-2000:])
    # asking for more GPUs than exist uses what is there; bad arguments are errors, not crashes
    assert bnm.bnm_run_synth_multi_gpu(model._h, 1000, 64, DIST_U, b.SEED_DIST_U, out, 10, None) == used
    assert bnm.bnm_run_synth_multi_gpu(model._h, 1000, 1, 7, b.SEED_DIST_U, out, 10, None) < 0
