"""Several FC models over one image batch (MultiContext / bnm_multi_*, fused_fc_multi_kernel): every model's class ids and logits
equal the oracle's (oracle/checker.py) or the committed KAT fixtures, however the planner groups the models, for odd batch sizes,
repeated and permuted models, float input with non-finite images, calls in flight on two streams and random models of every
codec.  Each comparison is against the oracle, never the product against itself alone."""
import os
import subprocess

import numpy as np
import pytest
import torch

import bitnetmcu_amd as b
import util
import checker
from bitnetmcu_amd import synth, DIST_U, DIST_M
from test_gpu_parity import _random_model_text

pytestmark = pytest.mark.gpu

REPO = util.REPO
FC_ZOO = ["fc_4bitsym_64", "mcu_12k", "mcu_12k_fp130", "mcu_1k", "tern_96", "tern_96_sparse", "doc12k_binary", "doc12k_ternary",
          "doc12k_2bit", "doc12k_8bit"]
SMALL = ["fc_4bitsym_64", "mcu_12k", "mcu_12k_fp130", "mcu_1k"]


def zoo(*names):
    return [b.Model.from_zoo(n) for n in names]


def oracle(models, x, orc):
    got = [util.OracleModel(m, orc).infer(x, logits=True) for m in models]
    return np.stack([g[0] for g in got]), [g[1] for g in got]


def run_device(mc, x_dev, logits=True, stream=None):
    n = x_dev.shape[0]
    cls = torch.full((mc.k, n), -1, dtype=torch.int32, device=x_dev.device)
    lg = [torch.full((n, m.num_classes), -7, dtype=torch.int32, device=x_dev.device) for m in mc.models] if logits else None
    if x_dev.dtype == torch.float32:
        mc.infer_float_device(x_dev, cls, lg, stream=stream)
    else:
        mc.infer_device(x_dev, cls, lg, stream=stream)
    return cls, lg


def test_kat_fixtures_all_ten_fc_zoo_models_in_one_object(gpu_ok):
    models = zoo(*FC_ZOO)
    mc = b.MultiContext(models, device=0)
    assert mc.groups > 1
    for name in FC_ZOO:
        kat = np.load(os.path.join(util.GOLDEN, f"kat_{name}.npz"))
        cls, lg = mc.infer(kat["images"], logits=True)
        r = FC_ZOO.index(name)
        assert np.array_equal(cls[r], kat["cls"].astype(np.uint32)), name
        assert np.array_equal(lg[r], kat["logits"]), name
    mc.close()


def test_small_set_one_group_and_synthetic_parity(gpu_ok, orc):
    assert b.MultiContext(zoo("fc_4bitsym_64", "mcu_12k", "mcu_1k"), device=0).groups == 1
    models = zoo(*SMALL)
    mc = b.MultiContext(models, device=0)
    assert mc.groups in (1, 2)
    n = 300_000
    for dist in (DIST_U, DIST_M):
        imgs = torch.empty((n, 256), dtype=torch.int8, device="cuda:0")
        synth.fill_device(imgs, first=0, dist=dist)
        cls, lg = run_device(mc, imgs)
        torch.cuda.synchronize()
        x = synth.images(0, n, dist)
        want, want_lg = oracle(models, x, orc)
        assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want), dist
        for r in range(len(models)):
            assert np.array_equal(lg[r].cpu().numpy(), want_lg[r]), (dist, SMALL[r])


@pytest.mark.parametrize("n", [0, 1, 31, 33, 1_000_003])
def test_odd_batch_sizes(n, gpu_ok, orc):
    models = zoo(*SMALL)
    mc = b.MultiContext(models, device=0)
    imgs = torch.empty((max(n, 1), 256), dtype=torch.int8, device="cuda:0")
    synth.fill_device(imgs, first=17, dist=DIST_M)
    imgs = imgs[:n]
    cls, lg = run_device(mc, imgs)
    torch.cuda.synchronize()
    if n == 0:
        return
    idx = checker.sample_indices(n) if n > 100_000 else np.arange(n)
    ti = torch.from_numpy(idx).to("cuda:0")
    want, want_lg = oracle(models, imgs[ti].cpu().numpy(), orc)
    assert np.array_equal(cls[:, ti].cpu().numpy().astype(np.uint32), want)
    for r in range(len(models)):
        assert np.array_equal(lg[r][ti].cpu().numpy(), want_lg[r]), SMALL[r]
    # nothing beyond row n of any model was written
    assert (cls.shape == (len(models), n))


def test_repeated_and_permuted_models(gpu_ok, orc):
    x = np.concatenate([synth.images(3, 4000, DIST_U), synth.images(3, 4000, DIST_M)])
    base = zoo("mcu_12k_fp130", "mcu_1k", "doc12k_8bit", "fc_4bitsym_64")
    want, want_lg = oracle(base, x, orc)
    twice = b.MultiContext([base[0], base[1], base[0], base[2], base[1]], device=0)
    cls, lg = twice.infer(x, logits=True)
    assert np.array_equal(cls[0], cls[2]) and np.array_equal(cls[1], cls[4])
    assert np.array_equal(cls[[0, 1, 3]], want[[0, 1, 2]])
    assert np.array_equal(lg[2], want_lg[0]) and np.array_equal(lg[4], want_lg[1])
    perm = [2, 0, 3, 1]
    mc = b.MultiContext([base[p] for p in perm], device=0)
    cls, lg = mc.infer(x, logits=True)
    assert np.array_equal(cls, want[perm])
    for i, p in enumerate(perm):
        assert np.array_equal(lg[i], want_lg[p])


def test_float_input_quantised_once_and_nonfinite_counted(gpu_ok, orc):
    from test_gpu_float_nonfinite import images as float_images
    models = zoo(*SMALL)
    n = 5000
    x, bad = float_images(n, 11)
    mc = b.MultiContext(models, device=0)
    xd = torch.from_numpy(x).to("cuda:0")
    cls, lg = run_device(mc, xd)
    q = checker.quantize_input(np.where(bad[:, None], np.float32(0.0), x))
    want, want_lg = oracle(models, q, orc)
    assert np.array_equal(cls.cpu().numpy().astype(np.uint32), want)
    for r in range(len(models)):
        assert np.array_equal(lg[r].cpu().numpy(), want_lg[r]), SMALL[r]
    # the count: once per image (not per model), the single-model float path's count
    single = b.Context(models[0], device=0)
    single_cls = torch.empty(n, dtype=torch.int32, device="cuda:0")
    single.infer_float_device(xd, single_cls)
    assert mc.float_nonfinite == int(bad.sum()) == single.float_nonfinite
    run_device(mc, xd, logits=False)
    assert mc.float_nonfinite == 2 * int(bad.sum())


def test_two_streams_in_flight(gpu_ok, orc):
    models = zoo("fc_4bitsym_64", "mcu_1k", "doc12k_2bit", "doc12k_binary")
    mc = b.MultiContext(models, device=0)
    n = 200_003
    a = torch.empty((n, 256), dtype=torch.int8, device="cuda:0")
    c = torch.empty((n, 256), dtype=torch.int8, device="cuda:0")
    synth.fill_device(a, first=0, dist=DIST_U)
    synth.fill_device(c, first=0, dist=DIST_M)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for rep in range(3):
        for imgs, s in ((a, s1), (c, s2)):
            with torch.cuda.stream(s):
                outs.append((imgs, run_device(mc, imgs, stream=s)))
    torch.cuda.synchronize()
    for imgs, (cls, lg) in outs:
        idx = checker.sample_indices(n)
        ti = torch.from_numpy(idx).to("cuda:0")
        want, want_lg = oracle(models, imgs[ti].cpu().numpy(), orc)
        assert np.array_equal(cls[:, ti].cpu().numpy().astype(np.uint32), want)
        for r in range(len(models)):
            assert np.array_equal(lg[r][ti].cpu().numpy(), want_lg[r])


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_random_model_sets(seed, gpu_ok, orc):
    rng = np.random.default_rng(8800 + seed)
    need = {1: 32, 2: 16, 4: 8, 12: 8, 20: 8, 16: 4, 64: 8}
    want_k = int(rng.integers(2, 7))
    models = []
    os.environ["BNM_QUIET"] = "1"
    try:
        while len(models) < want_k:
            n_layers = int(rng.choice([3, 4]))
            if not models and seed % 2 == 0:
                codecs = [20] * n_layers      # FP1.3.0 throughout: its +128 weights take the second plane
            else:
                codecs = [int(c) for c in rng.choice([1, 2, 4, 12, 16, 20, 64], size=n_layers)]
            widths = []
            for k in range(1, n_layers):
                g = need[codecs[k]]
                hi = int(rng.choice([64, 96, 128, 192]))
                widths.append(int(rng.integers(1, hi // g + 1)) * g)
            n_classes = int(rng.integers(2, 65))
            m = b.Model.from_header_text(_random_model_text(rng, tuple(codecs), tuple(widths), n_classes))
            # only models a multi-model object accepts (a fused MFMA path: FP1.3.0 beside doubled codecs has none - refused)
            try:
                b.MultiContext([m], device=0).close()
            except b.BnmError as e:
                assert "fused" in str(e), e
                continue
            models.append(m)
    finally:
        os.environ.pop("BNM_QUIET", None)
    mc = b.MultiContext(models, device=0)
    x = np.concatenate([synth.images(seed, 1500, DIST_U), synth.images(seed, 1501, DIST_M), np.zeros((2, 256), np.int8),
                        np.full((2, 256), -128, np.int8), np.full((2, 256), 127, np.int8)])
    want, want_lg = oracle(models, x, orc)
    for n in (len(x), 65, 1):
        cls, lg = mc.infer(x[:n], logits=True)
        assert np.array_equal(cls, want[:, :n]), (seed, n)
        for r in range(len(models)):
            assert np.array_equal(lg[r], want_lg[r][:n]), (seed, r, n)


def test_cnn_models_are_refused(gpu_ok):
    with pytest.raises(b.BnmError, match="CNN"):
        b.MultiContext(zoo("fc_4bitsym_64", "cnn_64"), device=0)


def test_evaluate_compare_matches_the_oracle_counts(gpu_ok, orc):
    models = zoo("fc_4bitsym_64", "mcu_12k_fp130", "mcu_1k", "doc12k_2bit")
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((20_000, 256)) * rng.uniform(0.1, 2.0, (20_000, 1))).astype(np.float32)
    labels = rng.integers(0, 10, 20_000)
    res = b.evaluate.compare(models, x, labels)
    want, _ = oracle(models, checker.quantize_input(x), orc)
    k = len(models)
    dis = np.array([[int((want[i] != want[j]).sum()) for j in range(k)] for i in range(k)])
    assert np.array_equal(res["disagree"], dis)
    assert np.array_equal(res["pred"], want)
    assert res["accuracy"] == [float((want[i] == labels).mean()) for i in range(k)]
    assert b.evaluate.compare(models, x[:100])["accuracy"] is None


def test_c_example_prints_the_oracles_ids(gpu_ok, orc, tmp_path):
    hdr = os.path.join(REPO, "include")
    libdir = os.path.join(REPO, "bitnetmcu_amd")
    exe = tmp_path / "multi_infer"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", hdr,
                           os.path.join(REPO, "examples", "multi_infer.c"), "-L", libdir, "-lbitnetmcu_hip",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    names = ["mcu_1k", "fc_4bitsym_64", "mcu_12k_fp130"]
    headers = [os.path.join(util.GOLDEN, "_ref_headers", n + ".h") for n in names]
    x = synth.images(9, 777, DIST_M)
    img = tmp_path / "images.i8"
    img.write_bytes(x.tobytes())
    r = subprocess.run([str(exe), str(img)] + headers, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.array([[int(v) for v in line.split()] for line in r.stdout.strip().splitlines()], np.uint32).T
    want, _ = oracle([b.Model.from_header(h) for h in headers], x, orc)
    assert np.array_equal(got, want)
