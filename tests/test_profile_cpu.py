"""Activation profiles without a GPU: the C ABI's new symbols, the counter layout of every zoo model, the numpy statement of the
counters (tests/profile_ref.py) on the KAT fixtures, and the Python view of the counters."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import util
from util import GOLDEN, MODEL_NAMES, REPO
import bitnetmcu_amd as b
from bitnetmcu_amd import _lib as L
from bitnetmcu_amd.profile import ActivationProfile, layout
import profile_ref

NEW = ["bnm_model_profile_words", "bnm_infer_device_profiled", "bnm_infer_float_device_profiled", "bnm_ctx_set_profile_mode"]


def test_profile_symbols_are_declared_bound_and_exported(bnm):
    text = open(os.path.join(REPO, "include", "bitnetmcu_hip.h")).read()
    for name in NEW:
        assert re.search(r"BNM_API [^;]*\b%s\(" % name, text), name
        assert name in L.PROTOTYPES, name
        assert hasattr(bnm, name), name


def expected_widths(model):
    fcs = model.fc_layers()
    w = [model.layer(0).out_channels * 4] if model.kind == b.KIND_CNN else []
    return w + [li.n_output for _, li in fcs[:-1]]


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_profile_words_match_the_documented_layout(name, bnm):
    model = util.load_golden_model(name)
    widths = expected_widths(model)
    nc = model.num_classes
    n_layers = C.c_uint32(99)
    buf = (C.c_uint32 * 16)(*([7] * 16))
    words = bnm.bnm_model_profile_words(model._h, C.byref(n_layers), buf)
    assert n_layers.value == len(widths)
    assert list(buf)[:len(widths)] == widths and list(buf)[len(widths):] == [7] * (16 - len(widths))
    assert words == sum(2 * w + 128 for w in widths) + nc + nc * nc + 3
    assert bnm.bnm_model_profile_words(model._h, None, None) == words
    assert layout(model) == (words, widths)


def test_profile_words_of_no_model_is_zero(bnm):
    assert bnm.bnm_model_profile_words(None, None, None) == 0


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_numpy_counters_from_the_kat_activations_are_consistent(name):
    model = util.load_golden_model(name)
    k = np.load(os.path.join(GOLDEN, f"kat_{name}.npz"))
    acts = k["acts"]
    n = len(acts)
    cls = k["cls"][:n]
    nc = model.num_classes
    labels = (np.arange(n) % (nc + 2)).astype(np.int32) - 1      # -1 and nc are out of range
    w = profile_ref.profile_counters(model, acts, cls, labels)
    p = ActivationProfile(model, w)
    cols = profile_ref.profiled_columns(model, acts)
    assert cols.shape[1] == sum(p.width)
    col = 0
    for l in p.layers:
        x = cols[:, col:col + l.width]
        assert (x >= 0).all()
        assert int(l.hist.sum()) == n * l.width
        assert np.array_equal(l.active, (x != 0).sum(axis=0))
        assert int(l.hist[0]) == n * l.width - int(l.active.sum())
        assert int(l.sum.sum()) == int((np.arange(128) * l.hist).sum())
        col += l.width
    assert p.images == n and p.labelled == n
    assert p.label_out_of_range == int(((labels < 0) | (labels >= nc)).sum())
    assert int(p.confusion.sum()) == n - p.label_out_of_range
    assert np.array_equal(p.pred, np.bincount(cls, minlength=nc))
    assert p.accuracy() == pytest.approx(float((cls == labels).sum()) / n)
    # the classifier's columns are not a profiled layer: the numpy statement drops them
    assert acts.shape[1] - cols.shape[1] == nc


@pytest.mark.parametrize("name", ["fc_4bitsym_64", "mcu_cnn_16small", "tern_96"])
def test_oracle_activation_rows_are_the_kat_rows(name, orc):
    """The per-image oracle driver of tests/profile_ref.py reproduces the compiled reference's activation rows."""
    model = util.load_golden_model(name)
    k = np.load(os.path.join(GOLDEN, f"kat_{name}.npz"))
    n = len(k["acts"])
    cls, acts = profile_ref.oracle_acts(util.OracleModel(model, orc), k["images"][:n])
    assert np.array_equal(cls, k["cls"][:n]) and np.array_equal(acts, k["acts"])


def test_profile_statistics_helpers():
    model = util.load_golden_model("mcu_cnn_16small")
    words, widths = layout(model)
    nc = model.num_classes
    n = 10
    acts = np.zeros((n, sum(widths) + nc), np.int8)
    acts[:, 0] = 5                  # channel 0, feature 0: always 5
    acts[:3, 5] = 127               # channel 1, feature 1: 3 images
    acts[:, widths[0] + 1] = np.arange(n)      # FC layer 1, neuron 1: 0..9
    cls = np.arange(n) % nc
    p = ActivationProfile(model, profile_ref.profile_counters(model, acts, cls))
    assert p.labelled == 0 and p.images == n and np.isnan(p.accuracy())
    assert p.positive_fraction() == pytest.approx((10 + 3 + 9) / (n * sum(widths)))
    assert p.positive_fraction(0) == pytest.approx(13 / (n * widths[0]))
    assert np.array_equal(p.dead(1), np.delete(np.arange(widths[1]), 1))
    assert list(p.channel_activity()[:3]) == [10, 3, 0] and len(p.channel_activity()) == widths[0] // 4
    assert list(p.channel_activity("sum")[:2]) == [50, 381]
    # layer 1: n * W values, of which 9 are 1..9 once each and the rest 0
    q = np.array([n * widths[1] - 9] + [1] * 9, np.float64) / (n * widths[1])
    assert p.entropy_bits(1) == pytest.approx(float(-(q * np.log2(q)).sum()))
    assert p.code_capacity(1) == pytest.approx(p.entropy_bits(1) / 7)
    with pytest.raises(ValueError):
        ActivationProfile(model, np.zeros(words + 1, np.uint64))
    with pytest.raises(ValueError):
        ActivationProfile(util.load_golden_model("mcu_1k"), np.zeros(layout(util.load_golden_model("mcu_1k"))[0], np.uint64)).channel_activity()
