"""Activation profiles: the counters of bnm_infer_device_profiled (include/bitnetmcu_hip.h) as numpy arrays, with the statistics the
reference's workflow asks of a network (training.py log_positive_activations, exportquant.py print_stats, models.py
MaskingLayer.prune_channels) computed from the engine's int8 activations.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def layout(model):
    """(words, widths): the counter word count of `model` and the widths of its profiled layers (a CNN's 4*C front-end features,
    then every FC layer but the classifier), from bnm_model_profile_words."""
    n_layers = C.c_uint32(0)
    widths = (C.c_uint32 * max(1, model.num_layers))()
    words = model._lib.bnm_model_profile_words(model._h, C.byref(n_layers), widths)
    return int(words), [int(widths[i]) for i in range(n_layers.value)]


class ProfileLayer:
    """One profiled layer: active[j] (images with activation j > 0), sum[j] (sum of activation j), hist[v] (activations equal
    to v, v = 0..127), all uint64."""

    def __init__(self, width, active, sum_, hist):
        self.width = width
        self.active = active
        self.sum = sum_
        self.hist = hist


class ActivationProfile:
    """Exact integer statistics of a model's int8 activations over every image of the calls that filled the counters."""

    def __init__(self, model, counters):
        words, widths = layout(model)
        w = np.ascontiguousarray(counters).reshape(-1).view(np.uint64)
        if len(w) != words:
            raise ValueError(f"{len(w)} counter words, the model's layout has {words}")
        self.kind = model.kind
        self.n_classes = nc = model.num_classes
        self.channels = model.layer(0).out_channels if model.kind == L.KIND_CNN else 0
        self.layers = []
        o = 0
        for W in widths:
            self.layers.append(ProfileLayer(W, w[o:o + W].copy(), w[o + W:o + 2 * W].copy(), w[o + 2 * W:o + 2 * W + 128].copy()))
            o += 2 * W + 128
        self.pred = w[o:o + nc].copy()
        self.confusion = w[o + nc:o + nc + nc * nc].reshape(nc, nc).copy()
        o += nc + nc * nc
        self.labelled, self.label_out_of_range, self.images = (int(v) for v in w[o:o + 3])

    @property
    def width(self):
        return [l.width for l in self.layers]

    def positive_fraction(self, l=None):
        """Fraction of the int8 activations that are > 0, over every profiled layer (or layer l): the engine's analogue of
        training.py's log_positive_activations.  It counts the integer engine's ReLUNorm outputs, not the float QAT model's
        activations, so it is NOT the number the training script logs for the same network."""
        layers = self.layers if l is None else [self.layers[l]]
        total = sum(self.images * x.width for x in layers)
        return float(sum(int(x.active.sum()) for x in layers)) / total if total else 0.0

    def entropy_bits(self, l):
        """Entropy in bits of layer l's activation values over 0..127 (print_stats' formula, applied to activations)."""
        h = self.layers[l].hist.astype(np.float64)
        p = h[h > 0] / h.sum() if h.sum() else h[:0]
        return float(-(p * np.log2(p)).sum())

    def code_capacity(self, l):
        """Share of the 7 bits a ReLUNorm output can carry that layer l uses: entropy_bits(l) / 7."""
        return self.entropy_bits(l) / 7.0

    def dead(self, l):
        """Indices of layer l's neurons that were never > 0."""
        return np.flatnonzero(self.layers[l].active == 0)

    def channel_activity(self, stat="active"):
        """CNN models: the front end's features summed per block of 4 (feature 4c + p belongs to channel c), i.e. per group of
        MaskingLayer.prune_channels(groups=C).  stat: "active" (images with the feature > 0) or "sum" (activation sums)."""
        if self.kind != L.KIND_CNN:
            raise ValueError("channel_activity() needs a CNN model")
        v = getattr(self.layers[0], stat)
        return v.reshape(self.channels, 4).sum(axis=1, dtype=np.uint64)

    def accuracy(self):
        """Correct predictions over labelled images (labels outside [0, n_classes) count as wrong)."""
        return float(np.trace(self.confusion)) / self.labelled if self.labelled else float("nan")
