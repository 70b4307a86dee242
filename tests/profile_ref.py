"""numpy statement of the activation-profile counters (bnm_infer_device_profiled, include/bitnetmcu_hip.h), computed from
activation rows as the reference schedule writes them, and the oracle port's per-image activations to feed it."""
import ctypes as C

import numpy as np

from bitnetmcu_amd import _lib as L
from bitnetmcu_amd.profile import layout


def profiled_columns(model, acts):
    """Drop the classifier's ReLUNorm output (the last n_classes columns of a schedule's activation row): what is left are the
    profiled layers side by side."""
    return np.asarray(acts)[:, :acts.shape[1] - model.num_classes]


def profile_counters(model, acts, cls, labels=None):
    """uint64 counters of one call: acts [n][sum of all ReLUNorm widths] (classifier columns included), cls [n], labels [n] or None."""
    words, widths = layout(model)
    nc = model.num_classes
    a = profiled_columns(model, acts).astype(np.int64)
    n = len(a)
    out = np.zeros(words, np.uint64)
    o = col = 0
    for W in widths:
        x = a[:, col:col + W]
        out[o:o + W] = (x > 0).sum(axis=0)
        out[o + W:o + 2 * W] = x.sum(axis=0)
        out[o + 2 * W:o + 2 * W + 128] = np.bincount(x.reshape(-1), minlength=128)[:128]
        o += 2 * W + 128
        col += W
    cls = np.asarray(cls).astype(np.int64)
    out[o:o + nc] = np.bincount(cls, minlength=nc)[:nc]
    if labels is not None:
        lab = np.asarray(labels).astype(np.int64)
        ok = (lab >= 0) & (lab < nc)
        out[o + nc:o + nc + nc * nc] = np.bincount(lab[ok] * nc + cls[ok], minlength=nc * nc)[:nc * nc]
        out[o + nc + nc * nc] = n
        out[o + nc + nc * nc + 1] = int((~ok).sum())
    out[o + nc + nc * nc + 2] = n
    return out


def oracle_acts(om, images, threads=8):
    """The oracle port's class ids and activation rows (every ReLUNorm output) of int8 images [n][256], image by image
    (orc_fc_model / orc_cnn_model).  ctypes drops the GIL during each call: `threads` slices run side by side."""
    from concurrent.futures import ThreadPoolExecutor
    orc = om.orc
    x = np.ascontiguousarray(images, dtype=np.int8).reshape(-1, 256)
    model = om.model
    width = (model.layer(0).out_channels * 4 if model.kind == L.KIND_CNN else 0) + sum(li.n_output for _, li in model.fc_layers())
    acts = np.zeros((len(x), width), np.int8)
    cls = np.zeros(len(x), np.uint32)
    if om.front is not None:
        fn = orc.orc_cnn_model
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    else:
        fn = orc.orc_fc_model
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    fn.restype = C.c_uint32
    front = [C.byref(om.front)] if om.front is not None else []

    def run(lo, hi):
        lg = np.zeros(model.num_classes, np.int32)
        for i in range(lo, hi):
            cls[i] = fn(*([x[i].ctypes.data] + front + [om.arr, om.n_layers, lg.ctypes.data, acts[i].ctypes.data]))

    step = max(1, -(-len(x) // threads))
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda lo: run(lo, min(len(x), lo + step)), range(0, len(x), step)))
    return cls, acts
