"""Multi-model calls (bnm_multi_*, include/bitnetmcu_hip.h) on a machine without a GPU: the symbols exist and are bound, argument
errors are reported before anything touches the device, a call without a device is an error (never a fallback), and the C example
builds against the header with nothing but gcc.  The GPU runs: tests/test_gpu_multi_model.py."""
import ctypes as C
import os
import subprocess

import pytest

from bitnetmcu_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUP, EHIP = -1, -3, -4
SYMBOLS = ("bnm_multi_create", "bnm_multi_destroy", "bnm_multi_groups", "bnm_multi_infer_device", "bnm_multi_infer_float_device",
           "bnm_multi_infer_host", "bnm_multi_float_nonfinite")


def _models(lib, *names):
    import bitnetmcu_amd as b
    ms = [b.Model.from_zoo(n, lib) for n in names]
    return ms, (C.c_void_p * len(ms))(*[m._h.value for m in ms])


def test_symbols_are_exported_and_bound(bnm):
    for name in SYMBOLS:
        assert name in _lib.PROTOTYPES, name
        assert getattr(bnm, name).argtypes is not None, name


def test_create_rejects_bad_arguments_before_touching_the_device(bnm):
    ms, arr = _models(bnm, "fc_4bitsym_64", "mcu_1k")
    out = C.c_void_p()
    create = bnm.bnm_multi_create
    assert create(C.cast(arr, C.c_void_p), 0, -1, C.byref(out)) == EINVAL               # k == 0
    assert create(C.cast(arr, C.c_void_p), 17, -1, C.byref(out)) == EINVAL              # k > 16
    assert create(None, 2, -1, C.byref(out)) == EINVAL                                  # null model array
    assert create(C.cast(arr, C.c_void_p), 2, -1, None) == EINVAL                       # null output
    nulls = (C.c_void_p * 2)(ms[0]._h.value, None)
    assert create(C.cast(nulls, C.c_void_p), 2, -1, C.byref(out)) == EINVAL             # a null model
    cnn, carr = _models(bnm, "fc_4bitsym_64", "cnn_64")
    assert create(C.cast(carr, C.c_void_p), 2, -1, C.byref(out)) == EUNSUP             # a CNN
    assert b"CNN" in bnm.bnm_last_error()
    assert out.value is None


def test_infer_entry_points_reject_bad_arguments_before_touching_the_device(bnm):
    assert bnm.bnm_multi_groups(None) == EINVAL
    assert bnm.bnm_multi_infer_device(None, None, 0, None, None, None) == EINVAL
    assert bnm.bnm_multi_infer_float_device(None, None, 0, None, None, None) == EINVAL
    assert bnm.bnm_multi_infer_host(None, None, 0, None, None) == EINVAL
    assert bnm.bnm_multi_float_nonfinite(None, None) == EINVAL
    bnm.bnm_multi_destroy(None)      # a no-op


def test_without_a_device_create_is_an_error_not_a_fallback(bnm):
    ms, arr = _models(bnm, "fc_4bitsym_64", "mcu_1k")
    out = C.c_void_p()
    rc = bnm.bnm_multi_create(C.cast(arr, C.c_void_p), 2, -1, C.byref(out))
    if bnm.bnm_device_count() > 0:      # (on a GPU machine: a real object)
        assert rc == 0 and out.value is not None
        bnm.bnm_multi_destroy(out)
        return
    assert rc == EHIP
    assert out.value is None
    import bitnetmcu_amd as b
    with pytest.raises(b.BnmError):
        b.MultiContext(ms)


def test_c_example_compiles_against_the_header_with_gcc(tmp_path):
    hdr = os.path.join(REPO, "include")
    libdir = os.path.join(REPO, "bitnetmcu_amd")
    exe = tmp_path / "multi_infer"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", hdr,
                           os.path.join(REPO, "examples", "multi_infer.c"), "-L", libdir, "-lbitnetmcu_hip",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
