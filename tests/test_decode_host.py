"""The decoder's CPU-side checks: the yardstick ``decode_ref.decode``
against the reference's own recorded closed-loop outputs, the new C-ABI symbols,
their host-side argument checks (before any device call) and the range proof of
k_dequant_inv8x8's 24-bit multiplies."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from decode_ref import decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import decode_bounds  # noqa: E402

NEW = ("nh_dequant_inv8x8_planes", "nh_intra_decode_closed_workspace_bytes", "nh_intra_decode_planes_closed")


@pytest.mark.parametrize("tag", ["c3a", "c3b", "c3c"])
def test_decode_ref_reproduces_recorded_recon(golden, tag):
    """Guards the yardstick: passes without the feature."""
    g = golden("closed.npz")
    assert np.array_equal(decode(g[tag + "_modes"], g[tag + "_lvl"], int(g[tag + "_qp"])), g[tag + "_rec"])


def _lib_and_types():
    from nano_hevc import _lib
    return _lib, _lib.load(), _lib.PlaneSet


def test_new_symbols_exported():
    _lib, L, _ = _lib_and_types()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    from nano_hevc import gpu
    assert callable(gpu.dequant_inv8x8) and callable(gpu.intra_decode_closed)


FAKE = C.c_void_p(1 << 20)   # never dereferenced: the checks return first
BAD_SETS = {"pitch<width": (0, 0, 0, 64, 64, 56, 1, 1, 0), "width 0": (0, 0, 0, 0, 64, 64, 1, 1, 0),
            "height 0": (0, 0, 0, 64, 0, 64, 1, 1, 0), "width<0": (0, 0, 0, -8, 64, 64, 1, 1, 0),
            "planes 0": (0, 0, 0, 64, 64, 64, 0, 1, 0), "groups<0": (0, 0, 0, 64, 64, 64, 1, -1, 0)}


def test_dequant_inv8x8_host_checks_precede_any_device_call():
    _lib, L, PlaneSet = _lib_and_types()
    ok = PlaneSet(0, 0, 0, 64, 64, 64, 1, 1, 0)
    f = L.nh_dequant_inv8x8_planes
    for nsets in (0, -1, 9):
        assert f(FAKE, 2, FAKE, C.byref(ok), nsets, 30, None) == _lib.NH_EARG
        assert b"nsets" in L.nh_last_error()
    for lb in (0, 1, 3, 8):
        assert f(FAKE, lb, FAKE, C.byref(ok), 1, 30, None) == _lib.NH_EARG
        assert b"lvl_bytes" in L.nh_last_error()
    for args in ((None, 2, FAKE, C.byref(ok)), (FAKE, 2, None, C.byref(ok)), (FAKE, 4, FAKE, None)):
        assert f(*args, 1, 30, None) == _lib.NH_EARG
        assert b"null" in L.nh_last_error()
    for what, fields in BAD_SETS.items():
        for lb in (2, 4):
            assert f(FAKE, lb, FAKE, C.byref(PlaneSet(*fields)), 1, 30, None) == _lib.NH_EARG, what
            assert b"plane set" in L.nh_last_error(), what
    two = (PlaneSet * 2)(ok, PlaneSet(*BAD_SETS["pitch<width"]))   # the second set is checked too
    assert f(FAKE, 2, FAKE, two, 2, 30, None) == _lib.NH_EARG


def test_intra_decode_host_checks_precede_any_device_call():
    _lib, L, PlaneSet = _lib_and_types()
    ok = PlaneSet(0, 0, 0, 64, 64, 64, 1, 1, 0)
    f = L.nh_intra_decode_planes_closed
    for nsets in (0, -1, 9):
        assert f(FAKE, FAKE, C.byref(ok), nsets, 30, FAKE, FAKE, None) == _lib.NH_EARG
        assert b"nsets" in L.nh_last_error()
    for args in ((None, FAKE, C.byref(ok), 1, 30, FAKE, FAKE), (FAKE, None, C.byref(ok), 1, 30, FAKE, FAKE),
                 (FAKE, FAKE, None, 1, 30, FAKE, FAKE), (FAKE, FAKE, C.byref(ok), 1, 30, None, FAKE),
                 (FAKE, FAKE, C.byref(ok), 1, 30, FAKE, None)):
        assert f(*args, None) == _lib.NH_EARG
        assert b"null" in L.nh_last_error()
    for what, fields in BAD_SETS.items():
        assert f(FAKE, FAKE, C.byref(PlaneSet(*fields)), 1, 30, FAKE, FAKE, None) == _lib.NH_EARG, what
        assert b"plane set" in L.nh_last_error(), what
    assert f(FAKE, FAKE, C.byref(ok), 1, 30, FAKE, C.c_void_p((1 << 20) + 4), None) == _lib.NH_EARG
    assert b"8-byte" in L.nh_last_error()


def test_decode_workspace_bytes():
    _lib, L, PlaneSet = _lib_and_types()
    f = L.nh_intra_decode_closed_workspace_bytes
    ok = PlaneSet(0, 0, 0, 64, 48, 64, 1, 1, 0)
    assert f(C.byref(ok), 1) > 0
    assert f(C.byref(ok), 1) == L.nh_intra_rdo_closed_workspace_bytes(C.byref(ok), 1)   # one workspace layout
    assert f(C.byref(PlaneSet(0, 0, 0, 7, 7, 7, 1, 1, 0)), 1) > 0    # no full block: still a status word
    for what, fields in BAD_SETS.items():
        assert f(C.byref(PlaneSet(*fields)), 1) < 0, what
    assert f(C.byref(ok), 0) < 0 and f(C.byref(ok), 9) < 0 and f(None, 1) < 0


def test_dequant_inv8x8_24bit_bounds(capsys):
    """The proof behind the 24-bit multiplies of k_dequant_inv8x8 (tools/decode_bounds.py):
    the one-mad dequantiser equals quant.py for every int16 level at every QP, and the
    host's rule for the 24-bit inverse pass 1 (QP <= 40) is exactly where every
    dequantised coefficient fits signed 24 bits."""
    decode_bounds.main()
    out = capsys.readouterr().out
    assert "QP 40" in out and "QP 41" in out and "pass 2" in out
    assert decode_bounds.p24_rule(40) and not decode_bounds.p24_rule(41)
