"""nh_tu_rd_planes / nh_tu_encode_map_planes refuse every bad argument on the host,
before any HIP call: NH_EARG with a message, no device needed."""
import ctypes as C

import pytest

from nano_hevc import _lib
from nano_hevc._lib import PlaneSet

FAKE = C.c_void_p(1 << 20)   # never dereferenced: the checks return first
OK = (0, 0, 0, 64, 64, 64, 1, 1, 0)


def _rd(L, pset, ctb=32, qp=30, lam=100, ptrs=None):
    p = ptrs or [FAKE] * 6   # src, lvl, recon, tu, pm, stats
    return L.nh_tu_rd_planes(p[0], C.byref(pset) if pset is not None else None, ctb, qp, 1, lam, p[1], p[2], p[3], p[4],
                             p[5], None)


def _enc(L, pset, ctb=32, qp=30, lam=100, ptrs=None):
    p = ptrs or [FAKE] * 7   # src, tu, lvl, recon, pm, stats, work
    return L.nh_tu_encode_map_planes(p[0], p[1], C.byref(pset) if pset is not None else None, ctb, qp, 1, lam, p[2],
                                     p[3], p[4], p[5], p[6], None)


CALLS = [(_rd, 6, b"nh_tu_rd_planes"), (_enc, 7, b"nh_tu_encode_map_planes")]


@pytest.mark.parametrize("call,nptr,name", CALLS)
def test_refusals_precede_any_device_call(call, nptr, name):
    L = _lib.load()
    ok = PlaneSet(*OK)

    def refused(rc, text):
        assert rc == _lib.NH_EARG
        err = L.nh_last_error()
        assert name in err and text in err, err

    for ctb in (4, 8, 64, 0, 31):
        refused(call(L, ok, ctb=ctb), b"ctb")
    for w, h in ((66, 64), (64, 62), (63, 63)):
        refused(call(L, PlaneSet(0, 0, 0, w, h, 128, 1, 1, 0)), b"multiples of 4")
    for qp in (-1, 52, 1000):
        refused(call(L, ok, qp=qp), b"qp")
    for lam in (-1, 1 << 31, 1 << 40):
        refused(call(L, ok, lam=lam), b"lambda")
    for i in range(nptr):
        ptrs = [FAKE] * nptr
        ptrs[i] = None
        refused(call(L, ok, ptrs=ptrs), b"null")
    refused(call(L, None), b"null")
    bad_sets = [PlaneSet(0, 0, 0, 64, 64, 60, 1, 1, 0),      # pitch < width
                PlaneSet(0, 0, 0, 0, 64, 64, 1, 1, 0),       # no width
                PlaneSet(0, 0, 0, 64, 65536, 64, 1, 1, 0),   # too tall
                PlaneSet(0, 0, 0, 64, 64, 64, -1, 1, 0),
                PlaneSet(0, 0, 0, 64, 64, 64, 1, -1, 0),
                PlaneSet(-4, 0, 0, 64, 64, 64, 1, 1, 0)]
    for s in bad_sets:
        refused(call(L, s), b"plane set")
    # accepted limits pass the checks: a set without groups or planes is a no-op
    for s in (PlaneSet(0, 0, 0, 64, 64, 64, 1, 0, 0), PlaneSet(0, 0, 0, 64, 64, 64, 0, 3, 0)):
        for qp, lam in ((0, 0), (51, (1 << 31) - 1)):
            for ctb in (16, 32):
                assert call(L, s, ctb=ctb, qp=qp, lam=lam) == _lib.NH_OK


def test_workspace_size_needs_no_device():
    assert _lib.load().nh_tu_encode_map_workspace_bytes() >= 8
