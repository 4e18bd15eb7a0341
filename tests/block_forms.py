"""The three execution forms of a per-block call, for tests.

BlockCall::run (csrc/nh_blocks.hip) runs one device body either on the resident
block-call server (served), as a single-workgroup kernel whose inputs travel in
the kernel-argument block (small: 256 B / 1 KB / 3 KB blocks), or staged through
device memory.  predicted_form() restates that rule from the documented
constants, layout() restates what the shim hands to the C ABI per function, and
observed() reads which side of the server a call really took from
gpu.block_server_stats.  Nothing here needs a GPU until server_off() /
observed() are called.
"""
from __future__ import annotations

import contextlib

import numpy as np

K_SRV_IN = 8192          # kSrvIn: input bytes a served call may carry
K_SMALL_IN = 3072        # kSmallIn: the largest kernel-argument block
K_SMALL_OUT = 64 << 10   # kSmallOut: output bytes of the served and small forms
ARG_BLOCKS = (256, 1024, K_SMALL_IN)
DEFAULT_IDLE_US = 100

FORMS = ("served", "small256", "small1024", "small3072", "staged")


def _align16(n: int) -> int:
    return (int(n) + 15) // 16 * 16


def input_bytes(input_bytes_per_array) -> int:
    """BlockCall::in(): every array starts on a 16-byte boundary."""
    return sum(_align16(b) for b in input_bytes_per_array)


def predicted_form(input_bytes_per_array, output_bytes, servable, idle_us) -> str:
    total = input_bytes(input_bytes_per_array)
    if idle_us > 0 and servable and total <= K_SRV_IN and output_bytes <= K_SMALL_OUT:
        return "served"
    if total <= K_SMALL_IN and output_bytes <= K_SMALL_OUT:
        return next(f"small{b}" for b in ARG_BLOCKS if total <= b)
    return "staged"


def collapse(form: str) -> str:
    """What the stats can tell apart: the served counter or the kernel counter."""
    assert form in FORMS, form
    return "served" if form == "served" else "kernel"


def _small_int(a) -> bool:
    return a.dtype.kind in "iub" and a.dtype.itemsize <= 2


def layout(fn, args, kw=None):
    """(input bytes per array, output bytes, servable) of the one BlockCall the
    shim makes for fn(*args): the arrays as the C ABI takes them (nanohevc.h) --
    int64 reference rows, int16 sample pairs, int64 coefficients / levels, int32
    transform blocks and sad operands.  Reductions return through the
    accumulator word: no output bytes."""
    a = [np.asarray(x) for x in args[:2]]
    n = a[0].size
    if fn in ("residual_block", "reconstruct_block"):
        n = np.broadcast(a[0], a[1]).size
        return [2 * n, 2 * n], 2 * n, True
    if fn == "clip_to_pixel_range":
        return [8 * n], 2 * n, True
    if fn in ("quantize", "quantize_block", "dequantize", "dequantize_block"):
        assert a[0].dtype.kind == "i", "float coefficients take nh_quantize_abs"
        return [8 * n], 4 * n, True
    if fn in ("forward_transform", "inverse_transform"):
        size = a[0].shape[0]
        return [4 * size * size], 4 * size * size, True
    if fn in ("intra_dc_predict", "intra_planar_predict", "intra_angular_predict"):
        size = int(args[-1])
        return [8 * a[0].size, 8 * a[1].size], 2 * size * size, True
    if fn == "sad":
        n = np.broadcast(a[0], a[1]).size
        return [4 * n, 4 * n], 0, True
    if fn == "satd_4x4":
        return [64, 64], 8, True
    if fn in ("residual_energy", "count_nonzero"):
        return [8 * n], 0, True
    if fn in ("mse", "psnr"):
        n = np.broadcast(a[0], a[1]).size
        if _small_int(a[0]) and _small_int(a[1]):
            return [8 * n, 8 * n], 0, True           # the exact int64 SSE
        return [8 * n, 8 * n], 8, False              # float64 pairwise sum: never served
    if fn == "estimate_bits":
        return [8 * n], 8, False
    raise KeyError(fn)


def predicted_for(fn, args, kw, idle_us) -> str:
    ins, out, servable = layout(fn, args, kw)
    return predicted_form(ins, out, servable, idle_us)


def largest_n(form_of, want, hi=1 << 20) -> int:
    """The largest n in [1, hi] with form_of(n) in `want`, for a form_of whose
    forms change only once each as n grows (bisection)."""
    lo = 1
    assert form_of(lo) in want and form_of(hi) not in want
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if form_of(mid) in want:
            lo = mid
        else:
            hi = mid
    return lo


# ---------------------------------------------------------------- GPU side

def stats():
    from nano_hevc import gpu
    return gpu.block_server_stats()


@contextlib.contextmanager
def server_off():
    """Launch-per-call mode for the body; the idle time found is put back."""
    from nano_hevc import gpu
    idle = stats()["idle_us"]
    try:
        gpu.block_server_set_idle_us(0)
        yield idle
    finally:
        gpu.block_server_set_idle_us(idle)


def observed(call):
    """Runs call() once.  Returns (form, ok, value): form is "served" or "kernel"
    from the stats' deltas (exactly one BlockCall must have run), ok tells whether
    the call returned, value is its result or the exception it raised."""
    s0 = stats()
    try:
        ok, value = True, call()
    except Exception as e:   # the class is what the caller compares
        ok, value = False, e
    s1 = stats()
    d_srv, d_krn = s1["served"] - s0["served"], s1["kernel_calls"] - s0["kernel_calls"]
    assert d_srv + d_krn == 1, f"expected one block call, saw served +{d_srv}, kernel +{d_krn} ({value!r})"
    return ("served" if d_srv else "kernel"), ok, value
