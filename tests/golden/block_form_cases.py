"""Per-block calls at the thresholds between the three execution forms
(tests/block_forms.py restates the rule).

cases() rebuilds the same seeded calls every time; make_block_forms.py records
the REFERENCE's result (an array, a scalar, shape / dtype / SHA-256 of an array
above 4 KB, or the name of the exception it raised) per case into
block_forms.npz, and tests/test_block_forms_gpu.py runs every call on the
MI355X drop-in with the block-call server on and off and compares bit for bit.

Each case is (name, function name, args tuple, kwargs dict).  A name ends in
``__<form with the server on>__<form with the server off>``: the side of its
edge the case is meant to sit on, written down here by hand and checked against
block_forms.predicted_form by tests/test_block_forms_host.py.  Names starting
with ``b_`` are the threshold matrix, ``c_`` the first-error cases.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from block_forms import DEFAULT_IDLE_US, largest_n, layout, predicted_form  # noqa: E402

I32_MIN, I32_MAX = -2**31, 2**31 - 1
BIG_N = 262145            # 1024 workgroups x 256 lanes + 1: the staged grid-stride loop wraps

# (n at / above the edge for two int16 arrays, for one int64 array, forms on / off)
INPUT_EDGES = [
    ("in256_at", 64, 32, "served", "small256"),
    ("in256_above", 65, 33, "served", "small1024"),
    ("in1024_at", 256, 128, "served", "small1024"),
    ("in1024_above", 257, 129, "served", "small3072"),
    ("in3072_at", 768, 384, "served", "small3072"),
    ("in3072_above", 769, 385, "served", "staged"),
    ("in8192_at", 2048, 1024, "served", "staged"),
    ("in8192_above", 2049, 1025, "staged", "staged"),
]


def _form_of(fn, shape_args, idle_us):
    def f(n):
        ins, out, servable = layout(fn, shape_args(n))
        return predicted_form(ins, out, servable, idle_us)
    return f


def reduction_limits(fn, shape_args):
    """(the largest served n, the largest n of the small form) of a reduction,
    taken from predicted_form: the shim's arrays differ per function."""
    srv = largest_n(_form_of(fn, shape_args, DEFAULT_IDLE_US), ("served",))
    sml = largest_n(_form_of(fn, shape_args, 0), ("small256", "small1024", "small3072"))
    return srv, sml


def reduction_sizes(fn, shape_args):
    """The n of the reduction matrix with the forms each is meant to take (None:
    whichever argument block holds it): one lane; one workgroup whose stride wraps
    once (255 / 256 / 257); the last n of the 3 KB argument block and the next
    (the first staged n with the server off); the last served n and the next (the
    first staged n with it on); BIG_N."""
    srv, sml = reduction_limits(fn, shape_args)
    assert sml < srv < BIG_N
    ns = sorted({1, 255, 256, 257, sml, sml + 1, srv, srv + 1, BIG_N})
    return [(n, "served" if n <= srv else "staged", None if n <= sml else "staged") for n in ns]


def cases():
    rng = np.random.default_rng(31072)
    out = []

    def add(label, on, off, fn, *args, **kw):
        if off is None:     # below every threshold of interest: whichever argument block holds it
            ins, ob, servable = layout(fn, args)
            off = predicted_form(ins, ob, servable, 0)
        out.append((f"{label}__{on}__{off}", fn, args, kw))

    def i16(n):
        return rng.integers(-32768, 32768, n).astype(np.int16)

    def i32(shape):
        return rng.integers(I32_MIN, I32_MAX + 1, shape, dtype=np.int64).astype(np.int32)

    # ---- (b) input edges: two int16 arrays (whole range: the differences and sums wrap)
    for tag, n2, n1, on, off in INPUT_EDGES:
        add(f"b_{tag}_residual_block_n{n2}", on, off, "residual_block", i16(n2), i16(n2))
        add(f"b_{tag}_reconstruct_block_n{n2}", on, off, "reconstruct_block", i16(n2), i16(n2))
    # ---- one int64 array: clip, quantize, dequantize
    for tag, n2, n1, on, off in INPUT_EDGES:
        x = rng.integers(-700, 70000, n1)
        x[:4] = [-2**40, 2**40, 65535, 32768]
        add(f"b_{tag}_clip_bd8_n{n1}", on, off, "clip_to_pixel_range", x, 8)
        add(f"b_{tag}_clip_bd16_n{n1}", on, off, "clip_to_pixel_range", x.copy(), 16)     # 65535 -> int16 wrap
        c = i32(n1)
        c[:2] = [I32_MIN, I32_MAX]
        c[2:n1 // 2] = rng.integers(-3000, 3001, n1 // 2 - 2)
        for qp, size in ((0, 4), (51, 32)):
            for intra in (True, False):
                add(f"b_{tag}_quantize_qp{qp}_{'intra' if intra else 'inter'}_n{n1}", on, off,
                    "quantize", c.copy(), qp, size, intra)
        lv = i32(n1)                                   # level * scale << (qp_per - 4) wraps int32
        lv[:2] = [I32_MIN, I32_MAX]
        for qp in (0, 51):
            add(f"b_{tag}_dequantize_qp{qp}_n{n1}", on, off, "dequantize", lv.copy(), qp, 4)
    # ---- transforms: served with the server on; off, N <= 16 is small (64 B, the 256 B edge,
    # the 1024 B edge) and N = 32 (4096 B) staged
    for n, dst, off in ((4, True, "small256"), (4, False, "small256"), (8, False, "small256"),
                        (16, False, "small1024"), (32, False, "staged")):
        for fn in ("forward_transform", "inverse_transform"):
            key = f"{fn}_n{n}_{'dst' if dst else 'dct'}"
            add(f"b_tr_{key}_int32", "served", off, fn, i32((n, n)), dst)
            add(f"b_tr_{key}_res8", "served", off, fn, rng.integers(-255, 256, (n, n)).astype(np.int16), dst)
    # ---- the 64 KB output edge: 181 x 181 int16 is 65,522 B, 182 x 182 is 66,248 B
    for size, on, off in ((181, "served", "small256"), (182, "staged", "staged")):
        add(f"b_out_dc_{size}", on, off, "intra_dc_predict",
            rng.integers(0, 1024, 4).astype(np.int16), rng.integers(0, 1024, 4).astype(np.int16), size)
        for mode in (14, 30):                          # a negative and a positive angle; replicate-last fills the rest
            add(f"b_out_angular_m{mode}_{size}", on, off, "intra_angular_predict",
                rng.integers(0, 1024, 9).astype(np.int16), rng.integers(0, 1024, 9).astype(np.int16),
                int(rng.integers(0, 1024)), mode, size)
    t, l = rng.integers(0, 1024, 181).astype(np.int16), rng.integers(0, 1024, 181).astype(np.int16)
    add("b_out_planar_181", "served", "small3072", "intra_planar_predict", t, l, 1000, 17, 181)   # 2,896 B of inputs
    t, l = rng.integers(0, 1024, 182).astype(np.int16), rng.integers(0, 1024, 182).astype(np.int16)
    add("b_out_planar_182", "staged", "staged", "intra_planar_predict", t, l, 1000, 17, 182)     # 259 workgroups
    # ---- reductions through the LDS accumulator (served, small) and the device word (staged)
    def sad_args(n):
        a, b = i32(n), i32(n)                          # differences wrap int32
        a[0], b[0] = I32_MIN, 0                        # |INT32_MIN| stays INT32_MIN
        return a, b

    def energy_args(n):
        return (rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64),)     # squares wrap 2^64

    def sse_args(n):
        return i16(n), i16(n)                          # <= 16-bit samples: the exact int64 SSE

    def nnz_args(n):
        lv = rng.integers(-2**40, 2**40, n)
        lv[rng.random(n) < 0.5] = 0
        return (lv,)

    for fn, make, zero in (("sad", sad_args, lambda n: (np.zeros(n, np.int32), np.zeros(n, np.int32))),
                           ("residual_energy", energy_args, lambda n: (np.zeros(n, np.int64),)),
                           ("mse", sse_args, lambda n: (np.zeros(n, np.int16), np.zeros(n, np.int16))),
                           ("psnr", sse_args, lambda n: (np.full(n, 7, np.int16), np.full(n, 7, np.int16))),
                           ("count_nonzero", nnz_args, lambda n: (np.zeros(n, np.int64),))):
        sizes = reduction_sizes(fn, zero)
        for n, on, off in sizes:
            add(f"b_red_{fn}_n{n}", on, off, fn, *make(n))
        # an all-zero sum skips the accumulator's atomic: one workgroup, then the staged grid
        srv, sml = reduction_limits(fn, zero)
        add(f"b_red_{fn}_zero_n{sml}", "served", "small3072", fn, *zero(sml))
        add(f"b_red_{fn}_zero_n{srv + 1}", "staged", "staged", fn, *zero(srv + 1))
    add("b_red_satd_4x4_wrap", "served", "small256", "satd_4x4", i32((4, 4)), i32((4, 4)))
    # ---- the bodies that never run on the server: estimate_bits and the float64 mse.  n straddles
    # the 3072 B argument block and numpy's pairwise splits (8 terms, 128 terms, halves above 128);
    # levels of mixed magnitude make the float64 sum depend on the order of its additions
    def mixed(n):
        return rng.uniform(-9, 9, n) * 10.0 ** rng.integers(-3, 7, n)

    for n, form in ((7, "small256"), (8, "small256"), (128, "small1024"), (129, "small3072"), (300, "small3072"),
                    (384, "small3072"), (385, "staged")):
        add(f"b_ns_estimate_bits_n{n}", form, form, "estimate_bits", mixed(n))
    for n, form in ((7, "small256"), (8, "small256"), (64, "small1024"), (65, "small3072"), (128, "small3072"),
                    (129, "small3072"), (192, "small3072"), (193, "staged"), (300, "staged")):
        add(f"b_ns_mse_f64_n{n}", form, form, "mse", mixed(n), mixed(n))
    # ---- (c) the first error wins, in every form
    # size 32 (served / small): a short left (IndexError at row 20) against a corner whose numpy
    # arithmetic overflows at sample (0, 0); with a Python-int corner the math is exact and fits
    top32, left20 = np.full(32, 2000, np.int16), np.full(20, 100, np.int16)
    for tag, corner in (("pyint", 30000), ("int16", np.int16(30000)), ("uint8", np.uint8(7))):
        add(f"c_planar32_shortleft_{tag}", "served", "small1024", "intra_planar_predict", top32, left20, corner, 5, 32)
    # size 200 (staged, 157 workgroups): the int16 store overflows in row 0 from x = 139 (workgroup
    # 0); left runs out at row 20 (workgroup 15)
    top200, left20 = np.full(200, 100, np.int16), np.full(20, 100, np.int16)
    add("c_planar200_overflow_before_shortleft", "staged", "staged", "intra_planar_predict",
        top200, left20, 60000, 5, 200)
    # the other way round: left runs out at row 20, bottom_left overflows the store only from row 139
    add("c_planar200_shortleft_before_overflow", "staged", "staged", "intra_planar_predict",
        top200, left20, 5, 60000, 200)
    # size 182 (staged, one workgroup): angular corner and DC value outside int16
    add("c_angular182_corner_overflow", "staged", "staged", "intra_angular_predict",
        np.full(9, 100, np.int16), np.full(9, 100, np.int16), 40000, 26, 182)
    add("c_angular182_ref_overflow", "staged", "staged", "intra_angular_predict",
        np.array([1, 2, 3, 4, 5, 6, 7, 8, 70000]), np.full(9, 100, np.int16), 10, 30, 182)
    add("c_dc182_overflow", "staged", "staged", "intra_dc_predict",
        np.full(4, 2**40), np.full(4, 2**40), 182)
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def claimed_forms(name):
    """(form with the server on, form with it off) a case's name claims."""
    _, on, off = name.rsplit("__", 2)
    return on, off
