"""block_forms.npz and tests/block_forms.py, pinned without a GPU.

The fixture holds exactly the calls of tests/golden/block_form_cases.py; where
the CPU restatement (oracle/) has the function, its result equals what the
reference recorded; and predicted_form puts every case on the side of its edge
that the case's name claims -- so the GPU module (test_block_forms_gpu.py)
compares against data that is checked here, in forms that are checked here."""
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from block_form_cases import BIG_N, INPUT_EDGES, cases, claimed_forms, reduction_limits  # noqa: E402
from block_checks import oracle_result, same_bits  # noqa: E402
from block_forms import (DEFAULT_IDLE_US, FORMS, collapse, input_bytes, layout, predicted_for,  # noqa: E402
                         predicted_form)

CASES = cases()


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("block_forms.npz")


def test_fixture_holds_exactly_the_cases(fixture):
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)
    got = {k.split("_", 1)[1] for k in fixture if k.startswith(("out_", "sha_", "err_"))}
    assert got == set(names)
    for n in names:
        assert sum(p + n in fixture for p in ("out_", "sha_", "err_")) == 1, n
        if "sha_" + n in fixture:       # only results above 4 KB are recorded by hash
            assert int(np.prod(fixture["shape_" + n])) * np.dtype(str(fixture["dtype_" + n])).itemsize > 4096, n
    assert os.path.getsize(os.path.join(HERE, "golden", "block_forms.npz")) < \
        os.path.getsize(os.path.join(HERE, "golden", "transform.npz"))


def test_oracle_equals_the_recorded_results(fixture):
    checked = 0
    for name, fn, args, kw in CASES:
        if "err_" + name in fixture:
            continue
        got = oracle_result(fn, args, kw)
        if got is None:
            continue
        if "out_" + name in fixture:
            assert same_bits(got, fixture["out_" + name]), name
        else:
            assert got.dtype.str == str(fixture["dtype_" + name]) and got.shape == tuple(fixture["shape_" + name]), name
            assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(fixture["sha_" + name]), name
        checked += 1
    assert checked >= 100, checked


def test_first_error_cases_record_the_classes_the_reference_raises(fixture):
    want = {"c_planar32_shortleft_pyint": "IndexError", "c_planar32_shortleft_int16": "OverflowError",
            "c_planar32_shortleft_uint8": "OverflowError", "c_planar200_overflow_before_shortleft": "OverflowError",
            "c_planar200_shortleft_before_overflow": "IndexError", "c_angular182_corner_overflow": "OverflowError",
            "c_angular182_ref_overflow": "OverflowError", "c_dc182_overflow": "OverflowError"}
    got = {n.rsplit("__", 2)[0]: str(fixture["err_" + n]) for n, *_ in CASES if n.startswith("c_")}
    assert got == want


def test_predicted_form_rule():
    """The table of DESIGN.md §4.6, on both sides of every constant."""
    assert predicted_form([8192], 65536, True, 100) == "served"
    assert predicted_form([8193], 0, True, 100) == "staged"            # rounded up to 8208 B
    assert predicted_form([16], 65537, True, 100) == "staged"          # whatever the input size
    assert predicted_form([16], 65536, False, 100) == "small256"       # a non-servable body
    assert predicted_form([16], 65537, False, 100) == "staged"
    assert predicted_form([4096, 4096], 0, True, 100) == "served"
    assert predicted_form([4096, 4081], 0, True, 100) == "served"      # 4081 rounds up to 4096
    assert predicted_form([4096, 4097], 0, True, 100) == "staged"
    for total, form in ((0, "small256"), (256, "small256"), (257, "small1024"), (1024, "small1024"),
                        (1025, "small3072"), (3072, "small3072"), (3073, "staged")):
        assert predicted_form([total], 8, True, 0) == form, total
    assert predicted_form([120, 120], 8, True, 0) == "small256"        # 2 x 128
    assert predicted_form([121, 129], 8, True, 0) == "small1024"       # 128 + 144
    assert input_bytes([1, 17, 32]) == 16 + 32 + 32
    assert [collapse(f) for f in FORMS] == ["served", "kernel", "kernel", "kernel", "kernel"]


def test_every_case_sits_on_the_side_its_name_claims():
    for name, fn, args, kw in CASES:
        on, off = claimed_forms(name)
        assert on in FORMS and off in FORMS, name
        assert predicted_for(fn, args, kw, DEFAULT_IDLE_US) == on, name
        assert predicted_for(fn, args, kw, 0) == off, name
    # the input edges: exactly the edge, and one 16-byte step above it
    by_label = {n.rsplit("__", 2)[0]: (fn, args) for n, fn, args, _ in CASES}
    for tag, n2, n1, _, _ in INPUT_EDGES:
        edge = int(tag[2:].split("_")[0])
        for label in (f"b_{tag}_residual_block_n{n2}", f"b_{tag}_reconstruct_block_n{n2}", f"b_{tag}_clip_bd8_n{n1}",
                      f"b_{tag}_quantize_qp0_intra_n{n1}", f"b_{tag}_quantize_qp51_inter_n{n1}",
                      f"b_{tag}_dequantize_qp51_n{n1}"):
            fn, args = by_label[label]
            step = 16 * len(layout(fn, args)[0])       # every array rounds up on its own
            assert input_bytes(layout(fn, args)[0]) == (edge if tag.endswith("_at") else edge + step), label
    # transforms sit at 64 B, on the 256 B edge, on the 1024 B edge, and at 4096 B
    for n, total in ((4, 64), (8, 256), (16, 1024), (32, 4096)):
        fn, args = by_label[f"b_tr_forward_transform_n{n}_dct_int32"]
        assert input_bytes(layout(fn, args)[0]) == total
    # the output edge: 181 x 181 fits the 64 KB result buffer, 182 x 182 does not
    assert layout(*by_label["b_out_planar_181"])[1] == 65522 and layout(*by_label["b_out_planar_182"])[1] == 66248
    ins = layout(*by_label["b_out_planar_181"])[0]
    assert sum(ins) == 2896 and input_bytes(ins) == 2912          # the 3 KB argument block carries them
    # reductions: 8192 B and 3072 B over the shim's arrays (sad: two int32; mse: two int64; else one int64)
    z32, z64, z16 = (lambda n: (np.zeros(n, np.int32),) * 2), (lambda n: (np.zeros(n, np.int64),)), \
        (lambda n: (np.zeros(n, np.int16),) * 2)
    assert reduction_limits("sad", z32) == (1024, 384)
    assert reduction_limits("residual_energy", z64) == (1024, 384)
    assert reduction_limits("count_nonzero", z64) == (1024, 384)
    assert reduction_limits("mse", z16) == (512, 192)
    for fn in ("sad", "residual_energy", "mse", "psnr", "count_nonzero"):
        ns = {int(l.rsplit("_n", 1)[1]) for l in by_label if l.startswith(f"b_red_{fn}_n")}
        assert {1, 255, 256, 257, BIG_N} <= ns and len(ns) == 9, (fn, ns)
