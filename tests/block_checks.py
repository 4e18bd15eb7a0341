"""Comparison bodies of the per-block drop-in tests against the reference's
recorded fixtures (tests/golden), shared by the tests that run them with the
block-call server on (test_gpu_parity.py, test_dtypes_gpu.py) and the replay
with it off (test_block_forms_gpu.py).  Bar: bit-exact values, the same Python
type and the same exception class."""
import builtins
import hashlib
import warnings

import numpy as np
import pytest


def drop_in(fn):
    from nano_hevc import intra, quant, metrics, transform
    return next(getattr(m, fn) for m in (intra, quant, metrics, transform) if hasattr(m, fn))


def check_dtype_case(fixture, name, fn, args, kw):
    """One call of dtype_cases.py against dtypes.npz."""
    f = drop_in(fn)
    if "err_" + name in fixture:
        base = getattr(builtins, str(fixture["errbase_" + name]))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(base):
                f(*args, **kw)
        return
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = f(*args, **kw)
    exp = fixture["out_" + name]
    assert type(r).__name__ == str(fixture["rtype_" + name])
    got = np.asarray(r)
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(got, exp, equal_nan=got.dtype.kind == "f")


def check_transforms_golden(nh, g, key, n, dst):
    for x, y in zip(g[key + "_fwd_in"], g[key + "_fwd_out"]):
        out = nh.forward_transform(x, use_dst=dst)
        assert out.dtype == np.int32 and np.array_equal(out, y)
    for x, y in zip(g[key + "_inv_in"], g[key + "_inv_out"]):
        assert np.array_equal(nh.inverse_transform(x, use_dst=dst), y)


def check_quant_golden(nh, g):
    for a, qp in enumerate(g["q_qps"]):
        qp = int(qp)
        for b, size in enumerate([4, 8, 16, 32]):
            for c, intra in enumerate([True, False]):
                out = nh.quantize(g["q_vec32"], qp, size, intra)
                assert out.dtype == np.int32 and np.array_equal(out, g["q_out32"][a, b, c]), (qp, size, intra)
                assert np.array_equal(nh.quantize(g["q_vec16"], qp, size, intra), g["q_out16"][a, b, c])
        assert np.array_equal(nh.dequantize(g["dq_in"], qp, 4), g["dq_out"][a]), qp


def check_intra_golden(nh, g, n):
    for s in range(8):
        top = g[f"n{n}_top"][s, :g[f"n{n}_ntop"][s]]
        left = g[f"n{n}_left"][s, :g[f"n{n}_nleft"][s]]
        corner = int(g[f"n{n}_corner"][s])
        for m in range(35):
            st = int(g[f"n{n}_status"][s, m])
            if m == 0:
                t = top[:n] if top.size >= n else top
                l = left[:n] if left.size >= n else left
                fn = lambda: nh.intra_planar_predict(t, l, int(top[min(n, top.size) - 1]),
                                                     int(left[min(n, left.size) - 1]), n)
            elif m == 1:
                fn = lambda: nh.intra_dc_predict(top, left, n)
            else:
                fn = lambda: nh.intra_angular_predict(top, left, corner, m, n)
            if st == 0:
                out = fn()
                assert out.dtype == np.int16 and np.array_equal(out, g[f"n{n}_pred"][s, m]), (n, s, m)
            else:
                with pytest.raises({1: OverflowError, 2: IndexError}[st]):
                    fn()


def check_chain_config1(nh, g):
    pred = nh.intra_dc_predict(g["c1_top"], g["c1_left"], 4)
    res = nh.residual_block(g["c1_orig"], pred)
    coeff = nh.forward_transform(res, use_dst=True)
    assert np.array_equal(pred, g["c1_pred"]) and np.array_equal(res, g["c1_res"]) and np.array_equal(coeff, g["c1_coeff"])
    for qp in (20, 22):
        lvl = nh.quantize_block(coeff, qp)
        deq = nh.dequantize_block(lvl, qp)
        rres = nh.inverse_transform(deq, use_dst=True)
        rec = nh.clip_to_pixel_range(nh.reconstruct_block(pred, rres.astype(np.int16)))
        for k, v in (("lvl", lvl), ("deq", deq), ("rres", rres), ("recon", rec)):
            assert np.array_equal(v, g[f"c1_{k}_qp{qp}"]), (k, qp)


def check_metrics_golden(nh, g):
    for i, (a, b) in enumerate(zip(g["m_a8"], g["m_b8"])):
        assert nh.mse(a, b) == g["m_mse"][i]
        assert nh.psnr(a, b) == g["m_psnr"][i]
        assert nh.psnr(a, b, peak=1023) == g["m_psnr1023"][i]
    assert nh.psnr(g["m_a8"][0], g["m_a8"][0]) == float("inf")
    for i, (a, b) in enumerate(zip(g["m_a16"], g["m_b16"])):
        assert nh.mse(a, b) == g["m_mse16"][i]
        assert nh.sad(a, b) == g["m_sad16"][i]
        assert nh.residual_energy(a) == g["m_energy16"][i]
    for i, (a, b) in enumerate(zip(g["m_a32"], g["m_b32"])):
        assert nh.sad(a, b) == g["m_sad32"][i]
        assert nh.satd_4x4(a, b) == g["m_satd32"][i]
    for i, (a, b) in enumerate(zip(g["m_s4a"], g["m_s4b"])):
        assert nh.satd_4x4(a, b) == g["m_satd"][i]
    for i, e in enumerate(g["m_e64"]):
        assert nh.residual_energy(e) == g["m_energy64"][i]
    with pytest.raises(ValueError):
        nh.satd_4x4(np.arange(8), np.arange(8))


# ------------------------------------------------- block_forms.npz (block_form_cases.py)

def oracle_result(fn, args, kw=None):
    """fn(*args) by the CPU restatement (oracle/), or None where it has no such
    function (the metrics, the level helpers, planar with numpy-scalar corners)."""
    from oracle import oracle as O
    table = {
        "forward_transform": lambda x, dst=False: O.forward_transform(x, dst),
        "inverse_transform": lambda x, dst=False: O.inverse_transform(x, dst),
        "quantize": lambda c, qp, size, intra=True: O.quantize(c, qp, size, intra),
        "dequantize": lambda l, qp, size: O.dequantize(l, qp, size),
        "intra_dc_predict": lambda t, l, n: O.intra_dc(t, l, n),
        "intra_planar_predict": lambda t, l, tr, bl, n: O.intra_planar(t, l, tr, bl, n),
        "intra_angular_predict": lambda t, l, c, m, n: O.intra_angular(t, l, c, m, n),
        "residual_block": O.residual,
        "reconstruct_block": O.reconstruct,
        "clip_to_pixel_range": lambda x, bd=8: O.clip(x, bd),
    }
    if fn not in table or (fn == "intra_planar_predict" and not all(type(c) is int for c in args[2:4])):
        return None
    return table[fn](*args, **(kw or {}))


def same_bits(got, exp) -> bool:
    """Equal dtype, shape and bytes (a float64 result compares as its bits)."""
    got, exp = np.asarray(got), np.asarray(exp)
    return got.dtype == exp.dtype and got.shape == exp.shape and \
        np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(exp).tobytes()


def expected_error(fixture, name):
    """The builtin exception class the reference raised for this case, or None."""
    return getattr(builtins, str(fixture["err_" + name])) if "err_" + name in fixture else None


def check_form_result(fixture, name, value, locate=None):
    """A returned value against the recorded result of one block_form_cases.py
    case.  locate() -- for a result recorded by hash -- gives a second array of
    the expected samples, used only to name the first differing one."""
    assert "err_" + name not in fixture, f"{name}: returned, the reference raised {fixture['err_' + name]}"
    assert type(value).__name__ == str(fixture["rtype_" + name]), name
    got = np.asarray(value)
    if "out_" + name in fixture:
        exp = fixture["out_" + name]
        assert same_bits(got, exp), (name, got, exp)
        return
    assert got.dtype.str == str(fixture["dtype_" + name]) and got.shape == tuple(fixture["shape_" + name]), name
    if hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(fixture["sha_" + name]):
        return
    where = ""
    if locate is not None:
        exp = np.asarray(locate())
        bad = np.flatnonzero(got.ravel() != exp.ravel())
        where = (f": first differing sample {np.unravel_index(bad[0], got.shape)}: got {got.ravel()[bad[0]]}, "
                 f"oracle {exp.ravel()[bad[0]]} ({bad.size} differ)") if bad.size else ": equals the oracle"
    raise AssertionError(f"{name}: SHA-256 differs from the reference's{where}")
