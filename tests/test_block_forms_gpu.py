"""Per-block calls in every execution form, at the form thresholds.

BlockCall::run (csrc/nh_blocks.hip) runs one device body on the resident
block-call server (served), as a single-workgroup kernel fed through the
kernel-argument block (small: 256 B / 1 KB / 3 KB), or staged through device
memory.  With the default idle time the rest of the suite reaches served and
staged only; here (a) the recorded fixtures are replayed with the server off, so
every function's error paths and dtype corners run on k_small, (b) a matrix of
calls sits on both sides of every input and output threshold, each run with the
server on and off, (c) calls with two errors check that the one the reference
meets first wins in every form, and (d) one sequence walks served -> small ->
served -> staged -> small -> served.

Every comparison is bit-exact against what the reference recorded
(tests/golden/block_forms.npz, pinned on the CPU by test_block_forms_host.py),
exception classes included, and every case of (b)-(d) also asserts that the call
took the side of the server that block_forms.predicted_form gives for it."""
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from block_form_cases import cases, claimed_forms  # noqa: E402
from dtype_cases import cases as dtype_cases  # noqa: E402
import block_checks as K  # noqa: E402
from block_forms import collapse, observed, predicted_for, server_off, stats  # noqa: E402

CASES = cases()
DTYPE_CASES = dtype_cases()
_IDLE = {}


@pytest.fixture(scope="module")
def nh():
    import nano_hevc
    from nano_hevc import _lib
    assert _lib.device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    _IDLE.setdefault("before", stats()["idle_us"])
    yield nano_hevc
    # the 262,145-element reductions grew the staged form's buffers (grow-only): hand the context
    # back as a fresh process has it (test_staging_contexts_do_not_grow measures from there)
    _lib.check(_lib.load().nh_release_staging(), "release_staging")


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("block_forms.npz")


# ------------------------------------------------------------------ (a) the fixtures with the server off

class replay:
    """Launch-per-call mode around a replay: no call may be served."""

    def __enter__(self):
        self.off = server_off()
        self.off.__enter__()
        self.s0 = stats()
        assert self.s0["idle_us"] == 0

    def __exit__(self, *exc):
        s1 = stats()
        self.off.__exit__(*exc)
        if exc[0] is None:
            assert s1["served"] == self.s0["served"] and s1["launches"] == self.s0["launches"], (self.s0, s1)
            assert s1["kernel_calls"] > self.s0["kernel_calls"], (self.s0, s1)
        return False


def test_replay_dtype_cases(nh, golden):
    fx = golden("dtypes.npz")
    with replay():
        for name, fn, args, kw in DTYPE_CASES:
            try:
                K.check_dtype_case(fx, name, fn, args, kw)
            except BaseException as e:       # name the case, keep the failure
                raise AssertionError(f"dtype case {name} with the server off: {e!r}") from e


@pytest.mark.parametrize("n", [4, 8, 16, 32])
def test_replay_intra_golden(nh, golden, n):
    with replay():
        K.check_intra_golden(nh, golden("intra.npz"), n)


@pytest.mark.parametrize("key,n,dst", [("n4_dst", 4, True), ("n4_dct", 4, False), ("n8_dct", 8, False),
                                       ("n16_dct", 16, False), ("n32_dct", 32, False)])
def test_replay_transforms_golden(nh, golden, key, n, dst):
    with replay():
        K.check_transforms_golden(nh, golden("transform.npz"), key, n, dst)


def test_replay_quant_golden(nh, golden):
    with replay():
        K.check_quant_golden(nh, golden("quant.npz"))


def test_replay_metrics_golden(nh, golden):
    with replay():
        K.check_metrics_golden(nh, golden("metrics.npz"))


def test_replay_chain_config1(nh, golden):
    with replay():
        K.check_chain_config1(nh, golden("chain.npz"))


# ------------------------------------------------------------------ (b), (c) the threshold matrix and first errors

def _run_case(fixture, name, fn, args, kw, idle_us):
    """One recorded call: the observed side of the server equals the predicted
    form's, then the value (or the exception class) equals the reference's."""
    want = predicted_for(fn, args, kw, idle_us)
    assert want == claimed_forms(name)[0 if idle_us else 1], name
    f = K.drop_in(fn)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        form, ok, value = observed(lambda: f(*args, **kw))
    assert form == collapse(want), f"{name}: ran as {form}, predicted form {want} (idle time {idle_us} us)"
    err = K.expected_error(fixture, name)
    if err is not None:
        assert not ok, f"{name} ({want}): returned, the reference raised {err.__name__}"
        assert type(value) is err, f"{name} ({want}): raised {value!r}, the reference raised {err.__name__}"
        return
    assert ok, f"{name} ({want}): raised {value!r}"
    K.check_form_result(fixture, name, value, locate=lambda: K.oracle_result(fn, args, kw))


@pytest.mark.parametrize("mode", ["server_on", "server_off"])
@pytest.mark.parametrize("name,fn,args,kw", CASES, ids=[c[0] for c in CASES])
def test_case_in_both_modes(nh, fixture, name, fn, args, kw, mode):
    if mode == "server_on":
        idle = stats()["idle_us"]
        assert idle > 0, "the block-call server is expected to be on by default"
        _run_case(fixture, name, fn, args, kw, idle)
    else:
        with server_off():
            _run_case(fixture, name, fn, args, kw, 0)


# ------------------------------------------------------------------ (d) hand-over between the forms

def _small_calls(rng):
    """Ten calls that are served with the server on and small with it off."""
    n = 8
    top, left = rng.integers(0, 256, 2 * n + 1).astype(np.int16), rng.integers(0, 256, 2 * n + 1).astype(np.int16)
    a, b = rng.integers(-32768, 32768, (n, n)).astype(np.int16), rng.integers(-32768, 32768, (n, n)).astype(np.int16)
    c32 = rng.integers(-2**31, 2**31, (16, 16), dtype=np.int64).astype(np.int32)
    lv = rng.integers(-3000, 3001, (n, n)).astype(np.int32)
    return [("intra_dc_predict", (top[:n], left[:n], n)),
            ("intra_planar_predict", (top[:n], left[:n], int(top[n]), int(left[n]), n)),
            ("intra_angular_predict", (top, left, int(top[0]), int(rng.integers(2, 35)), n)),
            ("residual_block", (a, b)),
            ("forward_transform", (a, False)),
            ("inverse_transform", (c32, False)),
            ("quantize", (c32, int(rng.integers(0, 52)), 16, True)),
            ("dequantize", (lv, int(rng.integers(0, 52)), n)),
            ("sad", (lv, lv[::-1].copy())),
            ("count_nonzero", (lv * (lv > 0),))]


def _staged_calls(rng):
    """Ten calls that are staged in either mode: inputs above 8 KB or outputs above 64 KB."""
    n = 4100
    a, b = rng.integers(-32768, 32768, n).astype(np.int16), rng.integers(-32768, 32768, n).astype(np.int16)
    x = rng.integers(-700, 70000, 1100)
    c = rng.integers(-2**31, 2**31, 1100, dtype=np.int64).astype(np.int32)
    t, l = rng.integers(0, 1024, 182).astype(np.int16), rng.integers(0, 1024, 182).astype(np.int16)
    s = rng.integers(-40000, 40000, 1100).astype(np.int32)
    return [("residual_block", (a, b)), ("reconstruct_block", (a, b)), ("clip_to_pixel_range", (x, 10)),
            ("quantize", (c, 30, 8, False)), ("dequantize", (c, 44, 8)),
            ("intra_planar_predict", (t, l, 900, 30, 182)), ("intra_dc_predict", (t[:4], l[:4], 182)),
            ("sad", (s, s[::-1].copy())), ("count_nonzero", (s * (s > 0),)), ("residual_energy", (s,))]


_NUMPY = {"sad": lambda a, b: int(np.sum(np.abs(a.astype(np.int32) - b.astype(np.int32)))),   # metrics.py:24-26
          "count_nonzero": lambda l: int(np.count_nonzero(l)),                                # quant.py:171-173
          "residual_energy": lambda r: int(np.sum(r.astype(np.int64) ** 2))}                  # metrics.py:46-48


def _walk(calls, idle_us, want):
    """Runs the calls; each takes the predicted side of the server and equals the
    oracle (numpy's own expression for the three reductions the oracle lacks)."""
    for fn, args in calls:
        pred = predicted_for(fn, args, {}, idle_us)
        assert collapse(pred) == want, (fn, pred)
        form, ok, value = observed(lambda: K.drop_in(fn)(*args))
        assert form == want, f"{fn}: ran as {form}, predicted form {pred} (idle time {idle_us} us)"
        assert ok, (fn, value)
        exp = K.oracle_result(fn, args)
        if exp is None:
            exp = _NUMPY[fn](*args)
            assert type(value) is int and value == exp, (fn, pred, value, exp)
        else:
            assert K.same_bits(value, exp), (fn, pred)
    return len(calls)


def test_hand_over_between_forms(nh):
    from nano_hevc import gpu
    rng = np.random.default_rng(60)
    idle = stats()["idle_us"]
    assert idle > 0
    gpu.block_server_stop()                 # whatever ran before: the first served call launches a server
    ncalls = 0
    s = stats()
    ncalls += _walk(_small_calls(rng), idle, "served")                    # served
    s1 = stats()
    assert s1["launches"] > s["launches"], (s, s1)
    with server_off():                                                   # -> small (first k_small after a served call)
        ncalls += _walk(_small_calls(rng), 0, "kernel")
        s2 = stats()
        assert s2["launches"] == s1["launches"] and s2["served"] == s1["served"], (s1, s2)
    ncalls += _walk(_small_calls(rng), idle, "served")                    # -> served (relaunch behind a k_small)
    s3 = stats()
    assert s3["launches"] > s2["launches"], (s2, s3)
    ncalls += _walk(_staged_calls(rng), idle, "kernel")                   # -> staged (stop request, then k_staged)
    s4 = stats()
    assert s4["served"] == s3["served"], (s3, s4)
    with server_off():                                                   # -> small (k_small after k_staged)
        ncalls += _walk(_small_calls(rng), 0, "kernel")
        s5 = stats()
        assert s5["launches"] == s4["launches"] and s5["served"] == s4["served"], (s4, s5)
    ncalls += _walk(_small_calls(rng), idle, "served")                    # -> served
    s6 = stats()
    assert s6["launches"] > s5["launches"], (s5, s6)
    assert ncalls == 60
    assert s6["served"] - s["served"] == 30 and s6["kernel_calls"] - s["kernel_calls"] == 30, (s, s6)
    assert s6["idle_us"] == idle


def test_idle_time_is_what_it_was_before_the_module(nh):
    """server_off() leaks nothing: test_block_server_gpu.py asserts 0 < idle_us <= 100."""
    assert stats()["idle_us"] == _IDLE["before"] > 0
