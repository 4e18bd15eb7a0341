"""Float / bool / narrow-float inputs through the drop-in.

tests/golden/dtypes.npz holds, per call of tests/golden/dtype_cases.py, what the
REFERENCE returned (value, dtype and Python type) or which exception it raised
(recorded by make_golden.py --only dtypes.npz).  The MI355X drop-in must give
the same value bit for bit (float results included: mse / psnr are computed in
numpy's pairwise summation order on the device) or raise the same builtin
exception class."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from dtype_cases import cases  # noqa: E402
from block_checks import check_dtype_case  # noqa: E402

CASES = cases()


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(HERE, "golden", "dtypes.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_fixture_covers_every_case(fixture):
    names = {n for n, *_ in CASES}
    got = {k.split("_", 1)[1] for k in fixture if k.startswith(("out_", "err_"))}
    assert names == got


@pytest.mark.parametrize("name,fn,args,kw", CASES, ids=[c[0] for c in CASES])
def test_dtype_case_matches_reference(fixture, name, fn, args, kw):
    check_dtype_case(fixture, name, fn, args, kw)
