"""Record tests/golden/block_forms.npz by running the REFERENCE on the calls of
block_form_cases.py.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_block_forms.py [reference path]

Per case: out_<name> (the result as an array) with rtype_<name> (its Python
type), or -- for an array above 4 KB -- sha_<name> (SHA-256 of its C-order
bytes), shape_<name> and dtype_<name>, or err_<name> (the exception's class
name) with errbase_<name> (the builtin class it derives from).
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from block_form_cases import cases  # noqa: E402
from make_golden import _import_reference  # noqa: E402

NAME = "block_forms.npz"
FULL_BYTES = 4096        # larger results are recorded as shape, dtype and SHA-256
BASES = (ZeroDivisionError, OverflowError, IndexError, ValueError, TypeError, AttributeError)


def record(mods):
    out = {}
    for name, fn, args, kw in cases():
        f = next(getattr(m, fn) for m in mods if hasattr(m, fn))
        try:
            r = f(*args, **kw)
        except Exception as e:
            out["err_" + name] = np.array(type(e).__name__)
            out["errbase_" + name] = np.array(next(b.__name__ for b in BASES if isinstance(e, b)))
            continue
        a = np.asarray(r)
        out["rtype_" + name] = np.array(type(r).__name__)
        if a.nbytes > FULL_BYTES:
            out["sha_" + name] = np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())
            out["shape_" + name] = np.array(a.shape, np.int64)
            out["dtype_" + name] = np.array(a.dtype.str)
        else:
            out["out_" + name] = a
    return out


def main():
    mp = os.path.join(HERE, "manifest.json")
    manifest = json.load(open(mp))
    # default: where the manifest says the other fixtures were recorded from ("<repo> @ <path>")
    ref = sys.argv[1] if len(sys.argv) > 1 else manifest["reference"].rsplit("@ ", 1)[1]
    warnings.simplefilter("ignore")
    mods = _import_reference(ref)
    p = os.path.join(HERE, NAME)
    np.savez_compressed(p, **record(mods))
    manifest["files"][NAME] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    with open(mp, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(NAME, os.path.getsize(p), "bytes", manifest["files"][NAME])


if __name__ == "__main__":
    main()
