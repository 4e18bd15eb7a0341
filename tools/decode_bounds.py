"""Range proof for the 24-bit multiplies of k_dequant_inv8x8.

The kernel's short form serves levels inside int16 (every level of an int16
plane; the blocks of an int32 plane whose 64 levels all pass the int16 test):

  * dequantiser: one signed 24-bit mad, (l * dqs + dqr) >> dqsh with
    dqs = scale << max(0, per - 4).  Needs l and dqs inside signed 24 bits and
    the sum inside int32, and must equal quant.py:112-123 (int64, then
    astype(int32)) for every int16 l at every QP: enumerated here in full.
  * inverse pass 1 multiplies the dequantised coefficients themselves (the
    inverse butterfly multiplies first and adds after), so v_mad_i32_i24 is exact
    iff they fit signed 24 bits.  The host's rule is ``dqs <= 256`` (QP <= 40):
    asserted to be exactly the set of QPs whose coefficients all fit.
  * inverse pass 2 multiplies (acc + 128) >> 8 of a wrapped int32, which is in
    [-2^23, 2^23) whatever acc is: always exact.

Prints one line per QP and fails if a claim does not hold.
"""
import numpy as np

DQ = [40, 45, 51, 57, 64, 72]
I24_LO, I24_HI = -(1 << 23), (1 << 23) - 1


def short_params(qp):
    """(dqs, dqr, dqsh) as nh_dequant_inv8x8_planes computes them."""
    qp = max(0, min(51, qp))
    per, scale = qp // 6, DQ[qp % 6]
    if per < 4:
        return scale, 1 << (3 - per), 4 - per
    return scale << (per - 4), 0, 0


def p24_rule(qp):
    """The host's choice of the 24-bit pass 1 for int16-range levels."""
    return short_params(qp)[0] <= 256


def reference_dequant(level, qp):
    """quant.py:112-123 on an int64 array, before its astype(int32)."""
    qp = max(0, min(51, qp))
    per, scale = qp // 6, DQ[qp % 6]
    base = level.astype(np.int64) * scale
    if per < 4:
        sh = 4 - per
        return (base + (1 << (sh - 1))) >> sh
    return base << (per - 4)


def main():
    lv = np.arange(-32768, 32768, dtype=np.int64)          # every int16 level
    assert I24_LO <= lv.min() and lv.max() <= I24_HI       # the mad's level operand
    fits = []
    for qp in range(52):
        dqs, dqr, dqsh = short_params(qp)
        assert 0 < dqs <= I24_HI
        acc = lv * dqs + dqr
        assert -(1 << 31) <= acc.min() and acc.max() < (1 << 31), qp   # the mad's 32-bit sum never wraps
        short = acc >> dqsh
        ref = reference_dequant(lv, qp)
        assert np.array_equal(ref, ref.astype(np.int32)), qp            # astype(int32) changes nothing here
        assert np.array_equal(short, ref), qp
        ok = bool(I24_LO <= short.min() and short.max() <= I24_HI)
        assert ok == p24_rule(qp), qp
        fits.append(ok)
        print(f"QP {qp:2d}: dqs {dqs:5d}  coefficients [{short.min():10d}, {short.max():10d}]  "
              f"24-bit pass 1: {'yes' if ok else 'no (32-bit products)'}")
    assert fits == [qp <= 40 for qp in range(52)]
    # pass 2 operands: (acc + 128) >> 8 of any int32 (the +128 wraps like the int32 accumulator)
    for acc in (-(1 << 31), (1 << 31) - 1, (1 << 31) - 128, 0, -1):
        wrapped = ((acc + 128 + (1 << 31)) % (1 << 32)) - (1 << 31)
        assert I24_LO <= wrapped >> 8 <= I24_HI
    assert (-(1 << 31)) >> 8 == I24_LO and ((1 << 31) - 1) >> 8 == I24_HI
    print("pass 2 operands: int32 >> 8 in [-2^23, 2^23): always inside signed 24 bits")


if __name__ == "__main__":
    main()
