#!/usr/bin/env python3
"""Operand bounds of k_intra_rdo_n's chains (csrc/nh_rdo_n.hip).

The chain of every mode starts from an int16 residual (residual_block wraps to
int16 whatever the prediction), so its bounds do not depend on the mode.  For
DST4, DCT4, DCT16 and DCT32 and every QP 0..51 this enumerates, with the
worst-case L1 bounds of the integer bases:

* every data operand of a 24-bit multiply (Mul24 / v_mad_i32_i24) fits signed
  24 bits: the forward butterflies' operands are sums of at most N inputs, the
  inverse butterflies multiply their inputs directly;
* quant_s's range: |coefficient| <= 2^17, so |c * mf/2 + offset| < 2^31;
* dequant_s: the level fits the 24-bit multiply and |l * dqs + dqr| < 2^31, so the
  32-bit form equals dequantize_block's int64 one.

Sums inside a transform pass are taken mod 2^32 by the kernel and by the
reference alike; only the multiply operands need a range.
"""
from __future__ import annotations

import numpy as np

import packed_bounds as pb

KINDS = ((4, True), (4, False), (16, False), (32, False))
I24 = 1 << 23


def bounds(n, dst, qp, x0=32768):
    """Worst-case magnitudes along one chain for residuals |x| <= x0."""
    T = pb.mat(n, dst)
    l2 = int(np.log2(n))
    s = l2 + 5
    row = int(abs(T).sum(1).max())          # forward: y[k] = sum_n T[k][n] x[n]
    col = int(abs(T).sum(0).max())          # inverse: x[n] = sum_k T[k][n] y[k]
    per, rem = qp // 6, qp % 6
    f1_op = x0 if dst else x0 * n           # butterfly sums of up to N inputs
    f1 = pb.shift_bound(row * x0, s)
    f2_op = f1 if dst else f1 * n
    coef = pb.shift_bound(row * f1, s)
    level = pb.quant(coef, qp, l2, True)
    sh = 14 + per + l2
    quant_acc = coef * (pb.QS[rem] // 2) + ((1 << sh) // 3 >> 1) + (1 << (sh - 1))
    dqs = pb.DQ[rem] << max(0, per - 4)
    deq_acc = level * dqs + (1 << (3 - per) if per < 4 else 0)
    deq = abs(pb.dequant(level, qp))
    i1 = pb.shift_bound(col * deq, s)
    return {"fwd1_operand": f1_op, "fwd2_operand": f2_op, "coef": coef, "level": level, "quant_acc": quant_acc,
            "dequant_acc": deq_acc, "inv1_operand": deq, "inv2_operand": i1}


def check(n, dst, qp):
    b = bounds(n, dst, qp)
    for k in ("fwd1_operand", "fwd2_operand", "level", "inv1_operand", "inv2_operand"):
        assert b[k] < I24, (n, dst, qp, k, b[k])
    assert b["coef"] <= 1 << 17, (n, dst, qp, b["coef"])
    assert b["quant_acc"] < 1 << 31 and b["dequant_acc"] < 1 << 31, (n, dst, qp, b)
    return b


def main():
    for n, dst in KINDS:
        worst = {}
        for qp in range(52):
            for k, v in check(n, dst, qp).items():
                worst[k] = max(worst.get(k, 0), v)
        print(f"{'DST' if dst else 'DCT'}{n}: " + ", ".join(f"{k} {v}" for k, v in worst.items()))


if __name__ == "__main__":
    main()
