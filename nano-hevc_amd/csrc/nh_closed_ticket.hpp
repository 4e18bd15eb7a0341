// Ticket -> (set, plane, block row) map of the closed-loop row wavefronts
// (k_intra_rdo8_closed_tag, k_intra_dec8_closed).  Kept apart
// from the kernels so that host code can run it: tests/closed_ticket_check.cpp
// walks every ticket of many layouts (tests/test_closed_ticket_host.py).  It
// needs of its argument only order, nsets, max_bh and set[k].{row0, np, bh}.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NH_TICKET_FN __host__ __device__ __forceinline__
#else
#define NH_TICKET_FN inline
#endif

namespace nh {

NH_TICKET_FN int ticket_min(int a, int b) { return a < b ? a : b; }

// order 0: plane-major (every row of plane 0, then plane 1, ...).  order 1:
// row-major across planes (block row 0 of every plane of every set, then block
// row 1, ...): a row waits for the row above from step 2*by of its plane on,
// so claiming rows in by order keeps the 1,024 resident waves on rows that can
// start (plane-major parks the lower rows of the first planes on their
// wavefront lag while later planes wait for a slot): 874 -> 590 block steps
// for 8 1080p YUV420 frames in a slot simulation.  Both orders claim row by-1
// of a plane before row by, so a wave only waits on a running or finished row.
template <class Args>
NH_TICKET_FN void closed_ticket(const Args& a, int t, int& si, int& pl, int& by) {
    if (a.order == 0) {
        si = 0;
        for (int k = 1; k < a.nsets; ++k)
            if (t >= a.set[k].row0) si = k;
        const auto& S = a.set[si];
        const int local = t - S.row0;
        pl = local / S.bh;
        by = local - pl * S.bh;
        return;
    }
    // prefix(b) = rows with block row < b = sum_k np_k * min(b, bh_k); largest b with prefix(b) <= t
    int lo = 0, hi = a.max_bh - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        int64_t pre = 0;
        for (int k = 0; k < a.nsets; ++k) pre += (int64_t)a.set[k].np * ticket_min(mid, a.set[k].bh);
        if (pre <= t) lo = mid; else hi = mid - 1;
    }
    by = lo;
    int64_t r = t;
    for (int k = 0; k < a.nsets; ++k) r -= (int64_t)a.set[k].np * ticket_min(by, a.set[k].bh);
    si = 0;
    for (int k = 0; k < a.nsets; ++k) {
        if (by >= a.set[k].bh || a.set[k].np == 0) continue;
        if (r < a.set[k].np) { si = k; break; }
        r -= a.set[k].np;
    }
    pl = (int)r;
}

}  // namespace nh

#undef NH_TICKET_FN
