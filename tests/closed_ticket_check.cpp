// Host property check of closed_ticket (nano-hevc_amd/csrc/nh_closed_ticket.hpp),
// the ticket -> (set, plane, block row) map of the closed-loop row wavefronts.
// Built with the sanitizers and run once by tests/test_closed_ticket_host.py.
//
// For both ticket orders, over every layout below:
//   1. tickets 0 .. total_rows-1 map one-to-one onto {(set, plane, by)};
//   2. within a plane the ticket of row by-1 is lower than the ticket of row by
//      (a wave only ever waits on a row that was claimed before its own);
//   3. in order 1, by never decreases with the ticket.
// Layouts: every configuration of 1..3 sets with np 0..3 and bh 0..4, seeded
// random configurations of up to 8 sets, the 64-frame 1080p YUV420 stream, and
// the layouts of tests/test_closed_wavefront_gpu.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "nh_closed_ticket.hpp"

namespace {

constexpr int kMaxSets = 8;   // NH_MAX_PLANE_SETS

struct Set {
    int32_t row0, np, bh;
};
struct Args {
    int32_t order, nsets, max_bh;
    Set set[kMaxSets];
};

long g_layouts = 0, g_tickets = 0;

// row0 / max_bh as closed_layout (nh_intraloop.hip) fills them: max_bh over every set, planes or not
Args layout(const std::vector<int>& np, const std::vector<int>& bh, int order, int64_t& total) {
    Args a{};
    a.order = order;
    a.nsets = (int)np.size();
    int64_t rows = 0;
    for (int k = 0; k < a.nsets; ++k) {
        a.set[k] = Set{(int32_t)rows, np[k], bh[k]};
        if (bh[k] > a.max_bh) a.max_bh = bh[k];
        rows += (int64_t)np[k] * bh[k];
    }
    total = rows;
    return a;
}

bool fail(const Args& a, const char* what, int t, int si, int pl, int by) {
    std::fprintf(stderr, "closed_ticket: %s: order %d ticket %d -> set %d plane %d by %d; sets (np x bh):", what,
                 a.order, t, si, pl, by);
    for (int k = 0; k < a.nsets; ++k) std::fprintf(stderr, " %dx%d", a.set[k].np, a.set[k].bh);
    std::fprintf(stderr, "\n");
    return false;
}

bool check(const std::vector<int>& np, const std::vector<int>& bh, int order) {
    int64_t total = 0;
    const Args a = layout(np, bh, order, total);
    if (total == 0) return true;   // no row: the kernels are not launched
    // slot of (set, plane, by): the set's first row + plane * bh + by (any bijection serves)
    std::vector<int32_t> ticket_of((size_t)total, -1);
    int last_by = 0;
    for (int t = 0; t < (int)total; ++t) {
        int si = -1, pl = -1, by = -1;
        nh::closed_ticket(a, t, si, pl, by);
        if (si < 0 || si >= a.nsets || pl < 0 || pl >= a.set[si].np || by < 0 || by >= a.set[si].bh)
            return fail(a, "outside the layout", t, si, pl, by);
        const size_t slot = (size_t)a.set[si].row0 + (size_t)pl * a.set[si].bh + by;
        if (ticket_of[slot] >= 0) return fail(a, "row claimed twice", t, si, pl, by);
        ticket_of[slot] = t;
        // the row above was claimed by a lower ticket: tickets run upwards, so "already claimed" is that
        if (by > 0 && ticket_of[slot - 1] < 0) return fail(a, "row above not claimed yet", t, si, pl, by);
        if (order == 1 && by < last_by) return fail(a, "by decreases in order 1", t, si, pl, by);
        last_by = by;
    }
    // total tickets, no slot twice, every slot inside [0, total): one-to-one and onto
    for (int64_t s = 0; s < total; ++s)
        if (ticket_of[(size_t)s] < 0) return fail(a, "a row has no ticket", (int)s, -1, -1, -1);
    ++g_layouts;
    g_tickets += total;
    return true;
}

bool both_orders(const std::vector<int>& np, const std::vector<int>& bh) {
    return check(np, bh, 0) && check(np, bh, 1);
}

}  // namespace

int main() {
    // every configuration of 1..3 sets, np 0..3, bh 0..4
    for (int n = 1; n <= 3; ++n) {
        int combos = 1;
        for (int k = 0; k < n; ++k) combos *= 20;
        for (int c = 0; c < combos; ++c) {
            std::vector<int> np(n), bh(n);
            for (int k = 0, v = c; k < n; ++k, v /= 20) {
                np[k] = (v % 20) / 5;
                bh[k] = (v % 20) % 5;
            }
            if (!both_orders(np, bh)) return 1;
        }
    }
    // seeded random configurations, up to 8 sets; a quarter of the sets have no plane or no row
    std::mt19937 rng(20240611u);
    for (int it = 0; it < 4000; ++it) {
        const int n = 1 + (int)(rng() % kMaxSets);
        std::vector<int> np(n), bh(n);
        for (int k = 0; k < n; ++k) {
            const unsigned kind = rng() % 8;
            np[k] = kind == 0 ? 0 : 1 + (int)(rng() % (it % 100 == 0 ? 600 : 16));
            bh[k] = kind == 1 ? 0 : 1 + (int)(rng() % (it % 10 == 0 ? 140 : 12));
        }
        if (!both_orders(np, bh)) return 1;
    }
    // 64 frames of 1080p YUV420: 64 Y planes of 135 block rows, 128 chroma planes of 67
    if (!both_orders({64, 128}, {135, 67})) return 1;
    // tests/test_closed_wavefront_gpu.py: the recycling call and the eight-set calls
    if (!both_orders({8192, 4096}, {3, 1})) return 1;
    if (!both_orders({2, 1, 3, 2, 1, 3, 2, 1}, {0, 1, 2, 5, 3, 1, 4, 2})) return 1;
    if (!both_orders({2, 1, 0, 2, 1, 3, 2, 1}, {0, 1, 2, 5, 3, 1, 0, 2})) return 1;
    std::printf("closed_ticket ok: %ld layouts, %ld tickets\n", g_layouts, g_tickets);
    return 0;
}
