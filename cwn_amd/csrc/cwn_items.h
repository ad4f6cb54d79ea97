// cwn_items.h -- the RECORD RULE of the item tables of the complex-blocked launches (cwn_layer_fused_f32: 32 ints,
// cwn_layer_bwd_own_f32: 16 ints; layouts: include/cwn_hip.h): the field names, the sets, and -- for a range of
// consecutive complexes given by its prefix sums -- whether the range fits one workgroup and what its record is.
// Host and device code.  Every builder and checker calls these definitions and restates none of them: the host
// builders (cwn_blockplan.cpp), the device builders (cwn_items_dev.hip), the host check of a table
// (cwn_layer.hip: items_check); the kernels (cwn_layer.hip, cwn_layer_bwd.hip) take the field names.  What a builder
// keeps to itself is its POLICY: which ranges it tries and in what order the records land.
//
// Device constraint, hence the form of everything below: a by-value kernel argument or a register array is never
// indexed with a run-time index (the compiler would copy the whole structure to scratch: the first form of the device
// builders took 23 us for eight slots, all of it scratch traffic) -- arrays are read with compile-time indices and the
// value is selected (sel3).
#pragma once
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_layer_bwd_own.h"

#if defined(__clang__)
#define CWN_ITEMS_UNROLL _Pragma("unroll")
#else
#define CWN_ITEMS_UNROLL
#endif

namespace cwn_items {

// the forward record
enum { I_FLAGS = 0, I_G, I_GR0, I_GN, I_CR0, I_CN, I_UE0, I_UNE, I_NT, I_TASK0, I_R1 = 23, I_ROWS, I_B1, I_B2, I_TOTAL };
enum { T_DIM = 0, T_R0, T_N, T_BE0, T_BNE, T_SR0, T_SN, T_INTS };
static_assert(I_TASK0 + 2 * T_INTS == I_R1 && I_TOTAL < CWN_LAYER_ITEM_INTS && CWN_LAYER_MAX_DIMS == 3, "record layout");

CWN_BWD_HD int64_t pad16(int64_t n) { return (n + 15) / 16 * 16; }
CWN_BWD_HD int64_t pad4(int64_t n) { return (n + 3) / 4 * 4; }
template <typename T>
CWN_BWD_HD T sel3(int i, T v0, T v1, T v2) { return i == 0 ? v0 : (i == 1 ? v1 : v2); }

// Sets in ascending order of dimension: a dimension with an upper adjacency is the GEMM dimension of a set (the top
// dimension rides as its second task when it has none itself), any other dimension is a set of its own.
// Sizes: cwn_layer_sizes or cwn_layer_sizes_dev (n_dims, has_up)
struct Set { int32_t g, n_tasks, tasks[2]; };
template <class Sizes>
inline int make_sets(const Sizes& in, Set (&sets)[CWN_LAYER_MAX_DIMS]) {
    int n = 0;
    for (int d = 0; d < in.n_dims;) {
        Set& s = sets[n++];
        s.tasks[0] = d;
        s.tasks[1] = 0;
        s.n_tasks = 1;
        if (in.has_up[d]) {
            s.g = d;
            if (d + 1 < in.n_dims && !in.has_up[d + 1] && d + 2 >= in.n_dims) s.tasks[s.n_tasks++] = d + 1;
        } else {
            s.g = -1;
        }
        d += s.n_tasks;
    }
    return n;
}

// A RANGE of consecutive complexes [a, b) is anything that answers, per dimension d, from the batch's prefix sums
// (absent tables: zeros):
//     cells(d), cell0(d)     number of cells, first cell
//     ups(d), up0(d)         number of entries of upper_index_d, first entry
//     bnds(d), bnd0(d)       the same for boundary_index_d
// The device builders load all of it into registers once per range, the host builders read the tables as they are asked:
// the rules below are written against these six questions and ask only for what their set needs.

// what a rule says of a range
enum {
    K_ITEM = 1,     // one item: the record is written
    K_SPLIT = 2,    // beyond a limit of one workgroup
    K_BAD = 4       // cells of a higher dimension, or entries, without cells of the set's first dimension: not a cell complex
};

// ---- forward ---------------------------------------------------------------------------------------------------------
// first staged row of the cells of g + 1 (round 4: a multiple of 16, no longer of the kernel's rows per load round)
CWN_BWD_HD int64_t first_coface_row(int64_t n_g) { return pad16(n_g); }
CWN_BWD_HD int64_t staged_rows(int64_t n_g, int64_t n_c) { return n_c > 0 ? first_coface_row(n_g) + pad16(n_c) : pad16(n_g); }
// = cwn_layer_fused_lds_bytes without its argument checks; idx_bytes: the index scratch (the same in both variants)
CWN_BWD_HD int64_t fwd_lds(int F, int64_t rows, int64_t src, int64_t idx_bytes) {
    return 3 * rows * (F + 8) * 2 + (src + 1) * F * 4 + idx_bytes;
}

// the derived fields [23..27] of a record that is not BIG
struct Derived { int64_t r1, rows, b1, b2, total; };
CWN_BWD_HD Derived derived(int64_t n_g, int64_t n_c, int64_t up_entries, int64_t b_entries0, int64_t b_entries1) {
    Derived D;
    D.r1 = first_coface_row(n_g);
    D.rows = staged_rows(n_g, n_c);
    D.b1 = pad4(up_entries);
    D.b2 = pad4(D.b1 + b_entries0);
    D.total = pad4(D.b2 + b_entries1);
    return D;
}

struct FwdRule {
    int F, variant, set, g, n_tasks, t0, t1;             // the set: cwn_items::Set
    // one workgroup's limits: staged rows, boundary sources in LDS, LDS bytes, (padded) rows of ONE product or 0
    int64_t row_cap, src_cap, lds_budget, half_cap, idx_bytes;
    static constexpr int kRecInts = CWN_LAYER_ITEM_INTS;

    CWN_BWD_HD int task(int t) const { return t == 0 ? t0 : t1; }
    template <class Range>
    CWN_BWD_HD int64_t b_entries(const Range& R, int d) const { return d > 0 ? R.bnds(d) : 0; }

    template <class Range>
    CWN_BWD_HD bool orphans(const Range& R) const { return g >= 0 && R.cells(t0) == 0 && n_tasks > 1 && R.cells(t1) > 0; }

    template <class Range>
    CWN_BWD_HD bool fits(const Range& R) const {
        const int64_t n0 = R.cells(t0), ncf = g >= 0 ? R.cells(g + 1) : 0;
        const int64_t rows = staged_rows(n0, ncf);
        int64_t src = 0, ents = pad4(g >= 0 ? R.ups(g) : 0);
        bool ok = true;
        for (int t = 0; t < n_tasks; ++t) {
            const int d = task(t);
            const int64_t be = b_entries(R, d);
            // (two-per-CU form: only task 0's sources are loaded into LDS; task 1 reads the staged cells of g)
            if (d > 0 && be > 0 && (variant == 0 || t == 0)) src += R.cells(d - 1);
            ents += pad4(be);
            ok = ok && R.cells(d) <= CWN_LAYER_TASK_ROWS;
        }
        ok = ok && rows <= row_cap && src <= src_cap && fwd_lds(F, rows, src, idx_bytes) <= lds_budget && ents <= CWN_LAYER_MAX_ENTRIES;
        if (half_cap > 0 && g >= 0) ok = ok && pad16(n0) <= half_cap && pad16(ncf) <= half_cap;
        return ok;
    }

    // big: the range is one complex that does NOT fit and is streamed by its workgroup: ranges only, [23..27] stay 0
    template <class Range>
    CWN_BWD_HD void record(const Range& R, bool big, int32_t (&r)[kRecInts]) const {
        CWN_ITEMS_UNROLL
        for (int k = 0; k < kRecInts; ++k) r[k] = 0;
        r[I_FLAGS] = (set << 8) | (big ? CWN_LAYER_ITEM_BIG : 0);
        const int64_t n0 = R.cells(t0);
        int64_t nc = 0, une = 0;
        int live = n_tasks;
        if (g >= 0) {
            r[I_G] = g;
            if (n0 > 0) {
                nc = R.cells(g + 1);
                une = R.ups(g);
                r[I_FLAGS] |= 1;
                r[I_GR0] = (int32_t)R.cell0(g);
                r[I_GN] = (int32_t)n0;
                r[I_CR0] = (int32_t)R.cell0(g + 1);
                r[I_CN] = (int32_t)nc;
                r[I_UE0] = (int32_t)R.up0(g);
                r[I_UNE] = (int32_t)une;
            } else {
                live = 1;
            }
        }
        r[I_NT] = live;
        int64_t bne[2] = {0, 0};
        CWN_ITEMS_UNROLL
        for (int t = 0; t < 2; ++t) {
            if (t < live) {
                const int d = task(t), o = I_TASK0 + T_INTS * t;
                bne[t] = b_entries(R, d);
                r[o + T_DIM] = d;
                r[o + T_R0] = (int32_t)R.cell0(d);
                r[o + T_N] = (int32_t)R.cells(d);
                r[o + T_BE0] = (int32_t)(d > 0 ? R.bnd0(d) : 0);
                r[o + T_BNE] = (int32_t)bne[t];
                if (d > 0 && bne[t] > 0) {          // boundary sources are staged only when read
                    r[o + T_SR0] = (int32_t)R.cell0(d - 1);
                    r[o + T_SN] = (int32_t)R.cells(d - 1);
                }
            }
        }
        if (!big) {
            const Derived D = derived(n0, nc, une, bne[0], bne[1]);
            r[I_R1] = (int32_t)D.r1;
            r[I_ROWS] = (int32_t)D.rows;
            r[I_B1] = (int32_t)D.b1;
            r[I_B2] = (int32_t)D.b2;
            r[I_TOTAL] = (int32_t)D.total;
        }
    }

    template <class Range>
    CWN_BWD_HD int classify(const Range& R, int32_t (&r)[kRecInts]) const {
        const bool ok = fits(R);
        if (ok) record(R, false, r);
        return (ok ? K_ITEM : K_SPLIT) | (orphans(R) ? K_BAD : 0);
    }
};

// sources of a finished record that take LDS: both tasks' in the 16-wave form, task 0's in the two-per-CU form
CWN_BWD_HD int64_t lds_sources(const int32_t* r, int variant) {
    return (int64_t)r[I_TASK0 + T_SN] + (variant == 0 ? r[I_TASK0 + T_INTS + T_SN] : 0);
}

// ---- backward, owner form (fields and LDS layout: cwn_layer_bwd_own.h) -----------------------------------------------
struct BwdRule {
    int F, set, d, flags;
    bool above;                     // there is a dimension d + 1
    int64_t lds_cap;                // what one item's layout may take
    static constexpr int kRecInts = CWN_LAYER_BWD_ITEM_INTS;

    // Sizes: n_dims, has_up.  The rule of the items of set S
    template <class Sizes>
    CWN_BWD_HD static BwdRule of(const Sizes& A, int F, int set, const Set& S, int64_t lds_cap) {
        namespace bo = cwn_bwd_own;
        const int d = S.tasks[0];
        const bool pa = sel3(d, A.has_up[0], A.has_up[1], A.has_up[2]) != 0;
        const bool pb = d > 0 && sel3(d - 1, A.has_up[0], A.has_up[1], A.has_up[2]) != 0;
        return BwdRule{F, set, d, (pa ? bo::F_PA : 0) | (pb ? bo::F_PB : 0) | (S.n_tasks == 2 ? bo::F_TOP : 0), d + 1 < A.n_dims, lds_cap};
    }

    // K_ITEM (r is the record), 0 (no owned cells: nothing to write), K_SPLIT or K_BAD
    template <class Range>
    CWN_BWD_HD int classify(const Range& R, int32_t (&r)[kRecInts]) const {
        namespace bo = cwn_bwd_own;
        const bool pa = (flags & bo::F_PA) != 0, pb = (flags & bo::F_PB) != 0, top = (flags & bo::F_TOP) != 0;
        const int64_t n_o = R.cells(d), n_a = above ? R.cells(d + 1) : 0, n_b = pb ? R.cells(d - 1) : 0;
        const int64_t ea = pa ? R.ups(d) : 0, eb = pb ? R.ups(d - 1) : 0, bd = above ? R.bnds(d + 1) : 0;
        if (n_o > bo::own_rows_cap(F) || (top && n_a > bo::top_rows_cap(F))) return K_SPLIT;
        if (ea > CWN_LAYER_MAX_ENTRIES || eb > CWN_LAYER_MAX_ENTRIES || bd > CWN_LAYER_MAX_ENTRIES) return K_SPLIT;
        if (n_a > 4096 || n_b > 4096) return K_SPLIT;                       // (keeps the layout arithmetic far inside int32)
        const bool need_a = pa || top || bd > 0;
        const bo::Layout L = bo::layout(F, flags, (int)n_o, need_a ? (int)n_a : 0, (int)n_b, (int)ea, (int)eb, (int)bd);
        if (L.total > lds_cap) return K_SPLIT;
        if (n_o == 0) return ((top && n_a > 0) || ea > 0 || eb > 0 || bd > 0) ? K_BAD : 0;
        CWN_ITEMS_UNROLL
        for (int k = 0; k < kRecInts; ++k) r[k] = 0;
        r[bo::R_FLAGS] = flags | (set << 8);
        r[bo::R_DIM] = d;
        r[bo::R_OWN_R0] = (int32_t)R.cell0(d);
        r[bo::R_OWN_N] = (int32_t)n_o;
        if (need_a) {
            r[bo::R_ABOVE_R0] = (int32_t)R.cell0(d + 1);
            r[bo::R_ABOVE_N] = (int32_t)n_a;
        }
        if (pb) {
            r[bo::R_BELOW_R0] = (int32_t)R.cell0(d - 1);
            r[bo::R_BELOW_N] = (int32_t)n_b;
            r[bo::R_UPB_E0] = (int32_t)R.up0(d - 1);
            r[bo::R_UPB_NE] = (int32_t)eb;
        }
        if (pa) {
            r[bo::R_UPA_E0] = (int32_t)R.up0(d);
            r[bo::R_UPA_NE] = (int32_t)ea;
        }
        if (bd > 0) {
            r[bo::R_BND_E0] = (int32_t)R.bnd0(d + 1);
            r[bo::R_BND_NE] = (int32_t)bd;
        }
        r[bo::R_LDS_BYTES] = L.total;
        return K_ITEM;
    }
};

}  // namespace cwn_items
