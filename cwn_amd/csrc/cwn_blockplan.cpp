// cwn_blockplan.cpp -- the item tables of the complex-blocked launches, built on the HOST (no GPU code).
//
// A batched complex is a disjoint union: the reference's collate offsets every index per complex
// (data/complex.py:148-169) and records where each complex's cells and index entries lie (`ptr`, data/complex.py:344,
// 432; `__slices__`, :349-394).  From those per-complex prefix sums this file cuts a batch into ITEMS -- contiguous
// ranges of complexes for one GEMM dimension, one workgroup each (record layout: include/cwn_hip.h).  Whether a range
// fits a workgroup and what its record is: cwn_items.h, the one rule this file shares with the device builders and the
// checker.  What is this file's own is the POLICY: ranges grow greedily up to a target number of items, a few splits of
// one launch's LDS between staged rows and boundary sources are tried so that the items are as few as they can be,
// heavy items come first.  A first version did this in Python (11 ms for a ZINC-like batch of 128, 90 ms for 1024:
// more than the forward pass it prepares); this one is a few tens of microseconds.
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <cstdlib>
#include <vector>
#include "cwn_items.h"

namespace {

using namespace cwn_items;

constexpr int kTargetItemsDefault = 128;      // per GEMM dimension: ~one workgroup per CU over the two sets of a 2-complex
// (CWN_LAYER_TARGET_ITEMS: tuning experiments -- how many complexes an item may hold at most = C / target)
static const int kTargetItems = [] {
    const char* e = getenv("CWN_LAYER_TARGET_ITEMS");
    const int v = e != nullptr ? atoi(e) : 0;
    return v > 0 ? v : kTargetItemsDefault;
}();

// a range of complexes [a, b) (cwn_items.h), read off the host's prefix sums as the rule asks
struct Span {
    const cwn_layer_sizes& in;
    int64_t a, b;
    int64_t first(const int64_t* p) const { return p ? p[a] : 0; }
    int64_t count(const int64_t* p) const { return p ? p[b] - p[a] : 0; }
    int64_t cells(int d) const { return count(in.cell_ptr[d]); }
    int64_t cell0(int d) const { return first(in.cell_ptr[d]); }
    int64_t ups(int d) const { return count(in.up_ptr[d]); }
    int64_t up0(int d) const { return first(in.up_ptr[d]); }
    int64_t bnds(int d) const { return count(in.b_ptr[d]); }
    int64_t bnd0(int d) const { return first(in.b_ptr[d]); }
};

// what both entry points ask of their arguments.  Every table is a prefix sum: starts at 0, never decreases, and its
// total fits the int32 fields of a record
bool valid(const cwn_layer_sizes* in, int32_t F, const int32_t* items, int64_t cap_items, const void* plan) {
    if (in == nullptr || plan == nullptr || (F != 64 && F != 128) || in->n_dims < 1 || in->n_dims > CWN_LAYER_MAX_DIMS ||
        in->n_complexes < 0 || (cap_items > 0 && items == nullptr))
        return false;
    auto prefix_sum = [n = in->n_complexes](const int64_t* p) {
        if (p[0] != 0) return false;
        for (int64_t c = 0; c < n; ++c)
            if (p[c + 1] < p[c]) return false;
        return p[n] <= INT32_MAX;
    };
    for (int d = 0; d < in->n_dims && in->n_complexes > 0; ++d) {
        if (in->cell_ptr[d] == nullptr || !prefix_sum(in->cell_ptr[d])) return false;
        if (in->has_up[d] && (d + 1 >= in->n_dims || in->up_ptr[d] == nullptr)) return false;
        if (in->up_ptr[d] != nullptr && !prefix_sum(in->up_ptr[d])) return false;
        if (in->b_ptr[d] != nullptr && !prefix_sum(in->b_ptr[d])) return false;
    }
    return true;
}

// what a table addresses, per dimension (cwn_layer_plan / cwn_layer_bwd_plan)
template <class Plan>
void plan_ends(const cwn_layer_sizes& in, Plan& plan) {
    const int64_t C = in.n_complexes;
    for (int d = 0; d < CWN_LAYER_MAX_DIMS; ++d) {
        const bool on = d < in.n_dims;
        plan.cells_end[d] = on ? in.cell_ptr[d][C] : 0;
        plan.up_end[d] = on && in.has_up[d] && in.up_ptr[d] ? in.up_ptr[d][C] : 0;
        plan.b_end[d] = on && d > 0 && in.b_ptr[d] ? in.b_ptr[d][C] : 0;
    }
}

// the records of one set (recs, `ints` each) onto out, heavy items first (stable): a workgroup with five row tiles
// should not start last
void append_heavy_first(const std::vector<int32_t>& recs, const std::vector<int64_t>& weight, int ints, std::vector<int32_t>& out) {
    std::vector<int64_t> order(weight.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int64_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return weight[a] > weight[b]; });
    for (int64_t i : order) out.insert(out.end(), recs.begin() + i * ints, recs.begin() + (i + 1) * ints);
}

int64_t group_max(int64_t C, int variant) { return std::max<int64_t>(1, C / (variant == 1 ? 2 * kTargetItems : kTargetItems)); }   // two workgroups a CU

// one greedy cut under the caps of `rule` (its set fields are filled in here).  >= 1 items, 0 nothing to do, -1 a
// single complex exceeds a cap or is no cell complex
int64_t build_with(const cwn_layer_sizes& in, FwdRule rule, std::vector<int32_t>& out, cwn_layer_plan& plan) {
    constexpr int kInts = FwdRule::kRecInts;
    const int64_t C = in.n_complexes;
    out.clear();
    Set sets[CWN_LAYER_MAX_DIMS];
    const int n_sets = make_sets(in, sets);
    const int64_t gmax = group_max(C, rule.variant);
    int64_t max_rows = 0, max_src = 0, max_item_lds = 0, n_big = 0;
    std::vector<int32_t> recs;
    std::vector<int64_t> weight;
    auto skipped = [&](int64_t c) { return in.skip != nullptr && in.skip[c]; };      // not in this table (ranges break at it)
    for (int s_ = 0; s_ < n_sets; ++s_) {
        rule.set = s_;
        rule.g = sets[s_].g;
        rule.n_tasks = sets[s_].n_tasks;
        rule.t0 = sets[s_].tasks[0];
        rule.t1 = sets[s_].tasks[1];
        recs.clear();
        weight.clear();
        for (int64_t c0 = 0; c0 < C;) {
            if (skipped(c0)) { ++c0; continue; }
            int64_t c1 = c0;
            while (c1 < C && c1 - c0 < gmax && !skipped(c1) && rule.fits(Span{in, c0, c1 + 1})) ++c1;
            const bool big = c1 == c0;          // not even this one complex fits a workgroup
            if (big && in.unfit != nullptr) {   // the caller serves it with another launch: marked, left out
                in.unfit[c0] = 1;
                ++c0;
                continue;
            }
            if (big) {
                if (!in.allow_big || rule.variant != 0) return -1;
                c1 = c0 + 1;                    // a BIG record of its own: the workgroup streams it (include/cwn_hip.h)
                ++n_big;
            }
            const Span R{in, c0, c1};
            if (rule.orphans(R)) return -1;
            int32_t r[kInts];
            rule.record(R, big, r);
            if (!big) {
                const int64_t src = lds_sources(r, rule.variant);
                max_rows = std::max<int64_t>(max_rows, r[I_ROWS]);
                max_src = std::max(max_src, src);
                max_item_lds = std::max(max_item_lds, fwd_lds(rule.F, r[I_ROWS], src, rule.idx_bytes));
            }
            recs.insert(recs.end(), r, r + kInts);
            weight.push_back((int64_t)r[I_TASK0 + T_N] + r[I_CN]);       // (a big item is the heaviest of its set: it starts first)
            c0 = c1;
        }
        plan.set_start[s_] = (int32_t)(out.size() / kInts);
        append_heavy_first(recs, weight, kInts, out);
    }
    for (int s_ = n_sets; s_ <= CWN_LAYER_MAX_DIMS; ++s_) plan.set_start[s_] = 0;
    plan.n_items = (int64_t)(out.size() / kInts);
    plan.max_gemm_rows = (int32_t)std::max<int64_t>(max_rows, 16);
    plan.max_source_rows = (int32_t)max_src;
    plan.variant = rule.variant;
    plan.lds_bytes = rule.variant == 1 ? max_item_lds : 0;
    plan.n_big = n_big;
    plan_ends(in, plan);
    return plan.n_items;
}

}  // namespace

extern "C" int64_t cwn_layer_items_build(const cwn_layer_sizes* in, int32_t F, int32_t* items, int64_t cap_items,
                                         cwn_layer_plan* plan) {
    if (!valid(in, F, items, cap_items, plan)) return CWN_LAYER_ITEMS_BAD_ARG;
    if (in->n_complexes == 0) return 0;
    const int variant = plan->variant;
    if (variant != 0 && variant != 1) return CWN_LAYER_ITEMS_BAD_ARG;
    if (cwn_layer_variant_round_rows(F, variant) <= 0) return CWN_LAYER_ITEMS_BAD_ARG;
    static const int64_t idx = (int64_t)cwn_layer_fused_lds_bytes(128, 16, 0) - 3 * 16 * (128 + 8) * 2 - 128 * 4;   // same in both variants
    const int64_t kLds = variant == 1 ? (int64_t)CWN_LAYER_W8_LDS_BYTES : (int64_t)160 * 1024;
    FwdRule rule{};
    rule.F = F;
    rule.variant = variant;
    rule.lds_budget = kLds;
    rule.half_cap = variant == 1 ? (int64_t)CWN_LAYER_W8_HALF_ROWS(F) : 0;
    rule.idx_bytes = idx;
    // one launch = one LDS size: the planes for the LARGEST staged block of any item plus the sources of the item with
    // the most of them (different items, in general).  A few splits of the LDS between the two are tried -- row cap
    // from the top down, the source cap = what is left -- and the one with the fewest items wins
    const int64_t cap = variant == 1 ? CWN_LAYER_W8_GEMM_ROWS(F) : CWN_LAYER_GEMM_ROWS(F);
    const int64_t src_max = variant == 1 ? CWN_LAYER_W8_SOURCE_ROWS(F) : CWN_LAYER_SOURCE_ROWS(F), step = std::max<int64_t>(16, cap / 8);
    std::vector<int32_t> cur, best;
    int64_t floor_items = 0;
    {
        Set sets_[CWN_LAYER_MAX_DIMS];
        const int n_sets_ = make_sets(*in, sets_);
        const int64_t gmax_ = group_max(in->n_complexes, variant);
        floor_items = (in->skip == nullptr) ? n_sets_ * ((in->n_complexes + gmax_ - 1) / gmax_) : -1;
    }
    cwn_layer_plan pc = *plan, pb = *plan;
    bool have = false, too_big = false;
    for (int64_t row_cap = cap; row_cap >= step; row_cap -= step) {
        // variant 1: every item lays out its own rows, so rows and sources are coupled per ITEM (inside build_with) and
        // one pass with both caps at their maxima is the whole search
        const int64_t src_cap = variant == 1 ? src_max : std::min(src_max, (kLds - fwd_lds(F, row_cap, -1, idx)) / (F * 4) - 1);
        if (src_cap < 16) continue;
        rule.row_cap = row_cap;
        rule.src_cap = src_cap;
        const int64_t n = build_with(*in, rule, cur, pc);
        if (n < 0) { too_big = true; if (variant == 1) break; continue; }
        if (n == 0 || (variant == 0 && fwd_lds(F, pc.max_gemm_rows, pc.max_source_rows, idx) > kLds)) continue;
        if (variant == 1) { best.swap(cur); pb = pc; have = true; break; }
        if (!have || pc.n_big < pb.n_big || (pc.n_big == pb.n_big && n < pb.n_items)) {      // fewest streamed complexes first
            best.swap(cur);
            pb = pc;
            have = true;
        } else if (n > pb.n_items + pb.n_items / 8) {
            break;                               // getting worse: smaller row caps only split more
        }
        // no table has fewer items than one per gmax complexes and set: the search is over (the usual case at small
        // batches: one complex per item whatever the split -- six more greedy passes were half of the 88 us a table cost)
        if (have && pb.n_big == 0 && pb.n_items == floor_items) break;
    }
    if (!have) return too_big ? CWN_LAYER_ITEMS_TOO_LARGE : 0;
    if (pb.n_items > cap_items) return CWN_LAYER_ITEMS_BAD_ARG;
    std::copy(best.begin(), best.end(), items);
    const int32_t* keep_items = plan->items;
    void* keep_cache = plan->csr_cache;
    *plan = pb;
    plan->items = keep_items;
    plan->csr_cache = keep_cache;
    return pb.n_items;
}

// ---- the OWNER form of the backward launch (include/cwn_hip.h: cwn_layer_bwd_own_f32) ------------------------------------
// Same sets as the forward (a top dimension without upper adjacency rides with the one below), one greedy cut per set
// under the limits of the kernel; the LDS of an item follows from its record (cwn_layer_bwd_own.h).
extern "C" int64_t cwn_layer_bwd_items_build(const cwn_layer_sizes* in, int32_t F, int32_t* items, int64_t cap_items,
                                             cwn_layer_bwd_plan* plan) {
    if (!valid(in, F, items, cap_items, plan)) return CWN_LAYER_ITEMS_BAD_ARG;
    const int64_t C = in->n_complexes;
    if (C == 0) return 0;
    constexpr int kI = BwdRule::kRecInts;
    Set sets[CWN_LAYER_MAX_DIMS];
    const int n_sets = make_sets(*in, sets);
    const int64_t gmax = group_max(C, 0);
    std::vector<int32_t> out, recs;
    std::vector<int64_t> weight;
    int64_t max_lds = 0;
    int32_t r[kI];
    for (int s_ = 0; s_ < n_sets; ++s_) {
        const BwdRule rule = BwdRule::of(*in, F, s_, sets[s_], cwn_bwd_own::kLdsCap);
        recs.clear();
        weight.clear();
        for (int64_t c0 = 0; c0 < C;) {
            int64_t c1 = c0;
            while (c1 < C && c1 - c0 < gmax && (rule.classify(Span{*in, c0, c1 + 1}, r) & K_SPLIT) == 0) ++c1;
            if (c1 == c0) return CWN_LAYER_ITEMS_TOO_LARGE;                   // not even this one complex fits a workgroup
            const Span R{*in, c0, c1};
            const int k = rule.classify(R, r);
            if (k & K_BAD) return CWN_LAYER_ITEMS_TOO_LARGE;
            c0 = c1;
            if (!(k & K_ITEM)) continue;                                      // no owned cells: nothing to write
            max_lds = std::max<int64_t>(max_lds, r[cwn_bwd_own::R_LDS_BYTES]);
            recs.insert(recs.end(), r, r + kI);
            weight.push_back(R.cells(rule.d) + (rule.above ? R.cells(rule.d + 1) : 0) + r[cwn_bwd_own::R_UPA_NE] + r[cwn_bwd_own::R_UPB_NE]);
        }
        append_heavy_first(recs, weight, kI, out);
    }
    const int64_t n_items = (int64_t)(out.size() / kI);
    if (n_items > cap_items) return CWN_LAYER_ITEMS_BAD_ARG;
    std::copy(out.begin(), out.end(), items);
    plan->n_items = n_items;
    plan->lds_bytes = max_lds;
    plan_ends(*in, *plan);
    return n_items;
}
