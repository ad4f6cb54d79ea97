// act_message_host_check.cpp -- the host launcher of the activated message (csrc/cwn_aggregate_act_body.h, launch_act) on
// its own, under the host sanitizers: the four entry points with the descriptors tests/test_act_message_host.py and
// tests/test_act_message_bwd_host.py refuse, n = 0 and eight empty descriptors.  Every call returns ahead of the first
// launch, so it needs no GPU.  Build and run (from the repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/act_message_host_check.cpp cwn_amd/csrc/cwn_aggregate_act.hip cwn_amd/csrc/cwn_aggregate_act_bwd.hip \
//       -o act_message_host_check && ./act_message_host_check
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../include/cwn_hip.h"

namespace {

int failures = 0;

void expect(int got, int want, const char* entry, const char* what) {
    if (got != want) {
        printf("FAIL %s, %s: %d, expected %d\n", entry, what, got, want);
        ++failures;
    }
}

template <class T> T* at(uintptr_t a) { return reinterpret_cast<T*>(a); }
constexpr uintptr_t P = 0x10000;      // made-up, aligned addresses: no call here gets as far as reading one

// descriptors that pass every check (a call with one of them alone would launch: each case below breaks one thing)
template <class Desc, class real> Desc good_fwd() {
    Desc d{};
    d.rowptr = at<int32_t>(P); d.ia = at<int32_t>(2 * P); d.ib = at<int32_t>(3 * P); d.A = at<real>(4 * P); d.B = at<real>(5 * P);
    d.self_x = at<real>(6 * P); d.eps = at<real>(7 * P); d.out = at<real>(8 * P); d.long_rows = at<int32_t>(9 * P);
    d.n_long = at<int32_t>(10 * P); d.n_dst = 10; d.F = 8; d.act = CWN_ACT_ELU; d.long_cap = 1; d.flags = CWN_AGG_SMALL_OPERANDS;
    return d;
}
template <class Desc, class real> Desc good_bwd() {
    Desc d{};
    d.rowptr = at<int32_t>(P); d.ig = at<int32_t>(2 * P); d.iq = at<int32_t>(3 * P); d.g = at<real>(4 * P); d.P = at<real>(5 * P);
    d.Q = at<real>(6 * P); d.out = at<real>(8 * P); d.long_rows = at<int32_t>(9 * P); d.n_long = at<int32_t>(10 * P);
    d.n_dst = 10; d.F = 8; d.act = CWN_ACT_ELU; d.long_cap = 1; d.flags = CWN_AGG_SMALL_OPERANDS;
    return d;
}

// what both directions refuse in the same way; `Fn` is the entry point, `good` its passing descriptor
template <class Desc, class real, class Fn> void common(const char* entry, Fn fn, const Desc good) {
    auto one = [&](Desc d, int want, const char* what) {
        expect(fn(&d, 1, nullptr), want, entry, what);
        if (want != CWN_ERR_BAD_ARG) return;
        Desc two[2] = {good, d};      // ... wherever it stands among descriptors that launch nothing themselves
        two[0].n_dst = 0;
        expect(fn(two, 2, nullptr), want, entry, what);
    };
    Desc d;
    d = good; d.act = -1; one(d, CWN_ERR_BAD_ARG, "act = -1");
    d = good; d.act = 5; one(d, CWN_ERR_BAD_ARG, "act = 5");
    d = good; d.F = 0; one(d, CWN_ERR_BAD_ARG, "F = 0");
    d = good; d.F = -3; one(d, CWN_ERR_BAD_ARG, "F < 0");
    d = good; d.n_dst = -1; one(d, CWN_ERR_BAD_ARG, "n_dst < 0");
    d = good; d.out = nullptr; one(d, CWN_ERR_BAD_ARG, "out NULL");
    d = good; d.n_dst = INT32_MAX; one(d, CWN_ERR_TOO_LARGE, "n_dst = 2^31 - 1");
    d = good; d.n_dst = (int64_t)1 << 40; one(d, CWN_ERR_TOO_LARGE, "n_dst = 2^40");
    d = good; d.out = at<real>(20 * P + sizeof(real) / 2); one(d, CWN_ERR_ALIGN, "out misaligned");
    d = good; d.act = 7; d.out = at<real>(P + 1); one(d, CWN_ERR_BAD_ARG, "a bad activation wins over a misaligned pointer");

    expect(fn(nullptr, 0, nullptr), CWN_OK, entry, "n = 0 without an array");
    d = good;
    expect(fn(&d, 0, nullptr), CWN_OK, entry, "n = 0 with an array");
    expect(fn(nullptr, 1, nullptr), CWN_ERR_BAD_ARG, entry, "n = 1 without an array");
    expect(fn(&d, -1, nullptr), CWN_ERR_BAD_ARG, entry, "n < 0");
    d.n_dst = 0;
    const std::vector<Desc> empty(CWN_MAX_DESCS + 1, d);        // exactly as long as the longest read below
    expect(fn(empty.data(), CWN_MAX_DESCS + 1, nullptr), CWN_ERR_BAD_ARG, entry, "n > CWN_MAX_DESCS");
    expect(fn(empty.data(), CWN_MAX_DESCS, nullptr), CWN_OK, entry, "eight empty descriptors");
}

template <class Desc, class real, class Fn> void forward(const char* entry, Fn fn) {
    const Desc good = good_fwd<Desc, real>();
    common<Desc, real>(entry, fn, good);
    auto one = [&](Desc d, int want, const char* what) { expect(fn(&d, 1, nullptr), want, entry, what); };
    const uintptr_t off = 20 * P + sizeof(real) / 2;
    Desc d;
    d = good; d.ia = nullptr; one(d, CWN_ERR_BAD_ARG, "ia NULL");
    d = good; d.ib = nullptr; one(d, CWN_ERR_BAD_ARG, "ib NULL");
    d = good; d.A = nullptr; one(d, CWN_ERR_BAD_ARG, "A NULL");
    d = good; d.B = nullptr; one(d, CWN_ERR_BAD_ARG, "B NULL");
    d = good; d.A = at<real>(off); one(d, CWN_ERR_ALIGN, "A misaligned");
    d = good; d.B = at<real>(off); one(d, CWN_ERR_ALIGN, "B misaligned");
    d = good; d.self_x = at<real>(off); one(d, CWN_ERR_ALIGN, "self_x misaligned");
    d = good; d.eps = at<real>(off); one(d, CWN_ERR_ALIGN, "eps misaligned");
    d = Desc{}; d.F = 8; d.act = CWN_ACT_ELU;
    one(d, CWN_OK, "an empty descriptor without pointers");
    d = good; d.n_dst = 0; d.rowptr = nullptr; d.ia = d.ib = nullptr; d.A = at<real>(0x30001); d.B = at<real>(0x30003);
    one(d, CWN_OK, "an absent adjacency does not look at the gathered operands");
}

template <class Desc, class real, class Fn> void backward(const char* entry, Fn fn) {
    const Desc good = good_bwd<Desc, real>();
    common<Desc, real>(entry, fn, good);
    auto one = [&](Desc d, int want, const char* what) { expect(fn(&d, 1, nullptr), want, entry, what); };
    const uintptr_t off = 20 * P + sizeof(real) / 2;
    Desc d;
    d = good; d.ig = nullptr; one(d, CWN_ERR_BAD_ARG, "ig NULL");
    d = good; d.iq = nullptr; one(d, CWN_ERR_BAD_ARG, "iq NULL");
    d = good; d.g = nullptr; one(d, CWN_ERR_BAD_ARG, "g NULL");
    d = good; d.P = nullptr; one(d, CWN_ERR_BAD_ARG, "P NULL");
    d = good; d.Q = nullptr; one(d, CWN_ERR_BAD_ARG, "Q NULL");
    d = good; d.g = at<real>(off); one(d, CWN_ERR_ALIGN, "g misaligned");
    d = good; d.P = at<real>(off); one(d, CWN_ERR_ALIGN, "P misaligned");
    d = good; d.Q = at<real>(off); one(d, CWN_ERR_ALIGN, "Q misaligned");
    d = Desc{}; d.F = 8; d.act = CWN_ACT_ELU;
    one(d, CWN_OK, "an empty descriptor without pointers");
    d = good; d.n_dst = 0; d.rowptr = nullptr; d.ig = d.iq = nullptr;
    d.g = at<real>(0x30001); d.P = at<real>(0x30003); d.Q = at<real>(0x30005);
    one(d, CWN_OK, "an absent plan does not look at the operands");
}

}  // namespace

int main() {
    forward<cwn_agg_act_desc, float>("cwn_aggregate_act_f32", cwn_aggregate_act_f32);
    forward<cwn_agg_act_desc_f64, double>("cwn_aggregate_act_f64", cwn_aggregate_act_f64);
    backward<cwn_agg_act_bwd_desc, float>("cwn_aggregate_act_bwd_f32", cwn_aggregate_act_bwd_f32);
    backward<cwn_agg_act_bwd_desc_f64, double>("cwn_aggregate_act_bwd_f64", cwn_aggregate_act_bwd_f64);
    printf(failures ? "%d checks failed\n" : "all checks passed\n", failures);
    return failures != 0;
}
