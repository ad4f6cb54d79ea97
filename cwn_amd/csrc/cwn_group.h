// cwn_group.h -- what every grouped launch shares, written once: one launch serves up to MAX descriptors, a workgroup finds
// the descriptor its block number belongs to in a table of MAX + 1 block starts (group_of; BlockFill builds the table on the
// host), and where the descriptor carries a device-side row count it reads that count in one of three ways (rows_*: the
// "DEVICE-SIDE ROW COUNTS" contract of include/cwn_hip.h).  Compiles with a plain host compiler too (tests/test_group_host.py).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define CWN_GROUP_FN __host__ __device__ __forceinline__
#define CWN_GROUP_UNROLL _Pragma("unroll")
#else
#define CWN_GROUP_FN inline
#define CWN_GROUP_UNROLL
#endif

namespace cwn {

// The descriptor of workgroup `block`: the last i < n with start[i] <= block (an empty descriptor shares its start with the
// next one and is never chosen).  A select chain over the whole bound, not a loop to n: the kernels unroll it into scalar
// compares of the kernel-argument table.
template <int MAX, typename T, typename B> CWN_GROUP_FN int group_of(const T* start, int n, B block) {
    int di = 0;
    CWN_GROUP_UNROLL
    for (int i = 1; i < MAX; ++i)
        if (i < n && block >= start[i]) di = i;
    return di;
}

// The rows of a batch that exist: `cap` (the host count, or the capacity of a static buffer) without a device count.
// `cap` is a reference so that a descriptor's field is read where the open-coded forms read it, in the branch without a
// count; a kernel that read its capacity FIRST passes a copy, (int64_t)P.C.  The check for every edit here, and for every new
// caller, is tools/isa_diff.sh on the caller's file: the device assembly does not change.  Where it did -- any helper in
// place of the same text, in gemm_kernel, gemm_tn_kernel, dense_stage_bwd_kernel, bn_finalize_kernel and
// norm_bwd_fused_kernel -- the kernel writes the expression out and names the helper it stands for.  (cwn_linear_stats.hip
// has not been moved to this header yet: its search, its clamp and its table fill are still its own.)
//
// rows_vouched: the device count as it is.  A store bounded by it relies on the collate guard: the step's collate kernel
// refuses a batch beyond the capacity before any of these kernels runs.
CWN_GROUP_FN int64_t rows_vouched(const int64_t* m_dev, const int64_t& cap) { return m_dev != nullptr ? *m_dev : cap; }

// rows_capped: never more than the capacity.  A store bounded by it stays inside the buffer whatever the count says; a
// negative count is no row at all only because the kernel's own loops run upwards from a row >= 0.
CWN_GROUP_FN int64_t rows_capped(const int64_t* m_dev, const int64_t& cap) {
    return m_dev != nullptr ? (*m_dev < cap ? *m_dev : cap) : cap;
}

// rows_clamped: in [0, cap].  A store bounded by it relies on nothing; for kernels that derive tile counts or divisors from
// the count, where a negative one would not simply bound an upward loop.
CWN_GROUP_FN int64_t rows_clamped(const int64_t* m_dev, const int64_t& cap) {
    if (m_dev == nullptr) return cap;
    const int64_t m = *m_dev;
    return m < 0 ? 0 : (m < cap ? m : cap);
}

// Host side: fills a block-start table of MAX + 1 entries.  push(i, nblk) gives descriptor i the next nblk workgroups and
// says whether the total still fits a grid (below INT32_MAX); close(n) writes the total behind the last descriptor, so that
// start[i + 1] - start[i] is descriptor i's count for every i < n, and returns it.
template <typename T, int N> struct BlockFill {     // N = MAX + 1, taken from the array: cwn::BlockFill fill(B.blk_start);
    T* start;
    int64_t total = 0;
    explicit BlockFill(T (&s)[N]) : start(s) {}
    bool push(int i, int64_t nblk) {
        start[i] = (T)total;
        total += nblk;
        return total < INT32_MAX;
    }
    int64_t close(int n) {
        for (int i = n; i < N; ++i) start[i] = (T)total;
        return total;
    }
};

}  // namespace cwn
