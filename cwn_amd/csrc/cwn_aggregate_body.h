// cwn_aggregate_body.h -- what the f32 and the f64 aggregate kernels share: the device code between
// the kernel's dispatch and the loads / stores (message forms, the folds of a row, self terms, hub
// rows through LDS) and the type-independent part of the host launchers.  One text, compiled once
// per element type: cwn_aggregate.hip and cwn_aggregate_f64.hip each define, ahead of the include,
//     using real = float | double;                  the element type
//     using desc_t = cwn_agg_desc | cwn_agg_desc_f64;   the descriptor (one layout, `real` pointers)
//     constexpr real kNegInf = -infinity of the type;   where a max fold starts: a row of -Inf messages gives -Inf, as amax does
// and, after it, the two functions that differ in more than the type: ld<VEC> / st<VEC> (declared
// below).  The kernels stay in their files under their own names: the f32 kernel's speed is decided
// by its register count and its instantiation names are pinned by tests/test_kernel_resources.py,
// so the device assembly of both files is held fixed across edits here (tools/isa_diff.sh).
// Aliases, not a template parameter, for that reason: nothing about a symbol's name changes.
#pragma once
#include "cwn_check.h"
#include "cwn_act.h"
#include "cwn_group.h"

namespace {

constexpr int kThreads = 256;

template <int VEC> struct Acc { real v[VEC]; };

// per file: the widest loads / stores of the type (float4 / float2 / float; double2 / double)
template <int VEC> __device__ __forceinline__ Acc<VEC> ld(const real* p);
template <int VEC> __device__ __forceinline__ void st(real* p, const Acc<VEC>& a);

template <int VEC>
__device__ __forceinline__ Acc<VEC> splat(real x) {
    Acc<VEC> a;
#pragma unroll
    for (int k = 0; k < VEC; ++k) a.v[k] = x;
    return a;
}

// Address of columns f.. of row `idx` of a row-major [*, F] matrix.  SMALL (every operand of
// the launch lies within 4 GiB of its base pointer: CWN_AGG_SMALL_OPERANDS + the output size): a
// 32-bit byte offset on the scalar base -- the global_load saddr form, one address register per
// load in flight instead of two and no 64-bit multiply (quarter rate) per gathered row.
template <bool SMALL>
__device__ __forceinline__ const real* row_at(const real* base, int64_t idx, int F, int f) {
    if constexpr (SMALL) {
        const uint32_t off = ((uint32_t)idx * (uint32_t)F + (uint32_t)f) * (uint32_t)sizeof(real);
        return reinterpret_cast<const real*>(reinterpret_cast<const char*>(base) + off);
    } else {
        return base + idx * F + f;
    }
}
template <bool SMALL>
__device__ __forceinline__ real* row_at(real* base, int64_t idx, int F, int f) {
    return const_cast<real*>(row_at<SMALL>(const_cast<const real*>(base), idx, F, f));
}

// message for one CSR position; `pre` is self_pre[i, f..] (mask form only)
template <int VEC, int OP>
__device__ __forceinline__ Acc<VEC> message(const Acc<VEC>& a, const Acc<VEC>& b, const Acc<VEC>& pre) {
    Acc<VEC> m;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        if constexpr (OP == CWN_MSG_A) m.v[k] = a.v[k];
        else if constexpr (OP == CWN_MSG_A_PLUS_B) m.v[k] = a.v[k] + b.v[k];
        else if constexpr (OP == CWN_MSG_A_TIMES_B) m.v[k] = a.v[k] * b.v[k];
        else if constexpr (OP == CWN_MSG_RELU_A_PLUS_B) m.v[k] = cwn_relu(a.v[k] + b.v[k]);
        else if constexpr (OP == CWN_MSG_RELU_A_PLUS_B_SQ) {
            const real r = cwn_relu(a.v[k] + b.v[k]);
            m.v[k] = r * r;
        } else if constexpr (OP == CWN_MSG_A_TIMES_2RELU) m.v[k] = real(2.0) * a.v[k] * cwn_relu(pre.v[k] + b.v[k]);
        else m.v[k] = cwn_relu_bwd(pre.v[k] + b.v[k], a.v[k]);
    }
    return m;
}

template <int VEC, int RED>
__device__ __forceinline__ void combine(Acc<VEC>& acc, const Acc<VEC>& m) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        if constexpr (RED == CWN_REDUCE_MAX) acc.v[k] = cwn_max(acc.v[k], m.v[k]);
        else acc.v[k] = acc.v[k] + m.v[k];
    }
}

// One group (G lanes, lane-in-group `gl`) folds CSR positions [start, end) of one destination
// row into a register accumulator, in CSR order.  Every lane of the group runs every loop with
// the same trip counts (the index fetch and the shuffles need all G lanes); lanes whose feature
// slice starts past F (`!active`) only skip the loads.
template <int VEC, int OP, int RED, bool SMALL>
__device__ __forceinline__ Acc<VEC> fold_range(const desc_t& D, int start, int end, int G, int gl,
                                               int f, bool active, const Acc<VEC>& pre) {
    constexpr bool kUsesB = (OP != CWN_MSG_A);
    const int F = D.F;
    const bool b_scalar = kUsesB && D.b_width == 1;
    Acc<VEC> acc = splat<VEC>(RED == CWN_REDUCE_MAX ? kNegInf : real(0.0));
    for (int base = start; base < end; base += G) {
        // cooperative index fetch: lane gl holds the indices of CSR position base+gl
        const int mine = base + gl;
        int my_ia = 0, my_ib = 0;
        if (mine < end) {
            my_ia = D.ia[mine];
            if constexpr (kUsesB) my_ib = D.ib[mine];
        }
        const int cnt = min(G, end - base);
        int t = 0;
        for (; t + 4 <= cnt; t += 4) {
            Acc<VEC> a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ia = __shfl(my_ia, t + u, G);
                int ib = 0;
                if constexpr (kUsesB) ib = __shfl(my_ib, t + u, G);
                a[u] = splat<VEC>(real(0.0));
                b[u] = splat<VEC>(real(0.0));
                if (active) {
                    a[u] = ld<VEC>(row_at<SMALL>(D.A, ia, F, f));
                    if constexpr (kUsesB)
                        b[u] = b_scalar ? splat<VEC>(*row_at<SMALL>(D.B, ib, 1, 0))
                                        : ld<VEC>(row_at<SMALL>(D.B, ib, F, f));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) combine<VEC, RED>(acc, message<VEC, OP>(a[u], b[u], pre));
        }
        for (; t < cnt; ++t) {
            const int ia = __shfl(my_ia, t, G);
            int ib = 0;
            if constexpr (kUsesB) ib = __shfl(my_ib, t, G);
            Acc<VEC> a = splat<VEC>(real(0.0)), b = splat<VEC>(real(0.0));
            if (active) {
                a = ld<VEC>(row_at<SMALL>(D.A, ia, F, f));
                if constexpr (kUsesB)
                    b = b_scalar ? splat<VEC>(*row_at<SMALL>(D.B, ib, 1, 0)) : ld<VEC>(row_at<SMALL>(D.B, ib, F, f));
            }
            combine<VEC, RED>(acc, message<VEC, OP>(a, b, pre));
        }
    }
    return acc;
}

// Narrow features (fewer than 8 feature lanes: F <= 16 in fp32, F <= 14 in fp64; REDDIT-like inputs
// have ONE scalar feature per vertex): the G lanes of a group are then S = G / GF entry slots x GF
// feature lanes, and for rows with more than kSplitRow entries every slot folds every S-th entry;
// the S partials are combined by a fixed xor tree.  One lane walking a 60-entry row alone is 15
// dependent round trips (the F = 1 layer of the REDDIT-like configuration took 30 us, longer than
// its F = 64 layers).  Rows up to kSplitRow entries keep the sequential order (bit-identical to
// index_add_), like every row of wide layers.
constexpr int kSplitRow = 16;

struct Operands {        // the descriptor fields a fold needs, by value (registers)
    const int32_t* ia;
    const int32_t* ib;
    const real* A;
    const real* B;
    int F, b_width;
};

template <int VEC, int OP, int RED, bool SMALL>
__device__ __forceinline__ Acc<VEC> fold_range_split(const Operands D, int start, int end, int G, int GF,
                                                     int gl, const Acc<VEC>& pre) {
    constexpr bool kUsesB = (OP != CWN_MSG_A);
    const int F = D.F;
    const bool b_scalar = kUsesB && D.b_width == 1;
    const int S = G / GF, e = gl / GF, f = (gl % GF) * VEC;
    const bool active = f < F;
    Acc<VEC> acc = splat<VEC>(RED == CWN_REDUCE_MAX ? kNegInf : real(0.0));
    for (int base = start; base < end; base += G) {
        const int mine = base + gl;
        int my_ia = 0, my_ib = 0;
        if (mine < end) {
            my_ia = D.ia[mine];
            if constexpr (kUsesB) my_ib = D.ib[mine];
        }
        const int cnt = min(G, end - base);
        for (int tb = 0; tb < cnt; tb += 2 * S) {          // uniform trip count over the group
            Acc<VEC> a[2], b[2];
            bool ok[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = tb + u * S + e;
                ok[u] = t < cnt;
                const int ia = __shfl(my_ia, ok[u] ? t : 0, G);
                int ib = 0;
                if constexpr (kUsesB) ib = __shfl(my_ib, ok[u] ? t : 0, G);
                a[u] = splat<VEC>(real(0.0));
                b[u] = splat<VEC>(real(0.0));
                if (active && ok[u]) {
                    a[u] = ld<VEC>(row_at<SMALL>(D.A, ia, F, f));
                    if constexpr (kUsesB)
                        b[u] = b_scalar ? splat<VEC>(*row_at<SMALL>(D.B, ib, 1, 0))
                                        : ld<VEC>(row_at<SMALL>(D.B, ib, F, f));
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (ok[u]) combine<VEC, RED>(acc, message<VEC, OP>(a[u], b[u], pre));
        }
    }
    for (int off = GF; off < G; off <<= 1) {               // entry slots -> slot 0, fixed tree
        Acc<VEC> o;
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = __shfl_xor(acc.v[k], off, G);
        combine<VEC, RED>(acc, o);
    }
    return acc;
}

// The self terms of a row slice ((1 + eps) x_i; in backward the two GIN self terms of a cell).  For
// the one-operand message they are loaded BEFORE the fold, next to the row pointers they do not
// depend on: fetched at the end they are a fourth dependent round trip (row pointers -> indices ->
// rows -> self) of a lane group that lives for one row.  The two-operand messages set the kernel's
// register count (fp32: 72 = 7 waves per SIMD, see aggregate_kernel) and have no room for 8 more
// live registers: they load late.
template <int VEC> struct SelfTerms { Acc<VEC> s1, s2; };

template <int VEC, int OP, bool SMALL>
__device__ __forceinline__ SelfTerms<VEC> load_self_early(const desc_t& D, int64_t row, int f, bool active) {
    SelfTerms<VEC> t{splat<VEC>(real(0.0)), splat<VEC>(real(0.0))};
    if constexpr (OP == CWN_MSG_A) {
        if (active && D.self_x != nullptr) t.s1 = ld<VEC>(row_at<SMALL>(D.self_x, row, D.F, f));
        if (active && D.self_x2 != nullptr) t.s2 = ld<VEC>(row_at<SMALL>(D.self_x2, row, D.F, f));
    }
    return t;
}

// mean / empty-max fix-up, self terms, one coalesced store of the row slice
template <int VEC, int OP, int RED, bool SMALL>
__device__ __forceinline__ void finish_row(const desc_t& D, int64_t row, int f, int len, real scale1,
                                           Acc<VEC> acc, const SelfTerms<VEC>& self) {
    const int F = D.F;
    if constexpr (RED == CWN_REDUCE_MEAN) {
        const real cntf = (real)max(len, 1);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] / cntf;
    }
    if constexpr (RED == CWN_REDUCE_MAX) {
        if (len == 0) acc = splat<VEC>(real(0.0));
    }
    if (D.self_x != nullptr) {
        const Acc<VEC> s1 = OP == CWN_MSG_A ? self.s1 : ld<VEC>(row_at<SMALL>(D.self_x, row, F, f));
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + scale1 * s1.v[k];
    }
    if (D.self_x2 != nullptr) {      // backward: the two GIN self terms of a cell, in one pass
        const real scale2 = real(1.0) + (D.eps2 != nullptr ? *D.eps2 : real(0.0));
        const Acc<VEC> s2 = OP == CWN_MSG_A ? self.s2 : ld<VEC>(row_at<SMALL>(D.self_x2, row, F, f));
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + scale2 * s2.v[k];
    }
    st<VEC>(row_at<SMALL>(D.out, row, F, f), acc);
}

// Workgroup `blk` of the `nblk` that serve descriptor D.
//   1. every lane group reduces its own destination row, sequentially in CSR (= original entry)
//      order: bit-identical to a sequential index_add_;
//   2. rows with more than CWN_LONG_ROW entries (hub cells of REDDIT-like complexes; listed by
//      cwn_csr_build) are skipped in 1 and taken round-robin by whole workgroups here: the R lane
//      groups of the block fold R contiguous chunks of the row, the partials meet in LDS and are
//      combined in chunk order -- deterministic, no atomics, and the kernel no longer waits for
//      one lane group to walk a 300-entry row alone.
template <int VEC, int OP, int RED, bool SMALL>
__device__ __forceinline__ void run_desc(const desc_t& D, int blk, int nblk, int G, int GF, real* part) {
    const int F = D.F;
    const int R = kThreads / G;  // lane groups (= rows in flight) per workgroup
    const int gl = threadIdx.x & (G - 1);
    const int gq = threadIdx.x / G;
    const bool has_long = D.long_rows != nullptr && D.n_long != nullptr && D.rowptr != nullptr;
    const int64_t row = (int64_t)blk * R + gq;
    // destination rows that exist (include/cwn_hip.h, "device-side row counts"; D.n_dst is then the capacity)
    const int64_t n_dst = cwn::rows_vouched(D.m_dev, D.n_dst);
    int start = 0, end = 0;
    if (row < n_dst && D.rowptr != nullptr) {
        start = D.rowptr[row];
        end = D.rowptr[row + 1];
    }
    // The long-row counters are only needed after the regular rows, eps at the end of a row.
    // Loaded here as VECTOR loads (per-lane address) issued AFTER the row pointers: vector loads
    // return in order, so waiting for the row pointers does not wait for these, whereas a scalar
    // load joins the kernel-argument loads in the one out-of-order scalar counter and puts a global
    // round trip (~0.5-1 us) in front of every workgroup's first row.
    const int nl_lane = has_long ? D.n_long[threadIdx.x & (CWN_LONG_PARTS - 1)] : 0;
    int z = 0;
    asm volatile("" : "+v"(z));  // a zero the compiler cannot fold: keeps the eps loads in VMEM
    const real self_scale = real(1.0) + (D.eps != nullptr ? D.eps[z] : real(0.0));
    if (row < n_dst) {  // whole groups take the branch together (G divides 64)
        if (has_long && end - start > CWN_LONG_ROW) {
            // left to the whole-workgroup pass below
        } else if (GF < G && end - start > kSplitRow) {
            const int f = (gl % GF) * VEC;
            const bool active = f < F;
            Acc<VEC> pre = splat<VEC>(real(0.0));
            if constexpr (OP == CWN_MSG_A_MASK_RELU || OP == CWN_MSG_A_TIMES_2RELU) {
                if (active) pre = ld<VEC>(row_at<SMALL>(D.self_pre, row, F, f));
            }
            const SelfTerms<VEC> self = load_self_early<VEC, OP, SMALL>(D, row, f, active && gl < GF);
            const Operands ops{D.ia, D.ib, D.A, D.B, D.F, D.b_width};
            const Acc<VEC> acc = fold_range_split<VEC, OP, RED, SMALL>(ops, start, end, G, GF, gl, pre);
            if (active && gl < GF)
                finish_row<VEC, OP, RED, SMALL>(D, row, f, end - start, self_scale, acc, self);
        } else {
            // feature chunks of G*VEC columns (one chunk when F <= G*VEC, the common case)
            for (int f0 = 0; f0 < F; f0 += G * VEC) {
                const int f = f0 + gl * VEC;
                const bool active = f < F;
                Acc<VEC> pre = splat<VEC>(real(0.0));
                if constexpr (OP == CWN_MSG_A_MASK_RELU || OP == CWN_MSG_A_TIMES_2RELU) {
                    if (active) pre = ld<VEC>(row_at<SMALL>(D.self_pre, row, F, f));
                }
                const SelfTerms<VEC> self = load_self_early<VEC, OP, SMALL>(D, row, f, active);
                const Acc<VEC> acc = fold_range<VEC, OP, RED, SMALL>(D, start, end, G, gl, f, active, pre);
                if (active) finish_row<VEC, OP, RED, SMALL>(D, row, f, end - start, self_scale, acc, self);
            }
        }
    }
    int n_long = 0, nl[CWN_LONG_PARTS];
#pragma unroll
    for (int p = 0; p < CWN_LONG_PARTS; ++p) {
        nl[p] = __builtin_amdgcn_readlane(nl_lane, p);
        n_long += nl[p];
    }
    for (int li = blk; li < n_long; li += nblk) {  // uniform over the workgroup
        int p = 0, k = li;
#pragma unroll
        for (int q = 0; q < CWN_LONG_PARTS - 1; ++q)     // li-th entry of the concatenated sub-lists
            if (p == q && k >= nl[q]) { k -= nl[q]; ++p; }
        const int64_t lrow = D.long_rows[(int64_t)p * D.long_cap + k];
        const int start = D.rowptr[lrow], end = D.rowptr[lrow + 1];
        const int chunk = (((end - start + R - 1) / R) + 3) & ~3;
        const int s = min(end, start + gq * chunk), e = min(end, s + chunk);
        for (int f0 = 0; f0 < F; f0 += G * VEC) {
            const int f = f0 + gl * VEC;
            const bool active = f < F;
            Acc<VEC> pre = splat<VEC>(real(0.0));
            if constexpr (OP == CWN_MSG_A_MASK_RELU || OP == CWN_MSG_A_TIMES_2RELU) {
                if (active) pre = ld<VEC>(row_at<SMALL>(D.self_pre, lrow, F, f));
            }
            Acc<VEC> acc = fold_range<VEC, OP, RED, SMALL>(D, s, e, G, gl, f, active, pre);
            if (gq != 0) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) part[threadIdx.x * VEC + k] = acc.v[k];
            }
            __syncthreads();
            if (gq == 0 && active) {
                for (int q = 1; q < R; ++q) {
                    Acc<VEC> m;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) m.v[k] = part[(q * G + gl) * VEC + k];
                    combine<VEC, RED>(acc, m);
                }
                const SelfTerms<VEC> self = load_self_early<VEC, OP, SMALL>(D, lrow, f, true);
                finish_row<VEC, OP, RED, SMALL>(D, lrow, f, end - start, self_scale, acc, self);
            }
            __syncthreads();
        }
    }
}

template <int VEC, int OP, bool SMALL>
__device__ __forceinline__ void run_desc_red(const desc_t& D, int blk, int nblk, int G, int GF, real* part) {
    switch (D.reduce) {
        case CWN_REDUCE_MEAN: run_desc<VEC, OP, CWN_REDUCE_MEAN, SMALL>(D, blk, nblk, G, GF, part); break;
        case CWN_REDUCE_MAX: run_desc<VEC, OP, CWN_REDUCE_MAX, SMALL>(D, blk, nblk, G, GF, part); break;
        default: run_desc<VEC, OP, CWN_REDUCE_ADD, SMALL>(D, blk, nblk, G, GF, part); break;
    }
}

// ---- host: what the two launchers decide alike.  The widest vector, the alignment rules and the
// lanes per row (B.group / B.fgroup) differ with the element type and stay in the .hip files. ----

inline int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

inline int pick_group(int F, int vec) {
    int g = pow2_at_least((F + vec - 1) / vec);
    return g > 64 ? 64 : g;
}

// CWN_OK, or why a descriptor is refused whatever its element type
inline int check_desc(const desc_t& D) {
    if (D.F <= 0 || D.n_dst < 0 || (D.n_dst > 0 && D.out == nullptr)) return CWN_ERR_BAD_ARG;
    if (D.msg_op < CWN_MSG_A || D.msg_op > CWN_MSG_A_TIMES_2RELU) return CWN_ERR_BAD_ARG;
    if (D.reduce < CWN_REDUCE_ADD || D.reduce > CWN_REDUCE_MAX) return CWN_ERR_BAD_ARG;
    if (D.msg_op >= CWN_MSG_RELU_A_PLUS_B && D.reduce != CWN_REDUCE_ADD) return CWN_ERR_BAD_ARG;
    if (D.rowptr != nullptr) {
        if (D.ia == nullptr || D.A == nullptr) return CWN_ERR_BAD_ARG;
        if (D.msg_op != CWN_MSG_A && (D.ib == nullptr || D.B == nullptr)) return CWN_ERR_BAD_ARG;
        if (D.msg_op != CWN_MSG_A && D.b_width != D.F && D.b_width != 1) return CWN_ERR_BAD_ARG;
        if ((D.msg_op == CWN_MSG_A_MASK_RELU || D.msg_op == CWN_MSG_A_TIMES_2RELU) && D.self_pre == nullptr) return CWN_ERR_BAD_ARG;
    }
    if (D.n_dst >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    return CWN_OK;
}

// NARROW kernel: some descriptor's rows have entry slots next to their feature lanes
template <class Batch>
bool any_narrow(const Batch& B) {
    bool narrow = false;
    for (int i = 0; i < B.n; ++i) narrow = narrow || B.fgroup[i] < B.group[i];
    return narrow;
}

// SMALL kernel (32-bit byte offsets): the caller vouches for the gathered operands, the row-aligned
// ones (out, self_x, self_x2, self_pre: [n_dst, F]) are checked here
template <class Batch>
bool all_small(const Batch& B) {
    bool small = true;
    for (int i = 0; i < B.n; ++i)
        small = small && (B.d[i].flags & CWN_AGG_SMALL_OPERANDS) != 0 &&
                (uint64_t)B.d[i].n_dst * (uint64_t)B.d[i].F * sizeof(real) < (1ull << 32);
    return small;
}

}  // namespace
