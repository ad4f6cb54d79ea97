// cwn_aggregate_f64.hip -- the float64 forms of cwn_aggregate.hip: fused gather -> message ->
// segmented reduce over destination-sorted CSR, and the plain row gather.  The strongly-regular-graph
// isomorphism experiments run in double precision (an untrained sum-aggregating network reaches 5e8
// and two isomorphic complexes must land within 0.01 of each other); gfx950 runs vector FP64 at the
// FP32 rate, so this is the same HBM-bound kernel with twice the bytes.
//
// The design is that of cwn_aggregate.hip (read its header first); what differs:
//   * a lane holds a 16-byte slice = TWO doubles (one when F is odd or a pointer is only 8-byte
//     aligned), so G = pow2 >= F / 2 capped at 64: F = 128 -> one row per wavefront, F = 16 (the SR
//     width) -> eight rows; wider rows take the chunk loop over G*VEC columns.
//   * rows with fewer than 8 feature lanes (F <= 14) get entry slots next to the feature lanes and
//     the entry-parallel fold above kSplitRow entries; every other row, and every row of at most
//     kSplitRow entries, is summed sequentially in CSR order: bit-identical to a sequential float64
//     index_add_.  Hub rows meet in LDS as doubles and are combined in chunk order.
//   * SMALL addressing is a 32-bit BYTE offset, so it needs rows * F * 8 < 2^32.
// A kernel of its own, not a template parameter of aggregate_kernel: that kernel's speed is decided
// by its register count and its instantiation names are pinned by the resource tests.
#include <hip/hip_runtime.h>
#include <float.h>
#include "../../include/cwn_hip.h"
#include "cwn_mem.h"

namespace {

constexpr int kThreads = 256;

struct AggBatch64 {
    cwn_agg_desc_f64 d[CWN_MAX_DESCS];
    int32_t blk_start[CWN_MAX_DESCS + 1];
    int32_t group[CWN_MAX_DESCS];  // lanes per destination row
    int32_t fgroup[CWN_MAX_DESCS]; // of which feature lanes (the rest are entry slots, narrow F only)
    int32_t n;
};

typedef double v2d __attribute__((ext_vector_type(2)));

template <int VEC> struct Acc { double v[VEC]; };

template <int VEC>
__device__ __forceinline__ Acc<VEC> ld(const double* p) {
    Acc<VEC> a;
    if constexpr (VEC == 2) {
        const v2d t = *reinterpret_cast<const v2d*>(p);
        a.v[0] = t.x; a.v[1] = t.y;
    } else {
        a.v[0] = *p;
    }
    return a;
}

// result rows are not read again by the launch that writes them: see cwn_mem.h
template <int VEC>
__device__ __forceinline__ void st(double* p, const Acc<VEC>& a) {
    if constexpr (VEC == 2) {
        const v2d v = {a.v[0], a.v[1]};
#if CWN_NT_STORE
        __builtin_nontemporal_store(v, reinterpret_cast<v2d*>(p));
#else
        *reinterpret_cast<v2d*>(p) = v;
#endif
    } else {
        *p = a.v[0];
    }
}

template <int VEC>
__device__ __forceinline__ Acc<VEC> splat(double x) {
    Acc<VEC> a;
#pragma unroll
    for (int k = 0; k < VEC; ++k) a.v[k] = x;
    return a;
}

// Address of columns f.. of row `idx` of a row-major [*, F] fp64 matrix.  SMALL (every operand of
// the launch lies within 4 GiB of its base pointer: CWN_AGG_SMALL_OPERANDS + the output size): a
// 32-bit byte offset on the scalar base -- the global_load saddr form, one address register per
// load in flight instead of two and no 64-bit multiply (quarter rate) per gathered row.
template <bool SMALL>
__device__ __forceinline__ const double* row_at(const double* base, int64_t idx, int F, int f) {
    if constexpr (SMALL) {
        const uint32_t off = ((uint32_t)idx * (uint32_t)F + (uint32_t)f) << 3;
        return reinterpret_cast<const double*>(reinterpret_cast<const char*>(base) + off);
    } else {
        return base + idx * F + f;
    }
}
template <bool SMALL>
__device__ __forceinline__ double* row_at(double* base, int64_t idx, int F, int f) {
    return const_cast<double*>(row_at<SMALL>(const_cast<const double*>(base), idx, F, f));
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
        else if constexpr (OP == CWN_MSG_RELU_A_PLUS_B) m.v[k] = fmax(a.v[k] + b.v[k], 0.0);
        else if constexpr (OP == CWN_MSG_RELU_A_PLUS_B_SQ) {
            const double r = fmax(a.v[k] + b.v[k], 0.0);
            m.v[k] = r * r;
        } else if constexpr (OP == CWN_MSG_A_TIMES_2RELU) m.v[k] = 2.0 * a.v[k] * fmax(pre.v[k] + b.v[k], 0.0);
        else m.v[k] = (pre.v[k] + b.v[k] > 0.0) ? a.v[k] : 0.0;
    }
    return m;
}

template <int VEC, int RED>
__device__ __forceinline__ void combine(Acc<VEC>& acc, const Acc<VEC>& m) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        if constexpr (RED == CWN_REDUCE_MAX) acc.v[k] = fmax(acc.v[k], m.v[k]);
        else acc.v[k] = acc.v[k] + m.v[k];
    }
}

// One group (G lanes, lane-in-group `gl`) folds CSR positions [start, end) of one destination
// row into a register accumulator, in CSR order.  Every lane of the group runs every loop with
// the same trip counts (the index fetch and the shuffles need all G lanes); lanes whose feature
// slice starts past F (`!active`) only skip the loads.
template <int VEC, int OP, int RED, bool SMALL>
__device__ __forceinline__ Acc<VEC> fold_range(const cwn_agg_desc_f64& D, int start, int end, int G, int gl,
                                               int f, bool active, const Acc<VEC>& pre) {
    constexpr bool kUsesB = (OP != CWN_MSG_A);
    const int F = D.F;
    const bool b_scalar = kUsesB && D.b_width == 1;
    Acc<VEC> acc = splat<VEC>(RED == CWN_REDUCE_MAX ? -DBL_MAX : 0.0);
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
                a[u] = splat<VEC>(0.0);
                b[u] = splat<VEC>(0.0);
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
            Acc<VEC> a = splat<VEC>(0.0), b = splat<VEC>(0.0);
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

// Narrow features (fewer than 8 feature lanes: F <= 14 with 16-B slices): the G lanes of a group are
// then S = G / GF entry slots x GF feature lanes, and for rows with more than kSplitRow entries
// every slot folds every S-th entry; the S partials are combined by a fixed xor tree.  Rows up to
// kSplitRow entries keep the sequential order (bit-identical to index_add_), like every row of
// wider features.
constexpr int kSplitRow = 16;

struct Operands {        // the descriptor fields a fold needs, by value (registers)
    const int32_t* ia;
    const int32_t* ib;
    const double* A;
    const double* B;
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
    Acc<VEC> acc = splat<VEC>(RED == CWN_REDUCE_MAX ? -DBL_MAX : 0.0);
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
                a[u] = splat<VEC>(0.0);
                b[u] = splat<VEC>(0.0);
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
// register count and load late, as in cwn_aggregate.hip.
template <int VEC> struct SelfTerms { Acc<VEC> s1, s2; };

template <int VEC, int OP, bool SMALL>
__device__ __forceinline__ SelfTerms<VEC> load_self_early(const cwn_agg_desc_f64& D, int64_t row, int f, bool active) {
    SelfTerms<VEC> t{splat<VEC>(0.0), splat<VEC>(0.0)};
    if constexpr (OP == CWN_MSG_A) {
        if (active && D.self_x != nullptr) t.s1 = ld<VEC>(row_at<SMALL>(D.self_x, row, D.F, f));
        if (active && D.self_x2 != nullptr) t.s2 = ld<VEC>(row_at<SMALL>(D.self_x2, row, D.F, f));
    }
    return t;
}

// mean / empty-max fix-up, self terms, one coalesced store of the row slice
template <int VEC, int OP, int RED, bool SMALL>
__device__ __forceinline__ void finish_row(const cwn_agg_desc_f64& D, int64_t row, int f, int len, double scale1,
                                           Acc<VEC> acc, const SelfTerms<VEC>& self) {
    const int F = D.F;
    if constexpr (RED == CWN_REDUCE_MEAN) {
        const double cntf = (double)max(len, 1);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] / cntf;
    }
    if constexpr (RED == CWN_REDUCE_MAX) {
        if (len == 0) acc = splat<VEC>(0.0);
    }
    if (D.self_x != nullptr) {
        const Acc<VEC> s1 = OP == CWN_MSG_A ? self.s1 : ld<VEC>(row_at<SMALL>(D.self_x, row, F, f));
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + scale1 * s1.v[k];
    }
    if (D.self_x2 != nullptr) {      // backward: the two GIN self terms of a cell, in one pass
        const double scale2 = 1.0 + (D.eps2 != nullptr ? *D.eps2 : 0.0);
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
__device__ __forceinline__ void run_desc(const cwn_agg_desc_f64& D, int blk, int nblk, int G, int GF, double* part) {
    const int F = D.F;
    const int R = kThreads / G;  // lane groups (= rows in flight) per workgroup
    const int gl = threadIdx.x & (G - 1);
    const int gq = threadIdx.x / G;
    const bool has_long = D.long_rows != nullptr && D.n_long != nullptr && D.rowptr != nullptr;
    const int64_t row = (int64_t)blk * R + gq;
    // destination rows that exist (include/cwn_hip.h, "device-side row counts"; D.n_dst is then the capacity)
    const int64_t n_dst = D.m_dev != nullptr ? *D.m_dev : D.n_dst;
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
    const double self_scale = 1.0 + (D.eps != nullptr ? D.eps[z] : 0.0);
    if (row < n_dst) {  // whole groups take the branch together (G divides 64)
        if (has_long && end - start > CWN_LONG_ROW) {
            // left to the whole-workgroup pass below
        } else if (GF < G && end - start > kSplitRow) {
            const int f = (gl % GF) * VEC;
            const bool active = f < F;
            Acc<VEC> pre = splat<VEC>(0.0);
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
                Acc<VEC> pre = splat<VEC>(0.0);
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
            Acc<VEC> pre = splat<VEC>(0.0);
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
__device__ __forceinline__ void run_desc_red(const cwn_agg_desc_f64& D, int blk, int nblk, int G, int GF, double* part) {
    switch (D.reduce) {
        case CWN_REDUCE_MEAN: run_desc<VEC, OP, CWN_REDUCE_MEAN, SMALL>(D, blk, nblk, G, GF, part); break;
        case CWN_REDUCE_MAX: run_desc<VEC, OP, CWN_REDUCE_MAX, SMALL>(D, blk, nblk, G, GF, part); break;
        default: run_desc<VEC, OP, CWN_REDUCE_ADD, SMALL>(D, blk, nblk, G, GF, part); break;
    }
}

// As in aggregate_kernel the gathers are latency-bound and registers decide the loads in flight.  A
// double2 slice costs the registers of a float4, but the accumulator, the self terms and every
// message temporary are twice as wide as their fp32 forms: the kernel is left to the compiler's own
// budget (no amdgpu_waves_per_eu), which builds without scratch.
// NARROW: some descriptor has fewer than 8 feature lanes; a separate instantiation so that the
// wide-feature kernel carries none of the entry-parallel code.
template <int VEC, bool NARROW, bool SMALL>
__global__ __launch_bounds__(kThreads)
void aggregate_f64_kernel(AggBatch64 B) {
    __shared__ double part[kThreads * VEC];
    int di = 0;
#pragma unroll
    for (int i = 1; i < CWN_MAX_DESCS; ++i)
        if (i < B.n && (int)blockIdx.x >= B.blk_start[i]) di = i;
    // By VALUE, not `const cwn_agg_desc_f64& D = B.d[di]`: cwn_aggregate.hip says what the reference form cost its
    // NARROW kernel (the whole batch struct in scratch).
    const cwn_agg_desc_f64 D = B.d[di];
    const int G = B.group[di], GF = NARROW ? B.fgroup[di] : G;
    const int blk = blockIdx.x - B.blk_start[di];
    const int nblk = B.blk_start[di + 1] - B.blk_start[di];
    switch (D.msg_op) {
        case CWN_MSG_A_PLUS_B: run_desc_red<VEC, CWN_MSG_A_PLUS_B, SMALL>(D, blk, nblk, G, GF, part); break;
        case CWN_MSG_A_TIMES_B: run_desc_red<VEC, CWN_MSG_A_TIMES_B, SMALL>(D, blk, nblk, G, GF, part); break;
        case CWN_MSG_RELU_A_PLUS_B:
            run_desc<VEC, CWN_MSG_RELU_A_PLUS_B, CWN_REDUCE_ADD, SMALL>(D, blk, nblk, G, GF, part); break;
        case CWN_MSG_A_MASK_RELU:
            run_desc<VEC, CWN_MSG_A_MASK_RELU, CWN_REDUCE_ADD, SMALL>(D, blk, nblk, G, GF, part); break;
        case CWN_MSG_RELU_A_PLUS_B_SQ:
            run_desc<VEC, CWN_MSG_RELU_A_PLUS_B_SQ, CWN_REDUCE_ADD, SMALL>(D, blk, nblk, G, GF, part); break;
        case CWN_MSG_A_TIMES_2RELU:
            run_desc<VEC, CWN_MSG_A_TIMES_2RELU, CWN_REDUCE_ADD, SMALL>(D, blk, nblk, G, GF, part); break;
        default: run_desc_red<VEC, CWN_MSG_A, SMALL>(D, blk, nblk, G, GF, part); break;
    }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void gather_rows_f64_kernel(const double* __restrict__ src,
                                                                   const int64_t* __restrict__ idx,
                                                                   double* __restrict__ out, int64_t n_idx,
                                                                   int F, int G) {
    const int rows_per_block = kThreads / G;
    const int gl = threadIdx.x & (G - 1);
    const int64_t e = (int64_t)blockIdx.x * rows_per_block + threadIdx.x / G;
    if (e >= n_idx) return;
    const int64_t r = idx[e];
    for (int f = gl * VEC; f < F; f += G * VEC) st<VEC>(out + e * F + f, ld<VEC>(src + r * F + f));
}

inline int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

inline int pick_group(int F, int vec) {
    int g = pow2_at_least((F + vec - 1) / vec);
    return g > 64 ? 64 : g;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

}  // namespace

extern "C" int cwn_aggregate_f64(const cwn_agg_desc_f64* descs, int n, cwn_stream_t stream_) {
    if (descs == nullptr || n <= 0 || n > CWN_MAX_DESCS) return CWN_ERR_BAD_ARG;
    AggBatch64 B{};
    B.n = n;
    int vec = 2;
    for (int i = 0; i < n; ++i) {
        const cwn_agg_desc_f64& D = descs[i];
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
        // widest vector every pointer and the row stride allow
        int v = (D.F % 2 == 0) ? 2 : 1;
        const void* ptrs[] = {D.A, D.b_width == D.F ? (const void*)D.B : nullptr, D.self_x,
                              D.self_pre, D.out, D.self_x2};
        for (const void* p : ptrs) {
            if (p == nullptr) continue;
            if (!aligned8(p)) return CWN_ERR_ALIGN;
            if (v == 2 && !aligned16(p)) v = 1;
        }
        const void* scalars[] = {D.b_width == 1 ? (const void*)D.B : nullptr, D.eps, D.eps2};
        for (const void* p : scalars)
            if (p != nullptr && !aligned8(p)) return CWN_ERR_ALIGN;
        if (v < vec) vec = v;
    }
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        B.d[i] = descs[i];
        B.fgroup[i] = pick_group(descs[i].F, vec);
        // narrow features (fewer than 8 feature lanes): at least two entry slots per row
        const bool few = (descs[i].F + vec - 1) / vec < 8;
        B.group[i] = B.fgroup[i] < 8 ? 8 : (few ? 2 * B.fgroup[i] : B.fgroup[i]);
        const int rows_per_block = kThreads / B.group[i];
        B.blk_start[i] = (int32_t)blocks;
        blocks += (descs[i].n_dst + rows_per_block - 1) / rows_per_block;
        if (blocks >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    }
    for (int i = n; i <= CWN_MAX_DESCS; ++i) B.blk_start[i] = (int32_t)blocks;
    if (blocks == 0) return CWN_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)blocks), block(kThreads);
    bool narrow = false, small = true;
    for (int i = 0; i < n; ++i) {
        narrow = narrow || B.fgroup[i] < B.group[i];
        // 32-bit byte offsets: the caller vouches for the gathered operands, the row-aligned ones
        // (out, self_x, self_x2, self_pre: [n_dst, F]) are checked here
        small = small && (descs[i].flags & CWN_AGG_SMALL_OPERANDS) != 0 &&
                (uint64_t)descs[i].n_dst * (uint64_t)descs[i].F * 8u < (1ull << 32);
    }
    auto launch = [&](auto kernel) { kernel<<<grid, block, 0, stream>>>(B); };
    const int variant = (vec == 2 ? 0 : 4) + (narrow ? 2 : 0) + (small ? 1 : 0);
    switch (variant) {
        case 0: launch(aggregate_f64_kernel<2, false, false>); break;
        case 1: launch(aggregate_f64_kernel<2, false, true>); break;
        case 2: launch(aggregate_f64_kernel<2, true, false>); break;
        case 3: launch(aggregate_f64_kernel<2, true, true>); break;
        case 4: launch(aggregate_f64_kernel<1, false, false>); break;
        case 5: launch(aggregate_f64_kernel<1, false, true>); break;
        case 6: launch(aggregate_f64_kernel<1, true, false>); break;
        default: launch(aggregate_f64_kernel<1, true, true>); break;
    }
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

extern "C" int cwn_gather_rows_f64(const double* src, int64_t n_src, int64_t F, const int64_t* idx,
                                   int64_t n_idx, double* out, cwn_stream_t stream_) {
    if (F <= 0 || n_idx < 0 || n_src < 0 || F >= INT32_MAX) return CWN_ERR_BAD_ARG;
    if (n_idx == 0) return CWN_OK;
    if (src == nullptr || idx == nullptr || out == nullptr) return CWN_ERR_BAD_ARG;
    if ((((uintptr_t)src) | ((uintptr_t)out)) & 7u) return CWN_ERR_ALIGN;
    int vec = (F % 2 == 0) ? 2 : 1;
    if (vec == 2 && !(aligned16(src) && aligned16(out))) vec = 1;
    const int G = pick_group((int)F, vec);
    const int rows_per_block = kThreads / G;
    const int64_t blocks = (n_idx + rows_per_block - 1) / rows_per_block;
    if (blocks >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)blocks), block(kThreads);
    if (vec == 2) gather_rows_f64_kernel<2><<<grid, block, 0, stream>>>(src, idx, out, n_idx, (int)F, G);
    else gather_rows_f64_kernel<1><<<grid, block, 0, stream>>>(src, idx, out, n_idx, (int)F, G);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}
