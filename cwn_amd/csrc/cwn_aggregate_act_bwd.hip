// cwn_aggregate_act_bwd.hip -- the backward of the activated coboundary message (cwn_aggregate_act.hip) as one launch,
// float32 and float64.  Over a TRANSPOSED plan, whose rows are the cells of the operand being differentiated:
//
//     out[r, :] = sum over p in row r, in CSR order, of  g[ig[p], :] * act'( P[r, :] + Q[iq[p], :] )
//
// P is the operand whose gradient this is (its own row r), Q the other operand gathered per entry, g the gradient of the
// stream's output gathered through the destination index, act one of the five CWN_ACT_* codes.  It is the shape of the ReLU
// stream's backward descriptor (CWN_MSG_A_MASK_RELU of cwn_aggregate_f32 / _f64: A = g, B, self_pre) with act' in place of
// the mask; that kernel's device code is held fixed (cwn_aggregate_body.h), hence entry points and a descriptor of their
// own, next to the forward's and in its style.  No self term: in this stream both operands are product outputs, and the
// (1 + eps) g and sum(g * x) parts of the gradient keep the code they have.
//
// Arithmetic: the pre-activation is recomputed as ONE add in the element type, P + Q, as the forward computes A + B (the
// add commutes: the same bits whichever operand is P); the activation's output, where act' needs it, is activate<ACT> of
// cwn_act.h, so it has the forward's bits; g * act' is activate_bwd<ACT> (torch's backward formulas; ReLU is a select).
// Product and accumulate are SEPARATE: acc = acc + (g * act'), a rounded multiply and a rounded add, never one fma -- on
// every path (the library is built with -ffp-contract=off).  With act = relu / id a row's sum is therefore the sum
// CWN_MSG_A_MASK_RELU / CWN_MSG_A computes for it.
//
// The mapping is that of cwn_aggregate_act.hip (read its header first): a GROUP of G lanes owns a row, a lane holds a
// 16-byte slice of the feature row (8 bytes or one element where width or alignment ask for it), the group fetches a
// segment's indices cooperatively and broadcasts them with __shfl, four gathered row PAIRS (g, Q) are in flight before the
// first multiply-add, rows are addressed with 32-bit byte offsets when every operand of the launch lies within 4 GiB of its
// base (row_at<SMALL>).  The vector width, the lanes per row and the entry slots are chosen PER DESCRIPTOR and dispatched
// inside the kernel, so a row's bits depend on its entries, F and its own operands -- not on the other descriptors.
// Sums: rows of at most CWN_LONG_ROW entries are folded sequentially in CSR order by one lane group (with fewer than 8
// feature lanes, rows above kSplitRow entries by the group's entry slots and a fixed xor tree); longer rows, from the
// long-row lists of cwn_csr_build, by a whole workgroup in contiguous chunks combined in chunk order through LDS.  Rows
// wider than one pass of the group are folded in feature chunks.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_act.h"
#include "cwn_check.h"
#include "cwn_mem.h"
#include "cwn_group.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSplitRow = 16;      // as in cwn_aggregate_act.hip: longer rows of narrow descriptors take the entry slots

template <class real> struct DescOf;
template <> struct DescOf<float> { using type = cwn_agg_act_bwd_desc; };
template <> struct DescOf<double> { using type = cwn_agg_act_bwd_desc_f64; };

template <class real>
struct BwdBatch {
    typename DescOf<real>::type d[CWN_MAX_DESCS];
    int32_t blk_start[CWN_MAX_DESCS + 1];
    int32_t group[CWN_MAX_DESCS];   // lanes per row
    int32_t fgroup[CWN_MAX_DESCS];  // of which feature lanes (the rest are entry slots, narrow F only)
    int32_t vec[CWN_MAX_DESCS];     // elements per lane
    int32_t n;
};

template <class real, int VEC> struct Acc { real v[VEC]; };

typedef double v2d __attribute__((ext_vector_type(2)));

template <int VEC>
__device__ __forceinline__ Acc<float, VEC> ld(const float* p) {
    Acc<float, VEC> a;
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        a.v[0] = t.x; a.v[1] = t.y; a.v[2] = t.z; a.v[3] = t.w;
    } else if constexpr (VEC == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        a.v[0] = t.x; a.v[1] = t.y;
    } else {
        a.v[0] = *p;
    }
    return a;
}

template <int VEC>
__device__ __forceinline__ Acc<double, VEC> ld(const double* p) {
    Acc<double, VEC> a;
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
__device__ __forceinline__ void st(float* p, const Acc<float, VEC>& a) {
    if constexpr (VEC == 4) {
        cwn::store_result4(p, a.v[0], a.v[1], a.v[2], a.v[3]);
    } else if constexpr (VEC == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(a.v[0], a.v[1]);
    } else {
        *p = a.v[0];
    }
}

template <int VEC>
__device__ __forceinline__ void st(double* p, const Acc<double, VEC>& a) {
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

template <class real, int VEC>
__device__ __forceinline__ Acc<real, VEC> splat(real x) {
    Acc<real, VEC> a;
#pragma unroll
    for (int k = 0; k < VEC; ++k) a.v[k] = x;
    return a;
}

// columns f.. of row `idx` of a row-major [*, F] matrix; SMALL: a 32-bit byte offset on the scalar base
template <bool SMALL, class real>
__device__ __forceinline__ const real* row_at(const real* base, int64_t idx, int F, int f) {
    if constexpr (SMALL) {
        const uint32_t off = ((uint32_t)idx * (uint32_t)F + (uint32_t)f) * (uint32_t)sizeof(real);
        return reinterpret_cast<const real*>(reinterpret_cast<const char*>(base) + off);
    } else {
        return base + idx * F + f;
    }
}
template <bool SMALL, class real>
__device__ __forceinline__ real* row_at(real* base, int64_t idx, int F, int f) {
    return const_cast<real*>(row_at<SMALL>(const_cast<const real*>(base), idx, F, f));
}

// acc += g * act'(p + q): one add for the pre-activation, a rounded product, a rounded add
template <class real, int VEC, int ACT>
__device__ __forceinline__ void add_grad(Acc<real, VEC>& acc, const Acc<real, VEC>& g, const Acc<real, VEC>& p,
                                         const Acc<real, VEC>& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + activate_bwd<ACT>(p.v[k] + q.v[k], g.v[k]);
}

template <class real>
struct Operands {        // the descriptor fields a fold needs, by value (registers)
    const int32_t* ig;
    const int32_t* iq;
    const real* g;
    const real* Q;
    int F;
};

// One group (G lanes, lane-in-group `gl`) folds CSR positions [start, end) of one row into a register accumulator, in CSR
// order; `p` is the lane's slice of the row's own operand.  Every lane of the group runs every loop with the same trip
// counts (the index fetch and the shuffles need all G lanes); lanes whose feature slice starts past F (`!active`) only
// skip the loads.
template <class real, int VEC, int ACT, bool SMALL>
__device__ __forceinline__ Acc<real, VEC> fold_range(const Operands<real> D, const Acc<real, VEC> p, int start, int end, int G,
                                                     int gl, int f, bool active) {
    const int F = D.F;
    Acc<real, VEC> acc = splat<real, VEC>(real(0.0));
    for (int base = start; base < end; base += G) {
        // cooperative index fetch: lane gl holds the indices of CSR position base+gl
        const int mine = base + gl;
        int my_ig = 0, my_iq = 0;
        if (mine < end) {
            my_ig = D.ig[mine];
            my_iq = D.iq[mine];
        }
        const int cnt = min(G, end - base);
        int t = 0;
        for (; t + 4 <= cnt; t += 4) {
            Acc<real, VEC> g[4], q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ig = __shfl(my_ig, t + u, G);
                const int iq = __shfl(my_iq, t + u, G);
                g[u] = splat<real, VEC>(real(0.0));
                q[u] = splat<real, VEC>(real(0.0));
                if (active) {
                    g[u] = ld<VEC>(row_at<SMALL>(D.g, ig, F, f));
                    q[u] = ld<VEC>(row_at<SMALL>(D.Q, iq, F, f));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) add_grad<real, VEC, ACT>(acc, g[u], p, q[u]);
        }
        for (; t < cnt; ++t) {
            const int ig = __shfl(my_ig, t, G);
            const int iq = __shfl(my_iq, t, G);
            Acc<real, VEC> g = splat<real, VEC>(real(0.0)), q = splat<real, VEC>(real(0.0));
            if (active) {
                g = ld<VEC>(row_at<SMALL>(D.g, ig, F, f));
                q = ld<VEC>(row_at<SMALL>(D.Q, iq, F, f));
            }
            add_grad<real, VEC, ACT>(acc, g, p, q);
        }
    }
    return acc;
}

// Fewer than 8 feature lanes: the G lanes of a group are S = G / GF entry slots x GF feature lanes, every slot folds every
// S-th entry of a row above kSplitRow entries and the S partials are combined by a fixed xor tree (cwn_aggregate_act.hip,
// fold_range_split).
template <class real, int VEC, int ACT, bool SMALL>
__device__ __forceinline__ Acc<real, VEC> fold_range_split(const Operands<real> D, const Acc<real, VEC> p, int start, int end,
                                                           int G, int GF, int gl) {
    const int F = D.F;
    const int S = G / GF, e = gl / GF, f = (gl % GF) * VEC;
    const bool active = f < F;
    Acc<real, VEC> acc = splat<real, VEC>(real(0.0));
    for (int base = start; base < end; base += G) {
        const int mine = base + gl;
        int my_ig = 0, my_iq = 0;
        if (mine < end) {
            my_ig = D.ig[mine];
            my_iq = D.iq[mine];
        }
        const int cnt = min(G, end - base);
        for (int tb = 0; tb < cnt; tb += 2 * S) {          // uniform trip count over the group
            Acc<real, VEC> g[2], q[2];
            bool ok[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = tb + u * S + e;
                ok[u] = t < cnt;
                const int ig = __shfl(my_ig, ok[u] ? t : 0, G);
                const int iq = __shfl(my_iq, ok[u] ? t : 0, G);
                g[u] = splat<real, VEC>(real(0.0));
                q[u] = splat<real, VEC>(real(0.0));
                if (active && ok[u]) {
                    g[u] = ld<VEC>(row_at<SMALL>(D.g, ig, F, f));
                    q[u] = ld<VEC>(row_at<SMALL>(D.Q, iq, F, f));
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (ok[u]) add_grad<real, VEC, ACT>(acc, g[u], p, q[u]);
        }
    }
    for (int off = GF; off < G; off <<= 1) {               // entry slots -> slot 0, fixed tree
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + __shfl_xor(acc.v[k], off, G);
    }
    return acc;
}

// the lane's slice of the row's own operand (zeros for a lane past F: its sums are never stored)
template <class real, int VEC, bool SMALL>
__device__ __forceinline__ Acc<real, VEC> own_slice(const real* P, int F, int64_t row, int f, bool active) {
    Acc<real, VEC> p = splat<real, VEC>(real(0.0));
    if (active) p = ld<VEC>(row_at<SMALL>(P, row, F, f));
    return p;
}

// What a lane knows about its row before the fold, computed once per kernel ahead of the dispatch on (vector width,
// activation): whatever is common to the forms is computed here, once, so that none of its scalar conditions is live across
// the dispatch (cwn_aggregate_act.hip, RowCtx).
struct RowCtx {
    int G, GF, R;        // lanes per row, of which feature lanes; rows per workgroup
    int gl, gq;          // lane in group, group in workgroup
    int64_t row;
    int start, end;      // the row's CSR positions (0, 0: no row, or no plan)
    int nl_lane;         // n_long[lane & 7], or 0 without long-row lists
    bool has_row, has_long;
    // what only the long-row pass reads, held in VECTOR registers while the rows are folded (uniform values; the pass takes
    // them back with readfirstlane)
    int blk_v, nblk_v, long_cap_v;
    const int32_t* long_rows_v;
    const int32_t* rowptr_v;
};

// Every lane group reduces its own row; then the workgroups share the rows of the long-row lists round-robin.  A row
// without entries, and every row of an absent plan, gets zeros.
template <class real, int VEC, int ACT, bool SMALL>
__device__ __forceinline__ void run_desc(const typename DescOf<real>::type& D, const RowCtx& c, real* part) {
    const int F = D.F;
    const int G = c.G, GF = c.GF, R = c.R, gl = c.gl, gq = c.gq;
    const int start = c.start, end = c.end;
    const Operands<real> ops{D.ig, D.iq, D.g, D.Q, D.F};
    if (c.has_row) {  // whole groups take the branch together (G divides 64)
        if (c.has_long && end - start > CWN_LONG_ROW) {
            // left to the whole-workgroup pass below
        } else if (GF < G && end - start > kSplitRow) {
            const int f = (gl % GF) * VEC;
            const Acc<real, VEC> p = own_slice<real, VEC, SMALL>(D.P, F, c.row, f, f < F);
            const Acc<real, VEC> acc = fold_range_split<real, VEC, ACT, SMALL>(ops, p, start, end, G, GF, gl);
            if (f < F && gl < GF) st<VEC>(row_at<SMALL>(D.out, c.row, F, f), acc);
        } else {
            // feature chunks of G*VEC columns (one chunk when F <= G*VEC, the common case)
            for (int f0 = 0; f0 < F; f0 += G * VEC) {
                const int f = f0 + gl * VEC;
                const bool active = f < F;
                // (a row without entries reads nothing: its P row may not exist when the plan is absent)
                const Acc<real, VEC> p = own_slice<real, VEC, SMALL>(D.P, F, c.row, f, active && end > start);
                const Acc<real, VEC> acc = fold_range<real, VEC, ACT, SMALL>(ops, p, start, end, G, gl, f, active);
                if (active) st<VEC>(row_at<SMALL>(D.out, c.row, F, f), acc);
            }
        }
    }
    const int nl_lane = c.nl_lane;
    const int blk = __builtin_amdgcn_readfirstlane(c.blk_v), nblk = __builtin_amdgcn_readfirstlane(c.nblk_v);
    const int long_cap = __builtin_amdgcn_readfirstlane(c.long_cap_v);
    // lanes 0..7 of every wave hold the lengths of the eight sub-lists: read through shuffles, they stay in vector registers
    int n_long_v = 0;
#pragma unroll
    for (int p = 0; p < CWN_LONG_PARTS; ++p) n_long_v += __shfl(nl_lane, p);
    const int n_long = __builtin_amdgcn_readfirstlane(n_long_v);
    for (int li = blk; li < n_long; li += nblk) {  // uniform over the workgroup
        int p = 0, k = li;
#pragma unroll
        for (int q = 0; q < CWN_LONG_PARTS - 1; ++q) {   // li-th entry of the concatenated sub-lists
            const int nq = __shfl(nl_lane, q);
            if (p == q && k >= nq) { k -= nq; ++p; }
        }
        const int64_t lrow = c.long_rows_v[(int64_t)p * long_cap + k];
        const int lstart = c.rowptr_v[lrow], lend = c.rowptr_v[lrow + 1];
        const int chunk = (((lend - lstart + R - 1) / R) + 3) & ~3;
        const int s = min(lend, lstart + gq * chunk), e = min(lend, s + chunk);
        for (int f0 = 0; f0 < F; f0 += G * VEC) {
            const int f = f0 + gl * VEC;
            const bool active = f < F;
            const Acc<real, VEC> own = own_slice<real, VEC, SMALL>(D.P, F, lrow, f, active);
            Acc<real, VEC> acc = fold_range<real, VEC, ACT, SMALL>(ops, own, s, e, G, gl, f, active);
            if (gq != 0) {
#pragma unroll
                for (int k2 = 0; k2 < VEC; ++k2) part[threadIdx.x * VEC + k2] = acc.v[k2];
            }
            __syncthreads();
            if (gq == 0 && active) {
                for (int q = 1; q < R; ++q) {               // partials in chunk order
#pragma unroll
                    for (int k2 = 0; k2 < VEC; ++k2) acc.v[k2] = acc.v[k2] + part[(q * G + gl) * VEC + k2];
                }
                st<VEC>(row_at<SMALL>(D.out, lrow, F, f), acc);
            }
            __syncthreads();
        }
    }
}

template <class real, int VEC, bool SMALL>
__device__ __forceinline__ void run_desc_act(const typename DescOf<real>::type& D, const RowCtx& c, real* part) {
    switch (D.act) {
        case CWN_ACT_RELU: run_desc<real, VEC, CWN_ACT_RELU, SMALL>(D, c, part); break;
        case CWN_ACT_ELU: run_desc<real, VEC, CWN_ACT_ELU, SMALL>(D, c, part); break;
        case CWN_ACT_TANH: run_desc<real, VEC, CWN_ACT_TANH, SMALL>(D, c, part); break;
        case CWN_ACT_SIGMOID: run_desc<real, VEC, CWN_ACT_SIGMOID, SMALL>(D, c, part); break;
        default: run_desc<real, VEC, CWN_ACT_ID, SMALL>(D, c, part); break;
    }
}

// The gathers are latency-bound and the activations carry their own temporaries: the register budget is left to the
// compiler (no amdgpu_waves_per_eu), which builds every form without scratch (tests/test_act_message_bwd_resources.py).
template <class real, bool SMALL>
__global__ __launch_bounds__(kThreads) void aggregate_act_bwd_kernel(BwdBatch<real> B) {
    constexpr int kMaxVec = 16 / (int)sizeof(real);
    __shared__ real part[kThreads * kMaxVec];
    const int di = cwn::group_of<CWN_MAX_DESCS>(B.blk_start, B.n, (int)blockIdx.x);
    // By VALUE: a reference into B put the whole batch struct of the f32 aggregate kernel in scratch (cwn_aggregate.hip).
    const typename DescOf<real>::type D = B.d[di];
    const int vec = B.vec[di];
    RowCtx c;
    c.G = B.group[di];
    c.GF = B.fgroup[di];
    const int blk = blockIdx.x - B.blk_start[di];
    const int nblk = B.blk_start[di + 1] - B.blk_start[di];
    const int lg = __builtin_ctz(c.G);             // G is a power of two
    c.R = kThreads >> lg;
    c.gl = threadIdx.x & (c.G - 1);
    c.gq = threadIdx.x >> lg;
    c.has_long = D.long_rows != nullptr && D.n_long != nullptr && D.rowptr != nullptr;
    c.row = (int64_t)blk * c.R + c.gq;
    c.has_row = c.row < D.n_dst;                   // a host count: every row below n_dst exists (no m_dev)
    c.start = c.end = 0;
    if (c.has_row && D.rowptr != nullptr) {
        c.start = D.rowptr[c.row];
        c.end = D.rowptr[c.row + 1];
    }
    // the long-row counters are only needed after the regular rows: vector loads issued after the row pointers
    c.nl_lane = c.has_long ? D.n_long[threadIdx.x & (CWN_LONG_PARTS - 1)] : 0;
    int z = 0;
    asm volatile("" : "+v"(z));  // a zero the compiler cannot fold: keeps the values below in vector registers
    c.blk_v = blk + z;
    c.nblk_v = nblk + z;
    c.long_cap_v = D.long_cap + z;
    c.long_rows_v = D.long_rows + z;
    c.rowptr_v = D.rowptr + z;
    if constexpr (kMaxVec == 4) {
        if (vec == 4) { run_desc_act<real, 4, SMALL>(D, c, part); return; }
    }
    if (vec == 2) run_desc_act<real, 2, SMALL>(D, c, part);
    else run_desc_act<real, 1, SMALL>(D, c, part);
}

// ---- host ----

inline int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// Validation, the per-descriptor geometry and the launch.  Neither allocates nor synchronises.
template <class real>
int launch_act_bwd(const typename DescOf<real>::type* descs, int n, cwn_stream_t stream_) {
    using Desc = typename DescOf<real>::type;
    constexpr int kMaxVec = 16 / (int)sizeof(real);
    if (n < 0 || n > CWN_MAX_DESCS || (n > 0 && descs == nullptr)) return CWN_ERR_BAD_ARG;
    BwdBatch<real> B{};
    B.n = n;
    bool small = true;
    for (int i = 0; i < n; ++i) {
        const Desc& D = descs[i];
        if (D.F <= 0 || D.n_dst < 0 || (D.n_dst > 0 && D.out == nullptr)) return CWN_ERR_BAD_ARG;
        if (!known_act(D.act)) return CWN_ERR_BAD_ARG;
        if (D.rowptr != nullptr && (D.ig == nullptr || D.iq == nullptr || D.g == nullptr || D.P == nullptr || D.Q == nullptr))
            return CWN_ERR_BAD_ARG;
        if (D.n_dst >= INT32_MAX) return CWN_ERR_TOO_LARGE;
        // widest vector every pointer and the row stride allow: 16 bytes, 8, or one element
        int v = kMaxVec;
        while (v > 1 && D.F % v != 0) v >>= 1;
        const bool plan = D.rowptr != nullptr;
        const void* rows[] = {plan ? D.g : nullptr, plan ? D.P : nullptr, plan ? D.Q : nullptr, D.out};
        for (const void* p : rows) {
            if (p == nullptr) continue;
            if (!aligned_to(p, sizeof(real))) return CWN_ERR_ALIGN;
            while (v > 1 && !aligned_to(p, v * sizeof(real))) v >>= 1;
        }
        B.d[i] = D;
        B.vec[i] = v;
        const int lanes = (D.F + v - 1) / v;
        int fg = pow2_at_least(lanes);
        if (fg > 64) fg = 64;
        B.fgroup[i] = fg;
        // narrow features (fewer than 8 feature lanes): entry slots next to them, as the forward lays them out
        if (sizeof(real) == 4) B.group[i] = fg < 8 ? 8 : fg;
        else B.group[i] = fg < 8 ? 8 : (lanes < 8 ? 2 * fg : fg);
        small = small && (D.flags & CWN_AGG_SMALL_OPERANDS) != 0 &&
                (uint64_t)D.n_dst * (uint64_t)D.F * sizeof(real) < (1ull << 32);
    }
    cwn::BlockFill fill(B.blk_start);
    for (int i = 0; i < n; ++i) {
        const int rows_per_block = kThreads / B.group[i];
        if (!fill.push(i, (B.d[i].n_dst + rows_per_block - 1) / rows_per_block)) return CWN_ERR_TOO_LARGE;
    }
    const int64_t blocks = fill.close(n);
    if (blocks == 0) return CWN_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)blocks), block(kThreads);
    if (small) aggregate_act_bwd_kernel<real, true><<<grid, block, 0, stream>>>(B);
    else aggregate_act_bwd_kernel<real, false><<<grid, block, 0, stream>>>(B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

}  // namespace

extern "C" int cwn_aggregate_act_bwd_f32(const cwn_agg_act_bwd_desc* descs, int n, cwn_stream_t stream) {
    return launch_act_bwd<float>(descs, n, stream);
}

extern "C" int cwn_aggregate_act_bwd_f64(const cwn_agg_act_bwd_desc_f64* descs, int n, cwn_stream_t stream) {
    return launch_act_bwd<double>(descs, n, stream);
}
