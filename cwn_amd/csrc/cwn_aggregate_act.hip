// cwn_aggregate_act.hip -- the coboundary message of a non-ReLU model as one launch, float32 and float64:
//
//     out[i, :] = sum over p in row i, in CSR order, of act(A[ia[p], :] + B[ib[p], :])  +  (1 + eps) * self_x[i, :]
//
// with act one of the five CWN_ACT_* codes.  The activation follows the Linear of act(Linear(cat(x_j, up_attr))), so the
// split of the ReLU stream -- Y1 = X W[:, :F]^T + b per source cell, Y2 = X_attr W[:, F:]^T per shared cell, gathered and
// added per entry -- holds for every activation; what cwn_aggregate_f32 / _f64 lack is an activation other than ReLU, and
// their device code is held fixed (cwn_aggregate_body.h).  Hence entry points and a descriptor of their own, in this file.
//
// The mapping is that of cwn_aggregate.hip (read its header first): a GROUP of G lanes owns a destination row, a lane
// holds a 16-byte slice of the feature row, the group fetches a segment's indices cooperatively and broadcasts them with
// __shfl, four gathered rows are in flight before the first add, rows are addressed with 32-bit byte offsets when every
// operand of the launch lies within 4 GiB of its base (row_at<SMALL>).  What differs:
//   * one text for both element types (a template parameter; nothing pins these kernels' names);
//   * the vector width, the lanes per row and the entry slots are chosen PER DESCRIPTOR and dispatched inside the kernel,
//     so a row's bits depend on its entries, F and its own operands -- not on the other descriptors of the launch;
//   * only what the activated message needs: add, a full-width B, one self term, host row counts.
// Sums: rows of at most CWN_LONG_ROW entries are folded sequentially in CSR order by one lane group (with fewer than 8
// feature lanes, rows above kSplitRow entries by the group's entry slots and a fixed xor tree); longer rows, from the
// long-row lists of cwn_csr_build, by a whole workgroup in contiguous chunks combined in chunk order through LDS.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_act.h"
#include "cwn_check.h"
#include "cwn_mem.h"
#include "cwn_group.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSplitRow = 16;      // as in cwn_aggregate_body.h: longer rows of narrow descriptors take the entry slots

template <class real> struct DescOf;
template <> struct DescOf<float> { using type = cwn_agg_act_desc; };
template <> struct DescOf<double> { using type = cwn_agg_act_desc_f64; };

template <class real>
struct ActBatch {
    typename DescOf<real>::type d[CWN_MAX_DESCS];
    int32_t blk_start[CWN_MAX_DESCS + 1];
    int32_t group[CWN_MAX_DESCS];   // lanes per destination row
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

// acc += act(a + b): one add for the pre-activation, in the element type
template <class real, int VEC, int ACT>
__device__ __forceinline__ void add_message(Acc<real, VEC>& acc, const Acc<real, VEC>& a, const Acc<real, VEC>& b) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + activate<ACT>(a.v[k] + b.v[k]);
}

template <class real>
struct Operands {        // the descriptor fields a fold needs, by value (registers)
    const int32_t* ia;
    const int32_t* ib;
    const real* A;
    const real* B;
    int F;
};

// One group (G lanes, lane-in-group `gl`) folds CSR positions [start, end) of one destination row into a register
// accumulator, in CSR order.  Every lane of the group runs every loop with the same trip counts (the index fetch and the
// shuffles need all G lanes); lanes whose feature slice starts past F (`!active`) only skip the loads.
template <class real, int VEC, int ACT, bool SMALL>
__device__ __forceinline__ Acc<real, VEC> fold_range(const Operands<real> D, int start, int end, int G, int gl, int f,
                                                     bool active) {
    const int F = D.F;
    Acc<real, VEC> acc = splat<real, VEC>(real(0.0));
    for (int base = start; base < end; base += G) {
        // cooperative index fetch: lane gl holds the indices of CSR position base+gl
        const int mine = base + gl;
        int my_ia = 0, my_ib = 0;
        if (mine < end) {
            my_ia = D.ia[mine];
            my_ib = D.ib[mine];
        }
        const int cnt = min(G, end - base);
        int t = 0;
        for (; t + 4 <= cnt; t += 4) {
            Acc<real, VEC> a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ia = __shfl(my_ia, t + u, G);
                const int ib = __shfl(my_ib, t + u, G);
                a[u] = splat<real, VEC>(real(0.0));
                b[u] = splat<real, VEC>(real(0.0));
                if (active) {
                    a[u] = ld<VEC>(row_at<SMALL>(D.A, ia, F, f));
                    b[u] = ld<VEC>(row_at<SMALL>(D.B, ib, F, f));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) add_message<real, VEC, ACT>(acc, a[u], b[u]);
        }
        for (; t < cnt; ++t) {
            const int ia = __shfl(my_ia, t, G);
            const int ib = __shfl(my_ib, t, G);
            Acc<real, VEC> a = splat<real, VEC>(real(0.0)), b = splat<real, VEC>(real(0.0));
            if (active) {
                a = ld<VEC>(row_at<SMALL>(D.A, ia, F, f));
                b = ld<VEC>(row_at<SMALL>(D.B, ib, F, f));
            }
            add_message<real, VEC, ACT>(acc, a, b);
        }
    }
    return acc;
}

// Fewer than 8 feature lanes: the G lanes of a group are S = G / GF entry slots x GF feature lanes, every slot folds every
// S-th entry of a row above kSplitRow entries and the S partials are combined by a fixed xor tree (cwn_aggregate_body.h,
// fold_range_split: one lane walking a 95-entry row of the F = 1 layer alone is 24 dependent round trips).
template <class real, int VEC, int ACT, bool SMALL>
__device__ __forceinline__ Acc<real, VEC> fold_range_split(const Operands<real> D, int start, int end, int G, int GF, int gl) {
    const int F = D.F;
    const int S = G / GF, e = gl / GF, f = (gl % GF) * VEC;
    const bool active = f < F;
    Acc<real, VEC> acc = splat<real, VEC>(real(0.0));
    for (int base = start; base < end; base += G) {
        const int mine = base + gl;
        int my_ia = 0, my_ib = 0;
        if (mine < end) {
            my_ia = D.ia[mine];
            my_ib = D.ib[mine];
        }
        const int cnt = min(G, end - base);
        for (int tb = 0; tb < cnt; tb += 2 * S) {          // uniform trip count over the group
            Acc<real, VEC> a[2], b[2];
            bool ok[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = tb + u * S + e;
                ok[u] = t < cnt;
                const int ia = __shfl(my_ia, ok[u] ? t : 0, G);
                const int ib = __shfl(my_ib, ok[u] ? t : 0, G);
                a[u] = splat<real, VEC>(real(0.0));
                b[u] = splat<real, VEC>(real(0.0));
                if (active && ok[u]) {
                    a[u] = ld<VEC>(row_at<SMALL>(D.A, ia, F, f));
                    b[u] = ld<VEC>(row_at<SMALL>(D.B, ib, F, f));
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (ok[u]) add_message<real, VEC, ACT>(acc, a[u], b[u]);
        }
    }
    for (int off = GF; off < G; off <<= 1) {               // entry slots -> slot 0, fixed tree
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + __shfl_xor(acc.v[k], off, G);
    }
    return acc;
}

// the self term, loaded late (the two-operand messages of cwn_aggregate.hip do the same), one coalesced store of the slice
template <class real, int VEC, bool SMALL>
__device__ __forceinline__ void finish_row(const real* self_x, real* out, int F, int64_t row, int f, real scale1,
                                           Acc<real, VEC> acc) {
    if (self_x != nullptr) {
        const Acc<real, VEC> s1 = ld<VEC>(row_at<SMALL>(self_x, row, F, f));
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + scale1 * s1.v[k];
    }
    st<VEC>(row_at<SMALL>(out, row, F, f), acc);
}

// What a lane knows about its row before the fold, computed once per kernel ahead of the dispatch on (vector width,
// activation) -- fifteen forms in float32 (16, 8 and 4 bytes per lane x five activations), ten in float64.  The kernel must
// not spill: whatever is common to the forms is computed here, once, so that none of its scalar conditions is live
// across the dispatch.
template <class real>
struct RowCtx {
    int blk, nblk;       // workgroup `blk` of the `nblk` that serve the descriptor (kernel prologue only)
    int G, GF, R;        // lanes per row, of which feature lanes; rows per workgroup
    int gl, gq;          // lane in group, group in workgroup
    int64_t row;
    int start, end;      // the row's CSR positions (0, 0: no row, or no adjacency)
    int nl_lane;         // n_long[lane & 7], or 0 without long-row lists
    real self_scale;     // 1 + eps
    bool has_row, has_long;
    // What only the long-row pass reads, held in VECTOR registers while the rows are folded (the values are uniform; the
    // pass takes them back with readfirstlane): the folds need the scalar registers, the float64 activations keep their
    // polynomial coefficients in scalar pairs.
    int blk_v, nblk_v, long_cap_v;
    const int32_t* long_rows_v;
    const int32_t* rowptr_v;
};

// Every lane group reduces its own destination row; then the workgroups share the rows of the long-row lists round-robin
// (cwn_aggregate_body.h, run_desc).
template <class real, int VEC, int ACT, bool SMALL>
__device__ __forceinline__ void run_desc(const typename DescOf<real>::type& D, const RowCtx<real>& c, real* part) {
    const int F = D.F;
    const int G = c.G, GF = c.GF, R = c.R, gl = c.gl, gq = c.gq;
    const int start = c.start, end = c.end;
    const real self_scale = c.self_scale;
    const Operands<real> ops{D.ia, D.ib, D.A, D.B, D.F};
    if (c.has_row) {  // whole groups take the branch together (G divides 64)
        if (c.has_long && end - start > CWN_LONG_ROW) {
            // left to the whole-workgroup pass below
        } else if (GF < G && end - start > kSplitRow) {
            const int f = (gl % GF) * VEC;
            const Acc<real, VEC> acc = fold_range_split<real, VEC, ACT, SMALL>(ops, start, end, G, GF, gl);
            if (f < F && gl < GF) finish_row<real, VEC, SMALL>(D.self_x, D.out, F, c.row, f, self_scale, acc);
        } else {
            // feature chunks of G*VEC columns (one chunk when F <= G*VEC, the common case)
            for (int f0 = 0; f0 < F; f0 += G * VEC) {
                const int f = f0 + gl * VEC;
                const bool active = f < F;
                const Acc<real, VEC> acc = fold_range<real, VEC, ACT, SMALL>(ops, start, end, G, gl, f, active);
                if (active) finish_row<real, VEC, SMALL>(D.self_x, D.out, F, c.row, f, self_scale, acc);
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
            Acc<real, VEC> acc = fold_range<real, VEC, ACT, SMALL>(ops, s, e, G, gl, f, active);
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
                finish_row<real, VEC, SMALL>(D.self_x, D.out, F, lrow, f, self_scale, acc);
            }
            __syncthreads();
        }
    }
}

template <class real, int VEC, bool SMALL>
__device__ __forceinline__ void run_desc_act(const typename DescOf<real>::type& D, const RowCtx<real>& c, real* part) {
    switch (D.act) {
        case CWN_ACT_RELU: run_desc<real, VEC, CWN_ACT_RELU, SMALL>(D, c, part); break;
        case CWN_ACT_ELU: run_desc<real, VEC, CWN_ACT_ELU, SMALL>(D, c, part); break;
        case CWN_ACT_TANH: run_desc<real, VEC, CWN_ACT_TANH, SMALL>(D, c, part); break;
        case CWN_ACT_SIGMOID: run_desc<real, VEC, CWN_ACT_SIGMOID, SMALL>(D, c, part); break;
        default: run_desc<real, VEC, CWN_ACT_ID, SMALL>(D, c, part); break;
    }
}

// The gathers are latency-bound and the activations carry their own temporaries: the register budget is left to the
// compiler (no amdgpu_waves_per_eu), which builds every form without scratch (tests/test_act_message_resources.py).
template <class real, bool SMALL>
__global__ __launch_bounds__(kThreads) void aggregate_act_kernel(ActBatch<real> B) {
    constexpr int kMaxVec = 16 / (int)sizeof(real);
    __shared__ real part[kThreads * kMaxVec];
    const int di = cwn::group_of<CWN_MAX_DESCS>(B.blk_start, B.n, (int)blockIdx.x);
    // By VALUE: a reference into B put the whole batch struct of the f32 aggregate kernel in scratch (cwn_aggregate.hip).
    const typename DescOf<real>::type D = B.d[di];
    const int vec = B.vec[di];
    RowCtx<real> c;
    c.G = B.group[di];
    c.GF = B.fgroup[di];
    c.blk = blockIdx.x - B.blk_start[di];
    c.nblk = B.blk_start[di + 1] - B.blk_start[di];
    const int lg = __builtin_ctz(c.G);             // G is a power of two
    c.R = kThreads >> lg;
    c.gl = threadIdx.x & (c.G - 1);
    c.gq = threadIdx.x >> lg;
    c.has_long = D.long_rows != nullptr && D.n_long != nullptr && D.rowptr != nullptr;
    c.row = (int64_t)c.blk * c.R + c.gq;
    c.has_row = c.row < D.n_dst;                   // a host count: every row below n_dst exists (no m_dev)
    c.start = c.end = 0;
    if (c.has_row && D.rowptr != nullptr) {
        c.start = D.rowptr[c.row];
        c.end = D.rowptr[c.row + 1];
    }
    // The long-row counters are only needed after the regular rows, eps at the end of a row: vector loads issued after
    // the row pointers, so that waiting for the row pointers does not wait for these (cwn_aggregate_body.h, run_desc).
    c.nl_lane = c.has_long ? D.n_long[threadIdx.x & (CWN_LONG_PARTS - 1)] : 0;
    int z = 0;
    asm volatile("" : "+v"(z));  // a zero the compiler cannot fold: keeps the eps load in VMEM
    c.self_scale = real(1.0) + (D.eps != nullptr ? D.eps[z] : real(0.0));
    c.blk_v = c.blk + z;
    c.nblk_v = c.nblk + z;
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
int launch_act(const typename DescOf<real>::type* descs, int n, cwn_stream_t stream_) {
    using Desc = typename DescOf<real>::type;
    constexpr int kMaxVec = 16 / (int)sizeof(real);
    if (n < 0 || n > CWN_MAX_DESCS || (n > 0 && descs == nullptr)) return CWN_ERR_BAD_ARG;
    ActBatch<real> B{};
    B.n = n;
    bool small = true;
    for (int i = 0; i < n; ++i) {
        const Desc& D = descs[i];
        if (D.F <= 0 || D.n_dst < 0 || (D.n_dst > 0 && D.out == nullptr)) return CWN_ERR_BAD_ARG;
        if (!known_act(D.act)) return CWN_ERR_BAD_ARG;
        if (D.rowptr != nullptr && (D.ia == nullptr || D.ib == nullptr || D.A == nullptr || D.B == nullptr)) return CWN_ERR_BAD_ARG;
        if (D.n_dst >= INT32_MAX) return CWN_ERR_TOO_LARGE;
        // widest vector every pointer and the row stride allow: 16 bytes, 8, or one element
        int v = kMaxVec;
        while (v > 1 && D.F % v != 0) v >>= 1;
        const void* rows[] = {D.rowptr != nullptr ? D.A : nullptr, D.rowptr != nullptr ? D.B : nullptr, D.self_x, D.out};
        for (const void* p : rows) {
            if (p == nullptr) continue;
            if (!aligned_to(p, sizeof(real))) return CWN_ERR_ALIGN;
            while (v > 1 && !aligned_to(p, v * sizeof(real))) v >>= 1;
        }
        if (D.eps != nullptr && !aligned_to(D.eps, sizeof(real))) return CWN_ERR_ALIGN;
        B.d[i] = D;
        B.vec[i] = v;
        const int lanes = (D.F + v - 1) / v;
        int fg = pow2_at_least(lanes);
        if (fg > 64) fg = 64;
        B.fgroup[i] = fg;
        // narrow features (fewer than 8 feature lanes): entry slots next to them, as cwn_aggregate_f32 / _f64 lay them out
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
    if (small) aggregate_act_kernel<real, true><<<grid, block, 0, stream>>>(B);
    else aggregate_act_kernel<real, false><<<grid, block, 0, stream>>>(B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

}  // namespace

extern "C" int cwn_aggregate_act_f32(const cwn_agg_act_desc* descs, int n, cwn_stream_t stream) {
    return launch_act<float>(descs, n, stream);
}

extern "C" int cwn_aggregate_act_f64(const cwn_agg_act_desc_f64* descs, int n, cwn_stream_t stream) {
    return launch_act<double>(descs, n, stream);
}
