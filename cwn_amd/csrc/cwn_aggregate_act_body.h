// cwn_aggregate_act_body.h -- what the forward and the backward of the activated coboundary message share
// (cwn_aggregate_act.hip, cwn_aggregate_act_bwd.hip): the folds of a row, the long-row pass through LDS, the dispatch on
// (vector width, activation), the kernel's prologue and the host launcher.  One text; each file instantiates it with a
// FORM, a struct of static functions that says what its direction sums and which operands it has.
//
// A form defines
//     using real = float | double;   using Desc = its descriptor (include/cwn_hip.h)
//     operands(D)                    Operands<real>{i0, i1, X0, X1, F}: the two index arrays of a CSR position and the two
//                                    matrices gathered through them
//     term<VEC, ACT>(acc, x0, x1, own)          acc = acc + (the term of one entry); `own` is the row's own slice
//     own<VEC, SMALL>(D, row, f, active)        the lane's slice of the row's own operand, zeros for a form without one and
//                                               for `!active` (the row of an absent plan may not exist: it is not read)
//     finish<VEC, SMALL>(D, row, f, self_scale, acc)   whatever is added to a finished sum, and the store of the slice
//     self_scale(D, z)               the factor finish gets, read once per kernel; z is a zero the compiler cannot fold
//     plan_complete(D)               host: with a plan (rowptr) every operand the folds read is there
//     pointers(D)                    host: HostPointers{rows, scalar} -- the row pointers that take part in the alignment
//                                    check and the choice of the vector width (absent ones null), and a pointer that only
//                                    has to be aligned to the element
// and, in its file, the batch struct (d, blk_start, group, fgroup, vec, n) and the __global__ kernel, which declares the
// LDS partials and calls run_block: kernel and batch struct keep the names of their file.
//
// The mapping is that of cwn_aggregate.hip (read its header first): a GROUP of G lanes owns a row, a lane holds a 16-byte
// slice of the feature row (8 bytes or one element where width or alignment ask for it), the group fetches a segment's
// indices cooperatively and broadcasts them with __shfl, four gathered row pairs are in flight before the first term, rows
// are addressed with 32-bit byte offsets when every operand of the launch lies within 4 GiB of its base (row_at<SMALL>).
// What differs from that file:
//   * one text for both element types (a template parameter; nothing pins these kernels' names);
//   * the vector width, the lanes per row and the entry slots are chosen PER DESCRIPTOR and dispatched inside the kernel,
//     so a row's bits depend on its entries, F and its own operands -- not on the other descriptors of the launch;
//   * only what the activated message needs: full-width operands, host row counts.
// Sums: rows of at most CWN_LONG_ROW entries are folded sequentially in CSR order by one lane group (with fewer than 8
// feature lanes, rows above kSplitRow entries by the group's entry slots and a fixed xor tree); longer rows, from the
// long-row lists of cwn_csr_build, by a whole workgroup in contiguous chunks combined in chunk order through LDS.  Rows
// wider than one pass of the group are folded in feature chunks.  A row without entries, and every row of an absent plan,
// gets what finish makes of zeros.  No atomics.
//
// Arithmetic, in both directions: the pre-activation is ONE add in the element type; a product and the accumulate are
// separate, a rounded multiply and a rounded add, never one fma (the library is built with -ffp-contract=off); entries are
// added in CSR order.
#pragma once
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

template <class real>
struct Operands {        // the descriptor fields a fold needs, by value (registers)
    const int32_t* i0;
    const int32_t* i1;
    const real* X0;
    const real* X1;
    int F;
};

// One group (G lanes, lane-in-group `gl`) folds CSR positions [start, end) of one row into a register accumulator, in CSR
// order; `own` is the lane's slice of the row's own operand.  Every lane of the group runs every loop with the same trip
// counts (the index fetch and the shuffles need all G lanes); lanes whose feature slice starts past F (`!active`) only
// skip the loads.
template <class Form, int VEC, int ACT, bool SMALL, class real = typename Form::real>
__device__ __forceinline__ Acc<real, VEC> fold_range(const Operands<real> D, const Acc<real, VEC> own, int start, int end,
                                                     int G, int gl, int f, bool active) {
    const int F = D.F;
    Acc<real, VEC> acc = splat<real, VEC>(real(0.0));
    for (int base = start; base < end; base += G) {
        // cooperative index fetch: lane gl holds the indices of CSR position base+gl
        const int mine = base + gl;
        int my_i0 = 0, my_i1 = 0;
        if (mine < end) {
            my_i0 = D.i0[mine];
            my_i1 = D.i1[mine];
        }
        const int cnt = min(G, end - base);
        int t = 0;
        for (; t + 4 <= cnt; t += 4) {
            Acc<real, VEC> x0[4], x1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i0 = __shfl(my_i0, t + u, G);
                const int i1 = __shfl(my_i1, t + u, G);
                x0[u] = splat<real, VEC>(real(0.0));
                x1[u] = splat<real, VEC>(real(0.0));
                if (active) {
                    x0[u] = ld<VEC>(row_at<SMALL>(D.X0, i0, F, f));
                    x1[u] = ld<VEC>(row_at<SMALL>(D.X1, i1, F, f));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) Form::template term<VEC, ACT>(acc, x0[u], x1[u], own);
        }
        for (; t < cnt; ++t) {
            const int i0 = __shfl(my_i0, t, G);
            const int i1 = __shfl(my_i1, t, G);
            Acc<real, VEC> x0 = splat<real, VEC>(real(0.0)), x1 = splat<real, VEC>(real(0.0));
            if (active) {
                x0 = ld<VEC>(row_at<SMALL>(D.X0, i0, F, f));
                x1 = ld<VEC>(row_at<SMALL>(D.X1, i1, F, f));
            }
            Form::template term<VEC, ACT>(acc, x0, x1, own);
        }
    }
    return acc;
}

// Fewer than 8 feature lanes: the G lanes of a group are S = G / GF entry slots x GF feature lanes, every slot folds every
// S-th entry of a row above kSplitRow entries and the S partials are combined by a fixed xor tree (cwn_aggregate_body.h,
// fold_range_split: one lane walking a 95-entry row of the F = 1 layer alone is 24 dependent round trips).
template <class Form, int VEC, int ACT, bool SMALL, class real = typename Form::real>
__device__ __forceinline__ Acc<real, VEC> fold_range_split(const Operands<real> D, const Acc<real, VEC> own, int start,
                                                           int end, int G, int GF, int gl) {
    const int F = D.F;
    const int S = G / GF, e = gl / GF, f = (gl % GF) * VEC;
    const bool active = f < F;
    Acc<real, VEC> acc = splat<real, VEC>(real(0.0));
    for (int base = start; base < end; base += G) {
        const int mine = base + gl;
        int my_i0 = 0, my_i1 = 0;
        if (mine < end) {
            my_i0 = D.i0[mine];
            my_i1 = D.i1[mine];
        }
        const int cnt = min(G, end - base);
        for (int tb = 0; tb < cnt; tb += 2 * S) {          // uniform trip count over the group
            Acc<real, VEC> x0[2], x1[2];
            bool ok[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = tb + u * S + e;
                ok[u] = t < cnt;
                const int i0 = __shfl(my_i0, ok[u] ? t : 0, G);
                const int i1 = __shfl(my_i1, ok[u] ? t : 0, G);
                x0[u] = splat<real, VEC>(real(0.0));
                x1[u] = splat<real, VEC>(real(0.0));
                if (active && ok[u]) {
                    x0[u] = ld<VEC>(row_at<SMALL>(D.X0, i0, F, f));
                    x1[u] = ld<VEC>(row_at<SMALL>(D.X1, i1, F, f));
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (ok[u]) Form::template term<VEC, ACT>(acc, x0[u], x1[u], own);
        }
    }
    for (int off = GF; off < G; off <<= 1) {               // entry slots -> slot 0, fixed tree
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + __shfl_xor(acc.v[k], off, G);
    }
    return acc;
}

// What a lane knows about its row before the fold, computed once per kernel ahead of the dispatch on (vector width,
// activation) -- fifteen forms in float32 (16, 8 and 4 bytes per lane x five activations), ten in float64.  The kernel must
// not spill: whatever is common to the forms is computed here, once, so that none of its scalar conditions is live
// across the dispatch.
template <class real>
struct RowCtx {
    int G, GF, R;        // lanes per row, of which feature lanes; rows per workgroup
    int gl, gq;          // lane in group, group in workgroup
    int64_t row;
    int start, end;      // the row's CSR positions (0, 0: no row, or no plan)
    int nl_lane;         // n_long[lane & 7], or 0 without long-row lists
    real self_scale;     // Form::self_scale
    bool has_row, has_long;
    // What only the long-row pass reads, held in VECTOR registers while the rows are folded (the values are uniform; the
    // pass takes them back with readfirstlane): the folds need the scalar registers, the float64 activations keep their
    // polynomial coefficients in scalar pairs.
    int blk_v, nblk_v, long_cap_v;
    const int32_t* long_rows_v;
    const int32_t* rowptr_v;
};

// Every lane group reduces its own row; then the workgroups share the rows of the long-row lists round-robin
// (cwn_aggregate_body.h, run_desc).
template <class Form, int VEC, int ACT, bool SMALL, class real = typename Form::real>
__device__ __forceinline__ void run_desc(const typename Form::Desc& D, const RowCtx<real>& c, real* part) {
    const int F = D.F;
    const int G = c.G, GF = c.GF, R = c.R, gl = c.gl, gq = c.gq;
    const int start = c.start, end = c.end;
    const real self_scale = c.self_scale;
    const Operands<real> ops = Form::operands(D);
    if (c.has_row) {  // whole groups take the branch together (G divides 64)
        if (c.has_long && end - start > CWN_LONG_ROW) {
            // left to the whole-workgroup pass below
        } else if (GF < G && end - start > kSplitRow) {
            const int f = (gl % GF) * VEC;
            const Acc<real, VEC> own = Form::template own<VEC, SMALL>(D, c.row, f, f < F);
            const Acc<real, VEC> acc = fold_range_split<Form, VEC, ACT, SMALL>(ops, own, start, end, G, GF, gl);
            if (f < F && gl < GF) Form::template finish<VEC, SMALL>(D, c.row, f, self_scale, acc);
        } else {
            // feature chunks of G*VEC columns (one chunk when F <= G*VEC, the common case)
            for (int f0 = 0; f0 < F; f0 += G * VEC) {
                const int f = f0 + gl * VEC;
                const bool active = f < F;
                // (a row without entries reads nothing: its own row may not exist when the plan is absent)
                const Acc<real, VEC> own = Form::template own<VEC, SMALL>(D, c.row, f, active && end > start);
                const Acc<real, VEC> acc = fold_range<Form, VEC, ACT, SMALL>(ops, own, start, end, G, gl, f, active);
                if (active) Form::template finish<VEC, SMALL>(D, c.row, f, self_scale, acc);
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
            const Acc<real, VEC> own = Form::template own<VEC, SMALL>(D, lrow, f, active);
            Acc<real, VEC> acc = fold_range<Form, VEC, ACT, SMALL>(ops, own, s, e, G, gl, f, active);
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
                Form::template finish<VEC, SMALL>(D, lrow, f, self_scale, acc);
            }
            __syncthreads();
        }
    }
}

template <class Form, int VEC, bool SMALL, class real = typename Form::real>
__device__ __forceinline__ void run_desc_act(const typename Form::Desc& D, const RowCtx<real>& c, real* part) {
    switch (D.act) {
        case CWN_ACT_RELU: run_desc<Form, VEC, CWN_ACT_RELU, SMALL>(D, c, part); break;
        case CWN_ACT_ELU: run_desc<Form, VEC, CWN_ACT_ELU, SMALL>(D, c, part); break;
        case CWN_ACT_TANH: run_desc<Form, VEC, CWN_ACT_TANH, SMALL>(D, c, part); break;
        case CWN_ACT_SIGMOID: run_desc<Form, VEC, CWN_ACT_SIGMOID, SMALL>(D, c, part); break;
        default: run_desc<Form, VEC, CWN_ACT_ID, SMALL>(D, c, part); break;
    }
}

// The whole of a kernel but its LDS: `part` holds kThreads x 16 bytes.  The gathers are latency-bound and the activations
// carry their own temporaries: the kernels leave the register budget to the compiler (no amdgpu_waves_per_eu), which builds
// every form without scratch (tests/test_act_message_resources.py, tests/test_act_message_bwd_resources.py).
template <class Form, bool SMALL, class Batch, class real = typename Form::real>
__device__ __forceinline__ void run_block(const Batch& B, real* part) {
    constexpr int kMaxVec = 16 / (int)sizeof(real);
    const int di = cwn::group_of<CWN_MAX_DESCS>(B.blk_start, B.n, (int)blockIdx.x);
    // By VALUE: a reference into B put the whole batch struct of the f32 aggregate kernel in scratch (cwn_aggregate.hip).
    const typename Form::Desc D = B.d[di];
    const int vec = B.vec[di];
    RowCtx<real> c;
    c.G = B.group[di];
    c.GF = B.fgroup[di];
    const int blk = blockIdx.x - B.blk_start[di];      // workgroup `blk` of the `nblk` that serve the descriptor
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
    // The long-row counters are only needed after the regular rows, the self scale at the end of a row: vector loads issued
    // after the row pointers, so that waiting for the row pointers does not wait for these (cwn_aggregate_body.h, run_desc).
    c.nl_lane = c.has_long ? D.n_long[threadIdx.x & (CWN_LONG_PARTS - 1)] : 0;
    int z = 0;
    asm volatile("" : "+v"(z));  // a zero the compiler cannot fold: keeps what is added to it in vector registers
    c.self_scale = Form::self_scale(D, z);
    c.blk_v = blk + z;
    c.nblk_v = nblk + z;
    c.long_cap_v = D.long_cap + z;
    c.long_rows_v = D.long_rows + z;
    c.rowptr_v = D.rowptr + z;
    if constexpr (kMaxVec == 4) {
        if (vec == 4) { run_desc_act<Form, 4, SMALL>(D, c, part); return; }
    }
    if (vec == 2) run_desc_act<Form, 2, SMALL>(D, c, part);
    else run_desc_act<Form, 1, SMALL>(D, c, part);
}

// ---- host ----

struct HostPointers {
    const void* rows[4];     // null: absent
    const void* scalar;
};

inline int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// Validation, the per-descriptor geometry and the launch of `small_kernel` (32-bit row offsets) or `large_kernel`.  Neither
// allocates nor synchronises.  The order of the checks is the order of the return codes (tests/test_act_message_host.py,
// tests/test_act_message_bwd_host.py).
template <class Form, class Batch>
int launch_act(const typename Form::Desc* descs, int n, cwn_stream_t stream_, void (*small_kernel)(Batch),
               void (*large_kernel)(Batch)) {
    using Desc = typename Form::Desc;
    using real = typename Form::real;
    constexpr int kMaxVec = 16 / (int)sizeof(real);
    if (n < 0 || n > CWN_MAX_DESCS || (n > 0 && descs == nullptr)) return CWN_ERR_BAD_ARG;
    Batch B{};
    B.n = n;
    bool small = true;
    for (int i = 0; i < n; ++i) {
        const Desc& D = descs[i];
        if (D.F <= 0 || D.n_dst < 0 || (D.n_dst > 0 && D.out == nullptr)) return CWN_ERR_BAD_ARG;
        if (!known_act(D.act)) return CWN_ERR_BAD_ARG;
        if (D.rowptr != nullptr && !Form::plan_complete(D)) return CWN_ERR_BAD_ARG;
        if (D.n_dst >= INT32_MAX) return CWN_ERR_TOO_LARGE;
        // widest vector every pointer and the row stride allow: 16 bytes, 8, or one element
        int v = kMaxVec;
        while (v > 1 && D.F % v != 0) v >>= 1;
        const HostPointers ptrs = Form::pointers(D);
        for (const void* p : ptrs.rows) {
            if (p == nullptr) continue;
            if (!aligned_to(p, sizeof(real))) return CWN_ERR_ALIGN;
            while (v > 1 && !aligned_to(p, v * sizeof(real))) v >>= 1;
        }
        if (!aligned_to(ptrs.scalar, sizeof(real))) return CWN_ERR_ALIGN;
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
    (small ? small_kernel : large_kernel)<<<grid, block, 0, stream>>>(B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

}  // namespace
