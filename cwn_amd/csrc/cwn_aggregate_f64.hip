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
// A kernel of its own name; everything between its dispatch and ld / st is the text the f32 kernel
// compiles, cwn_aggregate_body.h.
#include <hip/hip_runtime.h>
#include <float.h>
#include "../../include/cwn_hip.h"
#include "cwn_mem.h"

namespace {

struct AggBatch64 {
    cwn_agg_desc_f64 d[CWN_MAX_DESCS];
    int32_t blk_start[CWN_MAX_DESCS + 1];
    int32_t group[CWN_MAX_DESCS];  // lanes per destination row
    int32_t fgroup[CWN_MAX_DESCS]; // of which feature lanes (the rest are entry slots, narrow F only)
    int32_t n;
};

using real = double;
using desc_t = cwn_agg_desc_f64;
constexpr real kNegInf = -__builtin_huge_val();

}  // namespace

#include "cwn_aggregate_body.h"

namespace {

typedef double v2d __attribute__((ext_vector_type(2)));

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
    const int di = cwn::group_of<CWN_MAX_DESCS>(B.blk_start, B.n, (int)blockIdx.x);
    // By VALUE: a reference into B put the whole batch struct of the f32 NARROW kernel in scratch
    // (20x slower; the measurement is at the same line of aggregate_kernel).
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

}  // namespace

extern "C" int cwn_aggregate_f64(const cwn_agg_desc_f64* descs, int n, cwn_stream_t stream_) {
    if (descs == nullptr || n <= 0 || n > CWN_MAX_DESCS) return CWN_ERR_BAD_ARG;
    AggBatch64 B{};
    B.n = n;
    int vec = 2;
    for (int i = 0; i < n; ++i) {
        const cwn_agg_desc_f64& D = descs[i];
        if (const int err = check_desc(D); err != CWN_OK) return err;
        // widest vector every pointer and the row stride allow
        int v = (D.F % 2 == 0) ? 2 : 1;
        const void* ptrs[] = {D.A, D.b_width == D.F ? (const void*)D.B : nullptr, D.self_x,
                              D.self_pre, D.out, D.self_x2};
        for (const void* p : ptrs) {
            if (p == nullptr) continue;
            if (!al8(p)) return CWN_ERR_ALIGN;
            if (v == 2 && !al16(p)) v = 1;
        }
        const void* scalars[] = {D.b_width == 1 ? (const void*)D.B : nullptr, D.eps, D.eps2};
        for (const void* p : scalars)
            if (p != nullptr && !al8(p)) return CWN_ERR_ALIGN;
        if (v < vec) vec = v;
    }
    cwn::BlockFill fill(B.blk_start);
    for (int i = 0; i < n; ++i) {
        B.d[i] = descs[i];
        B.fgroup[i] = pick_group(descs[i].F, vec);
        // narrow features (fewer than 8 feature lanes): at least two entry slots per row
        const bool few = (descs[i].F + vec - 1) / vec < 8;
        B.group[i] = B.fgroup[i] < 8 ? 8 : (few ? 2 * B.fgroup[i] : B.fgroup[i]);
        const int rows_per_block = kThreads / B.group[i];
        if (!fill.push(i, (B.d[i].n_dst + rows_per_block - 1) / rows_per_block)) return CWN_ERR_TOO_LARGE;
    }
    const int64_t blocks = fill.close(n);
    if (blocks == 0) return CWN_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)blocks), block(kThreads);
    const bool narrow = any_narrow(B), small = all_small(B);
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
    if (vec == 2 && !(al16(src) && al16(out))) vec = 1;
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
