// cwn_aggregate.hip -- fused gather -> message -> segmented reduce over destination-sorted CSR
// (K1 + message hook + K2 of SURVEY.md §2.2 in one pass), and the plain row gather (K1).
//
// HBM-bound byte work (≈0.25 FLOP/B): no MFMA here.  Mapping for gfx950:
//   * a GROUP of G lanes (G = power of two, 1..64) owns one destination row; each lane holds a
//     VEC-wide (16 B when F % 4 == 0) slice of the feature row, so a gathered source row is read
//     by one fully coalesced wave instruction (G*16 B contiguous) and the output row is written
//     once, coalesced.  F = 128 -> G = 32: two rows per wavefront; F = 64 -> four rows; F <= 4 ->
//     one lane per row.
//   * the segment's indices are fetched by the group cooperatively (one coalesced load of up to
//     G indices) and broadcast with ds_bpermute (__shfl), so the dependent chain is
//     index-load -> row-load instead of one round trip per entry; row loads are issued four at a
//     time before the first add.
//   * accumulation is sequential in CSR (= original entry) order in registers: deterministic and
//     bit-identical to a sequential index_add_; no atomics, no zero-fill pass, absent
//     adjacencies and empty rows write zeros directly.  Rows longer than CWN_LONG_ROW (hubs) are
//     the one exception: a whole workgroup folds such a row in R chunks combined in chunk order
//     (still deterministic; equal to the sequential sum up to fp32 re-association).
//   * one launch covers up to CWN_MAX_DESCS descriptors (all adjacencies of all dimensions of a
//     layer): blockIdx -> (descriptor, row tile) through a small prefix table in kernel args.
#include <hip/hip_runtime.h>
#include <float.h>
#include "../../include/cwn_hip.h"
#include "cwn_mem.h"

namespace {

struct AggBatch {
    cwn_agg_desc d[CWN_MAX_DESCS];
    int32_t blk_start[CWN_MAX_DESCS + 1];
    int32_t group[CWN_MAX_DESCS];  // lanes per destination row
    int32_t fgroup[CWN_MAX_DESCS]; // of which feature lanes (the rest are entry slots, narrow F only)
    int32_t n;
};

using real = float;
using desc_t = cwn_agg_desc;
constexpr real kNegInf = -__builtin_huge_valf();

}  // namespace

#include "cwn_aggregate_body.h"

namespace {

template <int VEC>
__device__ __forceinline__ Acc<VEC> ld(const float* p) {
    Acc<VEC> a;
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
__device__ __forceinline__ void st(float* p, const Acc<VEC>& a) {
    if constexpr (VEC == 4) {
        cwn::store_result4(p, a.v[0], a.v[1], a.v[2], a.v[3]);
    } else if constexpr (VEC == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(a.v[0], a.v[1]);
    } else {
        *p = a.v[0];
    }
}

// Registers decide this kernel's speed: the gathers are latency-bound, so throughput follows the
// number of loads in flight = waves per SIMD x 4..8.  Measured on the same code, 73 VGPRs (6 waves)
// vs 71 (7 waves): 6.5 vs 5.9 us at ZINC-128, 333 vs 298 us at batch 8192.  Forcing a budget with
// amdgpu_waves_per_eu on the 64-bit-address code is not the answer (12 bytes of scratch cost more
// than the wave gained); the SMALL addressing is: 64 VGPRs against 75, and with the attribute (it
// also holds the SGPRs under 96) 8 waves without a spill.
// NARROW: some descriptor has fewer than 8 feature lanes (F <= 16 with 16-B vectors): rows get 8
// lanes and the entry-parallel fold; a separate instantiation so that the wide-feature kernel (every
// layer of the molecular models) carries none of that code.
template <int VEC, bool NARROW, bool SMALL>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(SMALL ? 8 : 1, 8)))
void aggregate_kernel(AggBatch B) {
    __shared__ float part[kThreads * VEC];
    const int di = cwn::group_of<CWN_MAX_DESCS>(B.blk_start, B.n, (int)blockIdx.x);
    // By VALUE.  hipcc passes the batch struct through a private copy that it normally folds back
    // into kernarg loads; with `const cwn_agg_desc& D = B.d[di]` and enough inlined uses of D (the
    // NARROW variant) it stopped doing so and the whole 1.2-KB struct landed in scratch: every
    // descriptor field became a scratch load and the kernel ran 20x slower (measured: 23 -> 580 us).
    const cwn_agg_desc D = B.d[di];
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
__global__ __launch_bounds__(kThreads) void gather_rows_kernel(const float* __restrict__ src,
                                                               const int64_t* __restrict__ idx,
                                                               float* __restrict__ out, int64_t n_idx,
                                                               int F, int G) {
    const int rows_per_block = kThreads / G;
    const int gl = threadIdx.x & (G - 1);
    const int64_t e = (int64_t)blockIdx.x * rows_per_block + threadIdx.x / G;
    if (e >= n_idx) return;
    const int64_t r = idx[e];
    for (int f = gl * VEC; f < F; f += G * VEC) st<VEC>(out + e * F + f, ld<VEC>(src + r * F + f));
}

}  // namespace

extern "C" int cwn_aggregate_f32(const cwn_agg_desc* descs, int n, cwn_stream_t stream_) {
    if (descs == nullptr || n <= 0 || n > CWN_MAX_DESCS) return CWN_ERR_BAD_ARG;
    AggBatch B{};
    B.n = n;
    int vec = 4;
    for (int i = 0; i < n; ++i) {
        const cwn_agg_desc& D = descs[i];
        if (const int err = check_desc(D); err != CWN_OK) return err;
        // widest vector every pointer and the row stride allow
        int v = (D.F % 4 == 0) ? 4 : (D.F % 2 == 0 ? 2 : 1);
        const void* ptrs[] = {D.A, D.b_width == D.F ? (const void*)D.B : nullptr, D.self_x,
                              D.self_pre, D.out, D.self_x2};
        for (const void* p : ptrs) {
            if (p == nullptr) continue;
            if (((uintptr_t)p & 3u) != 0) return CWN_ERR_ALIGN;
            if (v == 4 && !al16(p)) v = al8(p) ? 2 : 1;
            if (v == 2 && !al8(p)) v = 1;
        }
        if (v < vec) vec = v;
    }
    cwn::BlockFill fill(B.blk_start);
    for (int i = 0; i < n; ++i) {
        B.d[i] = descs[i];
        B.fgroup[i] = pick_group(descs[i].F, vec);
        B.group[i] = B.fgroup[i] < 8 ? 8 : B.fgroup[i];     // narrow features: 8 lanes per row anyway
        const int rows_per_block = kThreads / B.group[i];
        if (!fill.push(i, (B.d[i].n_dst + rows_per_block - 1) / rows_per_block)) return CWN_ERR_TOO_LARGE;
    }
    const int64_t blocks = fill.close(n);
    if (blocks == 0) return CWN_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)blocks), block(kThreads);
    const bool narrow = any_narrow(B), small = all_small(B);
    auto launch = [&](auto kernel) { kernel<<<grid, block, 0, stream>>>(B); };
    const int variant = (vec == 4 ? 0 : vec == 2 ? 1 : 2) * 4 + (narrow ? 2 : 0) + (small ? 1 : 0);
    switch (variant) {
        case 0: launch(aggregate_kernel<4, false, false>); break;
        case 1: launch(aggregate_kernel<4, false, true>); break;
        case 2: launch(aggregate_kernel<4, true, false>); break;
        case 3: launch(aggregate_kernel<4, true, true>); break;
        case 4: launch(aggregate_kernel<2, false, false>); break;
        case 5: launch(aggregate_kernel<2, false, true>); break;
        case 6: launch(aggregate_kernel<2, true, false>); break;
        case 7: launch(aggregate_kernel<2, true, true>); break;
        case 8: launch(aggregate_kernel<1, false, false>); break;
        case 9: launch(aggregate_kernel<1, false, true>); break;
        case 10: launch(aggregate_kernel<1, true, false>); break;
        default: launch(aggregate_kernel<1, true, true>); break;
    }
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

extern "C" int cwn_gather_rows_f32(const float* src, int64_t n_src, int64_t F, const int64_t* idx,
                                   int64_t n_idx, float* out, cwn_stream_t stream_) {
    if (F <= 0 || n_idx < 0 || n_src < 0 || F >= INT32_MAX) return CWN_ERR_BAD_ARG;
    if (n_idx == 0) return CWN_OK;
    if (src == nullptr || idx == nullptr || out == nullptr) return CWN_ERR_BAD_ARG;
    if ((((uintptr_t)src) | ((uintptr_t)out)) & 3u) return CWN_ERR_ALIGN;
    int vec = (F % 4 == 0) ? 4 : (F % 2 == 0 ? 2 : 1);
    if (vec == 4 && !(al16(src) && al16(out))) vec = 2;
    if (vec == 2 && !(al8(src) && al8(out))) vec = 1;
    const int G = pick_group((int)F, vec);
    const int rows_per_block = kThreads / G;
    const int64_t blocks = (n_idx + rows_per_block - 1) / rows_per_block;
    if (blocks >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)blocks), block(kThreads);
    if (vec == 4) gather_rows_kernel<4><<<grid, block, 0, stream>>>(src, idx, out, n_idx, (int)F, G);
    else if (vec == 2) gather_rows_kernel<2><<<grid, block, 0, stream>>>(src, idx, out, n_idx, (int)F, G);
    else gather_rows_kernel<1><<<grid, block, 0, stream>>>(src, idx, out, n_idx, (int)F, G);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

extern "C" int cwn_abi_version(void) { return CWN_ABI_VERSION; }

extern "C" const char* cwn_target_arch(void) { return "gfx950"; }

extern "C" const char* cwn_error_string(int code) {
    switch (code) {
        case CWN_OK: return "ok";
        case CWN_ERR_BAD_ARG: return "bad argument";
        case CWN_ERR_TOO_LARGE: return "size does not fit int32";
        case CWN_ERR_WORKSPACE: return "workspace too small";
        case CWN_ERR_LAUNCH: return "kernel launch failed";
        case CWN_ERR_ALIGN: return "pointer misses its alignment (4 bytes; 16 for outputs, weights and packed buffers of the vectorised kernels)";
        default: return "unknown error";
    }
}
