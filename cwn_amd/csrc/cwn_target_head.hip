// cwn_target_head.hip -- the prediction head of a model that reads ONE marked cell per complex instead of a pooled readout:
// RingSparseCIN's `lin1(x[data.nodes.mask])` (mp/ring_exp_models.py:61-64).
//
//   cwn_target_head_f32       out[c, :] = W . x[target_row[c], :] + b                     one launch
//   cwn_target_head_bwd_f32   dx (every row: zeros, dlogits[c] . W on the target rows), dW, db     one launch (two beyond 64 complexes)
//
// torch spells the forward `x[mask]`: a nonzero (a host synchronisation: not capturable) plus an index, then a Linear.  Here
// the rows are numbers the batch carries (ComplexBatch.target_rows), and nothing of x is read but those rows.
//
// Forward: a wave64 per complex.  Lane l holds columns 4l .. 4l + 3 and 256 + 4l .. 256 + 4l + 3 of the one row (two 16-byte
// loads, H <= 512); a W of 16 .. 64 KiB sits in LDS once per workgroup, a smaller one (the ring experiment's 5 x 64) or a
// larger one is read through L2 -- those loads do not wait for the row; per class a dot product and a six-step xor
// reduction, whose result every lane holds -- lane k keeps class k, and the K logits leave as one store per lane.
//
// Backward, one launch of two kinds of workgroups:
//   * row chunks of dx: a workgroup owns 64 consecutive rows and writes every one of them -- zeros, or on a target row
//     sum_k dlogits[c, k] W[k, :].  target_row is ascending (complexes are contiguous in a batch), so the chunk finds its
//     targets by two binary searches (up to 4096 complexes: by one pass of the whole workgroup over target_row, whose loads
//     do not depend on each other); no separate zero fill, no race between a fill and the target rows.
//   * (group of 64 complexes, slab of 64 columns of dW) pairs: the group's rows of x and of dlogits are staged in LDS by
//     the whole workgroup, and thread (k, column quad) adds them ONE AFTER THE OTHER in complex order.  One group (<= 64
//     complexes): straight into dW / db.  More: into the group's slice of a workspace, and a second, tiny launch adds the
//     slices in group order.  No atomics: dW and db have the same bits on every run, and there is no second (ordered) form.
#include <hip/hip_runtime.h>
#include "../../include/cwn_hip.h"
#include "cwn_check.h"
#include "cwn_group.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kFwdBlock = kWaves;                  // complexes per workgroup of the forward: one per wave
constexpr size_t kLdsMin = 16 * 1024;              // a smaller W is read through L2 (no staging pass, no barrier)
constexpr int kScanMax = 4096;                     // complexes up to which a dx chunk scans target_row instead of searching it
constexpr int kChunkRows = 64;                     // rows of dx per workgroup
constexpr int kSlab = 64;                          // columns of dW per workgroup
constexpr int kStage = 64;                         // complexes staged at a time for dW
constexpr size_t kLdsMax = 64 * 1024;              // W beyond it is read from global memory

// floats of one group's slice of the workspace: dW [K, H], then db padded to whole 16-byte vectors
__host__ __device__ __forceinline__ int64_t slice_floats(int32_t H, int32_t K) { return (int64_t)K * H + ((K + 3) & ~3); }

__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }

struct FwdArgs {
    const float* x;
    const int32_t* target_row;
    const float* W;
    const float* bias;
    float* out;
    const int64_t* m_dev;
    int32_t* err;
    int64_t N, C, ldx, ldout;
    int32_t H, K;
};

template <bool kLdsW>
__global__ __launch_bounds__(kThreads) void target_head_kernel(FwdArgs P) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];     // [K][H] when kLdsW
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = P.H, K = P.K, nq = H >> 2;
    const int64_t C = cwn::rows_clamped(P.m_dev, (int64_t)P.C);
    const int64_t c0 = (int64_t)blockIdx.x * kFwdBlock;
    if (c0 >= C) return;                          // (uniform: before any barrier)
    if (kLdsW) {
        const float4* __restrict__ src = reinterpret_cast<const float4*>(P.W);
        float4* dst = reinterpret_cast<float4*>(wlds);
        for (int i = tid; i < K * nq; i += kThreads) dst[i] = src[i];
        __syncthreads();
    }
    const float* __restrict__ Wp = kLdsW ? wlds : P.W;
    const int q0 = lane, q1 = lane + 64;
    const int64_t c = c0 + wave;
    if (c >= C) return;                           // (wave-uniform; behind the only barrier)
    const int64_t t = P.target_row[c];
    const bool ok = t >= 0 && t < P.N;
    // a row outside x, or a row below its predecessor's (the backward's search needs them ascending)
    if (lane == 0 && P.err != nullptr && (!ok || (c > 0 && P.target_row[c - 1] > t))) atomicOr(P.err, 2);
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
    if (ok) {
        const float* __restrict__ row = P.x + t * P.ldx;
        if (q0 < nq) a0 = *reinterpret_cast<const float4*>(row + 4 * q0);
        if (q1 < nq) a1 = *reinterpret_cast<const float4*>(row + 4 * q1);
    }
    float res = 0.f;
    for (int k = 0; k < K; ++k) {
        float p = 0.f;
        if (q0 < nq) p = dot4(a0, *reinterpret_cast<const float4*>(Wp + (int64_t)k * H + 4 * q0));
        if (q1 < nq) p = p + dot4(a1, *reinterpret_cast<const float4*>(Wp + (int64_t)k * H + 4 * q1));
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_xor(p, s, 64);
        if (lane == k) res = p;
    }
    if (lane < K) P.out[c * P.ldout + lane] = P.bias != nullptr ? res + P.bias[lane] : res;
}

struct BwdArgs {
    const float* dl;
    const float* x;
    const int32_t* target_row;
    const float* W;
    float* dx;
    float* dW;          // one group: dW itself; more: the workspace, [group][slice_floats]
    float* db;          // one group: db or NULL; more: unused
    const int64_t* m_dev;
    int64_t N, C, lddl, ldx, lddx;
    int32_t H, K;
    uint32_t dx_blocks;
    int32_t slabs;      // column slabs of dW
    int32_t groups;     // groups of kStage complexes the capacity C has
};

// first c in [0, C) with target_row[c] >= row (C when there is none)
__device__ __forceinline__ int64_t lower_bound(const int32_t* __restrict__ t, int64_t C, int64_t row) {
    int64_t lo = 0, hi = C;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (t[mid] < row) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void target_head_bwd_kernel(BwdArgs P) {
    __shared__ __attribute__((aligned(16))) float xs[kStage * kSlab];     // [complex][column of the slab]
    __shared__ __attribute__((aligned(16))) float dls[kStage * 64];       // [complex][class]
    __shared__ int owner[kChunkRows];                                     // row of the chunk -> its first complex, or -1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = P.H, K = P.K, nq = H >> 2;
    const int64_t C = cwn::rows_clamped(P.m_dev, (int64_t)P.C);
    const int32_t* __restrict__ trow = P.target_row;

    if (blockIdx.x < P.dx_blocks) {
        // ---- 64 rows of dx ---------------------------------------------------------------------------------------------
        const int64_t row0 = (int64_t)blockIdx.x * kChunkRows;
        const int rows = (int)(P.N - row0 < kChunkRows ? P.N - row0 : kChunkRows);
        if (tid < kChunkRows) owner[tid] = -1;
        int64_t c_lo = 0, c_hi = C;
        if (C > kScanMax) {                       // (uniform) the chunk's complexes by two searches, else all of them
            c_lo = lower_bound(trow, C, row0);
            c_hi = lower_bound(trow, C, row0 + rows);
        }
        __syncthreads();
        for (int64_t c = c_lo + tid; c < c_hi; c += kThreads) {
            const int64_t t = trow[c];
            // (the first complex of a run of equal rows; the range check holds whatever the caller's order)
            if (t >= row0 && t < row0 + rows && (c == 0 || trow[c - 1] != t)) owner[t - row0] = (int)c;
        }
        __syncthreads();
        const int q0 = lane, q1 = lane + 64;
        for (int r = wave; r < rows; r += kWaves) {
            const int64_t row = row0 + r;
            float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
            const int first = owner[r];
            if (first >= 0) {                     // (wave-uniform)
                for (int64_t c = first; c < C && trow[c] == row; ++c) {
                    for (int k = 0; k < K; ++k) {
                        const float g = P.dl[c * P.lddl + k];
                        if (q0 < nq) {
                            const float4 w = *reinterpret_cast<const float4*>(P.W + (int64_t)k * H + 4 * q0);
                            a0.x += g * w.x; a0.y += g * w.y; a0.z += g * w.z; a0.w += g * w.w;
                        }
                        if (q1 < nq) {
                            const float4 w = *reinterpret_cast<const float4*>(P.W + (int64_t)k * H + 4 * q1);
                            a1.x += g * w.x; a1.y += g * w.y; a1.z += g * w.z; a1.w += g * w.w;
                        }
                    }
                }
            }
            float* __restrict__ out = P.dx + row * P.lddx;
            if (q0 < nq) *reinterpret_cast<float4*>(out + 4 * q0) = a0;
            if (q1 < nq) *reinterpret_cast<float4*>(out + 4 * q1) = a1;
        }
        return;
    }

    // ---- one group of 64 complexes x one slab of 64 columns of dW (slab 0: db too) -----------------------------------------
    const int item = (int)(blockIdx.x - P.dx_blocks);
    const int group = item / P.slabs, slab = item - group * P.slabs;
    const int col0 = slab * kSlab;
    const int64_t c0 = (int64_t)group * kStage;
    // more than one group: a group past the live count writes nothing (the second launch adds the live groups only)
    if (P.groups > 1 && c0 >= C) return;          // (uniform, before any barrier)
    const int hq = tid & 15, kk = tid >> 4;       // column quad of the slab; classes kk, kk + 16, kk + 32, kk + 48
    const int n = (int)(C - c0 < kStage ? (C - c0 > 0 ? C - c0 : 0) : kStage);
    for (int i = tid; i < kStage * (kSlab / 4); i += kThreads) {
        const int cl = i >> 4, q = i & 15;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cl < n && col0 + 4 * q < H) {
            const int64_t t = trow[c0 + cl];
            if (t >= 0 && t < P.N) v = *reinterpret_cast<const float4*>(P.x + t * P.ldx + col0 + 4 * q);
        }
        *reinterpret_cast<float4*>(xs + cl * kSlab + 4 * q) = v;
    }
    for (int i = tid; i < kStage * K; i += kThreads) {
        const int cl = i / K, k = i - cl * K;
        dls[cl * 64 + k] = cl < n ? P.dl[(c0 + cl) * P.lddl + k] : 0.f;      // (rows past the group: + 0 * 0)
    }
    __syncthreads();
    float4 acc[4];
    float bsum[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        bsum[j] = 0.f;
    }
#pragma unroll 8
    for (int cl = 0; cl < kStage; ++cl) {         // in complex order
        const float4 xv = *reinterpret_cast<const float4*>(xs + cl * kSlab + 4 * hq);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kk + 16 * j;
            if (k < K) {
                const float g = dls[cl * 64 + k];
                acc[j].x += g * xv.x; acc[j].y += g * xv.y; acc[j].z += g * xv.z; acc[j].w += g * xv.w;
                bsum[j] += g;
            }
        }
    }
    float* __restrict__ dW = P.groups > 1 ? P.dW + (int64_t)group * slice_floats(H, K) : P.dW;
    float* __restrict__ db = P.groups > 1 ? dW + (int64_t)K * H : P.db;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = kk + 16 * j;
        if (k >= K) continue;
        if (col0 + 4 * hq < H) *reinterpret_cast<float4*>(dW + (int64_t)k * H + col0 + 4 * hq) = acc[j];
        if (db != nullptr && slab == 0 && hq == 0) db[k] = bsum[j];
    }
}

// dW / db = the live groups' slices of the workspace, added in group order: element e of [K * H + K] per thread
__global__ __launch_bounds__(kThreads) void target_head_sum_kernel(const float* __restrict__ ws, float* __restrict__ dW,
                                                                   float* __restrict__ db, const int64_t* m_dev, int64_t C, int32_t H,
                                                                   int32_t K) {
    const int64_t live = cwn::rows_clamped(m_dev, C);
    const int groups = (int)((live + kStage - 1) / kStage);
    const int64_t per = slice_floats(H, K);
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= per) return;
    float acc = 0.f;
    for (int g = 0; g < groups; ++g) acc += ws[g * per + e];
    if (e < (int64_t)K * H) dW[e] = acc;
    else if (db != nullptr && e - (int64_t)K * H < K) db[e - (int64_t)K * H] = acc;
}

inline int check_shape(int64_t N, int64_t C, int32_t H, int32_t K) {
    if (N < 0 || C < 0 || H < 4 || H > CWN_TARGET_HEAD_MAX_H || (H & 3) != 0 || K < 1 || K > CWN_TARGET_HEAD_MAX_K) return CWN_ERR_BAD_ARG;
    if (N > INT32_MAX || C > INT32_MAX) return CWN_ERR_TOO_LARGE;
    return CWN_OK;
}

inline int64_t groups_of(int64_t C) { return (C + kStage - 1) / kStage; }

}  // namespace

extern "C" int cwn_target_head_f32(const float* x, int64_t N, int64_t ldx, const int32_t* target_row, int64_t C, const float* W,
                                   const float* bias, float* out, int64_t ldout, int32_t H, int32_t K, int32_t* err_flag,
                                   const int64_t* m_dev, cwn_stream_t stream_) {
    const int rc = check_shape(N, C, H, K);
    if (rc != CWN_OK) return rc;
    if (W == nullptr || ldx < H || ldout < K) return CWN_ERR_BAD_ARG;
    if (C > 0 && (target_row == nullptr || out == nullptr || (N > 0 && x == nullptr))) return CWN_ERR_BAD_ARG;
    if (!al16(x) || !al16(W) || (ldx & 3) != 0 || !al4(target_row) || !al4(bias) || !al4(out) || !al4(err_flag) || !al8(m_dev))
        return CWN_ERR_ALIGN;
    if (C == 0) return CWN_OK;
    FwdArgs P{x, target_row, W, bias, out, m_dev, err_flag, N, C, ldx, ldout, H, K};
    const unsigned blocks = (unsigned)((C + kFwdBlock - 1) / kFwdBlock);
    const size_t lds = (size_t)K * (size_t)H * sizeof(float);
    hipStream_t stream = (hipStream_t)stream_;
    if (lds >= kLdsMin && lds <= kLdsMax) target_head_kernel<true><<<dim3(blocks), dim3(kThreads), lds, stream>>>(P);
    else target_head_kernel<false><<<dim3(blocks), dim3(kThreads), 0, stream>>>(P);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

extern "C" size_t cwn_target_head_bwd_workspace_bytes(int64_t C, int32_t H, int32_t K) {
    if (C <= kStage || H < 1 || K < 1) return 0;
    return (size_t)groups_of(C) * (size_t)slice_floats(H, K) * sizeof(float);
}

extern "C" int cwn_target_head_bwd_f32(const float* dlogits, int64_t lddl, const float* x, int64_t N, int64_t ldx,
                                       const int32_t* target_row, int64_t C, const float* W, float* dx, int64_t lddx, float* dW,
                                       float* db, int32_t H, int32_t K, void* workspace, size_t workspace_bytes, const int64_t* m_dev,
                                       cwn_stream_t stream_) {
    const int rc = check_shape(N, C, H, K);
    if (rc != CWN_OK) return rc;
    if (lddl < K || (C > 0 && (dlogits == nullptr || target_row == nullptr))) return CWN_ERR_BAD_ARG;
    if (dx != nullptr && (W == nullptr || lddx < H)) return CWN_ERR_BAD_ARG;
    if (dW != nullptr && (ldx < H || (C > 0 && N > 0 && x == nullptr))) return CWN_ERR_BAD_ARG;
    if (dW == nullptr && db != nullptr) return CWN_ERR_BAD_ARG;
    if (dx != nullptr && ((const float*)dx == x || (const float*)dx == dlogits)) return CWN_ERR_BAD_ARG;
    const size_t need = dW != nullptr ? cwn_target_head_bwd_workspace_bytes(C, H, K) : 0;
    if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return CWN_ERR_WORKSPACE;
    if (!al16(W) || !al16(dx) || (lddx & 3) != 0 || !al16(dW) || !al4(dlogits) || !al4(target_row) || !al4(db) || !al8(m_dev))
        return CWN_ERR_ALIGN;
    if (dW != nullptr && (!al16(x) || (ldx & 3) != 0 || (need > 0 && !al16(workspace)))) return CWN_ERR_ALIGN;
    const int64_t dx_blocks = dx != nullptr ? (N + kChunkRows - 1) / kChunkRows : 0;
    const int64_t slabs = (H + kSlab - 1) / kSlab;
    const int64_t groups = C > kStage ? groups_of(C) : 1;       // (C == 0: one group that writes zeros)
    const int64_t dw_blocks = dW != nullptr ? slabs * groups : 0;
    if (dx_blocks + dw_blocks == 0) return CWN_OK;
    if (dx_blocks + dw_blocks >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    hipStream_t stream = (hipStream_t)stream_;
    BwdArgs P{dlogits, x, target_row, W, dx, groups > 1 ? (float*)workspace : dW, db, m_dev, N, C, lddl, ldx, lddx, H, K,
              (uint32_t)dx_blocks, (int32_t)slabs, (int32_t)groups};
    target_head_bwd_kernel<<<dim3((unsigned)(dx_blocks + dw_blocks)), dim3(kThreads), 0, stream>>>(P);
    if (hipGetLastError() != hipSuccess) return CWN_ERR_LAUNCH;
    if (dW != nullptr && groups > 1) {
        const int64_t per = slice_floats(H, K);
        target_head_sum_kernel<<<dim3((unsigned)((per + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream>>>(
            (const float*)workspace, dW, db, m_dev, C, H, K);
        if (hipGetLastError() != hipSuccess) return CWN_ERR_LAUNCH;
    }
    return CWN_OK;
}
