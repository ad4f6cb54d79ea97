// cwn_layernorm.hip -- torch.nn.LayerNorm((N,)) + ReLU over the rows of [M, N] matrices, forward and backward
// (graph_norm='ln' in update_up_nn / update_boundaries_nn / combine_nn, mp/nn.py:39-47, mp/layers.py:303-325).
//
//   cwn_layernorm_act_f32   out = act((z - mean_row) * rstd_row * gamma + beta)    (+ mean / rstd for the backward)
//   cwn_layernorm_bwd_f32   dz = rstd * (g - mean_N(g) - xhat * mean_N(g * xhat)),  g = dy * [out > 0] * gamma
//                           dbeta = sum_m dyh,  dgamma = sum_m dyh * xhat           (bit-reproducible: no atomics)
//
// LayerNorm is per ROW, so it cannot ride in the per-column prologue / epilogue BatchNorm uses in the GEMMs.  One wave64
// owns a row and keeps it in registers (N <= 1024: at most four float4 per lane), the row reductions are wave-level
// xor trees, a 256-thread workgroup walks a band of 64 rows, and up to CWN_MAX_NORM_DESCS matrices (every dimension and
// branch of a layer's stage) share a launch.  A descriptor whose pointers and strides are 16-byte aligned and whose N is
// a multiple of 4 moves 16 bytes per lane; any other takes the element-wise form -- chosen per descriptor, so one
// launch mixes both.
//
// Row statistics are two-pass in registers: the mean first, then the deviations from it.  The second pass also sums
// the deviations themselves: their mean is what rounding the mean to fp32 lost (for rows around 100 that is up to
// 4e-6, which rstd then multiplies), and taking it out of every deviation costs no extra reduction.  The backward does
// the same with the stored fp32 mean, so both passes see the same xhat.
#include <hip/hip_runtime.h>
#include "../../include/cwn_hip.h"
#include "cwn_check.h"
#include "cwn_act.h"
#include "cwn_group.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBand = 64;                         // rows per workgroup
constexpr int kRowsPerWave = kBand / kWaves;      // 16
constexpr int kMaxN = 1024;

struct LnBatch {
    cwn_ln_desc d[CWN_MAX_NORM_DESCS];
    int64_t ws_off[CWN_MAX_NORM_DESCS];           // backward: first float of the descriptor's [bands, 2, N] partials, -1: none wanted
    int32_t blk_start[CWN_MAX_NORM_DESCS + 1];
    int32_t vec[CWN_MAX_NORM_DESCS];              // 16-byte form
    int32_t n;
};

// A lane holds 4 * C elements of a row of up to 256 * C columns.  VEC: element e is column 4 * (lane + 64 * (e / 4)) + e % 4
// (float4 number lane + 64 j: a wave's load is 1 KiB of consecutive bytes); otherwise column lane + 64 * e.
template <bool VEC>
__device__ __forceinline__ int col_of(int lane, int e) {
    return VEC ? 4 * (lane + 64 * (e >> 2)) + (e & 3) : lane + 64 * e;
}

template <bool VEC, int C>
__device__ __forceinline__ void ld_row(float (&x)[4 * C], const float* __restrict__ p, int lane, int N, float fill) {
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int c = 4 * (lane + 64 * j);
            float4 t = make_float4(fill, fill, fill, fill);
            if (p != nullptr && c < N) t = *reinterpret_cast<const float4*>(p + c);      // (N % 4 == 0: whole vectors)
            x[4 * j] = t.x; x[4 * j + 1] = t.y; x[4 * j + 2] = t.z; x[4 * j + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4 * C; ++e) {
            const int c = lane + 64 * e;
            x[e] = (p != nullptr && c < N) ? p[c] : fill;
        }
    }
}

template <bool VEC, int C>
__device__ __forceinline__ void st_row(float* __restrict__ p, const float (&x)[4 * C], int lane, int N) {
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int c = 4 * (lane + 64 * j);
            if (c < N) *reinterpret_cast<float4*>(p + c) = make_float4(x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4 * C; ++e) {
            const int c = lane + 64 * e;
            if (c < N) p[c] = x[e];
        }
    }
}

// every lane gets the sum over the wave, in the same order for every row
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---- forward ------------------------------------------------------------------------------------------------------------
template <bool VEC, int C>
__device__ __forceinline__ void fwd_band(const cwn_ln_desc& D, int64_t row0, int64_t Mv) {
    constexpr int R = C == 1 ? 8 : (C == 2 ? 4 : 2);      // rows whose loads a wave has in flight together
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = D.N;
    const float fN = (float)N;                             // (divisions, not a reciprocal: a sum that is exact stays exact)
    const bool relu = D.relu != 0;
    float gm[4 * C], bt[4 * C];
    ld_row<VEC, C>(gm, D.gamma, lane, N, 1.0f);
    ld_row<VEC, C>(bt, D.beta, lane, N, 0.0f);
    for (int i0 = 0; i0 < kRowsPerWave; i0 += R) {
        float x[R][4 * C];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int64_t r = row0 + wave + kWaves * (i0 + q);
            ld_row<VEC, C>(x[q], r < Mv ? D.z + r * D.ldz : nullptr, lane, N, 0.0f);
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int64_t r = row0 + wave + kWaves * (i0 + q);
            if (r >= Mv) continue;                         // (wave-uniform)
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 4 * C; ++e) s += x[q][e];  // (columns >= N hold 0)
            float mean = wave_sum(s) / fN;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int e = 0; e < 4 * C; ++e) {
                const float d = col_of<VEC>(lane, e) < N ? x[q][e] - mean : 0.f;
                x[q][e] = d;
                s1 += d;
                s2 += d * d;
            }
            s1 = wave_sum(s1);
            s2 = wave_sum(s2);
            // the mean of the deviations is what the fp32 mean lost: sum (d - c)^2 = sum d^2 - N c^2 with c of the order of
            // one ulp of the mean (a correction of the two-pass variance, not E[x^2] - mean^2)
            const float c = s1 / fN;
            float var = s2 / fN - c * c;
            var = var < 0.f ? 0.f : var;              // (a NaN variance stays NaN)
            mean += c;
            const float rstd = 1.0f / sqrtf(var + D.eps);
            float o[4 * C];
#pragma unroll
            for (int e = 0; e < 4 * C; ++e) {
                const float y = (x[q][e] - c) * rstd * gm[e] + bt[e];
                o[e] = relu ? cwn_relu(y) : y;
            }
            st_row<VEC, C>(D.out + r * D.ldout, o, lane, N);
            if (lane == 0 && D.mean != nullptr) D.mean[r] = mean;
            if (lane == 0 && D.rstd != nullptr) D.rstd[r] = rstd;
        }
    }
}

__global__ __launch_bounds__(kThreads) void layernorm_act_kernel(LnBatch B) {
    const int di = cwn::group_of<CWN_MAX_NORM_DESCS>(B.blk_start, B.n, (int)blockIdx.x);
    const cwn_ln_desc& D = B.d[di];
    const int64_t row0 = (int64_t)((int)blockIdx.x - B.blk_start[di]) * kBand;
    const int64_t Mv = cwn::rows_capped(D.m_dev, D.M);
    if (row0 >= Mv) return;
    const int C = (D.N + 255) >> 8;
    if (B.vec[di]) {
        switch (C) {
            case 1: fwd_band<true, 1>(D, row0, Mv); break;
            case 2: fwd_band<true, 2>(D, row0, Mv); break;
            case 3: fwd_band<true, 3>(D, row0, Mv); break;
            default: fwd_band<true, 4>(D, row0, Mv); break;
        }
    } else {
        switch (C) {
            case 1: fwd_band<false, 1>(D, row0, Mv); break;
            case 2: fwd_band<false, 2>(D, row0, Mv); break;
            case 3: fwd_band<false, 3>(D, row0, Mv); break;
            default: fwd_band<false, 4>(D, row0, Mv); break;
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// A lane holds the same columns for every row its wave takes: dbeta / dgamma accumulate in registers over the band, the
// four waves meet in LDS and are summed in wave order, and the workgroup stores one [2, N] partial with plain stores.
template <bool VEC, int C>
__device__ __forceinline__ void bwd_band(const cwn_ln_desc& D, int64_t row0, int64_t Mv, float* __restrict__ part,
                                         float (*red)[2][kMaxN]) {
    constexpr int R = C == 1 ? 4 : (C == 2 ? 2 : 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = D.N;
    const float fN = (float)N;                             // (divisions, not a reciprocal: a sum that is exact stays exact)
    const bool relu = D.relu != 0;
    float gm[4 * C], adb[4 * C], adg[4 * C];
    ld_row<VEC, C>(gm, D.gamma, lane, N, 1.0f);
#pragma unroll
    for (int e = 0; e < 4 * C; ++e) adb[e] = adg[e] = 0.f;
    for (int i0 = 0; i0 < kRowsPerWave; i0 += R) {
        float z[R][4 * C], g[R][4 * C], o[R][4 * C], mu[R], rs[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int64_t r = row0 + wave + kWaves * (i0 + q);
            const bool ok = r < Mv;
            ld_row<VEC, C>(z[q], ok ? D.z + r * D.ldz : nullptr, lane, N, 0.0f);
            ld_row<VEC, C>(g[q], ok ? D.dy + r * D.lddy : nullptr, lane, N, 0.0f);
            ld_row<VEC, C>(o[q], ok && relu ? D.out + r * D.ldout : nullptr, lane, N, 1.0f);
            mu[q] = ok ? D.mean[r] : 0.f;
            rs[q] = ok ? D.rstd[r] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int64_t r = row0 + wave + kWaves * (i0 + q);
            if (r >= Mv) continue;                         // (wave-uniform)
            float sd = 0.f, sg = 0.f, sgd = 0.f;
#pragma unroll
            for (int e = 0; e < 4 * C; ++e) {
                const float dyh = o[q][e] > 0.f ? g[q][e] : 0.f;          // (relu == 0: o holds 1; columns >= N: dy holds 0)
                const float d = col_of<VEC>(lane, e) < N ? z[q][e] - mu[q] : 0.f;
                const float gg = dyh * gm[e];
                o[q][e] = dyh;
                z[q][e] = d;
                g[q][e] = gg;
                sd += d;
                sg += gg;
                sgd += gg * d;
            }
            sd = wave_sum(sd);
            sg = wave_sum(sg);
            sgd = wave_sum(sgd);
            // xhat = (d - c) * rstd with c the mean of the deviations (see the forward), so
            // mean_N(g * xhat) = rstd * (sum g d - c sum g) / N
            const float c = sd / fN, rstd = rs[q];
            const float k1 = sg / fN;
            const float k2 = rstd * (sgd - c * sg) / fN;
            float dz[4 * C];
#pragma unroll
            for (int e = 0; e < 4 * C; ++e) {
                const float xhat = col_of<VEC>(lane, e) < N ? (z[q][e] - c) * rstd : 0.f;
                dz[e] = rstd * (g[q][e] - k1 - xhat * k2);
                adb[e] += o[q][e];
                adg[e] += o[q][e] * xhat;
            }
            st_row<VEC, C>(D.dz + r * D.lddz, dz, lane, N);
        }
    }
    if (part == nullptr) return;                           // (uniform: neither dgamma nor dbeta is wanted)
#pragma unroll
    for (int e = 0; e < 4 * C; ++e) {
        const int c = col_of<VEC>(lane, e);
        if (c < N) {
            red[wave][0][c] = adb[e];
            red[wave][1][c] = adg[e];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < N; c += kThreads) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            t1 += red[w][0][c];
            t2 += red[w][1][c];
        }
        part[c] = t1;
        part[N + c] = t2;
    }
}

__global__ __launch_bounds__(kThreads) void layernorm_bwd_kernel(LnBatch B, float* __restrict__ ws) {
    __shared__ float red[kWaves][2][kMaxN];
    const int di = cwn::group_of<CWN_MAX_NORM_DESCS>(B.blk_start, B.n, (int)blockIdx.x);
    const cwn_ln_desc& D = B.d[di];
    const int64_t band = (int)blockIdx.x - B.blk_start[di];
    const int64_t row0 = band * kBand;
    const int64_t Mv = cwn::rows_capped(D.m_dev, D.M);
    if (row0 >= Mv) return;                                // (the sums kernel walks the bands below the count only)
    float* part = B.ws_off[di] >= 0 ? ws + B.ws_off[di] + band * 2 * D.N : nullptr;
    const int C = (D.N + 255) >> 8;
    if (B.vec[di]) {
        switch (C) {
            case 1: bwd_band<true, 1>(D, row0, Mv, part, red); break;
            case 2: bwd_band<true, 2>(D, row0, Mv, part, red); break;
            case 3: bwd_band<true, 3>(D, row0, Mv, part, red); break;
            default: bwd_band<true, 4>(D, row0, Mv, part, red); break;
        }
    } else {
        switch (C) {
            case 1: bwd_band<false, 1>(D, row0, Mv, part, red); break;
            case 2: bwd_band<false, 2>(D, row0, Mv, part, red); break;
            case 3: bwd_band<false, 3>(D, row0, Mv, part, red); break;
            default: bwd_band<false, 4>(D, row0, Mv, part, red); break;
        }
    }
}

// grid (column chunk of 256, descriptor): a thread owns a column and adds the workgroups' partials in workgroup order
__global__ __launch_bounds__(kThreads) void layernorm_bwd_sums_kernel(LnBatch B, const float* __restrict__ ws) {
    const cwn_ln_desc& D = B.d[blockIdx.y];
    const int c = blockIdx.x * kThreads + threadIdx.x;
    const int N = D.N;
    if (c >= N || B.ws_off[blockIdx.y] < 0) return;
    const int64_t Mv = cwn::rows_capped(D.m_dev, D.M);
    const int64_t bands = Mv > 0 ? (Mv + kBand - 1) / kBand : 0;
    const float* p = ws + B.ws_off[blockIdx.y] + c;
    float s1 = 0.f, s2 = 0.f;
    int64_t b = 0;
    for (; b + 4 <= bands; b += 4) {                       // four bands' loads in flight, added in band order
        float t1[4], t2[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            t1[u] = p[(b + u) * 2 * N];
            t2[u] = p[(b + u) * 2 * N + N];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s1 += t1[u];
            s2 += t2[u];
        }
    }
    for (; b < bands; ++b) {
        s1 += p[b * 2 * N];
        s2 += p[b * 2 * N + N];
    }
    if (D.dbeta != nullptr) D.dbeta[c] = D.accumulate ? D.dbeta[c] + s1 : s1;
    if (D.dgamma != nullptr) D.dgamma[c] = D.accumulate ? D.dgamma[c] + s2 : s2;
}

inline int64_t bands_of(int64_t M) { return (M + kBand - 1) / kBand; }

// Checks the descriptors and fills the launch record; `bwd`: the backward's operands.  *ws_floats: the partials' size.
int prepare(const cwn_ln_desc* descs, int n, bool bwd, LnBatch& B, int64_t* blocks_out, int64_t* ws_floats) {
    if (descs == nullptr || n <= 0 || n > CWN_MAX_NORM_DESCS) return CWN_ERR_BAD_ARG;
    B.n = n;
    cwn::BlockFill fill(B.blk_start);
    int64_t ws = 0;
    for (int i = 0; i < n; ++i) {
        const cwn_ln_desc& D = descs[i];
        if (D.M < 0 || D.N < 1 || D.N > kMaxN) return CWN_ERR_BAD_ARG;
        if (D.M > 0) {
            if (D.z == nullptr || D.ldz < D.N || D.out == nullptr || D.ldout < D.N) return CWN_ERR_BAD_ARG;
            if (!bwd && D.out == D.z) return CWN_ERR_BAD_ARG;
            if (bwd && (D.dy == nullptr || D.lddy < D.N || D.dz == nullptr || D.lddz < D.N || D.mean == nullptr ||
                        D.rstd == nullptr || D.dz == D.z))
                return CWN_ERR_BAD_ARG;
        }
        const void* ptrs[] = {D.z, D.gamma, D.beta, D.out, D.mean, D.rstd, D.dy, D.dz, D.dgamma, D.dbeta};
        for (const void* p : ptrs)
            if (!al4(p)) return CWN_ERR_ALIGN;
        if (D.m_dev != nullptr && ((uintptr_t)D.m_dev & 7u)) return CWN_ERR_ALIGN;
        bool vec = D.N % 4 == 0 && al16(D.z) && al16(D.out) && al16(D.gamma) && D.ldz % 4 == 0 && D.ldout % 4 == 0;
        if (bwd) vec = vec && al16(D.dy) && al16(D.dz) && D.lddy % 4 == 0 && D.lddz % 4 == 0;
        else vec = vec && al16(D.beta);
        B.d[i] = D;
        B.vec[i] = vec ? 1 : 0;
        if (!fill.push(i, bands_of(D.M))) return CWN_ERR_TOO_LARGE;
        B.ws_off[i] = -1;
        if (bwd && (D.dgamma != nullptr || D.dbeta != nullptr)) {
            B.ws_off[i] = ws;
            ws += bands_of(D.M) * 2 * D.N;
        }
    }
    *blocks_out = fill.close(n);
    *ws_floats = ws;
    return CWN_OK;
}

}  // namespace

extern "C" int cwn_layernorm_act_f32(const cwn_ln_desc* descs, int n, cwn_stream_t stream_) {
    LnBatch B{};
    int64_t blocks = 0, ws = 0;
    const int rc = prepare(descs, n, false, B, &blocks, &ws);
    if (rc != CWN_OK) return rc;
    if (blocks == 0) return CWN_OK;
    layernorm_act_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_>>>(B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

extern "C" size_t cwn_layernorm_bwd_workspace_bytes(const cwn_ln_desc* descs, int n) {
    LnBatch B{};
    int64_t blocks = 0, ws = 0;
    if (prepare(descs, n, true, B, &blocks, &ws) != CWN_OK) return 0;
    return (size_t)ws * sizeof(float);
}

extern "C" int cwn_layernorm_bwd_f32(const cwn_ln_desc* descs, int n, void* workspace, size_t workspace_bytes,
                                     cwn_stream_t stream_) {
    LnBatch B{};
    int64_t blocks = 0, ws = 0;
    const int rc = prepare(descs, n, true, B, &blocks, &ws);
    if (rc != CWN_OK) return rc;
    if (ws > 0 && (workspace == nullptr || workspace_bytes < (size_t)ws * sizeof(float))) return CWN_ERR_BAD_ARG;
    if (!al4(workspace)) return CWN_ERR_ALIGN;
    hipStream_t stream = (hipStream_t)stream_;
    if (blocks > 0) {
        layernorm_bwd_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(B, (float*)workspace);
        if (hipGetLastError() != hipSuccess) return CWN_ERR_LAUNCH;
    }
    bool sums = false;
    int nmax = 0;
    for (int i = 0; i < n; ++i) {
        if (B.ws_off[i] < 0) continue;
        sums = true;
        nmax = descs[i].N > nmax ? descs[i].N : nmax;
    }
    if (sums) {
        layernorm_bwd_sums_kernel<<<dim3((nmax + kThreads - 1) / kThreads, n), dim3(kThreads), 0, stream>>>(
            B, (const float*)workspace);
        if (hipGetLastError() != hipSuccess) return CWN_ERR_LAUNCH;
    }
    return CWN_OK;
}
