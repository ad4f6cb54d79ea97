// cwn_gin_tile.h -- what the one-launch GIN layers share behind their aggregation: gin_layer_kernel (cwn_gin.hip, the sum of
// x[col[p]]) and gine_layer_kernel (cwn_gine.hip, the sum of relu(x[col[p]] + e[eidx[p]])) differ in how a (row, column) work
// item folds its row's entries, and in nothing else.  Written once here: the geometry (256 threads, CWN_GIN_TM rows, two LDS
// panels at pitch CWN_GIN_MAX_WIDTH + 4), the panel's zero padding, the exact-fp32 MFMA product, the epilogue, the two
// stages that turn the panel of s into out, the launch flags, and the host-side argument and alias checks of a cwn_gin_desc.
// File-local names, as in cwn_act.h and cwn_check.h: include and call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_act.h"
#include "cwn_check.h"
#include "cwn_group.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxWidth = CWN_GIN_MAX_WIDTH;
constexpr int kTM = CWN_GIN_TM;
constexpr int kLdp = kMaxWidth + 4;               // panel pitch: 16-byte rows, 4 banks apart
constexpr int kRT = kTM / 16;                     // row tiles of a product, all of them on every wave
constexpr int kCT = kMaxWidth / 16 / kWaves;      // column tiles per wave (2)

static_assert(kTM % 16 == 0 && kMaxWidth % (16 * kWaves) == 0, "whole MFMA tiles");

struct GinArgs {
    cwn_gin_desc d;
    int32_t w1_vec;      // W1 readable as 16-byte vectors along k (w % 4 == 0, aligned)
    int32_t w2_vec;      // W2 likewise (H % 4 == 0, aligned)
    int32_t out_vec;     // out rows take 16-byte stores
};

// acc[ct][rt] += panel[rt * 16 + j][0 .. kp) . W[(wave + 4 ct) * 16 + j][0 .. K)^T   (W row-major [N, K], row stride K)
__device__ __forceinline__ void product(f32x4 (&acc)[kCT][kRT], const float* panel, const float* __restrict__ W, int K, int kp,
                                        int N, bool vec, int wave, int j, int g) {
    const int n_tiles = (N + 15) >> 4;
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct)
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) acc[ct][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kp; k0 += 16) {
        const int kk = k0 + 4 * g;                // this lane group's four k of the slab
        float wf[kCT][4];
#pragma unroll
        for (int ct = 0; ct < kCT; ++ct) {
            const int n = (wave + kWaves * ct) * 16 + j;
#pragma unroll
            for (int t = 0; t < 4; ++t) wf[ct][t] = 0.f;
            if (n >= N) continue;
            if (vec) {                            // (K % 4 == 0: the four k are inside the row or all beyond it)
                if (kk < K) {
                    const float4 v = *reinterpret_cast<const float4*>(W + (int64_t)n * K + kk);
                    wf[ct][0] = v.x; wf[ct][1] = v.y; wf[ct][2] = v.z; wf[ct][3] = v.w;
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (kk + t < K) wf[ct][t] = W[(int64_t)n * K + kk + t];
            }
        }
        f32x4 xb[kRT];
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) xb[rt] = *reinterpret_cast<const f32x4*>(panel + (rt * 16 + j) * kLdp + kk);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int ct = 0; ct < kCT; ++ct) {
                if (wave + kWaves * ct >= n_tiles) continue;          // (wave-uniform)
#pragma unroll
                for (int rt = 0; rt < kRT; ++rt)
                    acc[ct][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ct][t], xb[rt][t], acc[ct][rt], 0, 0, 0);
            }
    }
}

// act((z + bias) * scale + shift) of one output column (an absent operand is skipped, not multiplied by one)
__device__ __forceinline__ float epilogue(float z, int n, const float* __restrict__ bias, const float* __restrict__ scale,
                                          const float* __restrict__ shift, int act) {
    if (bias != nullptr) z = z + bias[n];
    if (scale != nullptr) z = z * scale[n];
    if (shift != nullptr) z = z + shift[n];
    return activate_rt(z, act);
}

// Columns [w, w rounded up to 16) of the panel of s: zeros (the product's K slabs read them).
__device__ __forceinline__ void zero_panel_padding(float* sp, int w, int kp1, int tid) {
    const int padc = kp1 - w;
    for (int i = tid; i < kTM * padc; i += kThreads) {
        const int r = i / padc;
        sp[r * kLdp + w + (i - r * padc)] = 0.f;
    }
}

// The rows of a launch that exist: the host count d.n, or with a device count (the counted entries, cwn_gin_layer_dev_f32 /
// cwn_gine_layer_dev_f32: d.n is then the CAPACITY that sized the grid) that count clamped to [0, d.n].  Read once per
// workgroup, before anything else; every row test of the fold and of stages_from_panel is against it.
__device__ __forceinline__ int64_t live_rows(const GinArgs& P, const int64_t* __restrict__ n_dev) {
    return cwn::rows_clamped(n_dev, P.d.n);
}

// The two stages behind the panel of s (complete in sp, the workgroup synchronised): h = act((s W1^T + b1) * scale1 + shift1)
// into hp, out = act_post(act((h W2^T + b2) * scale2 + shift2)) to memory, rows below `n` (live_rows) alone.
__device__ __forceinline__ void stages_from_panel(const GinArgs& P, const float* sp, float* hp, int64_t row0, int64_t n, int tid) {
    const int w = P.d.w, H = P.d.H;
    const int kp1 = (w + 15) & ~15, kp2 = (H + 15) & ~15;
    const int lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int act = P.d.act;
    f32x4 acc[kCT][kRT];
    product(acc, sp, P.d.W1, w, kp1, H, P.w1_vec != 0, wave, j, g);
    // acc[ct][rt][q] = z[row0 + rt * 16 + j][(wave + 4 ct) * 16 + 4 g + q]; the tiles below kp2 cover columns [0, kp2) once
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) {
        const int n0 = (wave + kWaves * ct) * 16 + 4 * g;
        if (n0 >= kp2) continue;
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) {
            f32x4 y;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                y[q] = n0 + q < H ? epilogue(acc[ct][rt][q], n0 + q, P.d.b1, P.d.scale1, P.d.shift1, act) : 0.f;
            *reinterpret_cast<f32x4*>(hp + (rt * 16 + j) * kLdp + n0) = y;
        }
    }
    __syncthreads();

    product(acc, hp, P.d.W2, H, kp2, H, P.w2_vec != 0, wave, j, g);
    const int act_post = P.d.act_post;
    float* __restrict__ out = P.d.out;
    const int64_t ldout = P.d.ldout;
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) {
        const int n0 = (wave + kWaves * ct) * 16 + 4 * g;
        if (n0 >= H) continue;
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) {
            const int64_t row = row0 + rt * 16 + j;
            if (row >= n) continue;
            float y[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                y[q] = n0 + q < H ? activate_rt(epilogue(acc[ct][rt][q], n0 + q, P.d.b2, P.d.scale2, P.d.shift2, act), act_post)
                                  : 0.f;
            float* p = out + row * ldout + n0;
            if (P.out_vec && n0 + 3 < H) {
                *reinterpret_cast<float4*>(p) = make_float4(y[0], y[1], y[2], y[3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (n0 + q < H) p[q] = y[q];
            }
        }
    }
}

// Do the elements of out [n, H] (stride ldout) and of x [n, w] (stride ldx) share an address?  Equal base pointers always;
// with one common row stride -- two column slices of one buffer -- when their column ranges meet.
inline bool gin_overlaps(const cwn_gin_desc& D) {
    if ((const float*)D.out == D.x) return true;
    if (D.ldx != D.ldout) return false;
    const int64_t ld = D.ldx;
    const int64_t delta = ((intptr_t)D.out - (intptr_t)D.x) / (int64_t)sizeof(float);     // out - x, in elements
    if (delta >= D.n * ld || -delta >= D.n * ld) return false;                              // disjoint row ranges
    const int64_t dc = ((delta % ld) + ld) % ld;      // out's first column, counted from x's
    return dc < D.w || ld - dc < D.H;
}

// The argument checks of a cwn_gin_desc (include/cwn_hip.h, "GINConv as one launch"), before any HIP call.
inline int gin_check(const cwn_gin_desc* desc) {
    if (desc == nullptr) return CWN_ERR_BAD_ARG;
    const cwn_gin_desc& D = *desc;
    if (D.w < 1 || D.w > kMaxWidth || D.H < 1 || D.H > kMaxWidth || D.n < 0) return CWN_ERR_BAD_ARG;
    if (!known_act(D.act) || !known_act(D.act_post)) return CWN_ERR_BAD_ARG;
    if (D.rowptr != nullptr && D.col == nullptr) return CWN_ERR_BAD_ARG;
    if (D.n > 0 && (D.x == nullptr || D.out == nullptr || D.W1 == nullptr || D.W2 == nullptr || D.ldx < D.w || D.ldout < D.H))
        return CWN_ERR_BAD_ARG;
    if (D.n > 0 && gin_overlaps(D)) return CWN_ERR_BAD_ARG;
    const void* ptrs[] = {D.x, D.rowptr, D.col, D.eps_dev, D.W1, D.b1, D.scale1, D.shift1, D.W2, D.b2, D.scale2, D.shift2, D.out};
    for (const void* p : ptrs)
        if (!al4(p)) return CWN_ERR_ALIGN;
    if ((D.n + kTM - 1) / kTM >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    return CWN_OK;
}

// The device count of a counted entry, behind the descriptor's own checks: required where there are rows, 8-byte aligned.
inline int gin_count_check(int64_t n, const int64_t* n_dev) {
    if (n > 0 && n_dev == nullptr) return CWN_ERR_BAD_ARG;
    if (((uintptr_t)n_dev & 7) != 0) return CWN_ERR_ALIGN;
    return CWN_OK;
}

// The kernel's arguments from a checked descriptor, and its grid.
inline GinArgs gin_args(const cwn_gin_desc& D) {
    GinArgs P{};
    P.d = D;
    P.w1_vec = D.w % 4 == 0 && al16(D.W1);
    P.w2_vec = D.H % 4 == 0 && al16(D.W2);
    P.out_vec = al16(D.out) && D.ldout % 4 == 0;
    return P;
}
inline unsigned gin_blocks(const cwn_gin_desc& D) { return (unsigned)((D.n + kTM - 1) / kTM); }

}  // namespace
