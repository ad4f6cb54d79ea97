// cwn_chain_tile.h -- the tile code that cwn_chain_f32.hip (two branches) and cwn_branches_f32.hip (three or four) share, the
// way cwn_gin_tile.h serves GIN and GINE: a workgroup of four wave64s owns 32 rows, a stage is an LDS panel [32][132] times a
// weight straight from global memory on v_mfma_f32_16x16x4_f32 (exact fp32), finished in the accumulator layout and written
// to a panel or to memory.  Operand roles and the K-slab walk are those of cwn_gin_tile.h: A = 16 weight rows (output
// columns), B = 16 panel rows, K in slabs of 16 in which lane group g = lane >> 4 owns k = 4g .. 4g + 3 -- the panel
// fragment is one 16-byte LDS read, a lane's four accumulator registers are four consecutive output columns of one row.
// (Its own product and not that header's: a weight here has a row stride -- the slices of a combine weight -- and the combine
// continues an accumulator.)  Nothing here splits K by anything but the widths: an output element is one chain of products
// in a k order fixed by the widths.  File-local names: include and call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_act.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxWidth = CWN_CHAIN_F32_MAX_WIDTH;
constexpr int kTM = CWN_CHAIN_F32_TM;
constexpr int kLdp = kMaxWidth + 4;               // panel pitch: 16-byte rows, 4 banks apart
constexpr int kRT = kTM / 16;                     // row tiles of a product, all of them on every wave
constexpr int kCT = kMaxWidth / 16 / kWaves;      // column tiles per wave (2)

static_assert(kTM % 16 == 0 && kMaxWidth % (16 * kWaves) == 0, "whole MFMA tiles");

__device__ __forceinline__ int round16(int v) { return (v + 15) & ~15; }

__device__ __forceinline__ void clear(f32x4 (&acc)[kCT][kRT]) {
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct)
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) acc[ct][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc[ct][rt] += panel[rt * 16 + j][0 .. K rounded up to 16) . W[(wave + 4 ct) * 16 + j][0 .. K)^T   (W row-major [N, K], row
// stride ldw; the panel holds zeros in its columns from K on)
__device__ __forceinline__ void product(f32x4 (&acc)[kCT][kRT], const float* panel, const float* __restrict__ W, int ldw, int K,
                                        int N, int wave, int j, int g) {
    const int kp = round16(K), n_tiles = (N + 15) >> 4;
    const bool vec = K % 4 == 0 && ldw % 4 == 0 && ((uintptr_t)W & 15) == 0;      // (uniform)
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
                    const float4 v = *reinterpret_cast<const float4*>(W + (int64_t)n * ldw + kk);
                    wf[ct][0] = v.x; wf[ct][1] = v.y; wf[ct][2] = v.z; wf[ct][3] = v.w;
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (kk + t < K) wf[ct][t] = W[(int64_t)n * ldw + kk + t];
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

// acc[ct][rt][q] = z[rt * 16 + j][(wave + 4 ct) * 16 + 4 g + q] -> panel, finished; the tiles below H rounded up to 16 cover
// those columns once, the ones from H on as zeros (the next product's K slabs read them)
__device__ __forceinline__ void to_panel(float* panel, const f32x4 (&acc)[kCT][kRT], int H, const float* bias, const float* scale,
                                         const float* shift, int act, int wave, int j, int g) {
    const int kp = round16(H);
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) {
        const int n0 = (wave + kWaves * ct) * 16 + 4 * g;
        if (n0 >= kp) continue;
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) {
            f32x4 y;
#pragma unroll
            for (int q = 0; q < 4; ++q) y[q] = n0 + q < H ? epilogue(acc[ct][rt][q], n0 + q, bias, scale, shift, act) : 0.f;
            *reinterpret_cast<f32x4*>(panel + (rt * 16 + j) * kLdp + n0) = y;
        }
    }
}

// rows [row0, row0 + kTM) of x [.., F] (row stride ld) -> panel; rows from n on and columns [F, F rounded up to 16): zeros
__device__ __forceinline__ void load_panel(float* panel, const float* __restrict__ x, int64_t ld, int64_t row0, int64_t n, int F,
                                           int tid) {
    const int kp = round16(F);
    for (int i = tid; i < kTM * kp; i += kThreads) {
        const int r = i / kp, c = i - r * kp;
        panel[r * kLdp + c] = (c < F && row0 + r < n) ? x[(row0 + r) * ld + c] : 0.f;
    }
}

// the last stage: acc, finished, -> rows [row0, row0 + kTM) below n of out [.., H] (row stride ld_out): one 16-byte store per
// lane and tile where out allows, scalar stores otherwise; edge columns and rows from n on masked
__device__ __forceinline__ void to_out(float* __restrict__ out, int64_t ld_out, int64_t row0, int64_t n, const f32x4 (&acc)[kCT][kRT],
                                       int H, const float* bias, const float* scale, const float* shift, int act, int wave, int j,
                                       int g) {
    const bool out_vec = ((uintptr_t)out & 15) == 0 && ld_out % 4 == 0;
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
                y[q] = n0 + q < H ? epilogue(acc[ct][rt][q], n0 + q, bias, scale, shift, act) : 0.f;
            float* p = out + row * ld_out + n0;
            if (out_vec && n0 + 3 < H) {
                *reinterpret_cast<float4*>(p) = make_float4(y[0], y[1], y[2], y[3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (n0 + q < H) p[q] = y[q];
            }
        }
    }
}

}  // namespace
