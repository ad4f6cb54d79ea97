// cwn_gin.hip -- a whole GINConv (torch_geometric's definition, the layer of mp/graph_models.py and of RingGIN,
// mp/ring_exp_models.py:76-130) in inference as ONE launch.  See include/cwn_hip.h, "GINConv as one launch".
//
//   cwn_gin_layer_f32   s   = (sum over the CSR entries of row i, in CSR order, of x[col[p], :]) + (1 + eps) * x[i, :]
//                       h   = act( (s W1^T + b1) * scale1 + shift1 )
//                       out = act_post( act( (h W2^T + b2) * scale2 + shift2 ) )
//
// The layer is deep and tiny in the ring experiment (16 layers over a few hundred rows): as torch modules it is an aggregation,
// two products, two bias adds, two BatchNorms and two activations, whose runtime is launch latency.  A workgroup of four
// wave64s owns CWN_GIN_TM = 32 destination rows:
//   1. every (row, column) of the tile is one work item: it folds the row's entries one after the other in CSR order,
//      whatever the row's length (four entries' loads in flight, added in entry order), adds (1 + eps) * x and writes s into
//      the LDS panel sp[32][132]; columns [w, w rounded up to 16) and rows past n hold zeros.
//   2. sp times W1 on v_mfma_f32_16x16x4_f32 (exact fp32) with the operand roles and K-slab walk of cwn_oriented.hip:
//      A = 16 weight rows (output columns), B = 16 panel rows, K in slabs of 16 in which lane group g = lane >> 4 owns
//      k = 4g .. 4g + 3 -- the panel fragment is one 16-byte LDS read, a lane's four accumulator registers are four
//      consecutive output columns of one row.  Weights come straight from global memory, row-major as torch.nn.Linear
//      holds them (at most 64 KiB a stage: L2-resident), as 16-byte vectors where the width and the alignment allow.
//   3. bias, folded norm and activation in the accumulator layout; h goes to the second panel hp[32][132] (columns [H, H
//      rounded up to 16) as zeros), never to memory.
//   4. hp times W2 likewise, the epilogue with act_post behind it, one 16-byte store per lane and tile where out allows
//      (edge columns and rows past n masked).
// No atomics; every output element is a function of its row's entries in order and the weights alone.
// LDS (static): gin_layer (2 x 32 x 132) elements = 33792 B in float32.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_act.h"
#include "cwn_check.h"

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

// Entries p0 .. p1 - 1 of one row, column c: acc += x[col[p]][c], one after the other (four entries' loads in flight,
// added in entry order).
__device__ __forceinline__ float fold_entries(const float* __restrict__ x, int64_t ldx, int c, const int32_t* __restrict__ col,
                                              int p0, int p1) {
    float acc = 0.f;
    int p = p0;
    for (; p + 3 < p1; p += 4) {
        int j[4];
        float a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) j[u] = col[p + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = x[(int64_t)j[u] * ldx + c];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = acc + a[u];
    }
    for (; p < p1; ++p) acc = acc + x[(int64_t)col[p] * ldx + c];
    return acc;
}

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

__global__ __launch_bounds__(kThreads) void gin_layer_kernel(GinArgs P) {
    __shared__ __attribute__((aligned(16))) float sp[kTM * kLdp];       // s, [kTM][kLdp]
    __shared__ __attribute__((aligned(16))) float hp[kTM * kLdp];       // h
    const int tid = threadIdx.x;
    const int w = P.d.w, H = P.d.H;
    const int kp1 = (w + 15) & ~15, kp2 = (H + 15) & ~15;
    const int64_t ldx = P.d.ldx;
    const float* __restrict__ x = P.d.x;
    const int64_t n = P.d.n;
    const int64_t row0 = (int64_t)blockIdx.x * kTM;
    if (row0 >= n) return;                        // (uniform; the grid has no such workgroup)

    // ---- 1. the panel of s ----------------------------------------------------------------------------------------------
    const int32_t* __restrict__ rowptr = P.d.rowptr;
    const int32_t* __restrict__ col = P.d.col;
    const float self = 1.f + (P.d.eps_dev != nullptr ? *P.d.eps_dev : 0.f);
    const int padc = kp1 - w;
    for (int i = tid; i < kTM * padc; i += kThreads) {
        const int r = i / padc;
        sp[r * kLdp + w + (i - r * padc)] = 0.f;
    }
    for (int i = tid; i < kTM * w; i += kThreads) {
        const int r = i / w, c = i - r * w;
        const int64_t row = row0 + r;
        float v = 0.f;                            // rows past n: zeros in the panel, nothing read, nothing stored
        if (row < n) {
            if (rowptr != nullptr) v = fold_entries(x, ldx, c, col, rowptr[row], rowptr[row + 1]);
            v = v + self * x[row * ldx + c];
        }
        sp[r * kLdp + c] = v;
    }
    __syncthreads();

    // ---- 2. h = act((s W1^T + b1) * scale1 + shift1), into the second panel ------------------------------------------------
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

    // ---- 3. out = act_post(act((h W2^T + b2) * scale2 + shift2)) --------------------------------------------------------------
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
bool overlaps(const cwn_gin_desc& D) {
    if ((const float*)D.out == D.x) return true;
    if (D.ldx != D.ldout) return false;
    const int64_t ld = D.ldx;
    const int64_t delta = ((intptr_t)D.out - (intptr_t)D.x) / (int64_t)sizeof(float);     // out - x, in elements
    if (delta >= D.n * ld || -delta >= D.n * ld) return false;                              // disjoint row ranges
    const int64_t dc = ((delta % ld) + ld) % ld;      // out's first column, counted from x's
    return dc < D.w || ld - dc < D.H;
}

int check(const cwn_gin_desc* desc) {
    if (desc == nullptr) return CWN_ERR_BAD_ARG;
    const cwn_gin_desc& D = *desc;
    if (D.w < 1 || D.w > kMaxWidth || D.H < 1 || D.H > kMaxWidth || D.n < 0) return CWN_ERR_BAD_ARG;
    if (!known_act(D.act) || !known_act(D.act_post)) return CWN_ERR_BAD_ARG;
    if (D.rowptr != nullptr && D.col == nullptr) return CWN_ERR_BAD_ARG;
    if (D.n > 0 && (D.x == nullptr || D.out == nullptr || D.W1 == nullptr || D.W2 == nullptr || D.ldx < D.w || D.ldout < D.H))
        return CWN_ERR_BAD_ARG;
    if (D.n > 0 && overlaps(D)) return CWN_ERR_BAD_ARG;
    const void* ptrs[] = {D.x, D.rowptr, D.col, D.eps_dev, D.W1, D.b1, D.scale1, D.shift1, D.W2, D.b2, D.scale2, D.shift2, D.out};
    for (const void* p : ptrs)
        if (!al4(p)) return CWN_ERR_ALIGN;
    if ((D.n + kTM - 1) / kTM >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    return CWN_OK;
}

}  // namespace

extern "C" int cwn_gin_layer_f32(const cwn_gin_desc* desc, cwn_stream_t stream_) {
    const int rc = check(desc);
    if (rc != CWN_OK) return rc;
    if (desc->n == 0) return CWN_OK;
    GinArgs P{};
    P.d = *desc;
    const cwn_gin_desc& D = P.d;
    P.w1_vec = D.w % 4 == 0 && al16(D.W1);
    P.w2_vec = D.H % 4 == 0 && al16(D.W2);
    P.out_vec = al16(D.out) && D.ldout % 4 == 0;
    const unsigned blocks = (unsigned)((D.n + kTM - 1) / kTM);
    gin_layer_kernel<<<dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream_>>>(P);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}
