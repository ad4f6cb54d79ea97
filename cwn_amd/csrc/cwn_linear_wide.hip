// cwn_linear_wide.hip -- a Linear product beyond cwn_gemm_f32's K, under a device-side row count:
//
//   cwn_linear_wide_f32   Y = [X | X2] W^T + bias     (W [N, K + K2], torch Linear layout)
//                         Y = [X | X2] W   + bias     (w_trans: W [K + K2, N], dX = dY W from the layer's own weight)
//                         1 <= N <= 256, K >= 1, K2 >= 0, K + K2 <= 512         up to CWN_MAX_DESCS products per launch
//
// cwn_gemm_f32 (cwn_gemm.hip) keeps the weight fragments of the WHOLE K in registers, which caps it at K + K2 <= 256: the
// combine network of a 160-wide layer (Linear(320 -> 160), the reference's CSL configuration) went to torch.cat + rocBLAS,
// which knows nothing of a static batch's row count.  This file is the product with K STREAMED.  See include/cwn_hip.h,
// "A wide Linear product under a row count".
//
// * A workgroup of four wave64s owns a 32-row x 128-column tile of one descriptor (N > 128: two column tiles): wave w
//   multiplies the columns [32w, 32w + 32) of the tile (2 x 2 tiles of v_mfma_f32_16x16x4_f32, 16 accumulator registers); a
//   wave whose columns lie at or beyond N stages operands and multiplies nothing.  A tile whose first row is at or beyond the
//   count ends before its first load; the tile the count ends in stores its rows below the count only.
// * The product is cwn_gemm_f32's exact form, element for element: A = 16 weight rows (output columns), B = 16 rows of X, K in
//   slabs of 16 ASCENDING, inside a slab lane group g = lane >> 4 owns k = 4g .. 4g + 3 and MFMA step t multiplies
//   component t; one accumulator chain per output element, the bias added last.  Columns of a slab at or beyond K + K2
//   are zeros in both operands, slabs that begin there are skipped.  A row's bits depend on its own operands alone: not on
//   M, the count, its position in the batch or its neighbours -- and at K + K2 <= 256 they are cwn_gemm_f32's (CWN_GEMM_EXACT).
// * NOTHING IS STATIONARY: K is walked in chunks of 64; a chunk of W and of the tile's rows of X goes global -> registers
//   -> LDS, the next chunk's loads are in flight during the MFMAs.  X and the natural W ([128 n][64 k]) are stored
//   XOR-swizzled (16-byte chunk ^ (row & 15)): every fragment is one conflict-free ds_read_b128.  The transposed W is staged
//   as it lies in memory ([64 k][128 n], rows padded to 132 floats) and its fragments are lifted with 4-byte reads: the
//   16 lanes of a lane group walk consecutive words, the four groups land 16 banks apart.
// * Global reads are row-contiguous, 16 bytes wide where pointer, stride and widths allow, element by element otherwise --
//   decided per operand (X / X2, W, Y) and descriptor on the host.  Rows at or beyond M are never addressed (clamped to
//   M - 1); rows in [count, M) are loaded -- they lie inside the buffer -- and may hold anything, NaN included: a row of X
//   only reaches its own row of Y, which is not stored.
// LDS (static): natural W (128 + 32) x 64 floats = 40960 B; transposed W 64 x 132 + 32 x 64 floats = 41984 B
// (CWN_LINEAR_WIDE_LDS_BYTES).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_mem.h"
#include "cwn_check.h"
#include "cwn_group.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kBM = 32;                   // rows of a tile
constexpr int kBN = 128;                  // columns of a tile
constexpr int kKC = 64;                   // k per LDS chunk
constexpr int kCPR = kKC / 4;             // 16-byte chunks per LDS row of X and of the natural W
constexpr int kRS = kBN + 4;              // LDS row stride of the transposed W, in floats
constexpr int kWU = kBN * kKC / 4 / kThreads;   // 16-byte pieces of a W chunk per thread (8), either layout
constexpr int kXU = kBM * kCPR / kThreads;      // ... of an X chunk (2)
constexpr int CT = 2, RT = 2;             // 16-column / 16-row MFMA tiles per wave

static_assert(kBN == 4 * 16 * CT && kBM == 16 * RT, "four waves side by side cover the tile");
static_assert((kBN * kKC > kKC * kRS ? kBN * kKC : kKC * kRS) * 4 + kBM * kKC * 4 <= CWN_LINEAR_WIDE_LDS_BYTES, "the stated LDS budget");

enum { kVecX = 1, kVecW = 2, kVecY = 4 };    // 16-byte accesses allowed (host-checked), per operand

struct WideBatch {
    cwn_linear_wide_desc d[CWN_MAX_DESCS];
    int32_t blk_start[CWN_MAX_DESCS + 1];    // first workgroup of each descriptor
    int32_t vec[CWN_MAX_DESCS];
    int32_t n;
};

__device__ __forceinline__ int lds_off(int row, int chunk) {   // in floats
    return row * kKC + ((chunk ^ (row & 15)) << 2);
}

struct Chunk {
    f32x4 w[kWU];
    f32x4 x[kXU];
};

// what the staging of a chunk reads: a descriptor's operands in registers
struct Src {
    const float *X, *X2, *W;
    int64_t ldx, ldx2, ldw, M, m_base;
    int N, K1, Ktot, n_tile, vec;            // n_tile: the tile's first output column
};

// The tile's 32 rows of X: a thread's piece is the 16-byte column c = tid & 15 of the rows (tid >> 4) + 16 u.
__device__ __forceinline__ void load_x(const Src& S, Chunk& ch, int k0) {
    const int sr = threadIdx.x >> 4, c = threadIdx.x & 15;
    const int k = k0 + 4 * c, Ktot = S.Ktot, K1 = S.K1;
#pragma unroll
    for (int u = 0; u < kXU; ++u) {
        const int r = sr + 16 * u;
        const int64_t grow = S.m_base + r < S.M ? S.m_base + r : S.M - 1;    // clamped: never outside the buffer
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (S.vec & kVecX) {             // K1 % 4 == 0 and K2 % 4 == 0: the piece lies in one operand
            const bool in = k < Ktot, second = in && k >= K1;
            const float* p = second ? S.X2 + grow * S.ldx2 + (k - K1) : S.X + grow * S.ldx + (in ? k : 0);
            const f32x4 ld = *reinterpret_cast<const f32x4*>(p);
            if (in) v = ld;
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int kt = k + t;
                const bool in = kt < Ktot, second = in && kt >= K1;
                const float ld = second ? S.X2[grow * S.ldx2 + (kt - K1)] : S.X[grow * S.ldx + (in ? kt : 0)];
                if (in) v[t] = ld;
            }
        }
        ch.x[u] = v;
    }
}

// The tile's chunk of W.  Natural layout: the 16-byte column c of the W rows n_tile + (tid >> 4) + 16 u.  Transposed: the
// 16-byte column c = tid & 31 (output columns n_tile + 4c ..) of the W rows k0 + (tid >> 5) + 8 u.
template <bool WT>
__device__ __forceinline__ void load_w(const Src& S, Chunk& ch, int k0) {
    const int Ktot = S.Ktot, N = S.N;
    if constexpr (WT) {
        const int sr = threadIdx.x >> 5, c = threadIdx.x & 31;
        const int n0 = S.n_tile + 4 * c;
#pragma unroll
        for (int u = 0; u < kWU; ++u) {
            const int k = k0 + sr + 8 * u;
            const float* row = S.W + (int64_t)(k < Ktot ? k : 0) * S.ldw;
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (S.vec & kVecW) {         // N % 4 == 0: the piece lies below N or at / beyond it as a whole
                const bool in = k < Ktot && n0 < N;
                const f32x4 ld = *reinterpret_cast<const f32x4*>(row + (n0 < N ? n0 : 0));
                if (in) v = ld;
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const bool in = k < Ktot && n0 + t < N;
                    const float ld = row[n0 + t < N ? n0 + t : 0];
                    if (in) v[t] = ld;
                }
            }
            ch.w[u] = v;
        }
    } else {
        const int sr = threadIdx.x >> 4, c = threadIdx.x & 15;
        const int k = k0 + 4 * c;
#pragma unroll
        for (int u = 0; u < kWU; ++u) {
            const int n = S.n_tile + sr + 16 * u;
            const float* row = S.W + (int64_t)(n < N ? n : N - 1) * S.ldw;     // rows at or beyond N repeat row N - 1: never stored
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (S.vec & kVecW) {         // Ktot % 4 == 0: the piece lies below Ktot or at / beyond it as a whole
                const f32x4 ld = *reinterpret_cast<const f32x4*>(row + (k < Ktot ? k : 0));
                if (k < Ktot) v = ld;
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float ld = row[k + t < Ktot ? k + t : 0];
                    if (k + t < Ktot) v[t] = ld;
                }
            }
            ch.w[u] = v;
        }
    }
}

template <bool WT>
__device__ __forceinline__ void store_chunk(const Chunk& ch, float* ldsW, float* ldsX) {
    if constexpr (WT) {
        const int sr = threadIdx.x >> 5, c = threadIdx.x & 31;
#pragma unroll
        for (int u = 0; u < kWU; ++u) *reinterpret_cast<f32x4*>(ldsW + (sr + 8 * u) * kRS + 4 * c) = ch.w[u];
    } else {
        const int sr = threadIdx.x >> 4, c = threadIdx.x & 15;
#pragma unroll
        for (int u = 0; u < kWU; ++u) *reinterpret_cast<f32x4*>(ldsW + lds_off(sr + 16 * u, c)) = ch.w[u];
    }
    const int sr = threadIdx.x >> 4, c = threadIdx.x & 15;
#pragma unroll
    for (int u = 0; u < kXU; ++u) *reinterpret_cast<f32x4*>(ldsX + lds_off(sr + 16 * u, c)) = ch.x[u];
}

template <bool WT>
__global__ __launch_bounds__(kThreads) void linear_wide_f32_kernel(WideBatch B) {
    constexpr int kWFloats = WT ? kKC * kRS : kBN * kKC;
    __shared__ __attribute__((aligned(16))) float smem[kWFloats + kBM * kKC];
    float* const ldsW = smem;
    float* const ldsX = smem + kWFloats;
    const int di = cwn::group_of<CWN_MAX_DESCS>(B.blk_start, B.n, (int)blockIdx.x);
    const cwn_linear_wide_desc& D = B.d[di];
    const int64_t M = D.M;
    const int64_t live = cwn::rows_clamped(D.m_dev, M);
    const int N = D.N, K1 = D.K, Ktot = D.K + D.K2;
    const int tiles_n = (N + kBN - 1) / kBN;
    const int tile = (int)blockIdx.x - B.blk_start[di];
    const int64_t m_base = (int64_t)(tile / tiles_n) * kBM;
    const int n_tile = (tile % tiles_n) * kBN;
    if (m_base >= live) return;              // (uniform, before any barrier) a tile without a row that exists: nothing is written

    const int vec = B.vec[di];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const Src S{D.X, D.X2, D.W, D.ldx, D.ldx2, D.ldw, M, m_base, N, K1, Ktot, n_tile, vec};

    const int w_base = wave * (16 * CT);     // the wave's first column inside the tile
    const bool multiplies = n_tile + w_base < N;      // (wave-uniform)
    f32x4 acc[CT][RT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[ct][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    Chunk ch;
    load_w<WT>(S, ch, 0);
    load_x(S, ch, 0);
    for (int k0 = 0; k0 < Ktot; k0 += kKC) {
        if (k0 > 0) __syncthreads();         // everyone is done with the previous chunk's fragments
        store_chunk<WT>(ch, ldsW, ldsX);
        __syncthreads();
        if (k0 + kKC < Ktot) {               // in flight during the MFMAs below
            load_w<WT>(S, ch, k0 + kKC);
            load_x(S, ch, k0 + kKC);
        }
        if (multiplies) {
#pragma unroll
            for (int sl = 0; sl < kKC / 16; ++sl) {
                if (k0 + 16 * sl < Ktot) {   // uniform; the columns of a slab at or beyond Ktot hold zeros
                    f32x4 x[RT], w[CT];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) x[rt] = *reinterpret_cast<const f32x4*>(ldsX + lds_off(rt * 16 + j, 4 * sl + g));
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        if constexpr (WT) {
#pragma unroll
                            for (int t = 0; t < 4; ++t) w[ct][t] = ldsW[(16 * sl + 4 * g + t) * kRS + w_base + ct * 16 + j];
                        } else {
                            w[ct] = *reinterpret_cast<const f32x4*>(ldsW + lds_off(w_base + ct * 16 + j, 4 * sl + g));
                        }
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt)
                                acc[ct][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[ct][t], x[rt][t], acc[ct][rt], 0, 0, 0);
                }
            }
        }
    }
    if (!multiplies) return;

    // epilogue: acc[ct][rt][r] = Y[m_base + rt * 16 + j][n_tile + w_base + ct * 16 + 4g + r] before the bias
    const int64_t ldy = D.ldy;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int n0 = n_tile + w_base + ct * 16 + 4 * g;
        float bias[4] = {0.f, 0.f, 0.f, 0.f};
        if (D.bias != nullptr) {
#pragma unroll
            for (int r = 0; r < 4; ++r) bias[r] = D.bias[n0 + r < N ? n0 + r : N - 1];   // clamped: unconditional loads
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int64_t row = m_base + rt * 16 + j;
            if (row < live && n0 < N) {      // live <= M: neither a row behind the count nor one beyond the buffer
                float* yp = D.Y + row * ldy + n0;
                const float y0 = acc[ct][rt][0] + bias[0], y1 = acc[ct][rt][1] + bias[1];
                const float y2 = acc[ct][rt][2] + bias[2], y3 = acc[ct][rt][3] + bias[3];
                if ((vec & kVecY) && n0 + 3 < N) cwn::store_result4(yp, y0, y1, y2, y3);
                else {
                    yp[0] = y0;
                    if (n0 + 1 < N) yp[1] = y1;
                    if (n0 + 2 < N) yp[2] = y2;
                    if (n0 + 3 < N) yp[3] = y3;
                }
            }
        }
    }
}

}  // namespace

extern "C" int cwn_linear_wide_f32(const cwn_linear_wide_desc* descs, int n, cwn_stream_t stream_) {
    if (n < 0 || n > CWN_MAX_DESCS || (descs == nullptr && n > 0)) return CWN_ERR_BAD_ARG;
    WideBatch B{};
    B.n = n;
    cwn::BlockFill fill(B.blk_start);
    for (int i = 0; i < n; ++i) {
        const cwn_linear_wide_desc& D = descs[i];
        if (D.M < 0 || D.N < 1 || D.N > CWN_LINEAR_WIDE_MAX_N || D.K < 1 || D.K2 < 0 || (int64_t)D.K + D.K2 > CWN_LINEAR_WIDE_MAX_K)
            return CWN_ERR_BAD_ARG;
        if ((D.w_trans != 0) != (descs[0].w_trans != 0)) return CWN_ERR_BAD_ARG;     // one weight layout per launch
        if ((D.X2 != nullptr) != (D.K2 > 0)) return CWN_ERR_BAD_ARG;
        if (D.ldx < D.K || D.ldw < (D.w_trans ? D.N : D.K + D.K2) || D.ldy < D.N || (D.K2 > 0 && D.ldx2 < D.K2)) return CWN_ERR_BAD_ARG;
        if (D.M > 0 && (D.X == nullptr || D.W == nullptr || D.Y == nullptr)) return CWN_ERR_BAD_ARG;
        const void* f32s[] = {D.X, D.X2, D.W, D.Y, D.bias};
        for (const void* p : f32s)
            if (!al4(p)) return CWN_ERR_ALIGN;
        if (!al8(D.m_dev)) return CWN_ERR_ALIGN;
        const bool k4 = D.K % 4 == 0 && D.K2 % 4 == 0;
        B.vec[i] = (al16(D.X) && D.ldx % 4 == 0 && k4 && (D.K2 == 0 || (al16(D.X2) && D.ldx2 % 4 == 0)) ? kVecX : 0) |
                   (al16(D.W) && D.ldw % 4 == 0 && (D.w_trans ? D.N % 4 == 0 : k4) ? kVecW : 0) |
                   (al16(D.Y) && D.ldy % 4 == 0 ? kVecY : 0);
        B.d[i] = D;
        // one workgroup per tile of the CAPACITY: those behind the count end at once
        if (!fill.push(i, ((D.M + kBM - 1) / kBM) * ((D.N + kBN - 1) / kBN))) return CWN_ERR_TOO_LARGE;
    }
    const int64_t blocks = fill.close(n);
    if (blocks == 0) return CWN_OK;
    if (descs[0].w_trans != 0)
        hipLaunchKernelGGL(linear_wide_f32_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_, B);
    else
        hipLaunchKernelGGL(linear_wide_f32_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_, B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}
