// cwn_linear_stats.hip -- the forward of a Linear stage that leaves BatchNorm band statistics over the rows that EXIST:
//
//   cwn_linear_stats_f32   Y = prologue([X | X2]) W^T + bias,  col_sum / col_sumsq[b] = column sums of y, y^2 over the
//                          rows [32b, 32b + 32) below the count                 up to CWN_MAX_DESCS products per launch
//
// cwn_gemm_f32 (cwn_gemm.hip) takes these statistics over all M rows of its descriptor and refuses a device-side row count
// next to them; cwn_dense_stage_f32 (cwn_stage.hip) carries the count at widths 64 and 128.  This file is the form with
// the count at ANY width 1 <= N <= 128, K + K2 <= 256 (hidden 48 / 32 / 16, a first layer over raw features): what a
// training step captured over the capacity-sized buffers of a static batch launches for such a stage.  See include/cwn_hip.h,
// "A Linear stage with band statistics under a row count".
//
// * A workgroup of four wave64s owns one 32-row band of one descriptor and all N <= 128 columns: wave w multiplies the
//   columns [32w, 32w + 32) (2 x 2 tiles of v_mfma_f32_16x16x4_f32, 16 accumulator registers); a wave whose columns lie at or
//   beyond N stages operands and multiplies nothing.  A band whose first row is at or beyond the count ends before its first load.
// * The product is cwn_gemm_f32's, element for element: A = 16 weight rows (output columns), B = 16 rows of X, K in slabs of
//   16 ascending, inside a slab lane group g = lane >> 4 owns k = 4g .. 4g + 3 and MFMA step t multiplies component t; one
//   accumulator chain per output element.  Columns of a slab at or beyond K + K2 are zeros in both operands, slabs that
//   begin there are skipped.  With the same descriptor and no count, Y and every band have cwn_gemm_f32's bits; a live
//   row's bits depend on neither the count nor the rows behind it.
// * NOTHING IS STATIONARY IN REGISTERS: K is walked in chunks of 64; a chunk of W ([128][64]) and of the band's rows of X
//   ([32][64], prologue applied on the way) goes global -> registers -> LDS, stored XOR-swizzled (16-byte chunk ^ (row & 15))
//   so that every fragment is one conflict-free ds_read_b128; the next chunk's loads are in flight during the MFMAs.
//   (The weight-stationary gemm_kernel keeps K/2 registers of W per lane and spills at K = 128 with a prologue.)
// * Global reads are row-contiguous (16 lanes read 256 B of one row), 16 bytes wide where pointer, stride and width allow,
//   element by element otherwise -- decided per operand (X / X2, W, Y) and descriptor on the host.  Rows at or beyond M are
//   never addressed (clamped to M - 1); rows in [count, M) are loaded -- they lie inside the buffer -- and may hold
//   anything, NaN included: a row of X only reaches its own row of Y, which is neither stored nor counted.
// * Statistics: fp64, the two row tiles of a lane summed in registers, then the 16 rows of a lane group by DPP rotations,
//   ONE plain store per column and band (no atomics, nothing to zero): cwn_gemm_f32's reduction tree, its bits.
// LDS (static): linear_stats_f32 (128 + 32) rows x 64 floats = 40960 B.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_mem.h"
#include "cwn_check.h"
#include "cwn_act.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kBM = 32;                   // rows of a workgroup: one statistics band
constexpr int kBN = 128;                  // columns of a workgroup: every column of the widest product
constexpr int kKC = 64;                   // k per LDS chunk
constexpr int kCPR = kKC / 4;             // 16-byte chunks per LDS row
constexpr int kMaxN = 128, kMaxK = 256;
constexpr int kWU = kBN * kCPR / kThreads;   // 16-byte pieces of a W chunk per thread (8)
constexpr int kXU = kBM * kCPR / kThreads;   // ... of an X chunk (2)
constexpr int CT = 2, RT = 2;             // 16-column / 16-row MFMA tiles per wave

static_assert(kBM == CWN_STAT_ROWS(32) * 32 && CWN_STAT_ROWS(33) == 2, "a workgroup is one 32-row band");
static_assert(kBN == 4 * 16 * CT && kBM == 16 * RT, "four waves side by side cover the tile");

enum { kVecX = 1, kVecW = 2, kVecY = 4 };    // 16-byte accesses allowed (host-checked), per operand

struct LinBatch {
    cwn_gemm_desc d[CWN_MAX_DESCS];
    int32_t blk_start[CWN_MAX_DESCS + 1];    // first workgroup of each descriptor
    int32_t vec[CWN_MAX_DESCS];
    int32_t n;
};

__device__ __forceinline__ int lds_off(int row, int chunk) {   // in floats
    return row * kKC + ((chunk ^ (row & 15)) << 2);
}

// v of the lane CTRL's rotation away within its 16-lane row (DPP row_ror:n = 0x120 + n), for a double
template <int CTRL>
__device__ __forceinline__ double row_ror_f64(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u & 0xffffffffull), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo));
}

struct Chunk {
    f32x4 w[kWU];
    f32x4 x[kXU];
};

// what the staging of a chunk reads: a descriptor's operands in registers
struct Src {
    const float *X, *X2, *W, *sc1, *sh1, *sc2, *sh2;
    int64_t ldx, ldx2, ldw, M, m_base;
    int N, K1, Ktot, n_wrows, vec;
    bool relu1, relu2;
};

// x of input column k < Ktot after the prologue of the producing stage
__device__ __forceinline__ float prologue(const Src& S, float x, int k) {
    const bool second = k >= S.K1;
    const int kk = second ? k - S.K1 : k;
    const float* const sc = second ? (const float*)S.sc2 : (const float*)S.sc1;
    const float* const sh = second ? (const float*)S.sh2 : (const float*)S.sh1;
    if (sc != nullptr) x = x * sc[kk] + sh[kk];
    if (second ? (bool)S.relu2 : (bool)S.relu1) x = cwn_relu(x);
    return x;
}

// A thread's piece of every chunk: the 16-byte column c = tid & 15 of the rows (tid >> 4) + 16 u.
__device__ __forceinline__ void load_chunk(const Src& S, Chunk& ch, int k0) {
    const int sr = threadIdx.x >> 4, c = threadIdx.x & 15;
    const int k = k0 + 4 * c, Ktot = S.Ktot, K1 = S.K1;
#pragma unroll
    for (int u = 0; u < kWU; ++u) {
        const int r = sr + 16 * u;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (r < S.n_wrows) {             // (uniform per u and wave: n_wrows is a multiple of 32)
            const float* row = S.W + (int64_t)(r < S.N ? r : S.N - 1) * S.ldw;
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
        }
        ch.w[u] = v;
    }
#pragma unroll
    for (int u = 0; u < kXU; ++u) {
        const int r = sr + 16 * u;
        const int64_t grow = S.m_base + r < S.M ? S.m_base + r : S.M - 1;    // clamped: never outside the buffer
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (S.vec & kVecX) {             // K1 % 4 == 0 and K2 % 4 == 0: the piece lies in one operand
            const bool in = k < Ktot, second = in && k >= K1;
            const float* p = second ? S.X2 + grow * S.ldx2 + (k - K1) : S.X + grow * S.ldx + (in ? k : 0);
            const f32x4 ld = *reinterpret_cast<const f32x4*>(p);
            if (in) {
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = prologue(S, ld[t], k + t);
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int kt = k + t;
                const bool in = kt < Ktot, second = in && kt >= K1;
                const float ld = second ? S.X2[grow * S.ldx2 + (kt - K1)] : S.X[grow * S.ldx + (in ? kt : 0)];
                if (in) v[t] = prologue(S, ld, kt);
            }
        }
        ch.x[u] = v;
    }
}

__device__ __forceinline__ void store_chunk(const Chunk& ch, float* ldsW, float* ldsX, int n_wrows) {
    const int sr = threadIdx.x >> 4, c = threadIdx.x & 15;
#pragma unroll
    for (int u = 0; u < kWU; ++u) {
        const int r = sr + 16 * u;
        if (r < n_wrows) *reinterpret_cast<f32x4*>(ldsW + lds_off(r, c)) = ch.w[u];
    }
#pragma unroll
    for (int u = 0; u < kXU; ++u) *reinterpret_cast<f32x4*>(ldsX + lds_off(sr + 16 * u, c)) = ch.x[u];
}

__global__ __launch_bounds__(kThreads) void linear_stats_f32_kernel(LinBatch B) {
    __shared__ __attribute__((aligned(16))) float smem[(kBN + kBM) * kKC];
    float* const ldsW = smem;
    float* const ldsX = smem + kBN * kKC;
    int di = 0;
#pragma unroll
    for (int i = 1; i < CWN_MAX_DESCS; ++i)
        if (i < B.n && (int)blockIdx.x >= B.blk_start[i]) di = i;
    const cwn_gemm_desc& D = B.d[di];
    const int64_t M = D.M;
    int64_t live = M;
    if (D.m_dev != nullptr) {
        const int64_t mv = *D.m_dev;
        live = mv < 0 ? 0 : (mv < M ? mv : M);
    }
    const int64_t m_base = (int64_t)((int)blockIdx.x - B.blk_start[di]) * kBM;
    if (m_base >= live) return;              // (uniform, before any barrier) a band without a row that exists: nothing is written

    const int vec = B.vec[di];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const float* const Xp = D.X;
    const float* const X2p = D.X2;
    const float* const Wp = D.W;
    const int64_t ldx = D.ldx, ldx2 = D.ldx2, ldw = D.ldw, ldy = D.ldy;
    const int N = D.N, K1 = D.K, Ktot = D.K + D.K2;
    const float* const sc1 = D.in_scale;
    const float* const sh1 = D.in_shift;
    const float* const sc2 = D.in_scale2;
    const float* const sh2 = D.in_shift2;
    const bool relu1 = (D.in_relu & 1) != 0, relu2 = (D.in_relu & 2) != 0;
    const int n_wrows = (N + 31) & ~31;      // W rows the multiplying waves read (rows at or beyond N repeat row N - 1)

    const Src S{Xp, X2p, Wp, sc1, sh1, sc2, sh2, ldx, ldx2, ldw, M, m_base, N, K1, Ktot, n_wrows, vec, relu1, relu2};

    const int n_base = wave * (16 * CT);
    const bool multiplies = n_base < N;      // (wave-uniform)
    f32x4 acc[CT][RT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[ct][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    Chunk ch;
    load_chunk(S, ch, 0);
    for (int k0 = 0; k0 < Ktot; k0 += kKC) {
        if (k0 > 0) __syncthreads();         // everyone is done with the previous chunk's fragments
        store_chunk(ch, ldsW, ldsX, n_wrows);
        __syncthreads();
        if (k0 + kKC < Ktot) load_chunk(S, ch, k0 + kKC);       // in flight during the MFMAs below
        if (multiplies) {
#pragma unroll
            for (int sl = 0; sl < kKC / 16; ++sl) {
                if (k0 + 16 * sl < Ktot) {   // uniform; the columns of a slab at or beyond Ktot hold zeros
                    f32x4 x[RT], w[CT];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) x[rt] = *reinterpret_cast<const f32x4*>(ldsX + lds_off(rt * 16 + j, 4 * sl + g));
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) w[ct] = *reinterpret_cast<const f32x4*>(ldsW + lds_off(n_base + ct * 16 + j, 4 * sl + g));
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

    // epilogue: acc[ct][rt][r] = Y[m_base + rt * 16 + j][n_base + ct * 16 + 4g + r] before the bias
    const bool stats = D.col_sum != nullptr;
    const int64_t band = m_base / kBM;       // < CWN_STAT_ROWS(live): the band holds a row that exists
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int n0 = n_base + ct * 16 + 4 * g;
        float bias[4] = {0.f, 0.f, 0.f, 0.f};
        if (D.bias != nullptr) {
#pragma unroll
            for (int r = 0; r < 4; ++r) bias[r] = D.bias[n0 + r < N ? n0 + r : N - 1];   // clamped: unconditional loads
        }
        double csum[4] = {0., 0., 0., 0.}, csq[4] = {0., 0., 0., 0.};   // fp64: see cwn_bn_finalize_f32
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int64_t row = m_base + rt * 16 + j;
            const bool exists = row < live;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float y = acc[ct][rt][r] + bias[r];
                acc[ct][rt][r] = y;
                if (stats && exists) {       // a predicate, not a product: what a row behind the count holds never arrives
                    csum[r] += (double)y;
                    csq[r] += (double)y * (double)y;
                }
            }
            if (exists && n0 < N) {
                float* yp = D.Y + row * ldy + n0;
                if ((vec & kVecY) && n0 + 3 < N) cwn::store_result4(yp, acc[ct][rt][0], acc[ct][rt][1], acc[ct][rt][2], acc[ct][rt][3]);
                else
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n0 + r < N) yp[r] = acc[ct][rt][r];
            }
        }
        if (stats && n0 < N) {               // (uniform per 16-lane row: the DPP rotations stay inside it)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double a = csum[r], b = csq[r];
                a += row_ror_f64<0x128>(a); b += row_ror_f64<0x128>(b);
                a += row_ror_f64<0x124>(a); b += row_ror_f64<0x124>(b);
                a += row_ror_f64<0x122>(a); b += row_ror_f64<0x122>(b);
                a += row_ror_f64<0x121>(a); b += row_ror_f64<0x121>(b);
                if (j == 0 && n0 + r < N) {
                    D.col_sum[band * N + n0 + r] = a;
                    D.col_sumsq[band * N + n0 + r] = b;
                }
            }
        }
    }
}

}  // namespace

extern "C" int cwn_linear_stats_f32(const cwn_gemm_desc* descs, int n, cwn_stream_t stream_) {
    if (n < 0 || n > CWN_MAX_DESCS || (descs == nullptr && n > 0)) return CWN_ERR_BAD_ARG;
    LinBatch B{};
    B.n = n;
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const cwn_gemm_desc& D = descs[i];
        if (D.M < 0 || D.N < 1 || D.N > kMaxN || D.K < 1 || D.K2 < 0 || (int64_t)D.K + D.K2 > kMaxK) return CWN_ERR_BAD_ARG;
        if (D.w_trans != 0 || D.bnb != nullptr || D.out_scale != nullptr || D.out_shift != nullptr || D.relu != 0 ||
            (D.flags & ~CWN_GEMM_EXACT) != 0)
            return CWN_ERR_BAD_ARG;          // cwn_gemm_f32's business
        if ((D.col_sum == nullptr) != (D.col_sumsq == nullptr)) return CWN_ERR_BAD_ARG;
        if ((D.X2 != nullptr) != (D.K2 > 0)) return CWN_ERR_BAD_ARG;
        if ((D.in_scale == nullptr) != (D.in_shift == nullptr) || (D.in_scale2 == nullptr) != (D.in_shift2 == nullptr)) return CWN_ERR_BAD_ARG;
        if (D.in_scale2 != nullptr && D.K2 == 0) return CWN_ERR_BAD_ARG;
        if (D.ldx < D.K || D.ldw < D.K + D.K2 || D.ldy < D.N || (D.K2 > 0 && D.ldx2 < D.K2)) return CWN_ERR_BAD_ARG;
        if (D.M > 0 && (D.X == nullptr || D.W == nullptr || D.Y == nullptr)) return CWN_ERR_BAD_ARG;
        const void* f32s[] = {D.X, D.X2, D.W, D.Y, D.bias, D.in_scale, D.in_shift, D.in_scale2, D.in_shift2};
        for (const void* p : f32s)
            if (!al4(p)) return CWN_ERR_ALIGN;
        if (!al8(D.col_sum) || !al8(D.col_sumsq) || !al8(D.m_dev)) return CWN_ERR_ALIGN;
        const bool k4 = D.K % 4 == 0 && D.K2 % 4 == 0;
        B.vec[i] = (al16(D.X) && D.ldx % 4 == 0 && k4 && (D.K2 == 0 || (al16(D.X2) && D.ldx2 % 4 == 0)) ? kVecX : 0) |
                   (al16(D.W) && D.ldw % 4 == 0 && k4 ? kVecW : 0) | (al16(D.Y) && D.ldy % 4 == 0 ? kVecY : 0);
        B.d[i] = D;
        B.blk_start[i] = (int32_t)blocks;
        blocks += CWN_STAT_ROWS(D.M);        // one workgroup per band of the CAPACITY: those behind the count end at once
        if (blocks >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    }
    for (int i = n; i <= CWN_MAX_DESCS; ++i) B.blk_start[i] = (int32_t)blocks;
    if (blocks == 0) return CWN_OK;
    hipLaunchKernelGGL(linear_stats_f32_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_, B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}
