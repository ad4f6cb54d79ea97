// cwn_dense_f64.hip -- the Linear layers of a float64 model, inference only: a grouped Y = act(X W^T + b)
// (cwn_linear_many_f64) and the whole update / combine part of a SparseCINConv layer for every dimension in one launch
// (cwn_update_chain_f64).  See include/cwn_hip.h, "The float64 dense path".
//
// The shapes are those of the strongly-regular-graph experiments: a few hundred rows by 16 (at most 64 / 128) columns.
// As torch modules every Linear is a dgemm, a bias add and an activation launch; all of them together are less work than
// one launch costs, so the forward is bound by the number of launches and nothing here tries to be a fast GEMM:
//   * a workgroup of 256 threads owns 16 rows.  A thread owns ONE output column c and RPT of the 16 rows (N <= 16: one
//     row, 32: two, 64: four, 128: eight), so a weight element read from LDS serves RPT fma, and the input elements of a
//     row are wave-uniform LDS broadcasts.
//   * the weight is staged TRANSPOSED in LDS (Ws[k][c], row pitch odd: the lanes of a wave read consecutive doubles), one
//     stage (chain kernel) or one chunk of 32 k (linear kernel) at a time: the five 64-wide matrices of a layer are
//     192 KiB, more than a CU holds, and read from L2 they are 512-byte strides per lane.
//   * an output element is one chain of fma() over k ascending from 0, then bias, affine, activation (the header's
//     arithmetic contract).  Which thread computes an element, and how many elements a thread has, changes no bit of it:
//     a row's result is a function of that row and the weights only.  fma() is written out; the file is compiled with
//     -ffp-contract=off like the rest of the library.
//   * the chain kernel keeps everything between its two inputs and its output in LDS and registers: a stage reads its
//     input tile, holds the results in registers across a barrier and overwrites the tile; the combine stage continues
//     ONE accumulator over the up tile and then the boundary tile -- the K-concatenation without a concatenation.
// LDS: chain 2 x 16 x 64 x 8 + 64 x 65 x 8 = 49 KiB, linear 16 x 128 x 8 + 32 x 129 x 8 = 48.3 KiB (static, three / CU).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_act.h"
#include "cwn_check.h"
#include "cwn_group.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = CWN_DENSE_F64_TILE_ROWS;
constexpr int kChainW = CWN_CHAIN_F64_MAX_WIDTH;       // 64: row pitch of the chain kernel's input tiles
constexpr int kChainWld = kChainW + 1;                 // pitch of its transposed weight
constexpr int kLinW = CWN_LINEAR_F64_MAX_WIDTH;        // 128: row pitch of the linear kernel's X tile
constexpr int kLinWld = kLinW + 1;
constexpr int kLinKc = 32;                             // k per staged weight chunk

struct LinearBatch {
    cwn_linear_desc_f64 d[CWN_LINEAR_F64_MAX_DESCS];
    int32_t blk_start[CWN_LINEAR_F64_MAX_DESCS + 1];
    int32_t n;
};

struct ChainBatch {
    cwn_chain_desc_f64 d[CWN_CHAIN_F64_MAX_DIMS];
    int32_t blk_start[CWN_CHAIN_F64_MAX_DIMS + 1];
    int32_t n;
};

// bias, affine, activation of column c
__device__ __forceinline__ double finish(double v, int c, const double* bias, const double* scale, const double* shift,
                                         int act) {
    if (bias != nullptr) v += bias[c];
    if (scale != nullptr) v = fma(v, scale[c], shift[c]);
    return activate_rt(v, act);
}

// W[c, k0 + k] (row stride ldw) -> ws[k * wld + c] for c < n_cols, k < kn
__device__ __forceinline__ void stage_weight(double* ws, int wld, const double* __restrict__ W, int64_t ldw, int n_cols,
                                             int kn) {
    for (int i = threadIdx.x; i < n_cols * kn; i += kThreads) {
        const int c = i / kn, k = i - c * kn;
        ws[k * wld + c] = W[(int64_t)c * ldw + k];
    }
}

// acc[j] += sum_k xs[j * xstep + k] * ws[k * wld], k ascending: the one chain of an output element
template <int RPT>
__device__ __forceinline__ void accumulate(double (&acc)[RPT], const double* xs, int xstep, const double* ws, int wld,
                                           int kn) {
    for (int k = 0; k < kn; ++k) {
        const double w = ws[k * wld];
#pragma unroll
        for (int j = 0; j < RPT; ++j) acc[j] = fma(xs[j * xstep + k], w, acc[j]);
    }
}

// ---- cwn_linear_many_f64 ---------------------------------------------------------------------------------------------
template <int NP>
__device__ __forceinline__ void linear_tile(const cwn_linear_desc_f64& D, int64_t row0, double* xs, double* ws) {
    constexpr int RL = kThreads / NP, RPT = kRows / RL;
    const int tid = threadIdx.x, c = tid % NP, rl = tid / NP;
    const int K = D.K, N = D.N;
    const int64_t left = D.M - row0;
    const int rows = left < kRows ? (int)left : kRows;
    for (int i = tid; i < kRows * K; i += kThreads) {
        const int r = i / K, k = i - r * K;
        xs[r * kLinW + k] = r < rows ? D.X[(row0 + r) * D.ldx + k] : 0.0;
    }
    double acc[RPT];
#pragma unroll
    for (int j = 0; j < RPT; ++j) acc[j] = 0.0;
    for (int k0 = 0; k0 < K; k0 += kLinKc) {
        const int kn = K - k0 < kLinKc ? K - k0 : kLinKc;
        if (k0 > 0) __syncthreads();                     // the previous chunk has been read
        stage_weight(ws, kLinWld, D.W + k0, D.ldw, N, kn);
        __syncthreads();
        if (c < N) accumulate<RPT>(acc, xs + rl * kLinW + k0, RL * kLinW, ws + c, kLinWld, kn);
    }
    if (c < N) {
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            const int r = rl + j * RL;
            if (r < rows) D.Y[(row0 + r) * D.ldy + c] = finish(acc[j], c, D.bias, nullptr, nullptr, D.act);
        }
    }
}

__global__ __launch_bounds__(kThreads) void linear_many_f64_kernel(LinearBatch B) {
    __shared__ double xs[kRows * kLinW];
    __shared__ double ws[kLinKc * kLinWld];
    const int di = cwn::group_of<CWN_LINEAR_F64_MAX_DESCS>(B.blk_start, B.n, (int)blockIdx.x);
    const cwn_linear_desc_f64 D = B.d[di];               // by value (a reference puts the batch struct in scratch)
    const int64_t row0 = (int64_t)((int)blockIdx.x - B.blk_start[di]) * kRows;
    if (D.N <= 16) linear_tile<16>(D, row0, xs, ws);
    else if (D.N <= 32) linear_tile<32>(D, row0, xs, ws);
    else if (D.N <= 64) linear_tile<64>(D, row0, xs, ws);
    else linear_tile<128>(D, row0, xs, ws);
}

// ---- cwn_update_chain_f64 --------------------------------------------------------------------------------------------
template <int HP>
__device__ __forceinline__ void chain_tile(const cwn_chain_desc_f64& D, int64_t row0, double* a, double* b, double* ws) {
    constexpr int RL = kThreads / HP, RPT = kRows / RL;
    const int tid = threadIdx.x, c = tid % HP, rl = tid / HP;
    const int F = D.F, H = D.H, act = D.act;
    const bool live = c < H;
    const int64_t left = D.n - row0;
    const int rows = left < kRows ? (int)left : kRows;
    for (int i = tid; i < kRows * F; i += kThreads) {
        const int r = i / F, k = i - r * F;
        const bool in = r < rows;
        a[r * kChainW + k] = in ? D.in_up[(row0 + r) * D.ld_up + k] : 0.0;
        b[r * kChainW + k] = in ? D.in_b[(row0 + r) * D.ld_b + k] : 0.0;
    }
    stage_weight(ws, kChainWld, D.W[0], F, H, F);
    __syncthreads();
    double acc[RPT];

    // one Linear + affine + activation on a tile, in place: tile -> registers -> barrier -> tile; the NEXT stage's weight
    // (W_next [H, kn_next], row stride ld_next) is staged while the tile is rewritten
    auto stage = [&](double* tile, int kn, int s, const double* W_next, int64_t ld_next, int kn_next) {
#pragma unroll
        for (int j = 0; j < RPT; ++j) acc[j] = 0.0;
        if (live) accumulate<RPT>(acc, tile + rl * kChainW, RL * kChainW, ws + c, kChainWld, kn);
        __syncthreads();                                 // every thread has read the tile and the weight
        if (live) {
#pragma unroll
            for (int j = 0; j < RPT; ++j)
                tile[(rl + j * RL) * kChainW + c] = finish(acc[j], c, D.bias[s], D.scale[s], D.shift[s], act);
        }
        stage_weight(ws, kChainWld, W_next, ld_next, H, kn_next);
        __syncthreads();
    };
    stage(a, F, 0, D.W[1], H, H);                        // update_up_nn
    stage(a, H, 1, D.W[2], F, F);
    stage(b, F, 2, D.W[3], H, H);                        // update_boundaries_nn
    stage(b, H, 3, D.W[4], 2 * H, H);                    // ... and the left half of combine_nn's weight
    // combine_nn: one accumulator over cat(up, boundary) -- k = 0 .. H-1 from the up tile, H .. 2H-1 from the other
#pragma unroll
    for (int j = 0; j < RPT; ++j) acc[j] = 0.0;
    if (live) accumulate<RPT>(acc, a + rl * kChainW, RL * kChainW, ws + c, kChainWld, H);
    __syncthreads();
    stage_weight(ws, kChainWld, D.W[4] + H, 2 * H, H, H);
    __syncthreads();
    if (live) {
        accumulate<RPT>(acc, b + rl * kChainW, RL * kChainW, ws + c, kChainWld, H);
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            const int r = rl + j * RL;
            if (r < rows) D.out[(row0 + r) * D.ld_out + c] = finish(acc[j], c, D.bias[4], D.scale[4], D.shift[4], act);
        }
    }
}

__global__ __launch_bounds__(kThreads) void update_chain_f64_kernel(ChainBatch B) {
    __shared__ double a[kRows * kChainW];
    __shared__ double b[kRows * kChainW];
    __shared__ double ws[kChainW * kChainWld];
    const int di = cwn::group_of<CWN_CHAIN_F64_MAX_DIMS>(B.blk_start, B.n, (int)blockIdx.x);
    const cwn_chain_desc_f64 D = B.d[di];
    const int64_t row0 = (int64_t)((int)blockIdx.x - B.blk_start[di]) * kRows;
    if (D.H <= 16) chain_tile<16>(D, row0, a, b, ws);
    else if (D.H <= 32) chain_tile<32>(D, row0, a, b, ws);
    else chain_tile<64>(D, row0, a, b, ws);
}

}  // namespace

extern "C" int cwn_linear_many_f64(const cwn_linear_desc_f64* descs, int n, cwn_stream_t stream_) {
    if (descs == nullptr || n < 1 || n > CWN_LINEAR_F64_MAX_DESCS) return CWN_ERR_BAD_ARG;
    LinearBatch B{};
    B.n = n;
    cwn::BlockFill fill(B.blk_start);
    for (int i = 0; i < n; ++i) {
        const cwn_linear_desc_f64& D = descs[i];
        if (D.M < 0 || D.K < 1 || D.K > CWN_LINEAR_F64_MAX_WIDTH || D.N < 1 || D.N > CWN_LINEAR_F64_MAX_WIDTH || !known_act(D.act))
            return CWN_ERR_BAD_ARG;
        if (D.M > 0) {
            if (D.X == nullptr || D.W == nullptr || D.Y == nullptr) return CWN_ERR_BAD_ARG;
            if (D.ldx < D.K || D.ldw < D.K || D.ldy < D.N) return CWN_ERR_BAD_ARG;
            if (!al8(D.X) || !al8(D.W) || !al8(D.Y) || !al8(D.bias)) return CWN_ERR_ALIGN;
        }
        B.d[i] = D;
        if (!fill.push(i, (D.M + kRows - 1) / kRows)) return CWN_ERR_TOO_LARGE;
    }
    const int64_t blocks = fill.close(n);
    if (blocks == 0) return CWN_OK;
    linear_many_f64_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_>>>(B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

extern "C" int cwn_update_chain_f64(const cwn_chain_desc_f64* descs, int n_dims, cwn_stream_t stream_) {
    if (descs == nullptr || n_dims < 1 || n_dims > CWN_CHAIN_F64_MAX_DIMS) return CWN_ERR_BAD_ARG;
    ChainBatch B{};
    B.n = n_dims;
    cwn::BlockFill fill(B.blk_start);
    for (int i = 0; i < n_dims; ++i) {
        const cwn_chain_desc_f64& D = descs[i];
        if (D.n < 0 || D.F < 1 || D.F > CWN_CHAIN_F64_MAX_WIDTH || D.H < 1 || D.H > CWN_CHAIN_F64_MAX_WIDTH || !known_act(D.act))
            return CWN_ERR_BAD_ARG;
        for (int s = 0; s < 5; ++s)
            if ((D.scale[s] == nullptr) != (D.shift[s] == nullptr)) return CWN_ERR_BAD_ARG;
        if (D.n > 0) {
            if (D.in_up == nullptr || D.in_b == nullptr || D.out == nullptr) return CWN_ERR_BAD_ARG;
            if (D.ld_up < D.F || D.ld_b < D.F || D.ld_out < D.H) return CWN_ERR_BAD_ARG;
            if (!al8(D.in_up) || !al8(D.in_b) || !al8(D.out)) return CWN_ERR_ALIGN;
            for (int s = 0; s < 5; ++s) {
                if (D.W[s] == nullptr) return CWN_ERR_BAD_ARG;
                if (!al8(D.W[s]) || !al8(D.bias[s]) || !al8(D.scale[s]) || !al8(D.shift[s])) return CWN_ERR_ALIGN;
            }
        }
        B.d[i] = D;
        if (!fill.push(i, (D.n + kRows - 1) / kRows)) return CWN_ERR_TOO_LARGE;
    }
    const int64_t blocks = fill.close(n_dims);
    if (blocks == 0) return CWN_OK;
    update_chain_f64_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_>>>(B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}
