// cwn_agnostic.hip -- MessagePassingAgnostic (mp/models.py:618-661), the control of the strongly-regular-graph experiment,
// as two launches, float32 and float64, inference.  See include/cwn_hip.h, "The message-passing-agnostic baseline".
//
//   cwn_embed_pool_*     P[c, h] = sum over the rows r of complex c of act(x[r, :] . W[h, :] + bias[h])   [/ max(rows, 1)]
//   cwn_agnostic_head_*  out[c, :] = W2 (sum over d of act(W1 P_d[c, :] + b1)) + b2
//
// The model is a reduce with a tiny product in front of it (K = 1 in the experiment, H = 256): as torch modules every
// dimension writes an [N, H] activation matrix that is read once, and H = 256 is beyond cwn_linear_many_f64, so every
// product is a dgemm launch.  Here nothing but x, the weights and the [C, H] / [C, O] results touches memory.
//
// embed_pool: a workgroup of four wave64s owns one (descriptor, complex, block of 64 columns).  A lane owns a column: the
// block of W is staged in LDS as ws[column][k] with the odd pitch kPitch (the lanes of a wave read 64 different banks, the
// staging writes consecutive addresses), and x[r, k] is wave-uniform.  The rows of a complex are cut into chunks of
// CWN_EMBED_POOL_CHUNK rows; chunk j belongs to wave j % 4, which folds its chunks in ascending order, row by row, into ONE
// accumulator; the four partials are combined as ((p0 + p1) + p2) + p3 through LDS.  So the order of the sum is a function
// of the number of rows of that complex alone -- not of C, of the complex's place in the batch or of the other
// descriptors.  Four rows are in flight at a time (four independent pre-activation chains and activations); they are
// ADDED one after the other.  No atomics.
//
// head: one workgroup per complex, a thread owns an output column.  W1 (then W2) passes through LDS in tiles of 256 rows x
// 32 k, pitch 33, read from memory along k (coalesced) and from LDS by row (conflict-free); with a W1 tile comes the
// matching piece of every P_d[c, :], so one pass over W1 serves all D dimensions (D accumulators per thread).  The sums
// s[c, :] stay in LDS for the second product.
//
// Every output element is one fma() chain over k ascending from 0, then the bias add, then the activation (the contract
// of cwn_dense_f64.hip); fma() is written out, the file is compiled with -ffp-contract=off like the rest of the library.
// LDS (static): embed_pool (64 x 129 + 256) elements = 34048 B in float32, 68096 B in float64;
//               head (256 x 33 + 8 x 32 + 1024) elements = 38912 B in float32, 77824 B in float64.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_act.h"
#include "cwn_check.h"
#include "cwn_group.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCols = 64;                                // columns of P per workgroup: one per lane
constexpr int kChunk = CWN_EMBED_POOL_CHUNK;             // rows per chunk
constexpr int kPitch = CWN_EMBED_POOL_MAX_K + 1;         // pitch of the staged block of W
constexpr int kRowsInFlight = 4;
constexpr int kMaxW = CWN_AGNOSTIC_MAX_WIDTH;            // widest H / O
constexpr int kKc = 32;                                  // k per staged weight tile of the head
constexpr int kWld = kKc + 1;

static_assert(kChunk % kRowsInFlight == 0, "a chunk is a whole number of row groups");
static_assert(CWN_MAX_DESCS * kKc <= kThreads, "one thread per element of the staged piece of P");

template <class real> struct PoolDescOf;
template <> struct PoolDescOf<float> { using type = cwn_embed_pool_desc; };
template <> struct PoolDescOf<double> { using type = cwn_embed_pool_desc_f64; };
template <class real> struct HeadDescOf;
template <> struct HeadDescOf<float> { using type = cwn_agnostic_head_desc; };
template <> struct HeadDescOf<double> { using type = cwn_agnostic_head_desc_f64; };

template <class real>
struct PoolBatch {
    typename PoolDescOf<real>::type d[CWN_MAX_DESCS];
    int32_t blk_start[CWN_MAX_DESCS + 1];
    int32_t n;
};

__device__ __forceinline__ float fmad(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double fmad(double a, double b, double c) { return fma(a, b, c); }

// ---- cwn_embed_pool_* --------------------------------------------------------------------------------------------------

// The partial sum of one wave: rows [start, end) of x, the chunks j = wave, wave + 4, ... in ascending order.  `w`: the
// lane's row of the staged block of W.  Everything but `w` and `bias` is wave-uniform.
template <class real, int ACT>
__device__ __forceinline__ real fold_chunks(const real* __restrict__ x, int64_t ldx, int K, int64_t start, int64_t end, int wave,
                                            const real* w, real bias) {
    real acc = real(0.0);
    for (int64_t c0 = start + (int64_t)wave * kChunk; c0 < end; c0 += (int64_t)kWaves * kChunk) {
        const int64_t ce = c0 + kChunk < end ? c0 + kChunk : end;
        for (int64_t r = c0; r < ce; r += kRowsInFlight) {
            const int nr = ce - r < kRowsInFlight ? (int)(ce - r) : kRowsInFlight;
            const real* xr = x + r * ldx;
            real z[kRowsInFlight];
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) z[u] = real(0.0);
            for (int k = 0; k < K; ++k) {
                const real wk = w[k];
#pragma unroll
                for (int u = 0; u < kRowsInFlight; ++u)
                    if (u < nr) z[u] = fmad(xr[u * ldx + k], wk, z[u]);
            }
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u)
                if (u < nr) acc = acc + activate<ACT>(z[u] + bias);          // in row order
        }
    }
    return acc;
}

template <class real>
__global__ __launch_bounds__(kThreads) void embed_pool_kernel(PoolBatch<real> B) {
    __shared__ real ws[kCols * kPitch];
    __shared__ real part[kThreads];
    const int di = cwn::group_of<CWN_MAX_DESCS>(B.blk_start, B.n, (int)blockIdx.x);
    const typename PoolDescOf<real>::type D = B.d[di];      // by value (cwn_aggregate_act.hip)
    const int blk = blockIdx.x - B.blk_start[di];
    const int nhb = (D.H + kCols - 1) / kCols;
    const int64_t c = blk / nhb;
    const int h0 = (blk - (int)c * nhb) * kCols;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = h0 + lane;
    // the rows of the complex, kept inside [0, N] whatever cell_ptr holds
    int64_t start = D.cell_ptr[c], end = D.cell_ptr[c + 1];
    start = start < 0 ? 0 : (start > D.N ? D.N : start);
    end = end < start ? start : (end > D.N ? D.N : end);
    if (start == end) {                                     // uniform over the workgroup: no row, a zero row
        if (tid < kCols && h < D.H) D.out[c * D.ldo + h] = real(0.0);
        return;
    }
    const int K = D.K;
    for (int i = tid; i < kCols * K; i += kThreads) {
        const int hl = i / K, k = i - hl * K;
        ws[hl * kPitch + k] = h0 + hl < D.H ? D.W[(int64_t)(h0 + hl) * D.ldw + k] : real(0.0);
    }
    const real bias = (D.bias != nullptr && h < D.H) ? D.bias[h] : real(0.0);
    __syncthreads();
    const real* w = ws + lane * kPitch;
    real acc;
    switch (D.act) {
        case CWN_ACT_RELU: acc = fold_chunks<real, CWN_ACT_RELU>(D.x, D.ldx, K, start, end, wave, w, bias); break;
        case CWN_ACT_ELU: acc = fold_chunks<real, CWN_ACT_ELU>(D.x, D.ldx, K, start, end, wave, w, bias); break;
        case CWN_ACT_TANH: acc = fold_chunks<real, CWN_ACT_TANH>(D.x, D.ldx, K, start, end, wave, w, bias); break;
        case CWN_ACT_SIGMOID: acc = fold_chunks<real, CWN_ACT_SIGMOID>(D.x, D.ldx, K, start, end, wave, w, bias); break;
        default: acc = fold_chunks<real, CWN_ACT_ID>(D.x, D.ldx, K, start, end, wave, w, bias); break;
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < kCols && h < D.H) {
        real total = part[lane];
#pragma unroll
        for (int q = 1; q < kWaves; ++q) total = total + part[q * 64 + lane];      // in wave order
        if (D.mean) total = total / real(end - start);
        D.out[c * D.ldo + h] = total;
    }
}

template <class real>
int launch_pool(const typename PoolDescOf<real>::type* descs, int n, cwn_stream_t stream_) {
    using Desc = typename PoolDescOf<real>::type;
    if (n < 0 || n > CWN_MAX_DESCS || (n > 0 && descs == nullptr)) return CWN_ERR_BAD_ARG;
    PoolBatch<real> B{};
    B.n = n;
    cwn::BlockFill fill(B.blk_start);
    for (int i = 0; i < n; ++i) {
        const Desc& D = descs[i];
        if (D.K < 1 || D.K > CWN_EMBED_POOL_MAX_K || D.H < 1 || D.H > CWN_AGNOSTIC_MAX_WIDTH) return CWN_ERR_BAD_ARG;
        if (!known_act(D.act) || (D.mean != 0 && D.mean != 1)) return CWN_ERR_BAD_ARG;
        if (D.N < 0 || D.C < 0 || D.ldx < D.K || D.ldw < D.K || D.ldo < D.H) return CWN_ERR_BAD_ARG;
        if (D.N > 0 && (D.x == nullptr || D.W == nullptr)) return CWN_ERR_BAD_ARG;
        if (D.C > 0 && (D.cell_ptr == nullptr || D.out == nullptr)) return CWN_ERR_BAD_ARG;
        if (D.N >= INT32_MAX || D.C >= INT32_MAX) return CWN_ERR_TOO_LARGE;
        for (const void* p : {(const void*)D.x, (const void*)D.W, (const void*)D.bias, (const void*)D.out})
            if (!aligned_to(p, sizeof(real))) return CWN_ERR_ALIGN;
        if (!aligned_to(D.cell_ptr, sizeof(int64_t))) return CWN_ERR_ALIGN;
        B.d[i] = D;
        if (!fill.push(i, D.C * ((D.H + kCols - 1) / kCols))) return CWN_ERR_TOO_LARGE;
    }
    const int64_t blocks = fill.close(n);
    if (blocks == 0) return CWN_OK;
    embed_pool_kernel<real><<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_>>>(B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

// ---- cwn_agnostic_head_* -----------------------------------------------------------------------------------------------

// W[row, k] for row < n_rows, k < kn (row stride ldw) -> wt[row * kWld + k]; 32 consecutive threads read one row's piece
template <class real>
__device__ __forceinline__ void stage_rows(real* wt, const real* __restrict__ W, int64_t ldw, int n_rows, int kn) {
#pragma unroll 8
    for (int i = threadIdx.x; i < n_rows * kKc; i += kThreads) {
        const int row = i / kKc, k = i % kKc;
        if (k < kn) wt[row * kWld + k] = W[(int64_t)row * ldw + k];
    }
}

template <class real>
__global__ __launch_bounds__(kThreads) void agnostic_head_kernel(typename HeadDescOf<real>::type D) {
    __shared__ real wt[kThreads * kWld];
    __shared__ real pt[CWN_MAX_DESCS * kKc];
    __shared__ real s[kMaxW];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int H = D.H, O = D.O, nd = D.D;
    // this thread's element of the staged pieces of P: dimension tid / 32, column tid % 32 of the piece.  The pointer is
    // picked with compile-time indices (an array of the argument struct indexed at run time goes to scratch).
    const int pd = tid / kKc, pk = tid % kKc;
    const real* prow = nullptr;
#pragma unroll
    for (int d = 0; d < CWN_MAX_DESCS; ++d)
        if (d == pd && d < nd && D.P[d] != nullptr) prow = D.P[d] + c * D.ldp[d];

    for (int j0 = 0; j0 < H; j0 += kThreads) {
        const int j = j0 + tid;
        const int nj = H - j0 < kThreads ? H - j0 : kThreads;
        real acc[CWN_MAX_DESCS];
#pragma unroll
        for (int d = 0; d < CWN_MAX_DESCS; ++d) acc[d] = real(0.0);
        for (int k0 = 0; k0 < H; k0 += kKc) {
            const int kn = H - k0 < kKc ? H - k0 : kKc;
            __syncthreads();                                  // the previous tile has been read
            stage_rows(wt, D.W1 + (int64_t)j0 * D.ldw1 + k0, D.ldw1, nj, kn);
            pt[tid] = (prow != nullptr && pk < kn) ? prow[k0 + pk] : real(0.0);      // an absent dimension: zeros
            __syncthreads();
            if (j < H) {
                const real* w = wt + tid * kWld;
                for (int k = 0; k < kn; ++k) {
                    const real wk = w[k];
#pragma unroll
                    for (int d = 0; d < CWN_MAX_DESCS; ++d)
                        if (d < nd) acc[d] = fmad(pt[d * kKc + k], wk, acc[d]);
                }
            }
        }
        if (j < H) {
            const real b = D.b1 != nullptr ? D.b1[j] : real(0.0);
            real sum = real(0.0);
#pragma unroll
            for (int d = 0; d < CWN_MAX_DESCS; ++d)
                if (d < nd) sum = sum + activate_rt<real>(acc[d] + b, D.act);        // d ascending
            s[j] = sum;
        }
    }
    for (int o0 = 0; o0 < O; o0 += kThreads) {
        const int o = o0 + tid;
        const int no = O - o0 < kThreads ? O - o0 : kThreads;
        real acc = real(0.0);
        for (int k0 = 0; k0 < H; k0 += kKc) {
            const int kn = H - k0 < kKc ? H - k0 : kKc;
            __syncthreads();                                  // the previous tile has been read, s is complete
            stage_rows(wt, D.W2 + (int64_t)o0 * D.ldw2 + k0, D.ldw2, no, kn);
            __syncthreads();
            if (o < O) {
                const real* w = wt + tid * kWld;
                for (int k = 0; k < kn; ++k) acc = fmad(s[k0 + k], w[k], acc);
            }
        }
        if (o < O) D.out[c * D.ldo + o] = acc + (D.b2 != nullptr ? D.b2[o] : real(0.0));
    }
}

template <class real>
int launch_head(const typename HeadDescOf<real>::type* desc, cwn_stream_t stream_) {
    if (desc == nullptr) return CWN_ERR_BAD_ARG;
    const auto& D = *desc;
    if (D.D < 1 || D.D > CWN_MAX_DESCS) return CWN_ERR_BAD_ARG;
    if (D.H < 1 || D.H > CWN_AGNOSTIC_MAX_WIDTH || D.O < 1 || D.O > CWN_AGNOSTIC_MAX_WIDTH) return CWN_ERR_BAD_ARG;
    if (!known_act(D.act) || D.C < 0) return CWN_ERR_BAD_ARG;
    if (D.ldw1 < D.H || D.ldw2 < D.H || D.ldo < D.O) return CWN_ERR_BAD_ARG;
    for (int d = 0; d < D.D; ++d)
        if (D.P[d] != nullptr && D.ldp[d] < D.H) return CWN_ERR_BAD_ARG;
    if (D.C > 0 && (D.W1 == nullptr || D.W2 == nullptr || D.out == nullptr)) return CWN_ERR_BAD_ARG;
    if (D.C >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    for (const void* p : {(const void*)D.W1, (const void*)D.b1, (const void*)D.W2, (const void*)D.b2, (const void*)D.out})
        if (!aligned_to(p, sizeof(real))) return CWN_ERR_ALIGN;
    for (int d = 0; d < D.D; ++d)
        if (!aligned_to(D.P[d], sizeof(real))) return CWN_ERR_ALIGN;
    if (D.C == 0) return CWN_OK;
    agnostic_head_kernel<real><<<dim3((unsigned)D.C), dim3(kThreads), 0, (hipStream_t)stream_>>>(D);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

}  // namespace

extern "C" int cwn_embed_pool_f32(const cwn_embed_pool_desc* descs, int n, cwn_stream_t stream) {
    return launch_pool<float>(descs, n, stream);
}

extern "C" int cwn_embed_pool_f64(const cwn_embed_pool_desc_f64* descs, int n, cwn_stream_t stream) {
    return launch_pool<double>(descs, n, stream);
}

extern "C" int cwn_agnostic_head_f32(const cwn_agnostic_head_desc* desc, cwn_stream_t stream) {
    return launch_head<float>(desc, stream);
}

extern "C" int cwn_agnostic_head_f64(const cwn_agnostic_head_desc_f64* desc, cwn_stream_t stream) {
    return launch_head<double>(desc, stream);
}
