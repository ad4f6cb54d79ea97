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
//      the LDS panel sp[32][132]; columns [w, w rounded up to 16) and rows past n hold zeros.  (n: the host count, or in
//      cwn_gin_layer_dev_f32 the device count clamped to the capacity -- live_rows, cwn_gin_tile.h; a workgroup whose first
//      row is not below it returns before it reads anything, rows behind it are neither read nor written.)
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
#include "cwn_gin_tile.h"     // the geometry, the product, the epilogue, the two stages and the checks: shared with cwn_gine.hip

namespace {

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

__global__ __launch_bounds__(kThreads) void gin_layer_kernel(GinArgs P, const int64_t* __restrict__ n_dev) {
    __shared__ __attribute__((aligned(16))) float sp[kTM * kLdp];       // s, [kTM][kLdp]
    __shared__ __attribute__((aligned(16))) float hp[kTM * kLdp];       // h
    const int tid = threadIdx.x;
    const int w = P.d.w;
    const int64_t ldx = P.d.ldx;
    const float* __restrict__ x = P.d.x;
    const int64_t n = live_rows(P, n_dev);        // (the host count, or the device count inside the capacity P.d.n)
    const int64_t row0 = (int64_t)blockIdx.x * kTM;
    if (row0 >= n) return;                        // (uniform; with a host count the grid has no such workgroup)

    // ---- 1. the panel of s ----------------------------------------------------------------------------------------------
    const int32_t* __restrict__ rowptr = P.d.rowptr;
    const int32_t* __restrict__ col = P.d.col;
    const float self = 1.f + (P.d.eps_dev != nullptr ? *P.d.eps_dev : 0.f);
    zero_panel_padding(sp, w, (w + 15) & ~15, tid);
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

    // ---- 2, 3, 4. the two stages (cwn_gin_tile.h) ---------------------------------------------------------------------------
    stages_from_panel(P, sp, hp, row0, n, tid);
}

}  // namespace

extern "C" int cwn_gin_layer_f32(const cwn_gin_desc* desc, cwn_stream_t stream_) {
    const int rc = gin_check(desc);
    if (rc != CWN_OK) return rc;
    if (desc->n == 0) return CWN_OK;
    const GinArgs P = gin_args(*desc);
    gin_layer_kernel<<<dim3(gin_blocks(P.d)), dim3(kThreads), 0, (hipStream_t)stream_>>>(P, nullptr);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

// The counted form: desc->n is the capacity (the grid, every address bound), *n_dev the rows that exist.
extern "C" int cwn_gin_layer_dev_f32(const cwn_gin_desc* desc, const int64_t* n_dev, cwn_stream_t stream_) {
    int rc = gin_check(desc);
    if (rc == CWN_OK) rc = gin_count_check(desc->n, n_dev);
    if (rc != CWN_OK) return rc;
    if (desc->n == 0) return CWN_OK;
    const GinArgs P = gin_args(*desc);
    gin_layer_kernel<<<dim3(gin_blocks(P.d)), dim3(kThreads), 0, (hipStream_t)stream_>>>(P, n_dev);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}
