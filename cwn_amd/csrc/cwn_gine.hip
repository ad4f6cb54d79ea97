// cwn_gine.hip -- a whole GINEConv (torch_geometric 1.6.3's definition, the layer of EmbedGIN, mp/molec_models.py:506-606) in
// inference as ONE launch.  See include/cwn_hip.h, "GINEConv as one launch".
//
//   cwn_gine_layer_f32  s   = (sum over the CSR entries p of row i, in CSR order, of relu(x[col[p], :] + e[eidx[p], :]))
//                             + (1 + eps) * x[i, :]
//                       h   = act( (s W1^T + b1) * scale1 + shift1 )
//                       out = act_post( act( (h W2^T + b2) * scale2 + shift2 ) )
//
// The geometry, the two products and the epilogues are those of gin_layer_kernel (cwn_gin.hip), from cwn_gin_tile.h: a
// workgroup of four wave64s owns CWN_GIN_TM = 32 destination rows, two LDS panels sp[32][132] and hp[32][132], exact-fp32
// v_mfma_f32_16x16x4_f32, widths 1 .. 128.  Only the fold differs: every (row, column) of the tile is one work item that walks
// its row's entries one after the other in CSR order, whatever the row's length -- four entries in flight, which is eight
// loads (x[col[p]][c] and e[eidx[p]][c]) -- and adds relu(x + e) in entry order.  The ReLU is cwn_relu (cwn_act.h): a NaN
// operand gives NaN, a -Inf message gives 0.  `eidx` is one int32 per CSR position and the kernel does not know what it
// means: the plan's shared-cell index (e holds one row per edge CELL and the [E, w] matrix of messages' attributes never
// exists) or the plan's perm (e holds one row per original entry, as a torch_geometric caller hands it).
// No atomics; every output element is a function of its row's entries in order and the weights alone.
// LDS (static): gine_layer (2 x 32 x 132) elements = 33792 B in float32.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_gin_tile.h"

namespace {

struct GineArgs {
    GinArgs g;
    const float* e;          // [n_e, w] row stride lde
    const int32_t* eidx;     // [E] row of e per CSR position
    int64_t lde;
};

// Entries p0 .. p1 - 1 of one row, column c: acc += relu(x[col[p]][c] + e[eidx[p]][c]), one after the other (four entries'
// loads -- eight loads -- in flight, added in entry order).
__device__ __forceinline__ float fold_entries(const float* __restrict__ x, int64_t ldx, const float* __restrict__ e, int64_t lde,
                                              int c, const int32_t* __restrict__ col, const int32_t* __restrict__ eidx, int p0,
                                              int p1) {
    float acc = 0.f;
    int p = p0;
    for (; p + 3 < p1; p += 4) {
        int j[4], k[4];
        float a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            j[u] = col[p + u];
            k[u] = eidx[p + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = x[(int64_t)j[u] * ldx + c];
            b[u] = e[(int64_t)k[u] * lde + c];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = acc + cwn_relu(a[u] + b[u]);
    }
    for (; p < p1; ++p) acc = acc + cwn_relu(x[(int64_t)col[p] * ldx + c] + e[(int64_t)eidx[p] * lde + c]);
    return acc;
}

__global__ __launch_bounds__(kThreads) void gine_layer_kernel(GineArgs A, const int64_t* __restrict__ n_dev) {
    __shared__ __attribute__((aligned(16))) float sp[kTM * kLdp];       // s, [kTM][kLdp]
    __shared__ __attribute__((aligned(16))) float hp[kTM * kLdp];       // h
    const GinArgs& P = A.g;
    const int tid = threadIdx.x;
    const int w = P.d.w;
    const int64_t ldx = P.d.ldx, lde = A.lde;
    const float* __restrict__ x = P.d.x;
    const float* __restrict__ e = A.e;
    const int64_t n = live_rows(P, n_dev);        // (the host count, or the device count inside the capacity P.d.n)
    const int64_t row0 = (int64_t)blockIdx.x * kTM;
    if (row0 >= n) return;                        // (uniform; with a host count the grid has no such workgroup)

    // ---- 1. the panel of s ----------------------------------------------------------------------------------------------
    const int32_t* __restrict__ rowptr = P.d.rowptr;
    const int32_t* __restrict__ col = P.d.col;
    const int32_t* __restrict__ eidx = A.eidx;
    const float self = 1.f + (P.d.eps_dev != nullptr ? *P.d.eps_dev : 0.f);
    zero_panel_padding(sp, w, (w + 15) & ~15, tid);
    for (int i = tid; i < kTM * w; i += kThreads) {
        const int r = i / w, c = i - r * w;
        const int64_t row = row0 + r;
        float v = 0.f;                            // rows past n: zeros in the panel, nothing read, nothing stored
        if (row < n) {
            if (rowptr != nullptr) v = fold_entries(x, ldx, e, lde, c, col, eidx, rowptr[row], rowptr[row + 1]);
            v = v + self * x[row * ldx + c];
        }
        sp[r * kLdp + c] = v;
    }
    __syncthreads();

    // ---- 2, 3, 4. the two stages (cwn_gin_tile.h) ---------------------------------------------------------------------------
    stages_from_panel(P, sp, hp, row0, n, tid);
}

// The checks of a cwn_gine_desc, before any HIP call: those of its cwn_gin_desc first.
inline int gine_check(const cwn_gine_desc* desc) {
    if (desc == nullptr) return CWN_ERR_BAD_ARG;
    const int rc = gin_check(&desc->g);
    if (rc != CWN_OK) return rc;
    if (desc->g.rowptr != nullptr && (desc->e == nullptr || desc->eidx == nullptr || desc->lde < desc->g.w || desc->n_e < 0))
        return CWN_ERR_BAD_ARG;
    if (!al4(desc->e) || !al4(desc->eidx)) return CWN_ERR_ALIGN;
    return CWN_OK;
}

inline int gine_launch(const cwn_gine_desc* desc, const int64_t* n_dev, cwn_stream_t stream_) {
    GineArgs A{};
    A.g = gin_args(desc->g);
    A.e = desc->e;
    A.eidx = desc->eidx;
    A.lde = desc->lde;
    gine_layer_kernel<<<dim3(gin_blocks(desc->g)), dim3(kThreads), 0, (hipStream_t)stream_>>>(A, n_dev);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

}  // namespace

extern "C" int cwn_gine_layer_f32(const cwn_gine_desc* desc, cwn_stream_t stream_) {
    const int rc = gine_check(desc);
    if (rc != CWN_OK) return rc;
    if (desc->g.n == 0) return CWN_OK;
    return gine_launch(desc, nullptr, stream_);
}

// The counted form: desc->g.n is the capacity (the grid, every address bound), *n_dev the rows that exist.
extern "C" int cwn_gine_layer_dev_f32(const cwn_gine_desc* desc, const int64_t* n_dev, cwn_stream_t stream_) {
    int rc = gine_check(desc);
    if (rc == CWN_OK) rc = gin_count_check(desc->g.n, n_dev);
    if (rc != CWN_OK) return rc;
    if (desc->g.n == 0) return CWN_OK;
    return gine_launch(desc, n_dev, stream_);
}
