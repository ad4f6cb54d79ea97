// cwn_oriented.hip -- OrientedConv (mp/layers.py:430-470) as ONE launch per layer: the edge-flow models EdgeOrient and
// EdgeMPNN (mp/models.py:476-615).
//
//   cwn_oriented_layer_f32   out = act( [ x | A_up o_up . x | A_dn o_dn . x ] . [ W ; W_up ; W_dn ]^T )
//   cwn_oriented_dz_f32      dz = dout * act'(out)                      (the backward's first step; act' is a function of out)
//
// The three update maps of the layer carry no bias (a bias would break the orientation equivariance), so the layer is one
// product over the concatenation of x and its two oriented aggregates.  A workgroup owns TM destination rows:
//   1. every (row, column) of the tile is one work item: it copies x and folds the row's entries of each stream in CSR
//      order -- the fold of cwn_aggregate_body.h, entry by entry, with the narrow-width split it takes for rows above 16
//      entries, so the optional agg_out is bit-identical to cwn_aggregate_f32 -- into an LDS panel [TM, K], K = 3w padded
//      to whole slabs of 16 with zeros.  The aggregates never reach HBM (agg_out: training only, for the weight gradients).
//   2. the panel times the weights on v_mfma_f32_16x16x4_f32 (exact fp32, the instruction of cwn_gemm.hip) with the
//      operand roles of cwn_gemm.hip: A = 16 weight rows (output columns), B = 16 panel rows, K walked in slabs of 16 in
//      which lane group g = lane >> 4 owns k = 4g .. 4g + 3 -- the panel fragment is one 16-byte LDS read, and a lane's four
//      accumulator registers are four consecutive output columns of one row.  Weights come straight from global memory
//      (at most 192 KiB for the whole layer: L2-resident): row-major [H, w] as torch.nn.Linear holds them, or the same
//      matrix read transposed (w_trans: the data gradient dx = [dZ | A^T o dZ ...] . [W ; W_up ; W_dn]).
//   3. activation in the accumulator layout, one 16-byte store per lane and tile (edge columns masked).
// Absent streams (rowptr == NULL) and an absent self map (w_self == NULL) take no room in the panel.
#include <hip/hip_runtime.h>
#include "../../include/cwn_hip.h"
#include "cwn_act.h"
#include "cwn_check.h"
#include "cwn_group.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSplitRow = 16;                     // = cwn_aggregate_body.h: rows above it take the split fold at narrow widths
constexpr int kMaxWidth = 128;

struct OrientedArgs {
    cwn_oriented_desc d;
    int32_t split;       // entry slots of the narrow fold (1: every row sequential), as cwn_aggregate_f32 picks them
    int32_t n_seg;       // blocks of the panel: self (when w_self), up, down (when present)
    int32_t kp;          // panel width: n_seg * w rounded up to 16
    int32_t w_vec;       // weights readable as 16-byte vectors along k (untransposed, w % 4 == 0, aligned)
    int32_t out_vec;     // out rows take 16-byte stores
};

struct Plan {
    const int32_t* rowptr;
    const int32_t* col;
    const int32_t* perm;
    const float* orient;
};

// Entries p0, p0 + step, ... < p1 of one row, column c: acc += x[col[p]][c] * orient[perm[p]], one after the other (four
// entries' loads in flight, added in entry order; mul and add stay separate instructions: -ffp-contract=off).
__device__ __forceinline__ float fold_entries(const float* __restrict__ x, int64_t ldx, int c, const Plan& S, int p0, int p1,
                                              int step) {
    float acc = 0.f;
    int p = p0;
    for (; p + 3 * step < p1; p += 4 * step) {
        int j[4];
        float o[4], a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) j[u] = S.col[p + u * step];
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = S.orient != nullptr ? S.orient[S.perm[p + u * step]] : 1.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = x[(int64_t)j[u] * ldx + c];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = acc + (S.orient != nullptr ? a[u] * o[u] : a[u]);
    }
    for (; p < p1; p += step) {
        const float a = x[(int64_t)S.col[p] * ldx + c];
        acc = acc + (S.orient != nullptr ? a * S.orient[S.perm[p]] : a);
    }
    return acc;
}

// One row of one stream.  `split` > 1 (narrow widths) and more than kSplitRow entries: slot e folds every split-th entry
// and the slots are added pairwise, neighbours first -- the xor tree of fold_range_split in cwn_aggregate_body.h as its
// slot 0 sees it (float addition commutes, so the tree's result does not depend on which side is the lane's own).
__device__ __forceinline__ float fold_row(const float* __restrict__ x, int64_t ldx, int c, const Plan& S, int start, int end,
                                          int split) {
    if (split <= 1 || end - start <= kSplitRow) return fold_entries(x, ldx, c, S, start, end, 1);
    float l0 = 0.f, l1 = 0.f, l2 = 0.f, res = 0.f;
    for (int e = 0; e < split; ++e) {
        float v = fold_entries(x, ldx, c, S, start + e, end, split);
        if (e & 1) {
            v = l0 + v;
            if (e & 2) {
                v = l1 + v;
                if (e & 4) v = l2 + v;
                else l2 = v;
            } else {
                l1 = v;
            }
        } else {
            l0 = v;
        }
        res = v;
    }
    return res;      // (split is a power of two <= 8: the last slot closes every open level)
}

// element (k, n) of block s of the stacked weights: k < w input column, n < H output column
__device__ __forceinline__ float weight_at(const float* __restrict__ W, int k, int n, int w, int H, bool trans) {
    return trans ? W[(int64_t)k * H + n] : W[(int64_t)n * w + k];
}

template <int TM>
__global__ __launch_bounds__(kThreads) void oriented_layer_kernel(OrientedArgs P) {
    extern __shared__ __attribute__((aligned(16))) float panel[];       // [TM][ldp]
    constexpr int RT = TM / 16;                   // row tiles of the product, all of them on every wave
    constexpr int CT = kMaxWidth / 16 / kWaves;   // column tiles per wave (2)
    const int tid = threadIdx.x;
    const int w = P.d.w, H = P.d.H, kp = P.kp, ldp = P.kp + 4;
    const int K = P.n_seg * w;
    const int64_t ldx = P.d.ldx;
    const float* __restrict__ x = P.d.x;
    const int64_t row0 = (int64_t)blockIdx.x * TM;
    const int64_t m = cwn::rows_capped(P.d.m_dev, (int64_t)P.d.n);
    if (row0 >= m) return;                        // (uniform: nothing of this tile exists)

    // ---- 1. the panel -------------------------------------------------------------------------------------------------
    const bool has_self = P.d.w_self != nullptr;
    const Plan up{P.d.up_rowptr, P.d.up_col, P.d.up_perm, P.d.up_orient};
    const Plan dn{P.d.dn_rowptr, P.d.dn_col, P.d.dn_perm, P.d.dn_orient};
    const int off_up = has_self ? w : 0;
    const int off_dn = off_up + (up.rowptr != nullptr ? w : 0);
    float* __restrict__ agg = P.d.agg_out;
    const int padc = kp - K;
    for (int i = tid; i < TM * padc; i += kThreads) {
        const int r = i / padc;
        panel[r * ldp + K + (i - r * padc)] = 0.f;
    }
    for (int i = tid; i < TM * w; i += kThreads) {
        const int r = i / w, c = i - r * w;
        const int64_t row = row0 + r;
        const bool live = row < m;                // rows past the count: zeros in the panel, nothing read, nothing stored
        if (has_self) panel[r * ldp + c] = live ? x[row * ldx + c] : 0.f;
        if (up.rowptr != nullptr) {
            float v = 0.f;
            if (live) v = fold_row(x, ldx, c, up, up.rowptr[row], up.rowptr[row + 1], P.split);
            panel[r * ldp + off_up + c] = v;
            if (agg != nullptr && live) agg[row * (2 * w) + c] = v;
        } else if (agg != nullptr && live) {
            agg[row * (2 * w) + c] = 0.f;
        }
        if (dn.rowptr != nullptr) {
            float v = 0.f;
            if (live) v = fold_row(x, ldx, c, dn, dn.rowptr[row], dn.rowptr[row + 1], P.split);
            panel[r * ldp + off_dn + c] = v;
            if (agg != nullptr && live) agg[row * (2 * w) + w + c] = v;
        } else if (agg != nullptr && live) {
            agg[row * (2 * w) + w + c] = 0.f;
        }
    }
    __syncthreads();

    // ---- 2. panel . weights^T -------------------------------------------------------------------------------------------
    const int lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const bool trans = P.d.w_trans != 0;
    // the blocks' weights in panel order (self, up, down; an absent one closes the gap)
    const bool has_up = up.rowptr != nullptr;
    const float* __restrict__ w0 = has_self ? P.d.w_self : (has_up ? P.d.w_up : P.d.w_dn);
    const float* __restrict__ w1 = has_self && has_up ? P.d.w_up : P.d.w_dn;
    const float* __restrict__ w2 = P.d.w_dn;
    const int n_tiles = (H + 15) >> 4;
    f32x4 acc[CT][RT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[ct][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kp; k0 += 16) {
        const int kk = k0 + 4 * g;                // this lane group's four k of the slab
        float wf[CT][4];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int n = (wave + kWaves * ct) * 16 + j;
#pragma unroll
            for (int t = 0; t < 4; ++t) wf[ct][t] = 0.f;
            if (n >= H) continue;
            if (P.w_vec) {                        // (w % 4 == 0: the four k lie in one block)
                if (kk < K) {
                    const int s = kk >= 2 * w ? 2 : (kk >= w ? 1 : 0);
                    const float* W = s == 0 ? w0 : (s == 1 ? w1 : w2);
                    const float4 v = *reinterpret_cast<const float4*>(W + (int64_t)n * w + (kk - s * w));
                    wf[ct][0] = v.x; wf[ct][1] = v.y; wf[ct][2] = v.z; wf[ct][3] = v.w;
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int k = kk + t;
                    if (k < K) {
                        const int s = k >= 2 * w ? 2 : (k >= w ? 1 : 0);
                        const float* W = s == 0 ? w0 : (s == 1 ? w1 : w2);
                        wf[ct][t] = weight_at(W, k - s * w, n, w, H, trans);
                    }
                }
            }
        }
        f32x4 xb[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) xb[rt] = *reinterpret_cast<const f32x4*>(panel + (rt * 16 + j) * ldp + kk);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                if (wave + kWaves * ct >= n_tiles) continue;          // (wave-uniform)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    acc[ct][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ct][t], xb[rt][t], acc[ct][rt], 0, 0, 0);
            }
    }

    // ---- 3. acc[ct][rt][q] = z[row0 + rt * 16 + j][(wave + 4 ct) * 16 + 4 g + q] ------------------------------------------
    const int act = P.d.act;
    float* __restrict__ out = P.d.out;
    const int64_t ldout = P.d.ldout;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int n0 = (wave + kWaves * ct) * 16 + 4 * g;
        if (n0 >= H) continue;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int64_t row = row0 + rt * 16 + j;
            if (row >= m) continue;
            float y[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) y[q] = activate_rt(acc[ct][rt][q], act);
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

struct DzArgs {
    const float* dout;
    const float* out;
    float* dz;
    const int64_t* m_dev;
    int64_t n, lddout, ldout, lddz;
    int32_t H, act;
};

__global__ __launch_bounds__(kThreads) void oriented_dz_kernel(DzArgs P) {
    const int64_t m = cwn::rows_capped(P.m_dev, (int64_t)P.n);
    const int64_t total = m * P.H;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t r = e / P.H;
        const int c = (int)(e - r * P.H);
        P.dz[r * P.lddz + c] = P.dout[r * P.lddout + c] * act_grad(P.act, P.out[r * P.ldout + c]);
    }
}

inline int tile_rows(int w) { return CWN_ORIENTED_TM(w); }

// The entry slots cwn_aggregate_f32 gives a row of width w (its vector width by w and the alignment of the gathered matrix
// and of the output; fewer than 8 feature lanes: the other lanes of the 8 are entry slots).
inline int split_of(const cwn_oriented_desc& D) {
    int vec = D.w % 4 == 0 ? 4 : (D.w % 2 == 0 ? 2 : 1);
    const void* ptrs[] = {D.x, D.agg_out};
    for (const void* p : ptrs) {
        if (vec == 4 && !al16(p)) vec = al8(p) ? 2 : 1;
        if (vec == 2 && !al8(p)) vec = 1;
    }
    int lanes = 1;
    while (lanes < (D.w + vec - 1) / vec) lanes <<= 1;
    return lanes < 8 ? 8 / lanes : 1;
}

int check(const cwn_oriented_desc* desc) {
    if (desc == nullptr) return CWN_ERR_BAD_ARG;
    const cwn_oriented_desc& D = *desc;
    if (D.w < 1 || D.w > kMaxWidth || D.H < 1 || D.H > kMaxWidth || D.n < 0) return CWN_ERR_BAD_ARG;
    if (!known_act(D.act)) return CWN_ERR_BAD_ARG;
    if ((D.up_rowptr == nullptr) != (D.w_up == nullptr) || (D.dn_rowptr == nullptr) != (D.w_dn == nullptr)) return CWN_ERR_BAD_ARG;
    if (D.up_rowptr != nullptr && (D.up_col == nullptr || (D.up_orient != nullptr && D.up_perm == nullptr))) return CWN_ERR_BAD_ARG;
    if (D.dn_rowptr != nullptr && (D.dn_col == nullptr || (D.dn_orient != nullptr && D.dn_perm == nullptr))) return CWN_ERR_BAD_ARG;
    if (D.n > 0 && (D.x == nullptr || D.out == nullptr || D.ldx < D.w || D.ldout < D.H)) return CWN_ERR_BAD_ARG;
    if (D.out != nullptr && ((const float*)D.out == D.x || D.out == D.agg_out)) return CWN_ERR_BAD_ARG;
    const void* ptrs[] = {D.x, D.up_rowptr, D.up_col, D.up_perm, D.up_orient, D.w_up, D.dn_rowptr, D.dn_col, D.dn_perm,
                          D.dn_orient, D.w_dn, D.w_self, D.out, D.agg_out};
    for (const void* p : ptrs)
        if (!al4(p)) return CWN_ERR_ALIGN;
    if (!al8(D.m_dev)) return CWN_ERR_ALIGN;
    if ((D.n + tile_rows(D.w) - 1) / tile_rows(D.w) >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    return CWN_OK;
}

}  // namespace

extern "C" int cwn_oriented_layer_f32(const cwn_oriented_desc* desc, cwn_stream_t stream_) {
    const int rc = check(desc);
    if (rc != CWN_OK) return rc;
    if (desc->n == 0) return CWN_OK;
    OrientedArgs P{};
    P.d = *desc;
    const cwn_oriented_desc& D = P.d;
    P.split = split_of(D);
    P.n_seg = (D.w_self != nullptr ? 1 : 0) + (D.up_rowptr != nullptr ? 1 : 0) + (D.dn_rowptr != nullptr ? 1 : 0);
    P.kp = (P.n_seg * D.w + 15) / 16 * 16;
    P.w_vec = D.w_trans == 0 && D.w % 4 == 0 && al16(D.w_self) && al16(D.w_up) && al16(D.w_dn);
    P.out_vec = al16(D.out) && D.ldout % 4 == 0;
    const int tm = tile_rows(D.w);
    const unsigned blocks = (unsigned)((D.n + tm - 1) / tm);
    const size_t lds = (size_t)tm * (size_t)(P.kp + 4) * sizeof(float);
    hipStream_t stream = (hipStream_t)stream_;
    if (tm == 128) oriented_layer_kernel<128><<<dim3(blocks), dim3(kThreads), lds, stream>>>(P);
    else oriented_layer_kernel<32><<<dim3(blocks), dim3(kThreads), lds, stream>>>(P);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

extern "C" int cwn_oriented_dz_f32(const float* dout, const float* out, float* dz, int64_t n, int32_t H, int64_t lddout,
                                   int64_t ldout, int64_t lddz, int32_t act, const int64_t* m_dev, cwn_stream_t stream_) {
    if (n < 0 || H < 1 || H > kMaxWidth || !known_act(act)) return CWN_ERR_BAD_ARG;
    if (n > 0 && (dout == nullptr || out == nullptr || dz == nullptr || lddout < H || ldout < H || lddz < H)) return CWN_ERR_BAD_ARG;
    if (!al4(dout) || !al4(out) || !al4(dz) || !al8(m_dev)) return CWN_ERR_ALIGN;
    if (n == 0) return CWN_OK;
    const int64_t want = (n * H + kThreads - 1) / kThreads;
    const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
    DzArgs P{dout, out, dz, m_dev, n, lddout, ldout, lddz, H, act};
    oriented_dz_kernel<<<dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream_>>>(P);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}
