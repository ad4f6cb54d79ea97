// cwn_chain_f32.hip -- the update and combine networks of a SparseCINConv layer (mp/layers.py:193-199) in float32 inference, for
// every dimension in ONE launch, at ANY width 1 .. 128 and with any of the five activations: the float32 sibling of
// cwn_update_chain_f64 (cwn_dense_f64.hip).  See include/cwn_hip.h, "The float32 update chain".
//
//   cwn_update_chain_f32   u   = act(aff1(act(aff0(in_up W0^T + b0)) W1^T + b1))
//                          b   = act(aff3(act(aff2(in_b  W2^T + b2)) W3^T + b3))
//                          out = act(aff4(cat(u, b) W4^T + b4))              aff(z) = z * scale + shift, each part optional
//
// cwn_update_mlp_f32 (cwn_mlp.hip) is the fast form of this at 64 / 128 with ReLU -- a bf16 split on packed weights; this
// file is the form for everything else (hidden 48 / 32 / 16, a first layer over raw features, elu / tanh / sigmoid / id),
// where the networks otherwise run as a grouped launch per stage with the hidden activations in memory, or as torch
// modules.  A workgroup of four wave64s owns CWN_CHAIN_F32_TM = 32 rows of one dimension:
//   1. both inputs go into two LDS panels pa[32][132], pb[32][132] (columns [F, F rounded up to 16) and rows at or beyond
//      the row count as zeros: nothing of such a row is read from memory).
//   2. a stage is a panel times a weight on v_mfma_f32_16x16x4_f32 (exact fp32) with the operand roles and K-slab walk of
//      cwn_gin_tile.h: A = 16 weight rows (output columns), B = 16 panel rows, K in slabs of 16 in which lane group
//      g = lane >> 4 owns k = 4g .. 4g + 3 -- the panel fragment is one 16-byte LDS read, a lane's four accumulator
//      registers are four consecutive output columns of one row.  (The tile code is cwn_chain_tile.h, shared with
//      cwn_branches_f32.hip; not cwn_gin_tile.h's product: a weight here has a row stride -- the two halves of W4 -- and the
//      combine continues an accumulator.)  Weights come straight from
//      global memory, row-major as torch.nn.Linear holds them, as 16-byte vectors where width and alignment allow.
//   3. bias, affine and activation in the accumulator layout; the result goes to a panel, never to memory:
//      pa -> ph -> pa (u), pb -> ph -> pb (b): the hidden panel is shared, a branch's result overwrites its input.
//   4. combine: ONE accumulator over pa against W4[:, :H] and then pb against W4[:, H:] -- the K-concatenation without a
//      concatenation -- the epilogue, one 16-byte store per lane and tile where out allows (edge columns and rows at or
//      beyond the count masked).
// No atomics, no split of K across lanes that depends on anything but the widths: an output element is one chain of
// products in a k order fixed by (F, H), so a row has the same bits alone or anywhere in any batch.
// LDS (static): update_chain_f32 (3 x 32 x 132) elements = 50688 B in float32.
#include "cwn_chain_tile.h"
#include "cwn_check.h"
#include "cwn_group.h"

namespace {

struct ChainBatch {
    cwn_chain_desc_f32 d[CWN_CHAIN_F32_MAX_DIMS];
    int32_t blk_start[CWN_CHAIN_F32_MAX_DIMS + 1];
    int32_t n;
};

__global__ __launch_bounds__(kThreads) void update_chain_f32_kernel(ChainBatch B) {
    __shared__ __attribute__((aligned(16))) float pa[kTM * kLdp];       // in_up, then u
    __shared__ __attribute__((aligned(16))) float pb[kTM * kLdp];       // in_b, then b
    __shared__ __attribute__((aligned(16))) float ph[kTM * kLdp];       // the hidden activation of the branch at work
    const int di = cwn::group_of<CWN_CHAIN_F32_MAX_DIMS>(B.blk_start, B.n, (int)blockIdx.x);
    const cwn_chain_desc_f32 D = B.d[di];                // by value (a reference puts the batch struct in scratch)
    const int64_t row0 = (int64_t)((int)blockIdx.x - B.blk_start[di]) * kTM;
    const int64_t n = cwn::rows_clamped(D.m_dev, D.n);   // (D.n: the capacity)
    if (row0 >= n) return;                               // (uniform: before any barrier)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int F = D.F, H = D.H, act = D.act;

    load_panel(pa, D.in_up, D.ld_up, row0, n, F, tid);
    load_panel(pb, D.in_b, D.ld_b, row0, n, F, tid);
    __syncthreads();

    f32x4 acc[kCT][kRT];
    clear(acc);                                          // update_up_nn
    product(acc, pa, D.W[0], F, F, H, wave, j, g);
    to_panel(ph, acc, H, D.bias[0], D.scale[0], D.shift[0], act, wave, j, g);
    __syncthreads();
    clear(acc);
    product(acc, ph, D.W[1], H, H, H, wave, j, g);
    to_panel(pa, acc, H, D.bias[1], D.scale[1], D.shift[1], act, wave, j, g);      // (pa was last read before the barrier above)
    __syncthreads();                                     // every wave has read ph
    clear(acc);                                          // update_boundaries_nn
    product(acc, pb, D.W[2], F, F, H, wave, j, g);
    to_panel(ph, acc, H, D.bias[2], D.scale[2], D.shift[2], act, wave, j, g);
    __syncthreads();
    clear(acc);
    product(acc, ph, D.W[3], H, H, H, wave, j, g);
    to_panel(pb, acc, H, D.bias[3], D.scale[3], D.shift[3], act, wave, j, g);
    __syncthreads();
    clear(acc);                                          // combine_nn: k = 0 .. H-1 from u, H .. 2H-1 from b, one accumulator
    product(acc, pa, D.W[4], 2 * H, H, H, wave, j, g);
    product(acc, pb, D.W[4] + H, 2 * H, H, H, wave, j, g);

    // (written out, not cwn_chain_tile.h's to_out, which stands for the same text: with the call this kernel's registers
    //  and assembly change -- tools/isa_diff.sh)
    float* __restrict__ out = D.out;
    const int64_t ld_out = D.ld_out;
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
                y[q] = n0 + q < H ? epilogue(acc[ct][rt][q], n0 + q, D.bias[4], D.scale[4], D.shift[4], act) : 0.f;
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

extern "C" int cwn_update_chain_f32(const cwn_chain_desc_f32* descs, int n_dims, cwn_stream_t stream_) {
    if (descs == nullptr || n_dims < 1 || n_dims > CWN_CHAIN_F32_MAX_DIMS) return CWN_ERR_BAD_ARG;
    ChainBatch B{};
    B.n = n_dims;
    cwn::BlockFill fill(B.blk_start);
    for (int i = 0; i < n_dims; ++i) {
        const cwn_chain_desc_f32& D = descs[i];
        if (D.n < 0 || D.F < 1 || D.F > kMaxWidth || D.H < 1 || D.H > kMaxWidth || !known_act(D.act)) return CWN_ERR_BAD_ARG;
        if (D.n > 0) {
            if (D.in_up == nullptr || D.in_b == nullptr || D.out == nullptr) return CWN_ERR_BAD_ARG;
            if (D.ld_up < D.F || D.ld_b < D.F || D.ld_out < D.H) return CWN_ERR_BAD_ARG;
            for (int s = 0; s < 5; ++s)
                if (D.W[s] == nullptr) return CWN_ERR_BAD_ARG;
            if (!al4(D.in_up) || !al4(D.in_b) || !al4(D.out) || !al8(D.m_dev)) return CWN_ERR_ALIGN;
            for (int s = 0; s < 5; ++s)
                if (!al4(D.W[s]) || !al4(D.bias[s]) || !al4(D.scale[s]) || !al4(D.shift[s])) return CWN_ERR_ALIGN;
        }
        B.d[i] = D;
        if (!fill.push(i, (D.n + kTM - 1) / kTM)) return CWN_ERR_TOO_LARGE;
    }
    const int64_t blocks = fill.close(n_dims);
    if (blocks == 0) return CWN_OK;
    update_chain_f32_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_>>>(B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}
