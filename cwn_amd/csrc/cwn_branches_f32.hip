// cwn_branches_f32.hip -- the update and combine networks of a CINppConv layer (mp/layers.py:255-260) in float32 inference, for
// every dimension in ONE launch, with three or four branches, at ANY width 1 .. 128 and with any of the five activations: what
// cwn_update_chain_f32 (cwn_chain_f32.hip) is for the two branches of SparseCINConv.  See include/cwn_hip.h, "The float32
// update branches".
//
//   cwn_update_branches_f32   h_k = act(aff(act(aff(in_k W[2k]^T + b[2k])) W[2k+1]^T + b[2k+1]))      k = 0 .. nb-1, nb = 3 | 4
//                             out = act(aff(cat(h_0 .. h_{nb-1}) W[2nb]^T + b[2nb]))     aff(z) = z * scale + shift, each part optional
//
// cwn_update_mlp3_f32 (cwn_mlp3.hip) is the fast form of this at 64 / 128 with ReLU, three branches and an (F, F) first layer
// -- a bf16 split on packed weights; this file is the form for everything else.  The tile code is cwn_chain_tile.h, shared
// with cwn_chain_f32.hip: a workgroup of four wave64s owns CWN_BRANCHES_F32_TM = 32 rows of one dimension and runs the
// branches ONE AFTER THE OTHER, so that LDS does not grow with nb:
//   1. in_k goes into the panel px[32][132] (columns [F, F rounded up to 16) and rows at or beyond the row count as zeros:
//      nothing of such a row is read from memory);
//   2. px -> ph (the hidden activation) -> px (h_k): two products on v_mfma_f32_16x16x4_f32 (exact fp32) with the weights
//      straight from global memory, row-major as torch.nn.Linear holds them; bias, affine and activation in the accumulator
//      layout; the results go to a panel, never to memory;
//   3. combine_acc += px . W[2nb][:, kH:(k+1)H]^T -- ONE accumulator (16 registers per lane) that stays in registers across
//      the branches, branch ascending and k ascending within a branch: the K-concatenation without a concatenation;
//   4. after the last branch the epilogue, one 16-byte store per lane and tile where out allows (edge columns and rows at
//      or beyond the count masked).
// No third panel: the next branch's input is loaded behind the combine product of the current one, not under it (the
// launch is a few microseconds on the batches it serves; tools/bench_branches_f32.py has the figures).
// No atomics, no split of K across lanes that depends on anything but the widths: an output element is one chain of
// products in a k order fixed by (F, H, nb), so a row has the same bits alone or anywhere in any batch.
// LDS (static): update_branches_f32 (2 x 32 x 132) elements = 33792 B in float32.
#include "cwn_chain_tile.h"
#include "cwn_check.h"
#include "cwn_group.h"

namespace {

constexpr int kMaxBranches = CWN_BRANCHES_F32_MAX_BRANCHES;

static_assert(CWN_BRANCHES_F32_MAX_WIDTH == kMaxWidth && CWN_BRANCHES_F32_TM == kTM, "the tile of cwn_chain_tile.h");
static_assert(CWN_BRANCHES_F32_STAGES == 2 * kMaxBranches + 1, "two stages per branch and the combine");

struct BranchesBatch {
    cwn_branches_desc_f32 d[CWN_BRANCHES_F32_MAX_DIMS];
    int32_t blk_start[CWN_BRANCHES_F32_MAX_DIMS + 1];
    int32_t n;
};
static_assert(sizeof(BranchesBatch) < 4096, "the by-value launch record stays below 4 KB of kernel arguments");

__global__ __launch_bounds__(kThreads) void update_branches_f32_kernel(BranchesBatch B) {
    __shared__ __attribute__((aligned(16))) float px[kTM * kLdp];       // in_k, then h_k
    __shared__ __attribute__((aligned(16))) float ph[kTM * kLdp];       // the hidden activation of the branch at work
    const int di = cwn::group_of<CWN_BRANCHES_F32_MAX_DIMS>(B.blk_start, B.n, (int)blockIdx.x);
    // The record of this dimension is READ WHERE IT IS USED, from the kernel-argument segment (B is the kernel's one argument,
    // at offset 0): a copy by value, as in cwn_chain_f32.hip, is 100 scalar registers here and spills them.
    typedef const __attribute__((address_space(4))) BranchesBatch* KernArgs;
    const __attribute__((address_space(4))) cwn_branches_desc_f32& D = ((KernArgs)__builtin_amdgcn_kernarg_segment_ptr())->d[di];
    const int64_t row0 = (int64_t)((int)blockIdx.x - B.blk_start[di]) * kTM;
    const int64_t cap = D.n;
    const int64_t n = cwn::rows_clamped(D.m_dev, cap);   // (D.n: the capacity)
    if (row0 >= n) return;                               // (uniform: before any barrier)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int F = D.F, H = D.H, act = D.act, nb = D.nb;
    constexpr int c4 = 2 * kMaxBranches, c3 = c4 - 2;    // the combine stage, 2 nb, with four and with three branches
    const bool four = nb == kMaxBranches;                // (uniform; a select of two constants, not an index)
    const float* __restrict__ Wc = four ? D.W[c4] : D.W[c3];

    f32x4 comb[kCT][kRT], acc[kCT][kRT];
    clear(comb);
#pragma unroll
    for (int k = 0; k < kMaxBranches; ++k) {             // (unrolled: the descriptor's arrays are indexed by constants)
        if (k >= nb) break;                              // (uniform)
        if (k > 0) __syncthreads();                      // every wave has read px (the combine product of branch k - 1)
        load_panel(px, D.ins[k], D.ld_in[k], row0, n, F, tid);
        __syncthreads();
        clear(acc);
        product(acc, px, D.W[2 * k], F, F, H, wave, j, g);
        to_panel(ph, acc, H, D.bias[2 * k], D.scale[2 * k], D.shift[2 * k], act, wave, j, g);
        __syncthreads();
        clear(acc);
        product(acc, ph, D.W[2 * k + 1], H, H, H, wave, j, g);
        to_panel(px, acc, H, D.bias[2 * k + 1], D.scale[2 * k + 1], D.shift[2 * k + 1], act, wave, j, g);   // (px was last read before the barrier above)
        __syncthreads();
        product(comb, px, Wc + k * H, nb * H, H, H, wave, j, g);      // k' = kH .. (k + 1)H - 1 of the one accumulator
    }
    to_out(D.out, D.ld_out, row0, n, comb, H, four ? D.bias[c4] : D.bias[c3], four ? D.scale[c4] : D.scale[c3],
           four ? D.shift[c4] : D.shift[c3], act, wave, j, g);
}

}  // namespace

extern "C" int cwn_update_branches_f32(const cwn_branches_desc_f32* descs, int n_dims, cwn_stream_t stream_) {
    if (descs == nullptr || n_dims < 1 || n_dims > CWN_BRANCHES_F32_MAX_DIMS) return CWN_ERR_BAD_ARG;
    BranchesBatch B{};
    B.n = n_dims;
    cwn::BlockFill fill(B.blk_start);
    for (int i = 0; i < n_dims; ++i) {
        const cwn_branches_desc_f32& D = descs[i];
        if (D.n < 0 || D.F < 1 || D.F > kMaxWidth || D.H < 1 || D.H > kMaxWidth || !known_act(D.act)) return CWN_ERR_BAD_ARG;
        if (D.nb < CWN_BRANCHES_F32_MIN_BRANCHES || D.nb > kMaxBranches) return CWN_ERR_BAD_ARG;
        const int stages = 2 * D.nb + 1;
        if (D.n > 0) {
            if (D.out == nullptr || D.ld_out < D.H) return CWN_ERR_BAD_ARG;
            for (int k = 0; k < D.nb; ++k)
                if (D.ins[k] == nullptr || D.ld_in[k] < D.F) return CWN_ERR_BAD_ARG;
            for (int s = 0; s < stages; ++s)
                if (D.W[s] == nullptr) return CWN_ERR_BAD_ARG;
            if (!al4(D.out) || !al8(D.m_dev)) return CWN_ERR_ALIGN;
            for (int k = 0; k < D.nb; ++k)
                if (!al4(D.ins[k])) return CWN_ERR_ALIGN;
            for (int s = 0; s < stages; ++s)
                if (!al4(D.W[s]) || !al4(D.bias[s]) || !al4(D.scale[s]) || !al4(D.shift[s])) return CWN_ERR_ALIGN;
        }
        B.d[i] = D;
        if (!fill.push(i, (D.n + kTM - 1) / kTM)) return CWN_ERR_TOO_LARGE;
    }
    const int64_t blocks = fill.close(n_dims);
    if (blocks == 0) return CWN_OK;
    update_branches_f32_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_>>>(B);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}
