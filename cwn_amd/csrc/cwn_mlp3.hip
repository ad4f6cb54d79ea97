// cwn_mlp3.hip -- the update / combine networks of a CIN++ layer in ONE launch (inference).
//
// What it replaces (reference): mp/layers.py:252-260, CINppCochainConv.forward behind propagate()
//     out_up = update_up_nn(out_up); out_down = update_down_nn(out_down); out_boundaries = update_boundaries_nn(out_boundaries)
//     return combine_nn(torch.cat([out_up, out_down, out_boundaries], dim=-1))
// with update_*_nn = [Linear(F->F), BatchNorm, ReLU] x 2 (mp/layers.py:383-410) and combine_nn = [Linear(3F->F), BatchNorm,
// ReLU] (:411-414), BatchNorm in eval mode folded into a per-column affine.  Until round 6 the library ran this as two grouped
// GEMM launches over nine descriptors + torch.cat + the combine as torch modules (~0.13 ms of a 0.16-ms layer at the ZINC
// batch of 128: profiles/r5_*cinpp*).
//
// The workgroup design is csrc/cwn_tile.h's (read its header first; csrc/cwn_mlp.hip is the two-branch kernel of SparseCIN
// layers on the same design): a workgroup of 8 waves takes 4096 / F rows of one cochain dimension through all seven Linear
// layers without leaving the CU, the activations of a stage go from the accumulators through the epilogue straight into the
// bf16 planes the next stage multiplies, the weights stream through two register sets one multiplication ahead.  What three
// branches change:
//   * the combine is accumulated BRANCH BY BRANCH: as soon as h_k = update_k(x_k) is in LDS its block of the combine product,
//     Wc[:, kF:(k+1)F] h_k, is added to a second accumulator set -- in the order of the cat (up, down, boundaries), i.e. the
//     k steps of a K = 3F product in their natural order -- so h_k's buffer is free for the next branch and THREE plane buffers
//     (78 KB at F = 128) serve three branches: two workgroups per CU, as the sequential form of the two-branch kernel;
//   * weight order (packed by cwn_update_mlp_pack_weights_f32): per branch k: W1_k, W2_k, Wc[:, kF:(k+1)F] -- the order the
//     launch multiplies in, so "the next weight" is always the next pointer.
//
//   x_up   --W1u--> relu(bn) --W2u--> relu(bn) = h_up --Wc[:, 0:F]----+
//   x_down --W1d--> relu(bn) --W2d--> relu(bn) = h_d  --Wc[:, F:2F]---+--> (+ bc) relu(bn) = y
//   x_b    --W1b--> relu(bn) --W2b--> relu(bn) = h_b  --Wc[:, 2F:3F]--+
//
// Arithmetic: the exact three-way bf16 split of csrc/cwn_split.h for every product (fp32 in, fp32 accumulate, fp32 out): the
// stages of the update networks are bit-identical to the grouped launches they replace (same split, MFMA order, epilogue).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "cwn_tile.h"
#include "cwn_group.h"

namespace {

constexpr int kThreads = cwn::kTileThreads;
constexpr int kBranches = 3;

// three buffers, two workgroups per CU, as the sequential form of cwn_mlp.hip: padded rows at 128, swizzled rows at 64
template <int F> struct Shape3 : cwn::TileShape<F, 2, F == 64> {
    static constexpr size_t kLdsBytes = 3 * Shape3::kBufBytes;
    static_assert(2 * kLdsBytes <= 160 * 1024, "two workgroups per CU");
};

struct Mlp3Batch {
    cwn_mlp3_dim d[CWN_LAYER_MAX_DIMS];
    int32_t blk_start[CWN_LAYER_MAX_DIMS + 1];
    int32_t n;
};

// (second __launch_bounds__ argument on HIP: minimum WAVES per SIMD -- two resident 8-wave workgroups are four)
template <int F>
__global__ __launch_bounds__(kThreads, 4) void update_mlp3_kernel(Mlp3Batch B) {
    using S = Shape3<F>;
    using WT = cwn::WaveTile<S>;
    using cwn::lds_barrier;
    constexpr int TM = S::kTM, kRT = S::kRT;
    constexpr size_t kBufBytes = S::kBufBytes;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* const P0 = reinterpret_cast<uint16_t*>(smem);
    uint16_t* const P1 = reinterpret_cast<uint16_t*>(smem + kBufBytes);
    uint16_t* const P2 = reinterpret_cast<uint16_t*>(smem + 2 * kBufBytes);
    const int di = cwn::group_of<CWN_LAYER_MAX_DIMS>(B.blk_start, B.n, (int)blockIdx.x);
    const cwn_mlp3_dim& D = B.d[di];
    const int64_t row0 = (int64_t)((int)blockIdx.x - B.blk_start[di]) * TM;
    const int64_t Mv = cwn::rows_vouched(D.m_dev, D.M);      // rows that exist (D.M is then the capacity)
    if (row0 >= Mv) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ct = wave % S::kNCT, rt0 = (wave / S::kNCT) * kRT;
    const int l15 = lane & 15, kq = lane >> 4;
    const WT W{ct, rt0, lane, l15, kq};

    typedef typename WT::RowRegs RowRegs;
    RowRegs vA;                          // ONE set of row registers: the next branch's rows are requested when the last were staged
    auto request_rows = [&](RowRegs& v, const float* X, int64_t ld) { WT::request_rows(v, X, ld, row0, D); };
    auto stage_rows = [&](const RowRegs& v, uint16_t* buf) { WT::stage_rows(v, buf); };
    typedef typename WT::WeightRegs WeightRegs;
    WeightRegs wfA, wfB;
    auto request_kstep = [&](WeightRegs& wf, int k, int ks) { WT::request_kstep(wf, D.w_packed[k], ks, ct, lane); };
    typedef typename WT::AccRegs AccRegs;
    AccRegs accS, accC;                 // the running stage / the combine, accumulated branch by branch
    auto clear = [&](AccRegs& acc) {
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) acc[rt] = cwn::frag_cd{0.f, 0.f, 0.f, 0.f};
    };
    // acc += buf x W^T; the k steps of weight `next` (>= 0) go into the OTHER register set between this product's MFMAs
    auto multiply = [&](AccRegs& acc, const uint16_t* buf, const WeightRegs& wf, WeightRegs& wnext, int next) {
        W.multiply(acc, buf, wf, [&](int ks) { if (next >= 0) request_kstep(wnext, next, ks); });
    };
    typedef typename WT::Consts Consts;
    Consts cS;
    auto request_consts = [&](Consts& c, int s) { W.request_consts(c, D, s); };
    auto finish = [&](const AccRegs& acc, const Consts& c, uint16_t* buf) { W.finish(acc, c, buf, D, row0, Mv); };

    // ---- the chain: weights 0 .. 8 in order, register sets alternating (weight k in set k % 2); every step ends in a barrier;
    // a buffer is overwritten at the earliest one barrier after its last read.
    //   step          reads      writes
    //   0             -          P0 = x_up
    //   1  W1u        P0         P1 = s1(up),   P2 = x_down
    //   2  W2u        P1         P0 = h_up
    //   3  Wc_u, W1d  P0, P2     C += .,        P1 = s1(down)
    //   4  W2d        P1         P2 = h_down,   P0 = x_b
    //   5  Wc_d, W1b  P2, P0     C += .,        P1 = s1(b)
    //   6  W2b        P1         P2 = h_b
    //   7  Wc_b       P2         C += . -> y
    request_rows(vA, D.x[0], D.ldx[0]);
    request_consts(cS, 0);
    W.request_weight(wfA, D.w_packed[0]);
    stage_rows(vA, P0);
    request_rows(vA, D.x[1], D.ldx[1]);                  //    x_down: in flight under step 1
    lds_barrier();
    clear(accS); multiply(accS, P0, wfA, wfB, 1);        // 1: W1u                 (W2u streams in)
    finish(accS, cS, P1);
    request_consts(cS, 1);
    stage_rows(vA, P2);                                  //    x_down
    lds_barrier();
    clear(accS); multiply(accS, P1, wfB, wfA, 2);        // 2: W2u                 (Wc_u)
    finish(accS, cS, P0);                                //    h_up
    request_consts(cS, 2);
    lds_barrier();
    clear(accC); multiply(accC, P0, wfA, wfB, 3);        // 3: C = Wc[:, 0:F] h_up (W1d)
    clear(accS); multiply(accS, P2, wfB, wfA, 4);        //    W1d                 (W2d)
    finish(accS, cS, P1);
    request_consts(cS, 3);
    lds_barrier();
    request_rows(vA, D.x[2], D.ldx[2]);                  //    x_b: in flight under step 4 (requested earlier its eight registers
                                                         //    are live across step 3, the widest one: four spilled at F = 128)
    clear(accS); multiply(accS, P1, wfA, wfB, 5);        // 4: W2d                 (Wc_d)
    finish(accS, cS, P2);                                //    h_down
    request_consts(cS, 4);
    stage_rows(vA, P0);                                  //    x_b
    lds_barrier();
    multiply(accC, P2, wfB, wfA, 6);                     // 5: C += Wc[:, F:2F] h_d (W1b)
    clear(accS); multiply(accS, P0, wfA, wfB, 7);        //    W1b                 (W2b)
    finish(accS, cS, P1);
    request_consts(cS, 5);
    lds_barrier();
    clear(accS); multiply(accS, P1, wfB, wfA, 8);        // 6: W2b                 (Wc_b)
    finish(accS, cS, P2);                                //    h_b
    request_consts(cS, 6);
    lds_barrier();
    multiply(accC, P2, wfA, wfB, -1);                    // 7: C += Wc[:, 2F:3F] h_b (cat order of mp/layers.py:260)
    finish(accC, cS, nullptr);
}

template <int F>
int launch_mlp3(Mlp3Batch& B, int64_t blocks, hipStream_t stream) {
    return cwn::launch_tile<&update_mlp3_kernel<F>>(Shape3<F>::kLdsBytes, blocks, stream, B);
}

}  // namespace

extern "C" int cwn_update_mlp3_f32(const cwn_mlp3_dim* dims, int n_dims, int32_t F, cwn_stream_t stream_) {
    if (dims == nullptr || n_dims < 1 || n_dims > CWN_LAYER_MAX_DIMS || (F != 64 && F != 128)) return CWN_ERR_BAD_ARG;
    const int TM = 4096 / F;
    Mlp3Batch B{};
    B.n = n_dims;
    cwn::BlockFill fill(B.blk_start);
    for (int i = 0; i < n_dims; ++i) {
        const cwn_mlp3_dim& D = dims[i];
        if (D.M < 0) return CWN_ERR_BAD_ARG;
        if (D.M > cwn_update_mlp_max_rows()) return CWN_ERR_TOO_LARGE;
        fill.push(i, (D.M + TM - 1) / TM);     // (at most cwn_update_mlp_max_rows() rows each: the total fits)
        B.d[i] = D;
        if (D.M == 0) continue;
        if (D.y == nullptr || D.ldy < F || D.ldy % 4) return CWN_ERR_BAD_ARG;
        if (!al16(D.y)) return CWN_ERR_ALIGN;
        for (int k = 0; k < kBranches; ++k) {
            if (D.x[k] == nullptr || D.ldx[k] < F || D.ldx[k] % 4) return CWN_ERR_BAD_ARG;
            if (!al16(D.x[k])) return CWN_ERR_ALIGN;
        }
        for (int k = 0; k < 3 * kBranches; ++k) {
            if (D.w_packed[k] == nullptr) return CWN_ERR_BAD_ARG;
            if (!al16(D.w_packed[k])) return CWN_ERR_ALIGN;
        }
        for (int s = 0; s < 2 * kBranches + 1; ++s) {
            if ((D.scale[s] == nullptr) != (D.shift[s] == nullptr)) return CWN_ERR_BAD_ARG;
            if (!(al16(D.bias[s]) && al16(D.scale[s]) && al16(D.shift[s]))) return CWN_ERR_ALIGN;
        }
    }
    const int64_t blocks = fill.close(n_dims);
    if (blocks == 0) return CWN_OK;
    hipStream_t stream = (hipStream_t)stream_;
    return F == 128 ? launch_mlp3<128>(B, blocks, stream) : launch_mlp3<64>(B, blocks, stream);
}
