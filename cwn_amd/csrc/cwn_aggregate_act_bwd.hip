// cwn_aggregate_act_bwd.hip -- the backward of the activated coboundary message (cwn_aggregate_act.hip) as one launch,
// float32 and float64.  Over a TRANSPOSED plan, whose rows are the cells of the operand being differentiated:
//
//     out[r, :] = sum over p in row r, in CSR order, of  g[ig[p], :] * act'( P[r, :] + Q[iq[p], :] )
//
// P is the operand whose gradient this is (its own row r), Q the other operand gathered per entry, g the gradient of the
// stream's output gathered through the destination index, act one of the five CWN_ACT_* codes.  It is the shape of the ReLU
// stream's backward descriptor (CWN_MSG_A_MASK_RELU of cwn_aggregate_f32 / _f64: A = g, B, self_pre) with act' in place of
// the mask; that kernel's device code is held fixed (cwn_aggregate_body.h), hence entry points and a descriptor of their
// own, next to the forward's.  No self term: in this stream both operands are product outputs, and the
// (1 + eps) g and sum(g * x) parts of the gradient keep the code they have.
//
// Arithmetic: the pre-activation is recomputed as ONE add in the element type, P + Q, as the forward computes A + B (the
// add commutes: the same bits whichever operand is P); the activation's output, where act' needs it, is activate<ACT> of
// cwn_act.h, so it has the forward's bits; g * act' is activate_bwd<ACT> (torch's backward formulas; ReLU is a select).
// Product and accumulate are SEPARATE: acc = acc + (g * act'), a rounded multiply and a rounded add, never one fma -- on
// every path (the library is built with -ffp-contract=off).  With act = relu / id a row's sum is therefore the sum
// CWN_MSG_A_MASK_RELU / CWN_MSG_A computes for it.
//
// The mapping, the folds and the launcher are cwn_aggregate_act_body.h's, shared with the forward.  This direction's own:
// the term g * act'(p + q), the row's own operand P (never read for a row without entries: with an absent plan it may not
// exist), and nothing added to the finished sum -- a row without entries, and every row of an absent plan, gets zeros.
#include "cwn_aggregate_act_body.h"

namespace {

template <class real> struct DescOf;
template <> struct DescOf<float> { using type = cwn_agg_act_bwd_desc; };
template <> struct DescOf<double> { using type = cwn_agg_act_bwd_desc_f64; };

template <class real>
struct BwdBatch {
    typename DescOf<real>::type d[CWN_MAX_DESCS];
    int32_t blk_start[CWN_MAX_DESCS + 1];
    int32_t group[CWN_MAX_DESCS];   // lanes per row
    int32_t fgroup[CWN_MAX_DESCS];  // of which feature lanes (the rest are entry slots, narrow F only)
    int32_t vec[CWN_MAX_DESCS];     // elements per lane
    int32_t n;
};

template <class real_>
struct BwdForm {
    using real = real_;
    using Desc = typename DescOf<real>::type;

    static __device__ __forceinline__ Operands<real> operands(const Desc& D) { return {D.ig, D.iq, D.g, D.Q, D.F}; }

    // acc += g * act'(p + q): one add for the pre-activation, a rounded product, a rounded add
    template <int VEC, int ACT>
    static __device__ __forceinline__ void term(Acc<real, VEC>& acc, const Acc<real, VEC>& g, const Acc<real, VEC>& q,
                                                const Acc<real, VEC>& p) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + activate_bwd<ACT>(p.v[k] + q.v[k], g.v[k]);
    }

    // the lane's slice of P's row (zeros for a lane past F: its sums are never stored)
    template <int VEC, bool SMALL>
    static __device__ __forceinline__ Acc<real, VEC> own(const Desc& D, int64_t row, int f, bool active) {
        Acc<real, VEC> p = splat<real, VEC>(real(0.0));
        if (active) p = ld<VEC>(row_at<SMALL>(D.P, row, D.F, f));
        return p;
    }

    template <int VEC, bool SMALL>
    static __device__ __forceinline__ void finish(const Desc& D, int64_t row, int f, real, const Acc<real, VEC>& acc) {
        st<VEC>(row_at<SMALL>(D.out, row, D.F, f), acc);
    }

    static __device__ __forceinline__ real self_scale(const Desc&, int) { return real(1.0); }

    static bool plan_complete(const Desc& D) {
        return D.ig != nullptr && D.iq != nullptr && D.g != nullptr && D.P != nullptr && D.Q != nullptr;
    }
    static HostPointers pointers(const Desc& D) {
        const bool plan = D.rowptr != nullptr;
        return {{plan ? D.g : nullptr, plan ? D.P : nullptr, plan ? D.Q : nullptr, D.out}, nullptr};
    }
};

template <class real, bool SMALL>
__global__ __launch_bounds__(kThreads) void aggregate_act_bwd_kernel(BwdBatch<real> B) {
    __shared__ real part[kThreads * (16 / (int)sizeof(real))];
    run_block<BwdForm<real>, SMALL>(B, part);
}

}  // namespace

extern "C" int cwn_aggregate_act_bwd_f32(const cwn_agg_act_bwd_desc* descs, int n, cwn_stream_t stream) {
    return launch_act<BwdForm<float>>(descs, n, stream, aggregate_act_bwd_kernel<float, true>,
                                      aggregate_act_bwd_kernel<float, false>);
}

extern "C" int cwn_aggregate_act_bwd_f64(const cwn_agg_act_bwd_desc_f64* descs, int n, cwn_stream_t stream) {
    return launch_act<BwdForm<double>>(descs, n, stream, aggregate_act_bwd_kernel<double, true>,
                                       aggregate_act_bwd_kernel<double, false>);
}
