// cwn_aggregate_act.hip -- the coboundary message of a non-ReLU model as one launch, float32 and float64:
//
//     out[i, :] = sum over p in row i, in CSR order, of act(A[ia[p], :] + B[ib[p], :])  +  (1 + eps) * self_x[i, :]
//
// with act one of the five CWN_ACT_* codes.  The activation follows the Linear of act(Linear(cat(x_j, up_attr))), so the
// split of the ReLU stream -- Y1 = X W[:, :F]^T + b per source cell, Y2 = X_attr W[:, F:]^T per shared cell, gathered and
// added per entry -- holds for every activation; what cwn_aggregate_f32 / _f64 lack is an activation other than ReLU, and
// their device code is held fixed (cwn_aggregate_body.h).  Hence entry points and a descriptor of their own, in this file.
//
// The mapping, the folds, the launcher and the arithmetic rules are cwn_aggregate_act_body.h's, shared with the backward
// (cwn_aggregate_act_bwd.hip).  This direction's own: the term act(a + b), no operand of the row itself, and one self term
// added to the finished sum.
#include "cwn_aggregate_act_body.h"

namespace {

template <class real> struct DescOf;
template <> struct DescOf<float> { using type = cwn_agg_act_desc; };
template <> struct DescOf<double> { using type = cwn_agg_act_desc_f64; };

template <class real>
struct ActBatch {
    typename DescOf<real>::type d[CWN_MAX_DESCS];
    int32_t blk_start[CWN_MAX_DESCS + 1];
    int32_t group[CWN_MAX_DESCS];   // lanes per destination row
    int32_t fgroup[CWN_MAX_DESCS];  // of which feature lanes (the rest are entry slots, narrow F only)
    int32_t vec[CWN_MAX_DESCS];     // elements per lane
    int32_t n;
};

template <class real_>
struct ActForm {
    using real = real_;
    using Desc = typename DescOf<real>::type;

    static __device__ __forceinline__ Operands<real> operands(const Desc& D) { return {D.ia, D.ib, D.A, D.B, D.F}; }

    // acc += act(a + b): one add for the pre-activation, in the element type
    template <int VEC, int ACT>
    static __device__ __forceinline__ void term(Acc<real, VEC>& acc, const Acc<real, VEC>& a, const Acc<real, VEC>& b,
                                                const Acc<real, VEC>&) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + activate<ACT>(a.v[k] + b.v[k]);
    }

    template <int VEC, bool SMALL>
    static __device__ __forceinline__ Acc<real, VEC> own(const Desc&, int64_t, int, bool) {
        return splat<real, VEC>(real(0.0));
    }

    // the self term, loaded late (the two-operand messages of cwn_aggregate.hip do the same), one coalesced store of the slice
    template <int VEC, bool SMALL>
    static __device__ __forceinline__ void finish(const Desc& D, int64_t row, int f, real scale1, Acc<real, VEC> acc) {
        if (D.self_x != nullptr) {
            const Acc<real, VEC> s1 = ld<VEC>(row_at<SMALL>(D.self_x, row, D.F, f));
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + scale1 * s1.v[k];
        }
        st<VEC>(row_at<SMALL>(D.out, row, D.F, f), acc);
    }

    // 1 + eps; z keeps the eps load in VMEM
    static __device__ __forceinline__ real self_scale(const Desc& D, int z) {
        return real(1.0) + (D.eps != nullptr ? D.eps[z] : real(0.0));
    }

    static bool plan_complete(const Desc& D) {
        return D.ia != nullptr && D.ib != nullptr && D.A != nullptr && D.B != nullptr;
    }
    static HostPointers pointers(const Desc& D) {
        const bool plan = D.rowptr != nullptr;
        return {{plan ? D.A : nullptr, plan ? D.B : nullptr, D.self_x, D.out}, D.eps};
    }
};

template <class real, bool SMALL>
__global__ __launch_bounds__(kThreads) void aggregate_act_kernel(ActBatch<real> B) {
    __shared__ real part[kThreads * (16 / (int)sizeof(real))];
    run_block<ActForm<real>, SMALL>(B, part);
}

}  // namespace

extern "C" int cwn_aggregate_act_f32(const cwn_agg_act_desc* descs, int n, cwn_stream_t stream) {
    return launch_act<ActForm<float>>(descs, n, stream, aggregate_act_kernel<float, true>, aggregate_act_kernel<float, false>);
}

extern "C" int cwn_aggregate_act_f64(const cwn_agg_act_desc_f64* descs, int n, cwn_stream_t stream) {
    return launch_act<ActForm<double>>(descs, n, stream, aggregate_act_kernel<double, true>, aggregate_act_kernel<double, false>);
}
