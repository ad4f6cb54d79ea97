// cwn_items_dev.hip -- the item tables of the complex-blocked launches (cwn_layer_fused_f32, cwn_layer_bwd_own_f32), built ON
// THE DEVICE from the device-resident prefix sums of a batch (the `ptr` / `__slices__` tables of data/complex.py:344-441, as
// cwn_collate_tables writes them).
//
// Why: the reference's training loop draws a new shuffled batch every step (data/data_loading.py:84-111,
// exp/train_utils.py:35-75).  With the table cut on the host (csrc/cwn_blockplan.cpp) every fresh batch costs a host pass
// over its per-complex sizes plus an upload -- 0.084 ms + H2D per batch measured in round 3, against a propagate step of
// 0.039 ms -- and a captured hipGraph cannot contain that upload at all.  Here the cut is two small launches inside the
// captured step: one workgroup per set, a thread per GROUP of consecutive complexes.
//
// The cut is simpler than the host's greedy one (which walks the complexes sequentially and tries several splits of the
// LDS): complexes are taken in groups of `group` consecutive ones; a group that fits the caps of a workgroup is one item,
// a group that does not is cut into its single complexes, a complex that does not fit alone sets CWN_ERR_BIT_UNFIT and gets
// no record.  Every record is what the host builder writes for the same range: whether a range fits and what its record is
// is cwn_items.h, which both call (tests/test_gpu_static.py compares the tables record for record).  Set s owns a FIXED
// region of the table; records past a set's own are zeroed (empty).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cwn_items.h"

namespace {

using namespace cwn_items;

constexpr int kThreads = 1024;

struct ItemsArgs {
    const int64_t* n_complexes;
    int64_t cap_c;
    const int64_t* cell_ptr[CWN_LAYER_MAX_DIMS];
    const int64_t* up_ptr[CWN_LAYER_MAX_DIMS];
    const int64_t* b_ptr[CWN_LAYER_MAX_DIMS];
    int32_t* items;
    int32_t* err;
    Set sets[CWN_LAYER_MAX_DIMS];
    int32_t set_start[CWN_LAYER_MAX_DIMS + 1];
    int32_t n_sets, n_dims, F, variant, group;
    int32_t has_up[CWN_LAYER_MAX_DIMS];
    int64_t row_cap, src_cap, lds_budget, half_cap, idx_bytes;
    int64_t bwd_lds;                 // backward table: the launch's dynamic LDS
    int64_t table_slot_stride;       // slots (blockIdx.y): int64 elements between the tables of consecutive slots ...
    int64_t items_slot_ints;         // ... and int32 elements between their item tables
};

// Everything below reads the kernel arguments with COMPILE-TIME indices (sel3, unrolled loops: cwn_items.h).

// workgroup-wide exclusive scan of one small integer per thread; returns the thread's offset, *total = the sum
__device__ __forceinline__ int block_scan(int v, int* total, int* lds /* [2 * 16] */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wid] = x;
    __syncthreads();
    if (wid == 0) {
        int s = lane < kThreads / 64 ? lds[lane] : 0;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const int y = __shfl_up(s, o, 64);
            if (lane >= o) s += y;
        }
        if (lane < kThreads / 64) lds[16 + lane] = s;
    }
    __syncthreads();
    const int off = (wid == 0 ? 0 : lds[16 + wid - 1]) + x - v;
    *total = lds[16 + kThreads / 64 - 1];
    __syncthreads();
    return off;
}

// the prefix sums of a range of complexes [a, b) of a slot, in registers (a range of cwn_items.h)
struct Range {
    int64_t c0[CWN_LAYER_MAX_DIMS], cn[CWN_LAYER_MAX_DIMS];     // cells
    int64_t u0[CWN_LAYER_MAX_DIMS], un[CWN_LAYER_MAX_DIMS];     // entries of upper_index_d
    int64_t b0[CWN_LAYER_MAX_DIMS], bn[CWN_LAYER_MAX_DIMS];     // entries of boundary_index_d
    __device__ __forceinline__ int64_t cells(int d) const { return sel3(d, cn[0], cn[1], cn[2]); }
    __device__ __forceinline__ int64_t cell0(int d) const { return sel3(d, c0[0], c0[1], c0[2]); }
    __device__ __forceinline__ int64_t ups(int d) const { return sel3(d, un[0], un[1], un[2]); }
    __device__ __forceinline__ int64_t up0(int d) const { return sel3(d, u0[0], u0[1], u0[2]); }
    __device__ __forceinline__ int64_t bnds(int d) const { return sel3(d, bn[0], bn[1], bn[2]); }
    __device__ __forceinline__ int64_t bnd0(int d) const { return sel3(d, b0[0], b0[1], b0[2]); }
};

__device__ __forceinline__ Range load_range(const ItemsArgs& A, int64_t o, int64_t a, int64_t b) {
    Range R;
#pragma unroll
    for (int d = 0; d < CWN_LAYER_MAX_DIMS; ++d) {
        R.c0[d] = R.cn[d] = R.u0[d] = R.un[d] = R.b0[d] = R.bn[d] = 0;
        if (d < A.n_dims) {
            const int64_t* cp = A.cell_ptr[d] + o;
            R.c0[d] = cp[a];
            R.cn[d] = cp[b] - R.c0[d];
            if (A.up_ptr[d] != nullptr) {
                const int64_t* up = A.up_ptr[d] + o;
                R.u0[d] = up[a];
                R.un[d] = up[b] - R.u0[d];
            }
            if (A.b_ptr[d] != nullptr) {
                const int64_t* bp = A.b_ptr[d] + o;
                R.b0[d] = bp[a];
                R.bn[d] = bp[b] - R.b0[d];
            }
        }
    }
    return R;
}

// One workgroup per set and slot, a thread per group of consecutive complexes: classify the group (Rule: cwn_items.h,
// FwdRule or BwdRule), count the records of the threads in front (workgroup scan), store; then zero the rest of the region.
template <class Rule>
__device__ __forceinline__ void build_items(const ItemsArgs& A, const Rule& G, int set) {
    constexpr int kRec = Rule::kRecInts;
    __shared__ int scan_lds[32];
    const int64_t o = (int64_t)blockIdx.y * A.table_slot_stride;
    int32_t* const items = A.items + (int64_t)blockIdx.y * A.items_slot_ints;
    const int64_t nc_dev = A.n_complexes[o];
    const int64_t C = nc_dev < A.cap_c ? (nc_dev < 0 ? 0 : nc_dev) : A.cap_c;
    const int region0 = sel3(set, A.set_start[0], A.set_start[1], A.set_start[2]);
    const int region1 = sel3(set, A.set_start[1], A.set_start[2], A.set_start[3]);
    const int64_t groups = (A.cap_c + A.group - 1) / A.group;
    int base = 0;
    bool unfit = false;
    auto store = [&](int slot, const int32_t (&r)[kRec]) {
        if (slot < region1) {
            for (int k = 0; k < kRec; k += 4) *reinterpret_cast<int4*>(items + (size_t)slot * kRec + k) = make_int4(r[k], r[k + 1], r[k + 2], r[k + 3]);
        } else {
            unfit = true;
        }
    };
    for (int64_t q0 = 0; q0 < groups; q0 += kThreads) {          // (uniform trip count)
        const int64_t a = (q0 + threadIdx.x) * A.group;
        const int64_t b = a + A.group < C ? a + A.group : C;
        int32_t r[kRec];
        int cnt = 0, whole = 0;
        if (a < C) {
            whole = G.classify(load_range(A, o, a, b), r);
            if (whole & K_ITEM) {
                cnt = 1;
            } else if (whole & K_SPLIT) {
                for (int64_t c = a; c < b; ++c) {
                    int32_t r1[kRec];
                    const int k = G.classify(load_range(A, o, c, c + 1), r1);
                    cnt += k & K_ITEM;
                    unfit = unfit || (k & (K_SPLIT | K_BAD)) != 0;
                }
            }
            unfit = unfit || (whole & K_BAD) != 0;
        }
        int total;
        const int off = block_scan(cnt, &total, scan_lds);
        if (cnt > 0) {
            int slot = region0 + base + off;
            if (whole & K_ITEM) {
                store(slot, r);
            } else {
                for (int64_t c = a; c < b; ++c)
                    if (G.classify(load_range(A, o, c, c + 1), r) & K_ITEM) store(slot++, r);
            }
        }
        base += total;
    }
    // records past the set's own: empty
    for (int i = region0 + base + (int)threadIdx.x; i < region1; i += kThreads) {
        int4* dst = reinterpret_cast<int4*>(items + (size_t)i * kRec);
#pragma unroll
        for (int k = 0; k < kRec / 4; ++k) dst[k] = make_int4(0, 0, 0, 0);
    }
    if (unfit) atomicOr(A.err, CWN_ERR_BIT_UNFIT);
}

__device__ __forceinline__ Set set_of(const ItemsArgs& A, int set) {
    const Set S0 = A.sets[0], S1 = A.sets[1], S2 = A.sets[2];
    return set == 0 ? S0 : (set == 1 ? S1 : S2);
}

__global__ __launch_bounds__(kThreads) void items_fwd_kernel(ItemsArgs A) {
    const int set = blockIdx.x;
    const Set S = set_of(A, set);
    build_items(A, FwdRule{A.F, A.variant, set, S.g, S.n_tasks, S.tasks[0], S.tasks[1], A.row_cap, A.src_cap, A.lds_budget, A.half_cap,
                           A.idx_bytes}, set);
}

__global__ __launch_bounds__(kThreads) void items_bwd_kernel(ItemsArgs A) {
    const int set = blockIdx.x;
    build_items(A, BwdRule::of(A, A.F, set, set_of(A, set), A.bwd_lds), set);
}

int fill_common(const cwn_layer_sizes_dev* in, int32_t F, int32_t group, int32_t* err_flag, ItemsArgs& A) {
    if (in == nullptr || (F != 64 && F != 128) || in->n_dims < 1 || in->n_dims > CWN_LAYER_MAX_DIMS || in->cap_complexes < 1 ||
        in->n_complexes == nullptr || group < 1 || err_flag == nullptr)
        return CWN_ERR_BAD_ARG;
    if (in->cap_complexes >= INT32_MAX / 4) return CWN_ERR_TOO_LARGE;
    for (int d = 0; d < in->n_dims; ++d) {
        if (in->cell_ptr[d] == nullptr) return CWN_ERR_BAD_ARG;
        if (in->has_up[d] && (d + 1 >= in->n_dims || in->up_ptr[d] == nullptr)) return CWN_ERR_BAD_ARG;
        A.cell_ptr[d] = in->cell_ptr[d];
        A.up_ptr[d] = in->up_ptr[d];
        A.b_ptr[d] = in->b_ptr[d];
        A.has_up[d] = in->has_up[d] ? 1 : 0;
    }
    A.n_complexes = in->n_complexes;
    A.cap_c = in->cap_complexes;
    A.n_dims = in->n_dims;
    A.F = F;
    A.group = group;
    A.err = err_flag;
    A.n_sets = make_sets(*in, A.sets);
    if (in->n_slots < 1 || in->n_slots > 1024 || (in->n_slots > 1 && in->table_slot_stride <= 0)) return CWN_ERR_BAD_ARG;
    A.table_slot_stride = in->n_slots > 1 ? in->table_slot_stride : 0;
    return CWN_OK;
}

}  // namespace

extern "C" int cwn_layer_items_build_dev(const cwn_layer_sizes_dev* in, int32_t F, const cwn_layer_plan* plan, int32_t group,
                                         int32_t* err_flag, cwn_stream_t stream_) {
    ItemsArgs A{};
    const int rc = fill_common(in, F, group, err_flag, A);
    if (rc != CWN_OK) return rc;
    if (plan == nullptr || plan->items == nullptr || plan->n_items < 1 || ((uintptr_t)plan->items & 15u)) return CWN_ERR_BAD_ARG;
    const int variant = plan->variant;
    if (variant != 0 && variant != 1) return CWN_ERR_BAD_ARG;
    A.items = const_cast<int32_t*>(plan->items);
    A.variant = variant;
    if (cwn_layer_variant_round_rows(F, variant) <= 0) return CWN_ERR_BAD_ARG;
    // the LDS split of the captured launch: the caller's (variant 0: one layout per launch; variant 1: per item inside
    // the launch's dynamic LDS)
    A.row_cap = plan->max_gemm_rows;
    A.src_cap = plan->max_source_rows;
    A.lds_budget = variant == 1 ? plan->lds_bytes : (int64_t)160 * 1024;
    A.half_cap = variant == 1 ? (int64_t)CWN_LAYER_W8_HALF_ROWS(F) : 0;
    A.idx_bytes = (int64_t)cwn_layer_variant_lds_bytes(128, variant, 16, 0) - 3 * 16 * (128 + 8) * 2 - 128 * 4;
    const int64_t cap_rows = variant == 1 ? CWN_LAYER_W8_GEMM_ROWS(F) : CWN_LAYER_GEMM_ROWS(F);
    const int64_t cap_src = variant == 1 ? CWN_LAYER_W8_SOURCE_ROWS(F) : CWN_LAYER_SOURCE_ROWS(F);
    if (A.row_cap < 16 || A.row_cap > cap_rows || A.src_cap < 0 || A.src_cap > cap_src || A.lds_budget <= 0) return CWN_ERR_BAD_ARG;
    if (variant == 0 && cwn_layer_fused_lds_bytes(F, (int32_t)A.row_cap, (int32_t)A.src_cap) == 0) return CWN_ERR_BAD_ARG;
    // fixed regions: set_start[0] = 0 <= set_start[1] <= ... ; the last set ends at n_items
    for (int s = 0; s <= A.n_sets; ++s) {
        const int64_t v = s == A.n_sets ? plan->n_items : plan->set_start[s];
        const int64_t lo = s == 0 ? 0 : A.set_start[s - 1];
        if ((s == 0 && v != 0) || v < lo || v > plan->n_items || v >= INT32_MAX) return CWN_ERR_BAD_ARG;
        A.set_start[s] = (int32_t)v;
    }
    A.items_slot_ints = plan->n_items * FwdRule::kRecInts;
    items_fwd_kernel<<<dim3(A.n_sets, in->n_slots), dim3(kThreads), 0, (hipStream_t)stream_>>>(A);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

extern "C" int cwn_layer_bwd_items_build_dev(const cwn_layer_sizes_dev* in, int32_t F, const cwn_layer_bwd_plan* plan, int32_t group,
                                             int32_t* err_flag, cwn_stream_t stream_) {
    ItemsArgs A{};
    const int rc = fill_common(in, F, group, err_flag, A);
    if (rc != CWN_OK) return rc;
    if (plan == nullptr || plan->items == nullptr || ((uintptr_t)plan->items & 15u)) return CWN_ERR_BAD_ARG;
    if (plan->lds_bytes <= 0 || plan->lds_bytes > cwn_bwd_own::kLdsCap) return CWN_ERR_BAD_ARG;
    if (plan->n_items != (int64_t)A.n_sets * in->cap_complexes) return CWN_ERR_BAD_ARG;     // one region of cap_complexes records per set
    A.items = const_cast<int32_t*>(plan->items);
    A.bwd_lds = plan->lds_bytes;
    for (int s = 0; s <= A.n_sets; ++s) A.set_start[s] = (int32_t)(s * in->cap_complexes);
    A.items_slot_ints = plan->n_items * BwdRule::kRecInts;
    items_bwd_kernel<<<dim3(A.n_sets, in->n_slots), dim3(kThreads), 0, (hipStream_t)stream_>>>(A);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}
