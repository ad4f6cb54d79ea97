// cwn_flow_head.hip -- the invariant readout head of EdgeOrient / EdgeMPNN (mp/models.py:531-545, :600-614) in float32,
// forward and backward.  See include/cwn_hip.h, "The edge-flow readout head".
//
//   pooled[c, :] = sum over the rows r of cochain c of f(x[r, :])      f = |.| or identity; / max(rows, 1) for 'mean'
//   out[c, :]    = W2 relu(W1 pooled[c, :] + b1) + b2
//
// A cochain of the flow experiments has thousands of rows and a batch has 64 cochains: one workgroup per cochain would pull
// 50 MB of x through 64 CUs.  The rows of a cochain are cut into CHUNKS of CWN_FLOW_HEAD_CHUNK consecutive rows, counted
// from the cochain's own first row; a chunk never spans two cochains.
//
// Slots.  The launches know N and C on the host and `ptr` on the device only, so the grid cannot be the exact number of
// chunks.  Cochain c owns the slots [first(c), first(c + 1)), first(c) = ptr[c] / CHUNK + c: strictly increasing in c, and
// first(c + 1) - first(c) = ptr[c + 1] / CHUNK - ptr[c] / CHUNK + 1 >= ceil(rows(c) / CHUNK), so its chunks fit (at most one
// slot per cochain stays idle).  There are N / CHUNK + C slots; workgroup b finds its cochain with a 64-ary search over
// first() -- one round trip for C <= 64, two up to 4096 -- and leaves at once when its slot is idle.
//
// Forward, launch 1 (one workgroup per slot): thread (q, s) owns the four columns 4 q .. 4 q + 3 and the rows s, s + S,
// s + 2 S, ... of the chunk (S = min(256 / ceil(K / 4), 32) row slots); it adds f(x) of its rows in ascending order onto an
// accumulator that starts at 0, the S partials of a column are then added in ascending s, and the chunk's sum is STORED to
// the slot's row of the workspace.  The 16-byte form (K % 4 == 0, x 16-byte aligned, ldx % 4 == 0) and the scalar form
// load differently and add in the same order: the bits do not depend on which of them ran.
// Forward, launch 2 (one workgroup per cochain): the chunk sums of the cochain are added in two interleaved chains (chunks
// 0, 2, 4, ... and 1, 3, 5, ..., each ascending, then chain 0 + chain 1), divided by max(rows, 1) for 'mean'; lin1 and lin2
// are one fmaf chain over k ascending from 0 per output, then the bias add, the weights staged through LDS in tiles of 32
// columns (pitch 33: coalesced from memory, conflict-free by row), as cwn_agnostic_head_f32 does.
// So every sum's order is a function of the cochain's own row count (and K): a cochain's prediction has the same bits
// alone, at any place of any batch, on every run.  No atomics.
//
// Backward: launch 1 (one workgroup per cochain) ds = W2^T g, dh = relu'(h) ds, dpooled = W1^T dh [/ max(rows, 1)] into the
// workspace; launch 2 (one workgroup per slot) dx[r, :] = sgn(x[r, :]) dpooled[c, :] over the chunk's rows, every row of
// every cochain written exactly once.
//
// The counted form (cwn_flow_head_dev_f32 / cwn_flow_head_bwd_dev_f32: a capacity-sized batch inside a captured graph) runs the
// SAME kernels: N and C of the launch are capacities, every workgroup reads the live cochain count (*c_dev) and the live row
// total (*n_dev, or ptr[live cochains]) first and works as if the launch had been given those -- slots, chunks, clamps and sums
// are the ones of the host-count launch over the trimmed tensors, so the bits are.  A workgroup whose slot lies behind the last
// live one leaves at once; a workgroup of an absent cochain (c >= the live count) writes zeros to its rows of out / pooled / h
// (forward) and dh / dpooled (backward) and reads nothing else.
//
// LDS (static): pool 4 KiB; head 128 x 33 + 256 + 128 floats = 18432 B; bwd 128 + 64 floats.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cwn_hip.h"
#include "cwn_act.h"
#include "cwn_check.h"
#include "cwn_group.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = CWN_FLOW_HEAD_CHUNK;
constexpr int kMaxW = CWN_FLOW_HEAD_MAX_WIDTH;           // widest K / H
constexpr int kMaxO = CWN_FLOW_HEAD_MAX_OUT;
constexpr int kMaxSlots = 32;                            // row slots of a chunk in the pooling launch
constexpr int kKc = 32;                                  // columns per staged weight tile
constexpr int kWld = kKc + 1;

static_assert(kMaxW <= kThreads / 2, "two chains of chunk sums per column");
static_assert(kMaxO <= kMaxW, "lin2's outputs share lin1's thread layout");

__device__ __forceinline__ int64_t clamp_row(int64_t v, int64_t N) { return v < 0 ? 0 : (v > N ? N : v); }

// The rows [start, end) of cochain c, kept inside [0, N] whatever ptr holds.
__device__ __forceinline__ void cochain_rows(const int64_t* __restrict__ ptr, int64_t c, int64_t N, int64_t& start, int64_t& end) {
    start = clamp_row(ptr[c], N);
    end = clamp_row(ptr[c + 1], N);
    if (end < start) end = start;
}

// The counted form: N and C arrive as capacities and become the live counts, clamped to them (c_dev NULL: host counts, as given).
__device__ __forceinline__ void live_counts(const int64_t* __restrict__ ptr, const int64_t* __restrict__ n_dev,
                                            const int64_t* __restrict__ c_dev, int64_t& N, int64_t& C) {
    if (c_dev == nullptr) return;
    C = cwn::rows_clamped(c_dev, C);
    N = clamp_row(n_dev != nullptr ? *n_dev : ptr[C], N);      // (open-coded: without n_dev the total is ptr's, not a count of its own)
}

// The cochain that owns slot b: the largest c < C with first(c) <= b, by a 64-ary search (every lane of the wave takes part).
// Whatever ptr holds the result lies in [0, C).
__device__ __forceinline__ int64_t find_cochain(const int64_t* __restrict__ ptr, int64_t C, int64_t N, int64_t b, int lane) {
    int64_t lo = 0, hi = C;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t i = lo + (int64_t)lane * step;
        const bool ok = i < hi && clamp_row(ptr[i], N) / kChunk + i <= b;
        const int cnt = __popcll(__ballot(ok));
        const int64_t nlo = lo + (int64_t)(cnt > 0 ? cnt - 1 : 0) * step;
        hi = nlo + step < hi ? nlo + step : hi;
        lo = nlo;
    }
    return lo;
}

// The chunk of slot b: its cochain and rows [r0, r1); false for an idle slot.  Uniform over the workgroup.
__device__ __forceinline__ bool slot_chunk(const int64_t* __restrict__ ptr, int64_t C, int64_t N, int64_t b, int lane, int64_t& c,
                                           int64_t& r0, int64_t& r1) {
    c = find_cochain(ptr, C, N, b, lane);
    int64_t start, end;
    cochain_rows(ptr, c, N, start, end);
    const int64_t j = b - (start / kChunk + c);
    if (j < 0 || j > (end - start) / kChunk) return false;
    r0 = start + j * kChunk;
    if (r0 >= end) return false;
    r1 = r0 + kChunk < end ? r0 + kChunk : end;
    return true;
}

template <bool VEC>
__device__ __forceinline__ float4 load_quad(const float* __restrict__ row, int q, int K) {
    if (VEC) return *reinterpret_cast<const float4*>(row + 4 * q);
    float4 v;
    v.x = 4 * q + 0 < K ? row[4 * q + 0] : 0.f;
    v.y = 4 * q + 1 < K ? row[4 * q + 1] : 0.f;
    v.z = 4 * q + 2 < K ? row[4 * q + 2] : 0.f;
    v.w = 4 * q + 3 < K ? row[4 * q + 3] : 0.f;
    return v;
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float* __restrict__ row, int q, int K, float4 v) {
    if (VEC) {
        *reinterpret_cast<float4*>(row + 4 * q) = v;
        return;
    }
    if (4 * q + 0 < K) row[4 * q + 0] = v.x;
    if (4 * q + 1 < K) row[4 * q + 1] = v.y;
    if (4 * q + 2 < K) row[4 * q + 2] = v.z;
    if (4 * q + 3 < K) row[4 * q + 3] = v.w;
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 abs4(float4 a) { return make_float4(fabsf(a.x), fabsf(a.y), fabsf(a.z), fabsf(a.w)); }

// ---- forward, launch 1: the sum of every chunk -----------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kThreads) void flow_pool_kernel(const float* __restrict__ x, int64_t N, int64_t ldx,
                                                             const int64_t* __restrict__ ptr, int64_t C, int K, int take_abs,
                                                             float* __restrict__ ws, const int64_t* __restrict__ n_dev,
                                                             const int64_t* __restrict__ c_dev) {
    __shared__ float4 part[kThreads];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    live_counts(ptr, n_dev, c_dev, N, C);
    if (b >= N / kChunk + C) return;                          // (behind the last live slot: nothing is touched)
    int64_t c, r0, r1;
    if (!slot_chunk(ptr, C, N, b, tid & 63, c, r0, r1)) return;
    const int cols = (K + 3) >> 2;
    const int slots = kThreads / cols < kMaxSlots ? kThreads / cols : kMaxSlots;
    const int q = tid % cols, s = tid / cols;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s < slots) {
        // four rows requested before the first is added; they are ADDED one after the other, in row order
        for (int64_t r = r0 + s; r < r1; r += 4 * (int64_t)slots) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t rr = r + (int64_t)u * slots;
                v[u] = rr < r1 ? load_quad<VEC>(x + rr * ldx, q, K) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r + (int64_t)u * slots < r1) acc = add4(acc, take_abs ? abs4(v[u]) : v[u]);
        }
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < cols) {
        float4 total = part[tid];
        for (int t = 1; t < slots; ++t) total = add4(total, part[t * cols + tid]);     // in slot order
        store_quad<VEC>(ws + b * K, tid, K, total);
    }
}

// W[row, k0 + k] for row < n_rows, k < kn (contiguous rows of ldw floats) -> wt[row * kWld + k]
__device__ __forceinline__ void stage_rows(float* wt, const float* __restrict__ W, int ldw, int n_rows, int kn) {
    for (int i = threadIdx.x; i < n_rows * kKc; i += kThreads) {
        const int row = i / kKc, k = i % kKc;
        if (k < kn) wt[row * kWld + k] = W[(int64_t)row * ldw + k];
    }
}

// out[tid] = sum_k in[k] * W[tid, k] over k ascending from 0, for tid < n_out; W [n_out, n_in] contiguous
__device__ __forceinline__ float dense_row(float* wt, const float* in, const float* __restrict__ W, int n_out, int n_in) {
    const int tid = threadIdx.x;
    float acc = 0.f;
    for (int k0 = 0; k0 < n_in; k0 += kKc) {
        const int kn = n_in - k0 < kKc ? n_in - k0 : kKc;
        __syncthreads();                                      // the previous tile has been read, `in` is complete
        stage_rows(wt, W + k0, n_in, n_out, kn);
        __syncthreads();
        if (tid < n_out) {
            const float* w = wt + tid * kWld;
            for (int k = 0; k < kn; ++k) acc = fmaf(in[k0 + k], w[k], acc);
        }
    }
    return acc;
}

// ---- forward, launch 2: the chunk sums of a cochain in chunk order, lin1, ReLU, lin2 ------------------------------------------------
__global__ __launch_bounds__(kThreads) void flow_head_kernel(const float* __restrict__ ws, const int64_t* __restrict__ ptr, int64_t N,
                                                             const float* __restrict__ W1, const float* __restrict__ b1,
                                                             const float* __restrict__ W2, const float* __restrict__ b2,
                                                             float* __restrict__ out, int64_t ldout, float* __restrict__ pooled_out,
                                                             float* __restrict__ h_out, int K, int H, int O, int mean, int64_t C,
                                                             const int64_t* __restrict__ n_dev, const int64_t* __restrict__ c_dev) {
    __shared__ float wt[kMaxW * kWld];
    __shared__ float pl[kThreads];
    __shared__ float sh[kMaxW];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    live_counts(ptr, n_dev, c_dev, N, C);
    if (c >= C) {                                             // an absent cochain of a capacity-sized batch: zeros, nothing read
        if (tid < O) out[c * ldout + tid] = 0.f;
        if (pooled_out != nullptr && tid < K) pooled_out[c * K + tid] = 0.f;
        if (h_out != nullptr && tid < H) h_out[c * H + tid] = 0.f;
        return;
    }
    int64_t start, end;
    cochain_rows(ptr, c, N, start, end);
    const int64_t rows = end - start;
    const int64_t n_chunks = (rows + kChunk - 1) / kChunk, first = start / kChunk + c;
    const int k = tid & (kMaxW - 1), chain = tid / kMaxW;
    float acc = 0.f;
    if (k < K) {
#pragma unroll 4
        for (int64_t j = chain; j < n_chunks; j += kThreads / kMaxW) acc = acc + ws[(first + j) * K + k];
    }
    pl[tid] = acc;
    __syncthreads();
    float p = 0.f;
    if (tid < K) {
        p = pl[tid] + pl[kMaxW + tid];
        if (mean) p = p / (float)(rows > 0 ? rows : 1);
        if (pooled_out != nullptr) pooled_out[c * K + tid] = p;
    }
    __syncthreads();
    if (tid < K) pl[tid] = p;
    float h = dense_row(wt, pl, W1, H, K);
    if (tid < H) {
        h = h + (b1 != nullptr ? b1[tid] : 0.f);
        if (h_out != nullptr) h_out[c * H + tid] = h;
        sh[tid] = cwn_relu(h);                                // a NaN stays a NaN
    }
    const float o = dense_row(wt, sh, W2, O, H);
    if (tid < O) out[c * ldout + tid] = o + (b2 != nullptr ? b2[tid] : 0.f);
}

// ---- backward, launch 1: the gradient of every cochain's pooled row ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void flow_head_bwd_small_kernel(const float* __restrict__ g, int64_t ldg, const float* __restrict__ h,
                                                                       const int64_t* __restrict__ ptr, int64_t N,
                                                                       const float* __restrict__ W1, const float* __restrict__ W2,
                                                                       float* __restrict__ dh_out, float* __restrict__ dpooled, int K, int H,
                                                                       int O, int mean, int64_t C, const int64_t* __restrict__ n_dev,
                                                                       const int64_t* __restrict__ c_dev) {
    __shared__ float gs[kMaxO];
    __shared__ float dhs[kMaxW];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    live_counts(ptr, n_dev, c_dev, N, C);
    if (c >= C) {                                             // an absent cochain: its row of g / h is never read
        if (dh_out != nullptr && tid < H) dh_out[c * H + tid] = 0.f;
        if (tid < K) dpooled[c * K + tid] = 0.f;
        return;
    }
    if (tid < O) gs[tid] = g[c * ldg + tid];
    __syncthreads();
    if (tid < H) {
        float ds = 0.f;
        for (int o = 0; o < O; ++o) ds = fmaf(gs[o], W2[o * H + tid], ds);          // o ascending
        const float dh = cwn_relu_bwd(h[c * H + tid], ds);
        if (dh_out != nullptr) dh_out[c * H + tid] = dh;
        dhs[tid] = dh;
    }
    __syncthreads();
    if (tid < K) {
        float dp = 0.f;
        for (int j = 0; j < H; ++j) dp = fmaf(dhs[j], W1[j * K + tid], dp);         // j ascending
        if (mean) {
            int64_t start, end;
            cochain_rows(ptr, c, N, start, end);
            dp = dp / (float)(end - start > 0 ? end - start : 1);
        }
        dpooled[c * K + tid] = dp;
    }
}

// ---- backward, launch 2: dx over the rows of every chunk ---------------------------------------------------------------------------------
__device__ __forceinline__ float sgn_times(float x, float d) { return x > 0.f ? d : (x < 0.f ? -d : 0.f); }

template <bool VEC>
__global__ __launch_bounds__(kThreads) void flow_head_dx_kernel(const float* __restrict__ x, int64_t N, int64_t ldx,
                                                                const int64_t* __restrict__ ptr, int64_t C, int K, int take_abs,
                                                                const float* __restrict__ dpooled, float* __restrict__ dx, int64_t lddx,
                                                                const int64_t* __restrict__ n_dev, const int64_t* __restrict__ c_dev) {
    const int tid = threadIdx.x;
    live_counts(ptr, n_dev, c_dev, N, C);
    if ((int64_t)blockIdx.x >= N / kChunk + C) return;        // (behind the last live slot: rows at or beyond the count stay as they are)
    int64_t c, r0, r1;
    if (!slot_chunk(ptr, C, N, (int64_t)blockIdx.x, tid & 63, c, r0, r1)) return;
    const int cols = (K + 3) >> 2;
    const int slots = kThreads / cols;
    const int q = tid % cols, s = tid / cols;
    if (s >= slots) return;
    const float4 d = load_quad<VEC>(dpooled + c * K, q, K);
    for (int64_t r = r0 + s; r < r1; r += 4 * (int64_t)slots) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t rr = r + (int64_t)u * slots;
            v[u] = (take_abs && rr < r1) ? load_quad<VEC>(x + rr * ldx, q, K) : make_float4(1.f, 1.f, 1.f, 1.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t rr = r + (int64_t)u * slots;
            if (rr >= r1) continue;
            const float4 o = take_abs ? make_float4(sgn_times(v[u].x, d.x), sgn_times(v[u].y, d.y), sgn_times(v[u].z, d.z),
                                                    sgn_times(v[u].w, d.w))
                                      : d;
            store_quad<VEC>(dx + rr * lddx, q, K, o);
        }
    }
}

// what both launchers check alike; CWN_OK or the error
int check_shapes(int64_t N, int64_t C, int64_t ldx, int32_t K, int32_t H, int32_t O, int32_t take_abs, int32_t mean) {
    if (K < 1 || K > kMaxW || H < 1 || H > kMaxW || O < 1 || O > kMaxO) return CWN_ERR_BAD_ARG;
    if ((take_abs != 0 && take_abs != 1) || (mean != 0 && mean != 1)) return CWN_ERR_BAD_ARG;
    if (N < 0 || C < 0 || ldx < K) return CWN_ERR_BAD_ARG;
    if (N >= INT32_MAX || C >= INT32_MAX || N / kChunk + C >= INT32_MAX) return CWN_ERR_TOO_LARGE;
    return CWN_OK;
}

}  // namespace

extern "C" size_t cwn_flow_head_workspace_floats(int64_t N, int64_t C, int32_t K) {
    if (N < 0 || C < 0 || K < 1) return 0;
    return (size_t)((N / kChunk + C) * (int64_t)K);
}

// Both forms of the forward: host counts (n_dev = c_dev = NULL) and the counted one (N, C capacities).
static int flow_head_fwd(const float* x, int64_t N, int64_t ldx, const int64_t* ptr, int64_t C, const float* W1, const float* b1,
                         const float* W2, const float* b2, float* out, int64_t ldout, float* pooled_out, float* h_out, int32_t K, int32_t H,
                         int32_t O, int32_t take_abs, int32_t mean, const int64_t* n_dev, const int64_t* c_dev, bool counted,
                         float* workspace, size_t workspace_floats, cwn_stream_t stream_) {
    const int bad = check_shapes(N, C, ldx, K, H, O, take_abs, mean);
    if (bad != CWN_OK) return bad;
    if (ldout < O) return CWN_ERR_BAD_ARG;
    if (N > 0 && x == nullptr) return CWN_ERR_BAD_ARG;
    if (C > 0 && (ptr == nullptr || W1 == nullptr || W2 == nullptr || out == nullptr || workspace == nullptr)) return CWN_ERR_BAD_ARG;
    if (counted && C > 0 && c_dev == nullptr) return CWN_ERR_BAD_ARG;
    for (const void* p : {(const void*)x, (const void*)W1, (const void*)b1, (const void*)W2, (const void*)b2, (const void*)out,
                          (const void*)pooled_out, (const void*)h_out})
        if (!al4(p)) return CWN_ERR_ALIGN;
    if (!al8(ptr) || !al8(n_dev) || !al8(c_dev) || !al16(workspace)) return CWN_ERR_ALIGN;
    if (C == 0) return CWN_OK;
    if (workspace_floats < cwn_flow_head_workspace_floats(N, C, K)) return CWN_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const unsigned slots = (unsigned)(N / kChunk + C);
    if (N > 0) {
        if (K % 4 == 0 && al16(x) && ldx % 4 == 0)
            flow_pool_kernel<true><<<dim3(slots), dim3(kThreads), 0, stream>>>(x, N, ldx, ptr, C, K, take_abs, workspace, n_dev, c_dev);
        else
            flow_pool_kernel<false><<<dim3(slots), dim3(kThreads), 0, stream>>>(x, N, ldx, ptr, C, K, take_abs, workspace, n_dev, c_dev);
        if (hipGetLastError() != hipSuccess) return CWN_ERR_LAUNCH;
    }
    flow_head_kernel<<<dim3((unsigned)C), dim3(kThreads), 0, stream>>>(workspace, ptr, N, W1, b1, W2, b2, out, ldout, pooled_out, h_out, K, H,
                                                                       O, mean, C, n_dev, c_dev);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

static int flow_head_bwd(const float* g_out, int64_t ldg, const float* h, const float* x, int64_t N, int64_t ldx, const int64_t* ptr,
                         int64_t C, const float* W1, const float* W2, float* dx, int64_t lddx, float* dh_out, int32_t K, int32_t H, int32_t O,
                         int32_t take_abs, int32_t mean, const int64_t* n_dev, const int64_t* c_dev, bool counted, float* workspace,
                         size_t workspace_floats, cwn_stream_t stream_) {
    const int bad = check_shapes(N, C, ldx, K, H, O, take_abs, mean);
    if (bad != CWN_OK) return bad;
    if (ldg < O || (dx != nullptr && lddx < K)) return CWN_ERR_BAD_ARG;
    if (N > 0 && dx != nullptr && take_abs && x == nullptr) return CWN_ERR_BAD_ARG;
    if (C > 0 && (ptr == nullptr || g_out == nullptr || h == nullptr || W1 == nullptr || W2 == nullptr || workspace == nullptr))
        return CWN_ERR_BAD_ARG;
    if (counted && C > 0 && c_dev == nullptr) return CWN_ERR_BAD_ARG;
    if (dx != nullptr && dx == x) return CWN_ERR_BAD_ARG;
    for (const void* p : {(const void*)g_out, (const void*)h, (const void*)x, (const void*)W1, (const void*)W2, (const void*)dx,
                          (const void*)dh_out})
        if (!al4(p)) return CWN_ERR_ALIGN;
    if (!al8(ptr) || !al8(n_dev) || !al8(c_dev) || !al16(workspace)) return CWN_ERR_ALIGN;
    if (C == 0) return CWN_OK;
    if (workspace_floats < cwn_flow_head_workspace_floats(N, C, K)) return CWN_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    flow_head_bwd_small_kernel<<<dim3((unsigned)C), dim3(kThreads), 0, stream>>>(g_out, ldg, h, ptr, N, W1, W2, dh_out, workspace, K, H, O,
                                                                                 mean, C, n_dev, c_dev);
    if (hipGetLastError() != hipSuccess) return CWN_ERR_LAUNCH;
    if (dx == nullptr || N == 0) return CWN_OK;
    const unsigned slots = (unsigned)(N / kChunk + C);
    if (K % 4 == 0 && (!take_abs || (al16(x) && ldx % 4 == 0)) && al16(dx) && lddx % 4 == 0)
        flow_head_dx_kernel<true><<<dim3(slots), dim3(kThreads), 0, stream>>>(x, N, ldx, ptr, C, K, take_abs, workspace, dx, lddx, n_dev, c_dev);
    else
        flow_head_dx_kernel<false><<<dim3(slots), dim3(kThreads), 0, stream>>>(x, N, ldx, ptr, C, K, take_abs, workspace, dx, lddx, n_dev, c_dev);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

extern "C" int cwn_flow_head_f32(const float* x, int64_t N, int64_t ldx, const int64_t* ptr, int64_t C, const float* W1,
                                 const float* b1, const float* W2, const float* b2, float* out, int64_t ldout, float* pooled_out,
                                 float* h_out, int32_t K, int32_t H, int32_t O, int32_t take_abs, int32_t mean, float* workspace,
                                 size_t workspace_floats, cwn_stream_t stream) {
    return flow_head_fwd(x, N, ldx, ptr, C, W1, b1, W2, b2, out, ldout, pooled_out, h_out, K, H, O, take_abs, mean, nullptr, nullptr, false,
                         workspace, workspace_floats, stream);
}

extern "C" int cwn_flow_head_bwd_f32(const float* g_out, int64_t ldg, const float* h, const float* x, int64_t N, int64_t ldx,
                                     const int64_t* ptr, int64_t C, const float* W1, const float* W2, float* dx, int64_t lddx,
                                     float* dh_out, int32_t K, int32_t H, int32_t O, int32_t take_abs, int32_t mean, float* workspace,
                                     size_t workspace_floats, cwn_stream_t stream) {
    return flow_head_bwd(g_out, ldg, h, x, N, ldx, ptr, C, W1, W2, dx, lddx, dh_out, K, H, O, take_abs, mean, nullptr, nullptr, false,
                         workspace, workspace_floats, stream);
}

extern "C" int cwn_flow_head_dev_f32(const float* x, int64_t N, int64_t ldx, const int64_t* ptr, int64_t C, const float* W1,
                                     const float* b1, const float* W2, const float* b2, float* out, int64_t ldout, float* pooled_out,
                                     float* h_out, int32_t K, int32_t H, int32_t O, int32_t take_abs, int32_t mean, const int64_t* n_dev,
                                     const int64_t* c_dev, float* workspace, size_t workspace_floats, cwn_stream_t stream) {
    return flow_head_fwd(x, N, ldx, ptr, C, W1, b1, W2, b2, out, ldout, pooled_out, h_out, K, H, O, take_abs, mean, n_dev, c_dev, true,
                         workspace, workspace_floats, stream);
}

extern "C" int cwn_flow_head_bwd_dev_f32(const float* g_out, int64_t ldg, const float* h, const float* x, int64_t N, int64_t ldx,
                                         const int64_t* ptr, int64_t C, const float* W1, const float* W2, float* dx, int64_t lddx,
                                         float* dh_out, int32_t K, int32_t H, int32_t O, int32_t take_abs, int32_t mean,
                                         const int64_t* n_dev, const int64_t* c_dev, float* workspace, size_t workspace_floats,
                                         cwn_stream_t stream) {
    return flow_head_bwd(g_out, ldg, h, x, N, ldx, ptr, C, W1, W2, dx, lddx, dh_out, K, H, O, take_abs, mean, n_dev, c_dev, true,
                         workspace, workspace_floats, stream);
}
