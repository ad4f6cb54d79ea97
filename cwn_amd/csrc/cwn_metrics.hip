// cwn_metrics.hip -- the evaluation half of an epoch on the device (exp/train_utils.py:92-211: eval() and the Evaluator).
//
//   cwn_metric_rank_f32         per column: the integer rank counts behind ROC-AUC and average precision (ties exact)
//   cwn_metric_abs_err_f32      per column: sum |pred - y| in float64 and the labeled count            (MAE)
//   cwn_metric_argmax_hits_f32  rows whose FIRST maximal column is their class                          (accuracy)
//   cwn_metric_pdist_below_f64  pairs i < j of float64 rows closer than eps in the Euclidean norm       (isomorphism)
//   cwn_loss_segments_f32       the criterion of every batch of an epoch in one launch, no gradient     (mean_loss)
//
// House rules: plain pointers, the caller owns every buffer (workspace sizes: the *_workspace_bytes functions), nothing
// here allocates, frees or synchronises.  No atomics: every sum goes through per-workgroup partials in the workspace and a
// finishing launch that adds them in a fixed order, so every result -- the float64 ones included -- is the same bits on
// every run.
//
// Rank counts.  With scores s and labels in {0, 1, NaN = unlabeled}, over the labeled rows of one column:
//     lt_i = #{negatives j: s_j < s_i}, eq_i = #{negatives j: s_j == s_i}, ge_i = #{positives j: s_j >= s_i}   (i positive)
//     AUC = (sum_i lt_i + 0.5 sum_i eq_i) / (n_pos n_neg)            (Mann-Whitney U with half credit for ties)
//     AP  = (1 / n_pos) sum_i ge_i / (ge_i + n_neg - lt_i)           (precision at every positive's own threshold)
// Only positives are `i` rows: a first launch compacts their scores per column (order-preserving, ballot + prefix), the
// counting launch gives every positive a thread and streams ALL rows of the column through LDS in tiles of 256 -- n_pos * n
// comparisons, not n^2 -- and workgroups past a column's positives leave at once.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/cwn_hip.h"
#include "cwn_check.h"

namespace {

constexpr int kT = CWN_METRIC_TILE;          // threads of a workgroup = rows of a tile (256)
constexpr int kMaxParts = 1024;              // workgroups of a strided reduction, per column
constexpr int kPT = CWN_METRIC_PDIST_TILE;   // rows of a pdist tile (64)
constexpr int kPC = 32;                      // columns of a pdist tile staged at a time

static_assert(kT == 256 && kPT == 64, "the thread maps below are written for these");

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) <= 3.402823466e38f; }    // false for NaN and +-inf

// fixed trees over the 256 threads of a workgroup (deterministic); the result is valid in thread 0
__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = kT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    return sh[0];
}
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = kT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    return sh[0];
}
__device__ __forceinline__ int64_t block_or_i64(int64_t v, int64_t* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = kT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] |= sh[threadIdx.x + off];
        __syncthreads();
    }
    return sh[0];
}

inline int64_t tiles_of(int64_t n) { return (n + kT - 1) / kT; }
inline int64_t parts_of(int64_t n) {          // workgroups of a strided reduction over n rows: a function of n alone
    int64_t p = (n + 8 * kT - 1) / (8 * kT);
    return p < 1 ? 1 : (p > kMaxParts ? kMaxParts : p);
}

// ---- rank counts ----------------------------------------------------------------------------------------------------------
// workspace of cwn_metric_rank_f32, per column t (nt = tiles_of(n)):
//   head   int64 [cols][4]        n_pos, n_neg, flag bits, unused
//   part_i int64 [cols][nt][2]    sum lt, sum eq of a tile of positives
//   part_d double [cols][nt]      sum of the precision terms of a tile of positives
//   pos    float [cols][nt * 256] the positives' scores, in row order
struct RankWs {
    int64_t* head;
    int64_t* part_i;
    double* part_d;
    float* pos;
    int64_t nt;
};

inline size_t rank_ws_bytes(int64_t n, int64_t cols) {
    const int64_t nt = tiles_of(n);
    return (size_t)cols * (size_t)(4 * 8 + nt * 2 * 8 + nt * 8 + nt * kT * 4);
}
inline RankWs rank_ws(void* ws, int64_t n, int64_t cols) {
    RankWs w;
    w.nt = tiles_of(n);
    w.head = static_cast<int64_t*>(ws);
    w.part_i = w.head + cols * 4;
    w.part_d = reinterpret_cast<double*>(w.part_i + cols * w.nt * 2);
    w.pos = reinterpret_cast<float*>(w.part_d + cols * w.nt);
    return w;
}

// one workgroup per column: count, flag and compact (the k-th positive of the column in row order lands at pos[k])
__global__ __launch_bounds__(kT) void rank_compact_kernel(const float* __restrict__ pred, const float* __restrict__ y, int64_t n,
                                                          int64_t cols, RankWs w) {
    __shared__ int wave_cnt[kT / 64];
    __shared__ int64_t sh[kT];
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float* pos = w.pos + t * w.nt * kT;
    int64_t base = 0, neg = 0, flag = 0;
    for (int64_t r0 = 0; r0 < n; r0 += kT) {
        const int64_t r = r0 + tid;
        bool is_pos = false;
        float s = 0.f;
        if (r < n) {
            const float l = y[r * cols + t];
            s = pred[r * cols + t];
            if (l == l) {                                   // NaN: unlabeled, ignored (exp/train_utils.py:131)
                if (l == 1.f) is_pos = true;
                else if (l == 0.f) ++neg;
                else flag |= CWN_METRIC_FLAG_LABEL;         // neither 0, 1 nor NaN: counted nowhere, reported
                if (!is_finite(s) && (l == 1.f || l == 0.f)) flag |= CWN_METRIC_FLAG_NONFINITE;
            }
        }
        const unsigned long long m = __ballot(is_pos);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int k = 0; k < kT / 64; ++k) {
            const int c = wave_cnt[k];
            before += k < wv ? c : 0;
            total += c;
        }
        if (is_pos) pos[base + before] = s;                 // base + before < n_pos <= n <= nt * 256
        base += total;
        __syncthreads();                                    // wave_cnt is rewritten by the next round
    }
    const int64_t n_neg = block_sum_i64(neg, sh);
    const int64_t flags = block_or_i64(flag, sh);
    if (tid == 0) {
        w.head[t * 4 + 0] = base;
        w.head[t * 4 + 1] = n_neg;
        w.head[t * 4 + 2] = flags;
        w.head[t * 4 + 3] = 0;
    }
}

// grid (nt, cols): a thread per positive of the tile, every row of the column through LDS.  A row sits in the tile as
// (its score if it is a negative, else NaN; its score if it is a positive, else NaN): three compares per pair, an
// unlabeled row matches none of them.
__global__ __launch_bounds__(kT) void rank_count_kernel(const float* __restrict__ pred, const float* __restrict__ y, int64_t n,
                                                        int64_t cols, RankWs w) {
    __shared__ float2 tile[kT];
    __shared__ int64_t sh_i[kT];
    __shared__ double sh_d[kT];
    const int64_t t = blockIdx.y, tl = blockIdx.x;
    const int64_t n_pos = w.head[t * 4 + 0], n_neg = w.head[t * 4 + 1];
    if (tl * kT >= n_pos) return;                           // (the whole workgroup: no positives in this tile)
    const int tid = threadIdx.x;
    const int64_t i = tl * kT + tid;
    const bool active = i < n_pos;
    const float nanf_ = __int_as_float(0x7fc00000);
    const float si = active ? w.pos[t * w.nt * kT + i] : nanf_;
    int lt = 0, eq = 0, ge = 0;                             // n < 2^31 (checked by the entry point)
    for (int64_t r0 = 0; r0 < n; r0 += kT) {
        const int64_t r = r0 + tid;
        float2 e = make_float2(nanf_, nanf_);
        if (r < n) {
            const float l = y[r * cols + t], s = pred[r * cols + t];
            if (l == 0.f) e.x = s;
            else if (l == 1.f) e.y = s;
        }
        __syncthreads();                                    // the previous tile has been read
        tile[tid] = e;
        __syncthreads();
        const int lim = (n - r0) < kT ? (int)(n - r0) : kT;
        for (int k = 0; k < lim; ++k) {
            const float2 v = tile[k];                       // one address for the wave: a broadcast read
            lt += v.x < si ? 1 : 0;
            eq += v.x == si ? 1 : 0;
            ge += v.y >= si ? 1 : 0;
        }
    }
    // precision at this positive's threshold: positives / everything labeled with a score >= s_i (ge >= 1: itself)
    const double term = (active && ge > 0) ? (double)ge / (double)((int64_t)ge + (n_neg - (int64_t)lt)) : 0.0;
    const int64_t s_lt = block_sum_i64(active ? lt : 0, sh_i);
    const int64_t s_eq = block_sum_i64(active ? eq : 0, sh_i);
    const double s_d = block_sum_f64(term, sh_d);
    if (tid == 0) {
        w.part_i[(t * w.nt + tl) * 2 + 0] = s_lt;
        w.part_i[(t * w.nt + tl) * 2 + 1] = s_eq;
        w.part_d[t * w.nt + tl] = s_d;
    }
}

// one workgroup per column: the tiles' partials in a fixed order (thread k takes tiles k, k + 256, ...; then the tree)
__global__ __launch_bounds__(kT) void rank_finish_kernel(int64_t cols, RankWs w, int64_t* __restrict__ counts,
                                                         double* __restrict__ ap_sum, int32_t* __restrict__ flag) {
    __shared__ int64_t sh_i[kT];
    __shared__ double sh_d[kT];
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t n_pos = w.head[t * 4 + 0];
    const int64_t tiles = (n_pos + kT - 1) / kT;            // <= nt: the tiles rank_count_kernel wrote
    int64_t lt = 0, eq = 0;
    double d = 0.0;
    for (int64_t k = tid; k < tiles; k += kT) {
        lt += w.part_i[(t * w.nt + k) * 2 + 0];
        eq += w.part_i[(t * w.nt + k) * 2 + 1];
        d += w.part_d[t * w.nt + k];
    }
    lt = block_sum_i64(lt, sh_i);
    eq = block_sum_i64(eq, sh_i);
    d = block_sum_f64(d, sh_d);
    if (tid == 0) {
        counts[t * 4 + 0] = n_pos;
        counts[t * 4 + 1] = w.head[t * 4 + 1];
        counts[t * 4 + 2] = lt;
        counts[t * 4 + 3] = eq;
        ap_sum[t] = d;
    }
    if (blockIdx.x == 0) {
        int64_t f = 0;
        for (int64_t c = tid; c < cols; c += kT) f |= w.head[c * 4 + 2];
        f = block_or_i64(f, sh_i);
        if (tid == 0) *flag = (int32_t)f;
    }
}

// ---- strided reductions: MAE and accuracy ------------------------------------------------------------------------------------
// grid (parts, cols); partials pd / pi [cols][parts]
__global__ __launch_bounds__(kT) void abs_err_kernel(const float* __restrict__ pred, const float* __restrict__ y, int64_t n,
                                                     int64_t cols, double* __restrict__ pd, int64_t* __restrict__ pi) {
    __shared__ int64_t sh_i[kT];
    __shared__ double sh_d[kT];
    const int64_t t = blockIdx.y, parts = gridDim.x;
    double acc = 0.0;
    int64_t cnt = 0;
    for (int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x; r < n; r += parts * kT) {
        const float l = y[r * cols + t];
        if (l == l) {
            acc += fabs((double)pred[r * cols + t] - (double)l);
            ++cnt;
        }
    }
    acc = block_sum_f64(acc, sh_d);
    cnt = block_sum_i64(cnt, sh_i);
    if (threadIdx.x == 0) {
        pd[t * parts + blockIdx.x] = acc;
        pi[t * parts + blockIdx.x] = cnt;
    }
}

// a thread per row: numpy's argmax (the FIRST maximal column; a NaN counts as maximal, the first NaN wins)
__global__ __launch_bounds__(kT) void argmax_hits_kernel(const float* __restrict__ pred, const int64_t* __restrict__ y, int64_t n,
                                                         int64_t C, int64_t* __restrict__ pi) {
    __shared__ int64_t sh_i[kT];
    const int64_t parts = gridDim.x;
    int64_t hits = 0;
    for (int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x; r < n; r += parts * kT) {
        const float* p = pred + r * C;
        float best = p[0];
        int64_t arg = 0;
        for (int64_t j = 1; j < C; ++j) {
            const float v = p[j];
            if (best == best && !(v <= best)) {             // v > best, or v is the row's first NaN
                best = v;
                arg = j;
            }
        }
        hits += arg == y[r] ? 1 : 0;
    }
    hits = block_sum_i64(hits, sh_i);
    if (threadIdx.x == 0) pi[blockIdx.x] = hits;
}

// one workgroup per column: out_d[t] = sum_k pd[t][k], out_i[t] = sum_k pi[t][k] (either pair may be NULL), fixed order
__global__ __launch_bounds__(kT) void sum_parts_kernel(const double* __restrict__ pd, const int64_t* __restrict__ pi, int64_t parts,
                                                       double* __restrict__ out_d, int64_t* __restrict__ out_i) {
    __shared__ int64_t sh_i[kT];
    __shared__ double sh_d[kT];
    const int64_t t = blockIdx.x;
    double d = 0.0;
    int64_t c = 0;
    for (int64_t k = threadIdx.x; k < parts; k += kT) {
        if (pd != nullptr) d += pd[t * parts + k];
        if (pi != nullptr) c += pi[t * parts + k];
    }
    d = block_sum_f64(d, sh_d);
    c = block_sum_i64(c, sh_i);
    if (threadIdx.x == 0) {
        if (out_d != nullptr) out_d[t] = d;
        if (out_i != nullptr) out_i[t] = c;
    }
}

// ---- pairs below eps (float64) ---------------------------------------------------------------------------------------------------
// grid (tiles, tiles): workgroup (bi, bj), bi <= bj, holds rows [64 bi, +64) and [64 bj, +64) in LDS, 32 columns at a time;
// thread: row i = tid & 63 of the first tile against rows (tid >> 6) + 4 k, k < 16, of the second (one address per wave
// for those: a broadcast).  Rows of 33 doubles: the lanes' 8-byte reads of a column fall on distinct bank pairs.
__global__ __launch_bounds__(kT) void pdist_below_kernel(const double* __restrict__ x, int64_t n, int64_t d, double eps,
                                                         int64_t* __restrict__ pi) {
    __shared__ double xi[kPT][kPC + 1];
    __shared__ double xj[kPT][kPC + 1];
    __shared__ int64_t sh_i[kT];
    const int64_t bi = blockIdx.y, bj = blockIdx.x, tiles = gridDim.x;
    const int tid = threadIdx.x;
    if (bi > bj) {                                          // (the whole workgroup) the pair (bj, bi) counts these
        if (tid == 0) pi[bi * tiles + bj] = 0;
        return;
    }
    const int il = tid & 63, jl = tid >> 6;
    double acc[kPT / 4];
#pragma unroll
    for (int k = 0; k < kPT / 4; ++k) acc[k] = 0.0;
    for (int64_t c0 = 0; c0 < d; c0 += kPC) {
        __syncthreads();                                    // the previous chunk has been read
#pragma unroll
        for (int k = 0; k < kPT * kPC / kT; ++k) {
            const int e = tid + kT * k, row = e / kPC, col = e % kPC;
            const int64_t gi = bi * kPT + row, gj = bj * kPT + row, gc = c0 + col;
            xi[row][col] = (gi < n && gc < d) ? x[gi * d + gc] : 0.0;      // zeros past the edges: no contribution
            xj[row][col] = (gj < n && gc < d) ? x[gj * d + gc] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < kPC; ++c) {
            const double a = xi[il][c];
#pragma unroll
            for (int k = 0; k < kPT / 4; ++k) {
                const double df = a - xj[jl + 4 * k][c];
                acc[k] += df * df;
            }
        }
    }
    int64_t below = 0;
    const int64_t gi = bi * kPT + il;
#pragma unroll
    for (int k = 0; k < kPT / 4; ++k) {
        const int64_t gj = bj * kPT + jl + 4 * k;
        below += (gi < gj && gj < n && sqrt(acc[k]) < eps) ? 1 : 0;
    }
    below = block_sum_i64(below, sh_i);
    if (tid == 0) pi[bi * tiles + bj] = below;
}

// ---- the criterion of every batch of an epoch ----------------------------------------------------------------------------------
// One workgroup per batch b: rows ptr[b] .. ptr[b + 1] of pred [n_rows, cols]; the element losses are cwn_loss_cols_f32's
// (cwn_norm.hip: torch's definitions, fp32), summed in float64, mean over the labeled entries, NaN when there are none.
__global__ __launch_bounds__(kT) void loss_segments_kernel(int kind, const float* __restrict__ pred, const float* __restrict__ y,
                                                           const int64_t* __restrict__ ptr, int64_t n_rows, int64_t cols,
                                                           float* __restrict__ out) {
    __shared__ int64_t sh_i[kT];
    __shared__ double sh_d[kT];
    const int64_t b = blockIdx.x;
    int64_t lo = ptr[b], hi = ptr[b + 1];
    lo = lo < 0 ? 0 : (lo > n_rows ? n_rows : lo);          // never outside pred, whatever the table holds
    hi = hi < lo ? lo : (hi > n_rows ? n_rows : hi);
    double s = 0.0;
    int64_t cnt = 0;
    if (kind == CWN_LOSS_CE) {
        const int64_t* cls = reinterpret_cast<const int64_t*>(y);
        for (int64_t r = lo + threadIdx.x; r < hi; r += kT) {
            const int64_t c = cls[r];
            if (c < 0) continue;                            // torch's ignore_index is negative
            ++cnt;
            if (c >= cols) {                                // no column for the class: NaN, never a silent smaller mean
                s = (double)__int_as_float(0x7fc00000);
                continue;
            }
            const float* p = pred + r * cols;
            float m = p[0];
            for (int64_t j = 1; j < cols; ++j) m = fmaxf(m, p[j]);
            float z = 0.f;
            for (int64_t j = 0; j < cols; ++j) z += expf(p[j] - m);
            s += (double)((m + logf(z)) - p[c]);
        }
    } else {
        for (int64_t i = lo * cols + threadIdx.x; i < hi * cols; i += kT) {
            const float p = pred[i], t = y[i], df = p - t;
            if (!(t == t)) continue;                        // a NaN target is no label
            float l;
            if (kind == CWN_LOSS_L1) l = fabsf(df);
            else if (kind == CWN_LOSS_MSE) l = df * df;
            else l = fmaxf(p, 0.f) - p * t + log1pf(expf(-fabsf(p)));
            s += (double)l;
            ++cnt;
        }
    }
    s = block_sum_f64(s, sh_d);
    cnt = block_sum_i64(cnt, sh_i);
    if (threadIdx.x == 0) out[b] = cnt > 0 ? (float)(s / (double)cnt) : __int_as_float(0x7fc00000);
}

inline int launched() { return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH; }

}  // namespace

extern "C" size_t cwn_metric_rank_workspace_bytes(int64_t n, int64_t cols) {
    if (n <= 0 || cols <= 0 || n > INT32_MAX || cols > 65535) return 0;
    return rank_ws_bytes(n, cols);
}

extern "C" int cwn_metric_rank_f32(const float* pred, const float* y, int64_t n, int64_t cols, void* workspace,
                                   size_t workspace_bytes, int64_t* counts, double* ap_sum, int32_t* flag, cwn_stream_t stream_) {
    if (n <= 0 || cols <= 0 || pred == nullptr || y == nullptr || workspace == nullptr || counts == nullptr || ap_sum == nullptr ||
        flag == nullptr)
        return CWN_ERR_BAD_ARG;
    if (n > INT32_MAX || cols > 65535) return CWN_ERR_TOO_LARGE;           // int32 counters per row; grid.y
    if (workspace_bytes < rank_ws_bytes(n, cols)) return CWN_ERR_WORKSPACE;
    if (!al4(pred) || !al4(y) || !al8(workspace) || !al8(counts) || !al8(ap_sum) || !al4(flag)) return CWN_ERR_ALIGN;
    const RankWs w = rank_ws(workspace, n, cols);
    hipStream_t s = (hipStream_t)stream_;
    rank_compact_kernel<<<dim3((unsigned)cols), dim3(kT), 0, s>>>(pred, y, n, cols, w);
    rank_count_kernel<<<dim3((unsigned)w.nt, (unsigned)cols), dim3(kT), 0, s>>>(pred, y, n, cols, w);
    rank_finish_kernel<<<dim3((unsigned)cols), dim3(kT), 0, s>>>(cols, w, counts, ap_sum, flag);
    return launched();
}

extern "C" size_t cwn_metric_abs_err_workspace_bytes(int64_t n, int64_t cols) {
    if (n <= 0 || cols <= 0 || cols > 65535) return 0;
    return (size_t)cols * (size_t)parts_of(n) * 16;
}

extern "C" int cwn_metric_abs_err_f32(const float* pred, const float* y, int64_t n, int64_t cols, void* workspace,
                                      size_t workspace_bytes, double* sum, int64_t* count, cwn_stream_t stream_) {
    if (n <= 0 || cols <= 0 || pred == nullptr || y == nullptr || workspace == nullptr || sum == nullptr || count == nullptr)
        return CWN_ERR_BAD_ARG;
    if (cols > 65535) return CWN_ERR_TOO_LARGE;
    const int64_t parts = parts_of(n);
    if (workspace_bytes < (size_t)cols * (size_t)parts * 16) return CWN_ERR_WORKSPACE;
    if (!al4(pred) || !al4(y) || !al8(workspace) || !al8(sum) || !al8(count)) return CWN_ERR_ALIGN;
    double* pd = static_cast<double*>(workspace);
    int64_t* pi = reinterpret_cast<int64_t*>(pd + cols * parts);
    hipStream_t s = (hipStream_t)stream_;
    abs_err_kernel<<<dim3((unsigned)parts, (unsigned)cols), dim3(kT), 0, s>>>(pred, y, n, cols, pd, pi);
    sum_parts_kernel<<<dim3((unsigned)cols), dim3(kT), 0, s>>>(pd, pi, parts, sum, count);
    return launched();
}

extern "C" size_t cwn_metric_argmax_hits_workspace_bytes(int64_t n) {
    return n <= 0 ? 0 : (size_t)parts_of(n) * 8;
}

extern "C" int cwn_metric_argmax_hits_f32(const float* pred, const int64_t* y, int64_t n, int64_t C, void* workspace,
                                          size_t workspace_bytes, int64_t* hits, cwn_stream_t stream_) {
    if (n <= 0 || C <= 0 || pred == nullptr || y == nullptr || workspace == nullptr || hits == nullptr) return CWN_ERR_BAD_ARG;
    const int64_t parts = parts_of(n);
    if (workspace_bytes < (size_t)parts * 8) return CWN_ERR_WORKSPACE;
    if (!al4(pred) || !al8(y) || !al8(workspace) || !al8(hits)) return CWN_ERR_ALIGN;
    int64_t* pi = static_cast<int64_t*>(workspace);
    hipStream_t s = (hipStream_t)stream_;
    argmax_hits_kernel<<<dim3((unsigned)parts), dim3(kT), 0, s>>>(pred, y, n, C, pi);
    sum_parts_kernel<<<dim3(1), dim3(kT), 0, s>>>(nullptr, pi, parts, nullptr, hits);
    return launched();
}

extern "C" size_t cwn_metric_pdist_below_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    const int64_t tiles = (n + kPT - 1) / kPT;
    return tiles > 65535 ? 0 : (size_t)(tiles * tiles) * 8;
}

extern "C" int cwn_metric_pdist_below_f64(const double* x, int64_t n, int64_t d, double eps, void* workspace,
                                          size_t workspace_bytes, int64_t* count, cwn_stream_t stream_) {
    if (n <= 0 || d <= 0 || x == nullptr || workspace == nullptr || count == nullptr) return CWN_ERR_BAD_ARG;
    const int64_t tiles = (n + kPT - 1) / kPT;
    if (tiles > 65535) return CWN_ERR_TOO_LARGE;
    if (workspace_bytes < (size_t)(tiles * tiles) * 8) return CWN_ERR_WORKSPACE;
    if (!al8(x) || !al8(workspace) || !al8(count)) return CWN_ERR_ALIGN;
    int64_t* pi = static_cast<int64_t*>(workspace);
    hipStream_t s = (hipStream_t)stream_;
    pdist_below_kernel<<<dim3((unsigned)tiles, (unsigned)tiles), dim3(kT), 0, s>>>(x, n, d, eps, pi);
    sum_parts_kernel<<<dim3(1), dim3(kT), 0, s>>>(nullptr, pi, tiles * tiles, nullptr, count);
    return launched();
}

extern "C" int cwn_loss_segments_f32(int32_t kind, const float* pred, const float* y, const int64_t* ptr, int64_t n_batches,
                                     int64_t n_rows, int64_t cols, float* out, cwn_stream_t stream_) {
    if (kind < 0 || kind > CWN_LOSS_CE || n_batches <= 0 || n_rows < 0 || cols <= 0 || pred == nullptr || y == nullptr ||
        ptr == nullptr || out == nullptr)
        return CWN_ERR_BAD_ARG;
    if (n_batches > INT32_MAX) return CWN_ERR_TOO_LARGE;
    if (!al4(pred) || !(kind == CWN_LOSS_CE ? al8(y) : al4(y)) || !al8(ptr) || !al4(out)) return CWN_ERR_ALIGN;
    loss_segments_kernel<<<dim3((unsigned)n_batches), dim3(kT), 0, (hipStream_t)stream_>>>(kind, pred, y, ptr, n_rows, cols, out);
    return launched();
}
