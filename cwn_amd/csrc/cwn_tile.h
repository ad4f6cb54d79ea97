// cwn_tile.h -- the workgroup design of the dense-stage kernels, written once: update_mlp_kernel (cwn_mlp.hip),
// update_mlp3_kernel (cwn_mlp3.hip), dense_stage_kernel / dense_stage_ex_kernel / dense_stage_bwd_kernel (cwn_stage.hip).
//
// 512 threads = 8 waves take TM = 4096 / F rows of one descriptor (F = 64 or 128: the width of every Linear).  Wave w owns
// column tile w % (F / 16) and the two 16-row tiles 2 (w / (F / 16)), + 1.  An input tile is split ONCE per element into
// three bf16 planes in LDS (cwn_split.h); the packed weight (cwn_update_mlp_pack_weights_f32: fragment order, 1-KiB chunks)
// streams through register sets, one multiplication ahead, between the cwn::mfma_split6 steps.  The kernels keep what is
// theirs: the descriptors, the prologue of their rows, the chain of request_* / multiply / finish / lds_barrier calls.
//
// These kernels sit at their register limit, and the compiler's choices follow the exact form of this text.  The check for
// every edit of this header is tools/isa_diff.sh <file.hip> <rev> on the three files (cwn_mlp.hip with the Makefile's PRELOAD
// in ISA_DIFF_FLAGS, and once more with -DCWN_MLP_TIMING): the device assembly does not change.  What that check decided:
//   * everything is __forceinline__ and takes its compile-time constants from the shape; the wave's position (ct, rt0, lane,
//     l15, kq) comes from the WaveTile the kernel built once, never re-derived in a helper;
//   * what runs between two k steps is a callable (multiply's `between`), not a pointer or an index tested here: as a loaded
//     value the compile-time "nothing follows" becomes a test, and update_mlp3_kernel spills 136 registers;
//   * a descriptor's fields are read HERE, through a reference to the descriptor (request_rows, request_consts, finish), where
//     the kernels' own text read them: passed as values they are loaded at the call and the schedule changes;
//   * store_planes takes its float4 by value, and its two users in this header are two instantiations (SITE): through a
//     reference, or as one function with two callers, equivalent address arithmetic comes out in another form (157 lines of
//     update_mlp3_kernel<128>, 1297 of the stage kernels);
//   * request_kstep takes ct and lane as arguments: as a member, update_mlp_kernel<64, 2, true, true> forms its swizzle term
//     from another, equal value (229 lines);
//   * the kernels call these through one-line lambdas of their own, as their chains always did.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include "../../include/cwn_hip.h"
#include "cwn_split.h"
#include "cwn_check.h"
#include "cwn_act.h"
#include "cwn_mem.h"

namespace cwn {

constexpr int kTileThreads = 512;

// RT: 16-row tiles per wave (= float4 of an input tile per thread).
// bf16 elements per LDS row: F + 8 -- 16 bytes of padding make the fragment reads (16 rows x 16 B per quarter wave)
// conflict-free.  SWIZZLE (three-buffer kernels at width 64: three padded buffers of 64 rows are 2 KB beyond half a CU): the
// rows are unpadded and the 16-byte chunks of a row XOR-swizzled with (row >> 1) & 7 instead (col(): rows r, r + 1 differ in
// bank half, the eight row pairs of a fragment read in chunk).
template <int F, int RT, bool SWIZZLE> struct TileShape {
    static constexpr int kF = F, kRT = RT, kV = RT;
    static constexpr int kTM = RT * 2048 / F;
    static constexpr int kNCT = F / 16;
    static constexpr int kKS = F / 32;
    static constexpr int kRowStride = SWIZZLE ? F : F + 8;
    static __device__ __forceinline__ int col(int row, int c) {
        if constexpr (SWIZZLE) return (((c >> 3) ^ ((row >> 1) & 7)) << 3) | (c & 7);
        else return c;
    }
    static constexpr int kChunksPerTile = kKS * 3;    // packed weight: 1-KiB chunks per 16-column tile (k steps x planes)
    static constexpr size_t kPlaneElems = (size_t)kTM * kRowStride;
    static constexpr size_t kBufBytes = 3 * kPlaneElems * 2;   // three planes
    static_assert(kTM * (F / 4) == kV * kTileThreads && (kTM / 16) * kNCT == 8 * kRT, "tile shape");
};

// workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every outstanding GLOBAL load
// (s_waitcnt vmcnt(0)) -- here the tiles and the next weight, which are meant to keep streaming across the barrier
// (measured on update_mlp_kernel: 3.3 k cycles per stage spent in that wait)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

// row r of the tile at row0: rows past M (the capacity of the buffers) are clamped, not guarded -- their results are
// neither stored nor counted
__device__ __forceinline__ int64_t clamped_row(int64_t row0, int r, int64_t M) { return row0 + r < M ? row0 + r : M - 1; }

// The wave's position in the tile: ct its column tile, rt0 its first row tile, l15 = lane & 15, kq = lane >> 4.
// D[i][j] of an accumulator: i = output column kq * 4 + reg, j = row l15 -- a lane holds 4 consecutive columns of one row.
template <class S> struct WaveTile {
    typedef float4 RowRegs[S::kV];              // an input tile: TM rows x F / 4 float4, row-contiguous
    typedef uint4 WeightRegs[S::kKS][3];        // the stationary operand: this wave's 16 output columns, [k step][plane]
    typedef frag_cd AccRegs[S::kRT];
    int ct, rt0, lane, l15, kq;

    template <class Desc>
    static __device__ __forceinline__ void request_rows(RowRegs& v, const float* X, int64_t ld, int64_t row0, const Desc& D) {
#pragma unroll
        for (int i = 0; i < S::kV; ++i) {
            const int idx = threadIdx.x + i * kTileThreads, r = idx / (S::kF / 4), c4 = idx % (S::kF / 4);
            v[i] = reinterpret_cast<const float4*>(X + clamped_row(row0, r, D.M) * ld)[c4];
        }
    }
    // v, columns c .. c + 3 of tile row r: split and stored into the three planes of buf (SITE: see the head of the file)
    template <int SITE = 0>
    static __device__ __forceinline__ void store_planes(uint16_t* buf, int r, int c, float4 v) {
        uint2 ph, pm, pl;
        split4(v, ph, pm, pl);
        uint16_t* dst = buf + (size_t)r * S::kRowStride + S::col(r, c);
        *reinterpret_cast<uint2*>(dst) = ph;
        *reinterpret_cast<uint2*>(dst + S::kPlaneElems) = pm;
        *reinterpret_cast<uint2*>(dst + 2 * S::kPlaneElems) = pl;
    }
    static __device__ __forceinline__ void stage_rows(const RowRegs& v, uint16_t* buf) {
#pragma unroll
        for (int i = 0; i < S::kV; ++i) {
            const int idx = threadIdx.x + i * kTileThreads, r = idx / (S::kF / 4), c4 = idx % (S::kF / 4);
            store_planes(buf, r, c4 * 4, v[i]);
        }
    }

    // k step ks of this wave's column tile of a packed weight: three 1-KiB chunks, one per plane
    static __device__ __forceinline__ void request_kstep(WeightRegs& wf, const void* packed, int ks, int ct, int lane) {
        const unsigned char* wp = reinterpret_cast<const unsigned char*>(packed) + (size_t)ct * S::kChunksPerTile * 1024 + lane * 16;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) wf[ks][pl] = *reinterpret_cast<const uint4*>(wp + (ks * 3 + pl) * 1024);
    }
    __device__ __forceinline__ void request_weight(WeightRegs& wf, const void* packed) const {
#pragma unroll
        for (int ks = 0; ks < S::kKS; ++ks) request_kstep(wf, packed, ks, ct, lane);
    }
    // acc += buf x W^T (k steps in order, six terms each: cwn_split.h).  between(ks) runs after each k step: nothing, or the
    // request of k step ks of the NEXT weight into the other register set -- three 1-KiB loads a wave at a time, which the
    // address unit takes without making the wave wait (requested twelve at once after the stage, the waves sat in the issue
    // of their loads for 1.5 k cycles while the matrix pipe idled, and then multiplied while the address unit idled)
    template <class Between>
    __device__ __forceinline__ void multiply(AccRegs& acc, const uint16_t* buf, const WeightRegs& wf, Between&& between) const {
#pragma unroll
        for (int ks = 0; ks < S::kKS; ++ks) {
#pragma unroll
            for (int rt = 0; rt < S::kRT; ++rt) {
                const int row = (rt0 + rt) * 16 + l15;
                const uint16_t* p = buf + (size_t)row * S::kRowStride + S::col(row, ks * 32 + kq * 8);
                const uint4 xh = *reinterpret_cast<const uint4*>(p);
                const uint4 xm = *reinterpret_cast<const uint4*>(p + S::kPlaneElems);
                const uint4 xl = *reinterpret_cast<const uint4*>(p + 2 * S::kPlaneElems);
                acc[rt] = mfma_split6(wf[ks][0], wf[ks][1], wf[ks][2], xh, xm, xl, acc[rt]);
            }
            between(ks);
        }
    }

    // the epilogue constants of a stage (inference: bias and the folded BatchNorm) are requested BEFORE its MFMAs, and so
    // before the next weight: loads return in order, a constant behind 96 KB of weight is a wait for the weight (measured:
    // 4.4 k cycles a stage)
    struct Consts { float4 b, sc, sh; bool affine; };
    template <class Dim>
    __device__ __forceinline__ void request_consts(Consts& c, const Dim& D, int s) const {
        const int n0 = ct * 16 + kq * 4;
        c.b = make_float4(0.f, 0.f, 0.f, 0.f);
        c.sc = make_float4(1.f, 1.f, 1.f, 1.f);
        c.sh = c.b;
        if (D.bias[s] != nullptr) c.b = *reinterpret_cast<const float4*>(D.bias[s] + n0);
        c.affine = D.scale[s] != nullptr;
        if (c.affine) {
            c.sc = *reinterpret_cast<const float4*>(D.scale[s] + n0);
            c.sh = *reinterpret_cast<const float4*>(D.shift[s] + n0);
        }
    }
    // epilogue of a stage: + bias, folded BatchNorm, ReLU; then either into the planes of `buf` (the next stage's operand)
    // or, buf == NULL (the last stage), the rows that exist (row0 + r < Mv) to y
    template <class Dim>
    __device__ __forceinline__ void finish(const AccRegs& acc, const Consts& c, uint16_t* buf, const Dim& D, int64_t row0, int64_t Mv) const {
        const int n0 = ct * 16 + kq * 4;
        const float4 b4 = c.b, sc = c.sc, sh = c.sh;
        const bool affine = c.affine;
#pragma unroll
        for (int rt = 0; rt < S::kRT; ++rt) {
            float o[4] = {acc[rt][0] + b4.x, acc[rt][1] + b4.y, acc[rt][2] + b4.z, acc[rt][3] + b4.w};
            if (affine) {
                o[0] = o[0] * sc.x + sh.x;
                o[1] = o[1] * sc.y + sh.y;
                o[2] = o[2] * sc.z + sh.z;
                o[3] = o[3] * sc.w + sh.w;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = cwn_relu(o[q]);
            const int r = (rt0 + rt) * 16 + l15;
            if (buf != nullptr) store_planes<1>(buf, r, n0, make_float4(o[0], o[1], o[2], o[3]));
            else if (row0 + r < Mv) store_result4(D.y + (row0 + r) * D.ldy + n0, o[0], o[1], o[2], o[3]);
        }
    }
};

// ---- host side ----------------------------------------------------------------------------------------------------------

// Kernel<<<blocks, 512 threads, lds_bytes of dynamic LDS>>>(args...), the kernel's limit of dynamic LDS raised to lds_bytes
// once per process (above 64 KiB a launch fails without it)
template <auto Kernel, typename... Args>
int launch_tile(size_t lds_bytes, int64_t blocks, hipStream_t stream, const Args&... args) {
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [lds_bytes] {
        attr_err = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    });
    if (attr_err != hipSuccess) return CWN_ERR_LAUNCH;
    Kernel<<<dim3((unsigned)blocks), dim3(kTileThreads), lds_bytes, stream>>>(args...);
    return hipGetLastError() == hipSuccess ? CWN_OK : CWN_ERR_LAUNCH;
}

}  // namespace cwn
