// fx_imajor.hip — the two kernels around the emulation launch of an instance-major block (fx_imajor.hpp): a 2-D transposition
// between n streams of R words at a stride and the per-instance scratch [R][n].  gfx950, wave64, workgroups of 256 lanes.
//
// A workgroup moves a tile of TI instances x TR run-words through LDS, held as [TI][TR + 1] dwords.  On the stream side a
// wavefront access covers 64 / TR instances x TR consecutive words of their runs (TR = 64: 256 contiguous bytes of one stream), on
// the wide side 256 contiguous bytes of one scratch row.  With the odd pitch both LDS directions are conflict-free by the bank
// rule of ds_read_b32 / ds_write_b32 (bank = dword address mod 32, conflicts within a 32-lane half): along a run the 32 lanes hold
// consecutive dwords, across the runs lane l holds l * (TR + 1) + r = l + r (mod 32) for TR = 32 and 64.  Sixteen loads per
// lane are in flight before the barrier.  Every access is one dword: base and stride are only 4-byte aligned, and words are
// moved as bit patterns.  Lanes outside the n runs or the `rows` words touch no memory at all.
//
// Two tile shapes: 64 x 64, and 128 instances x 32 words for pieces of at most kNarrowRows words (the real-time block: 32 samples,
// mono), where a 64-word tile would be half empty.  Building with -DFX_IMAJOR_NARROW_ROWS=0 leaves the 64 x 64 tile alone: how the
// two were measured against each other.
#include <hip/hip_runtime.h>

#include "fx_imajor.hpp"

#ifndef FX_IMAJOR_NARROW_ROWS
#define FX_IMAJOR_NARROW_ROWS 32
#endif

namespace fx {

namespace {

constexpr int kLanes = 256;
constexpr int kTileWords = 4096;                  // TI * TR
constexpr int kPasses = kTileWords / kLanes;      // loads in flight per lane
constexpr long long kNarrowRows = FX_IMAJOR_NARROW_ROWS;

// grid.x = tiles of TI instances, grid.y strides over the tiles of TR run-words
template <int TI, int TR, bool kGather>
__device__ __forceinline__ void transposeTiles(const ImajorArgs& a) {
    static_assert(TI * TR == kTileWords && TI % 64 == 0 && (TR == 32 || TR == 64), "tile shape");
    __shared__ uint32_t tile[TI * (TR + 1)];
    const unsigned t = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * TI;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(a.in);
    uint32_t* out = reinterpret_cast<uint32_t*>(a.out);
    uint32_t* wide = reinterpret_cast<uint32_t*>(a.wide);
    for (long long r0 = (long long)blockIdx.y * TR; r0 < a.rows; r0 += (long long)gridDim.y * TR) {
        uint32_t v[kPasses];
        if (kGather) {
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, il = flat / TR, w = flat % TR;
                const long long inst = i0 + il, r = r0 + w;
                v[k] = (inst < a.n && r < a.rows) ? in[inst * a.stride + a.first + r] : 0u;
            }
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, il = flat / TR, w = flat % TR;
                tile[il * (TR + 1) + w] = v[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, rl = flat / TI, c = flat % TI;
                const long long inst = i0 + c, r = r0 + rl;
                if (inst < a.n && r < a.rows) wide[r * a.n + inst] = tile[c * (TR + 1) + rl];
            }
        } else {
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, rl = flat / TI, c = flat % TI;
                const long long inst = i0 + c, r = r0 + rl;
                v[k] = (inst < a.n && r < a.rows) ? wide[r * a.n + inst] : 0u;
            }
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, rl = flat / TI, c = flat % TI;
                tile[c * (TR + 1) + rl] = v[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, il = flat / TR, w = flat % TR;
                const long long inst = i0 + il, r = r0 + w;
                if (inst < a.n && r < a.rows) out[inst * a.stride + a.first + r] = tile[il * (TR + 1) + w];
            }
        }
        __syncthreads();   // (the tile is refilled by the next turn of the loop)
    }
}

template <int TI, int TR>
__global__ __launch_bounds__(kLanes) void fx_imajor_gather(ImajorArgs a) { transposeTiles<TI, TR, true>(a); }
template <int TI, int TR>
__global__ __launch_bounds__(kLanes) void fx_imajor_scatter(ImajorArgs a) { transposeTiles<TI, TR, false>(a); }

// (n - 1) * stride + first + rows words must be addressable as a 64-bit byte offset
inline bool badArgs(const ImajorArgs& a) {
    if (!a.wide || a.n < 1 || a.rows < 1 || a.rows >= ((long long)1 << 31) || a.first < 0 || a.first >= ((long long)1 << 31)) return true;
    if (a.stride < a.first + a.rows || a.n >= ((long long)1 << 31)) return true;
    return a.stride > (((long long)1 << 60) / a.n);
}

template <bool kGather>
hipError_t launch(const ImajorArgs& a, hipStream_t stream) {
    const bool narrow = a.rows <= kNarrowRows;
    const long long ti = narrow ? 128 : 64, tr = narrow ? 32 : 64;
    const long long across = (a.n + ti - 1) / ti, down = (a.rows + tr - 1) / tr;
    const dim3 grid((unsigned)across, (unsigned)(down < 65535 ? down : 65535));
    (void)hipGetLastError();
    if (kGather) {
        if (narrow) hipLaunchKernelGGL((fx_imajor_gather<128, 32>), grid, dim3(kLanes), 0, stream, a);
        else hipLaunchKernelGGL((fx_imajor_gather<64, 64>), grid, dim3(kLanes), 0, stream, a);
    } else {
        if (narrow) hipLaunchKernelGGL((fx_imajor_scatter<128, 32>), grid, dim3(kLanes), 0, stream, a);
        else hipLaunchKernelGGL((fx_imajor_scatter<64, 64>), grid, dim3(kLanes), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launchImajorGather(const ImajorArgs& a, hipStream_t stream) {
    if (badArgs(a) || !a.in) return hipErrorInvalidValue;
    return launch<true>(a, stream);
}

hipError_t launchImajorScatter(const ImajorArgs& a, hipStream_t stream) {
    if (badArgs(a) || !a.out) return hipErrorInvalidValue;
    return launch<false>(a, stream);
}

}  // namespace fx
