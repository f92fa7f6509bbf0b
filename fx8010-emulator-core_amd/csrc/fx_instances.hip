// fx_instances.hip — the kernels behind the per-instance state calls (fx_instances.hpp): a gather / scatter transposition
// between the three transposed state blocks and packed per-instance records, by an index list, and the scatter that rotates the
// delay lines of each record on its way (fx_inst_scatter_rot, below the two).  gfx950, wave64, workgroups of 256 lanes.
//
// A workgroup moves a tile of 64 list entries x 64 record words through LDS, held as [64][64 + 1] dwords - the shape and the odd
// pitch of fx_imajor.hip, conflict-free in both directions by the same bank rule (bank = dword address mod 32: along a record 32
// lanes hold consecutive dwords, across the entries lane l holds l * 65 + w = l + w (mod 32)).  On the batch side lanes run along
// the list entries: a wavefront access is one word of 64 listed instances, 256 contiguous bytes where the list names neighbours
// of one wavefront tile and one segment per lane where it does not (a scattered list costs that on any layout).  On the packed
// side lanes run along the words: 256 contiguous bytes of one record.  Sixteen loads per lane are in flight before the barrier.
// A lane's list entry does not depend on the pass (256 is a multiple of 64): it is loaded once per workgroup.
//
// Every access is one dword moved as a bit pattern, every offset is 64-bit (wave * slots * cols * 4 passes 2^32 for config5 at
// 262 144 instances).  Lanes beyond `count` or beyond the W words touch no memory; an entry outside [0, n) - the runtime refuses
// such lists before it launches - is skipped rather than followed.  No atomics: the words of a call's destinations are disjoint.
#include <hip/hip_runtime.h>

#include "fx_instances.hpp"

namespace fx {

namespace {

constexpr int kLanes = 256;
constexpr int kTI = 64;                          // list entries of a tile
constexpr int kTW = 64;                          // record words of a tile
constexpr int kPasses = kTI * kTW / kLanes;      // loads in flight per lane
constexpr int kRowsPerPass = kLanes / kTI;       // batch side: words of one entry column covered by a pass

// where word w of the lane's instance lives: stateAt = inst, iAt / xAt = its column in slot 0 of its wavefront tile
__device__ __forceinline__ uint32_t* wordOf(const InstArgs& a, long long w, long long stateAt, long long iAt, long long xAt) {
    if (w < a.stateRows) return a.state + w * a.nPad + stateAt;
    w -= a.stateRows;
    if (w < a.iSlots) return a.itram + iAt + w * a.cols;
    return a.xtram + xAt + (w - a.iSlots) * a.cols;
}

// grid.x = tiles of kTI list entries, grid.y strides over the tiles of kTW record words
template <bool kGather>
__device__ __forceinline__ void moveTiles(const InstArgs& a) {
    __shared__ uint32_t tile[kTI * (kTW + 1)];
    const unsigned t = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * kTI;
    const long long W = (long long)a.stateRows + a.iSlots + a.xSlots;
    // batch side: this lane's list entry, for every pass and every word tile
    const unsigned c = t % kTI, q = t / kTI;
    long long inst = -1;
    if (e0 + c < a.count) inst = a.list[e0 + c];
    const bool listed = inst >= 0 && inst < a.n;
    const long long wave = listed ? inst / a.cols : 0, col = listed ? inst % a.cols : 0;
    const long long iAt = wave * a.iSlots * a.cols + col, xAt = wave * a.xSlots * a.cols + col;
    for (long long w0 = (long long)blockIdx.y * kTW; w0 < W; w0 += (long long)gridDim.y * kTW) {
        uint32_t v[kPasses];
        if (kGather) {
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const long long w = w0 + k * kRowsPerPass + q;
                v[k] = (listed && w < W) ? *wordOf(a, w, inst, iAt, xAt) : 0u;
            }
#pragma unroll
            for (int k = 0; k < kPasses; ++k) tile[c * (kTW + 1) + k * kRowsPerPass + q] = v[k];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
                const long long e = e0 + el, w = w0 + wl;
                if (e < a.count && w < W) a.records[e * a.recStride + w] = tile[el * (kTW + 1) + wl];
            }
        } else {
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
                const long long e = e0 + el, w = w0 + wl;
                v[k] = (e < a.count && w < W) ? a.records[e * a.recStride + w] : 0u;
            }
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
                tile[el * (kTW + 1) + wl] = v[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const long long w = w0 + k * kRowsPerPass + q;
                if (listed && w < W && !(w >= a.skipLo && w < a.skipHi)) *wordOf(a, w, inst, iAt, xAt) = tile[c * (kTW + 1) + k * kRowsPerPass + q];
            }
        }
        __syncthreads();   // (the tile is refilled by the next turn of the loop)
    }
}

__global__ __launch_bounds__(kLanes) void fx_inst_gather(InstArgs a) { moveTiles<true>(a); }
__global__ __launch_bounds__(kLanes) void fx_inst_scatter(InstArgs a) { moveTiles<false>(a); }

// The scatter with the delay lines rotated per record (fxb_load_instances_rotated).  The rotation is applied on the packed side,
// where a wavefront reads 64 consecutive words of ONE record (its entry is wave-uniform): destination word j of a ring of Z slots
// reads record word base + (j - d < 0 ? j - d + Z : j - d), so the 256 contiguous bytes become at most two contiguous segments, at
// one word tile per record and line.  The batch side is the scatter's, access for access.  The pairs of the tile's 64 entries are
// loaded once per workgroup, into LDS.
__global__ __launch_bounds__(kLanes) void fx_inst_scatter_rot(InstRotArgs r) {
    __shared__ uint32_t tile[kTI * (kTW + 1)];
    __shared__ int rotOf[kTI * 2];
    const InstArgs& a = r.base;
    const unsigned t = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * kTI;
    const long long iBase = a.stateRows, xBase = iBase + a.iSlots, W = xBase + a.xSlots;
    if (t < 2 * kTI) {
        const long long e = e0 + t / 2;
        const int size = (t & 1) ? r.xSize : r.iSize;
        const int d = e < a.count ? r.rot[e * 2 + (t & 1)] : 0;
        rotOf[t] = (d > 0 && d < size) ? d : 0;
    }
    const unsigned c = t % kTI, q = t / kTI;
    long long inst = -1;
    if (e0 + c < a.count) inst = a.list[e0 + c];
    const bool listed = inst >= 0 && inst < a.n;
    const long long wave = listed ? inst / a.cols : 0, col = listed ? inst % a.cols : 0;
    const long long iAt = wave * a.iSlots * a.cols + col, xAt = wave * a.xSlots * a.cols + col;
    __syncthreads();
    for (long long w0 = (long long)blockIdx.y * kTW; w0 < W; w0 += (long long)gridDim.y * kTW) {
        uint32_t v[kPasses];
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
            const long long e = e0 + el, w = w0 + wl;
            long long from = w;
            if (w >= iBase) {
                const int line = w >= xBase ? 1 : 0;
                const long long base = line ? xBase : iBase, size = line ? r.xSize : r.iSize, j = w - base;
                if (j < size) {
                    const long long back = j - rotOf[el * 2 + line];
                    from = base + (back < 0 ? back + size : back);
                }
            }
            v[k] = (e < a.count && w < W) ? a.records[e * a.recStride + from] : 0u;
        }
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
            tile[el * (kTW + 1) + wl] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const long long w = w0 + k * kRowsPerPass + q;
            if (listed && w < W && !(w >= a.skipLo && w < a.skipHi)) *wordOf(a, w, inst, iAt, xAt) = tile[c * (kTW + 1) + k * kRowsPerPass + q];
        }
        __syncthreads();   // (the tile is refilled by the next turn of the loop)
    }
}

inline bool badArgs(const InstArgs& a, bool gather) {
    if (!a.state || !a.list || !a.records || a.count < 1 || a.count >= ((long long)1 << 31) || a.n < 1 || a.nPad < a.n) return true;
    if (a.stateRows < 1 || a.iSlots < 0 || a.xSlots < 0 || (a.iSlots > 0 && !a.itram) || (a.xSlots > 0 && !a.xtram)) return true;
    if (a.cols != 64 && a.cols != 128 && a.cols != 256) return true;
    const long long W = instanceWords(a);
    if (a.recStride == 0 ? gather : a.recStride < W) return true;
    if (a.recStride > (((long long)1 << 60) / a.count)) return true;
    return gather ? false : (a.skipLo < 0 || a.skipHi < a.skipLo || a.skipHi > a.stateRows);
}

template <bool kGather>
hipError_t launch(const InstArgs& a, hipStream_t stream) {
    const long long across = (a.count + kTI - 1) / kTI, down = (instanceWords(a) + kTW - 1) / kTW;
    const dim3 grid((unsigned)across, (unsigned)(down < 65535 ? down : 65535));
    (void)hipGetLastError();
    if (kGather) hipLaunchKernelGGL(fx_inst_gather, grid, dim3(kLanes), 0, stream, a);
    else hipLaunchKernelGGL(fx_inst_scatter, grid, dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launchInstGather(const InstArgs& a, hipStream_t stream) {
    if (badArgs(a, true)) return hipErrorInvalidValue;
    return launch<true>(a, stream);
}

hipError_t launchInstScatter(const InstArgs& a, hipStream_t stream) {
    if (badArgs(a, false)) return hipErrorInvalidValue;
    return launch<false>(a, stream);
}

hipError_t launchInstScatterRot(const InstRotArgs& r, hipStream_t stream) {
    const InstArgs& a = r.base;
    if (badArgs(a, false) || a.recStride == 0 || !r.rot || r.iSize < 0 || r.iSize > a.iSlots || r.xSize < 0 || r.xSize > a.xSlots) return hipErrorInvalidValue;
    const long long across = (a.count + kTI - 1) / kTI, down = (instanceWords(a) + kTW - 1) / kTW;
    const dim3 grid((unsigned)across, (unsigned)(down < 65535 ? down : 65535));
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_inst_scatter_rot, grid, dim3(kLanes), 0, stream, r);
    return hipGetLastError();
}

}  // namespace fx
