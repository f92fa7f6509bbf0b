// fx_tram.hip — the kernels behind the delay-line windows by list (fx_tram.hpp): a scatter of packed windows into one delay line
// of the batch at a list of instances, and the gather back - the transposition of fx_instances.hip restricted to one line and a
// word range, with a ring origin per entry.  gfx950, wave64, workgroups of 256 lanes.
//
// A workgroup moves a tile of 64 list entries x 64 window words through LDS, held as [64][64 + 1] dwords (conflict-free in both
// directions by the bank rule of fx_instances.hip).  On the batch side lanes run along the list entries: a wavefront access is
// one window word of 64 listed instances - 256 contiguous bytes where the list names neighbours of one wavefront tile that stand
// at one position, one segment per lane where it does not.  On the packed side lanes run along the words of one window: 256
// contiguous bytes of `values`.  Sixteen loads per lane are in flight before the barrier.
//
// Logical mode: a lane loads its entry's position word ONCE per workgroup and reduces the ring origin once - the only modulo -
// to the slot of window word 0: (p - 1 - first) mod Z, or (p + 1 + first) mod Z under the DANE addressing.  Window word j is then
// origin - j (origin + j), corrected by Z with one compare: j < nWords <= Z and 0 <= origin < Z keep it within one turn.  A
// position word outside 0 .. Z - 1 - a valid handle never holds one - makes the lane skip its entry: no slot outside the line is
// ever addressed.
//
// The contract of fx_instances.hip: every access is one dword moved as a bit pattern, every offset is 64-bit (wave * slots * cols
// * 4 passes 2^32 for config5 at 262 144 instances), lanes beyond `count` or beyond nWords touch no memory, an entry outside
// [0, n) - the runtime refuses such lists before it launches - is skipped rather than followed.  No atomics: the words of a
// scatter's destinations are disjoint.
#include <hip/hip_runtime.h>

#include "fx_tram.hpp"

namespace fx {

namespace {

constexpr int kLanes = 256;
constexpr int kTI = 64;                          // list entries of a tile
constexpr int kTW = 64;                          // window words of a tile
constexpr int kPasses = kTI * kTW / kLanes;      // loads in flight per lane
constexpr int kRowsPerPass = kLanes / kTI;       // batch side: words of one entry column covered by a pass

// grid.x = tiles of kTI list entries, grid.y strides over the tiles of kTW window words
template <bool kGather>
__device__ __forceinline__ void moveWindows(const TramListArgs& a) {
    __shared__ uint32_t tile[kTI * (kTW + 1)];
    __shared__ int live[kTI];   // gather: whether the tile's entry is followed (a skipped entry's window stays as it is)
    const unsigned t = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * kTI;
    // batch side: this lane's list entry and the slot of its window word 0, for every pass and every word tile
    const unsigned c = t % kTI, q = t / kTI;
    long long inst = -1;
    if (e0 + c < a.count) inst = a.list[e0 + c];
    bool listed = inst >= 0 && inst < a.n;
    int origin = a.first;
    if (listed && a.ringSize > 0) {
        const uint32_t p = a.state[(long long)a.posRow * a.nPad + inst];
        if (p >= (uint32_t)a.ringSize) listed = false;
        else {
            const int at = a.dane ? (int)p + 1 + a.first : (int)p - 1 - a.first;   // (p, first < Z <= 2^30: no overflow)
            const int m = at % a.ringSize;
            origin = m < 0 ? m + a.ringSize : m;
        }
    }
    const int step = (a.ringSize > 0 && !a.dane) ? -1 : 1;
    const long long wave = listed ? inst / a.cols : 0, col = listed ? inst % a.cols : 0;
    uint32_t* const column = a.line + wave * a.slots * a.cols + col;   // slot 0 of the lane's instance
    if (kGather) {
        if (q == 0) live[c] = listed ? 1 : 0;
        __syncthreads();
    }
    for (long long w0 = (long long)blockIdx.y * kTW; w0 < a.nWords; w0 += (long long)gridDim.y * kTW) {
        uint32_t v[kPasses];
        int slot[kPasses];   // -1: this lane has no word in this pass
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const long long j = w0 + k * kRowsPerPass + q;
            int s = -1;
            if (listed && j < a.nWords) {
                s = origin + step * (int)j;
                if (a.ringSize > 0) {
                    if (s < 0) s += a.ringSize;
                    else if (s >= a.ringSize) s -= a.ringSize;
                }
                if (s >= a.slots) s = -1;   // (cannot be: the launch refuses first + nWords > slots and ringSize > slots)
            }
            slot[k] = s;
        }
        if (kGather) {
#pragma unroll
            for (int k = 0; k < kPasses; ++k) v[k] = slot[k] >= 0 ? column[(long long)slot[k] * a.cols] : 0u;
#pragma unroll
            for (int k = 0; k < kPasses; ++k) tile[c * (kTW + 1) + k * kRowsPerPass + q] = v[k];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
                const long long e = e0 + el, j = w0 + wl;
                if (e < a.count && j < a.nWords && live[el]) a.values[e * a.valueStride + j] = tile[el * (kTW + 1) + wl];
            }
        } else {
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
                const long long e = e0 + el, j = w0 + wl;
                v[k] = (e < a.count && j < a.nWords) ? a.values[e * a.valueStride + j] : 0u;
            }
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
                tile[el * (kTW + 1) + wl] = v[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kPasses; ++k)
                if (slot[k] >= 0) column[(long long)slot[k] * a.cols] = tile[c * (kTW + 1) + k * kRowsPerPass + q];
        }
        __syncthreads();   // (the tile is refilled by the next turn of the loop)
    }
}

__global__ __launch_bounds__(kLanes) void fx_tram_gather(TramListArgs a) { moveWindows<true>(a); }
__global__ __launch_bounds__(kLanes) void fx_tram_scatter(TramListArgs a) { moveWindows<false>(a); }

inline bool badArgs(const TramListArgs& a, bool gather) {
    if (!a.line || !a.list || !a.values || a.count < 1 || a.count >= ((long long)1 << 31) || a.n < 1 || a.nPad < a.n) return true;
    if (a.slots < 1 || (a.cols != 64 && a.cols != 128 && a.cols != 256)) return true;
    if (a.first < 0 || a.nWords < 1) return true;
    if (a.ringSize == 0) {
        if ((long long)a.first + a.nWords > a.slots) return true;
    } else {
        if (a.ringSize < 1 || a.ringSize > a.slots || a.ringSize > (1 << 30) || !a.state || a.posRow < 0) return true;
        if (a.first >= a.ringSize || a.nWords > a.ringSize) return true;
    }
    if (a.valueStride == 0 ? gather : a.valueStride < a.nWords) return true;
    return a.valueStride > (((long long)1 << 60) / a.count);
}

template <bool kGather>
hipError_t launch(const TramListArgs& a, hipStream_t stream) {
    if (badArgs(a, kGather)) return hipErrorInvalidValue;
    const long long across = (a.count + kTI - 1) / kTI, down = ((long long)a.nWords + kTW - 1) / kTW;
    const dim3 grid((unsigned)across, (unsigned)(down < 65535 ? down : 65535));
    (void)hipGetLastError();
    if (kGather) hipLaunchKernelGGL(fx_tram_gather, grid, dim3(kLanes), 0, stream, a);
    else hipLaunchKernelGGL(fx_tram_scatter, grid, dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launchTramScatter(const TramListArgs& a, hipStream_t stream) { return launch<false>(a, stream); }
hipError_t launchTramGather(const TramListArgs& a, hipStream_t stream) { return launch<true>(a, stream); }

}  // namespace fx
