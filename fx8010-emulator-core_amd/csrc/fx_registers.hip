// fx_registers.hip — the kernels behind the register calls by list (fx_registers.hpp): a scatter of packed [key][entry] words
// into the register rows of the state block at a list of instances, and the gather back.  gfx950, wave64.
//
// Lanes run along the list entries.  A lane loads its entry once and walks the keys, kInFlight of them at a time: that many
// loads are issued before the first store waits for one.  On the packed side a wavefront touches 256 contiguous bytes of `values`
// per key; on the batch side one dword per lane - 256 contiguous bytes where the list names neighbours, one segment per lane
// where it does not (a scattered list costs that on any layout).  The row numbers are wave-uniform reads of a small table.
//
// At the sizes the calls are made for (a thousand entries, a handful of keys) this is a launch, not a transfer: a workgroup is
// ONE wavefront, so that a thousand entries are sixteen workgroups on sixteen CUs and the one-segment-per-lane accesses of a
// scattered list wait side by side, not behind each other in one CU's queue.  No LDS, no barrier.
//
// The contract of fx_instances.hip: every word moves as a bit pattern, every offset is 64-bit (row * nPad passes 2^31 words for
// a wide program at half a million instances), lanes beyond `count` touch no memory, an entry outside [0, n) or a row outside
// [0, stateRows) - the runtime refuses both before it launches - is skipped rather than followed.  No atomics: the words of a
// scatter are disjoint.
#include <hip/hip_runtime.h>

#include "fx_registers.hpp"

namespace fx {

namespace {

constexpr int kLanes = 64;       // one wavefront per workgroup
constexpr int kInFlight = 4;     // keys whose words a lane has in flight
constexpr long long kMaxGrid = 0x7fffffffLL;

template <bool kGather>
__device__ __forceinline__ void moveWords(const RegListArgs& a) {
    for (long long e = (long long)blockIdx.x * kLanes + threadIdx.x; e < a.count; e += (long long)gridDim.x * kLanes) {
        const long long inst = a.list[e];
        if (inst < 0 || inst >= a.n) continue;
        for (int k0 = 0; k0 < a.nKeys; k0 += kInFlight) {
            uint32_t v[kInFlight];
            long long row[kInFlight];
            bool live[kInFlight];
#pragma unroll
            for (int j = 0; j < kInFlight; ++j) {
                const int k = k0 + j;
                row[j] = k < a.nKeys ? (long long)a.rows[k] : -1;
                live[j] = row[j] >= 0 && row[j] < a.stateRows;
                if (live[j]) v[j] = kGather ? a.state[row[j] * a.nPad + inst] : a.values[(long long)k * a.count + e];
            }
#pragma unroll
            for (int j = 0; j < kInFlight; ++j) {
                if (!live[j]) continue;
                if (kGather) a.values[(long long)(k0 + j) * a.count + e] = v[j];
                else a.state[row[j] * a.nPad + inst] = v[j];
            }
        }
    }
}

__global__ __launch_bounds__(kLanes) void fx_reg_scatter(RegListArgs a) { moveWords<false>(a); }
__global__ __launch_bounds__(kLanes) void fx_reg_gather(RegListArgs a) { moveWords<true>(a); }

inline bool badArgs(const RegListArgs& a) {
    if (!a.state || !a.list || !a.rows || !a.values) return true;
    if (a.count < 1 || a.count >= ((long long)1 << 31) || a.nKeys < 1 || (long long)a.nKeys * a.count >= ((long long)1 << 31)) return true;
    return a.n < 1 || a.nPad < a.n || a.stateRows < 1;
}

template <bool kGather>
hipError_t launch(const RegListArgs& a, hipStream_t stream) {
    if (badArgs(a)) return hipErrorInvalidValue;
    const long long across = (a.count + kLanes - 1) / kLanes;
    const dim3 grid((unsigned)(across < kMaxGrid ? across : kMaxGrid));
    (void)hipGetLastError();
    if (kGather) hipLaunchKernelGGL(fx_reg_gather, grid, dim3(kLanes), 0, stream, a);
    else hipLaunchKernelGGL(fx_reg_scatter, grid, dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launchRegScatter(const RegListArgs& a, hipStream_t stream) { return launch<false>(a, stream); }
hipError_t launchRegGather(const RegListArgs& a, hipStream_t stream) { return launch<true>(a, stream); }

}  // namespace fx
