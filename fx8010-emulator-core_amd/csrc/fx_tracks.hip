// fx_tracks.hip — the kernels that expand list schedules into the event rows of per-instance tracks (fx_tracks.hpp).  gfx950,
// wave64.
//
// fx_track_hold is a pure stream: one read of a state row and E writes per word, E the events of the register in this block.
// 16 bytes per lane, 256-thread workgroups, a capped grid with a grid-stride loop along the row; the second grid dimension is the
// register, whose (state row, first event row, rows) triple is a wave-uniform read of the kernel arguments.  nPad is a multiple
// of 256 and both blocks come from hipMalloc (the rows behind a header rounded to 16 bytes), so every row is 16-byte aligned:
// the launch helper checks it.
//
// fx_track_scatter has its lanes along the entries of ONE schedule, as fx_reg_scatter has (one wavefront per workgroup: a
// thousand entries wait side by side on sixteen CUs).  A lane loads its instance once and walks the ranges - one per step that
// falls inside the block and key, computed on the host: the value row to read and the event rows it runs over.  One launch per
// schedule: the schedules of a block differ in their entry counts, so a second grid dimension would be sized by the longest list
// and need a table of descriptors in device memory; per launch the descriptor is the kernel's arguments.
//
// The contract of fx_instances.hip / fx_registers.hip: every word moves as a bit pattern, every offset is 64-bit, lanes beyond
// `count` touch no memory, an entry outside [0, n) or a row outside the buffer - the runtime refuses both before it launches -
// is skipped rather than followed.  No atomics: the words are disjoint.
#include <hip/hip_runtime.h>

#include "fx_tracks.hpp"

namespace fx {

namespace {

constexpr int kHoldThreads = 256;
constexpr long long kHoldGrid = 2048;   // workgroups along a row: 256 CUs x 8
constexpr int kLanes = 64;              // scatter: one wavefront per workgroup
constexpr long long kMaxGrid = 0x7fffffffLL;

__global__ __launch_bounds__(kHoldThreads) void fx_track_hold(TrackHoldArgs a) {
    const int t = (int)blockIdx.y;
    const long long srow = a.stateRow[t], first = a.firstRow[t], rows = a.rowCount[t];
    if (srow < 0 || srow >= a.stateRows || first < 0 || rows < 1 || first + rows > a.totalRows) return;
    const long long quads = a.nPad / 4;
    const uint4* src = reinterpret_cast<const uint4*>(a.state + srow * a.nPad);
    uint4* dst = reinterpret_cast<uint4*>(a.rows + first * a.nPad);
    for (long long i = (long long)blockIdx.x * kHoldThreads + threadIdx.x; i < quads; i += (long long)gridDim.x * kHoldThreads) {
        const uint4 v = src[i];
        for (long long e = 0; e < rows; ++e) dst[e * quads + i] = v;
    }
}

__global__ __launch_bounds__(kLanes) void fx_track_scatter(TrackScatterArgs a) {
    for (long long e = (long long)blockIdx.x * kLanes + threadIdx.x; e < a.count; e += (long long)gridDim.x * kLanes) {
        const long long inst = a.list[e];
        if (inst < 0 || inst >= a.n) continue;
        for (int j = 0; j < a.nRanges; ++j) {
            const TrackRange r = a.ranges[j];
            if (r.valueRow < 0 || r.valueRow >= a.valueRows || r.rowLo < 0 || r.rowHi > a.totalRows || r.rowLo >= r.rowHi) continue;
            const uint32_t v = a.values[(long long)r.valueRow * a.count + e];
            for (long long row = r.rowLo; row < r.rowHi; ++row) a.rows[row * a.nPad + inst] = v;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t launchTrackHold(const TrackHoldArgs& a, hipStream_t stream) {
    if (!a.state || !a.rows || !aligned16(a.state) || !aligned16(a.rows)) return hipErrorInvalidValue;
    if (a.nPad < 256 || a.nPad % 256 != 0 || a.totalRows < 1 || a.stateRows < 1 || a.nRegs < 1 || a.nRegs > kMaxTrackHolds) return hipErrorInvalidValue;
    const long long across = (a.nPad / 4 + kHoldThreads - 1) / kHoldThreads;
    const dim3 grid((unsigned)(across < kHoldGrid ? across : kHoldGrid), (unsigned)a.nRegs);
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_track_hold, grid, dim3(kHoldThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchTrackScatter(const TrackScatterArgs& a, hipStream_t stream) {
    if (!a.rows || !a.list || !a.values || !a.ranges) return hipErrorInvalidValue;
    if (a.count < 1 || a.count >= ((long long)1 << 31) || a.valueRows < 1 || (long long)a.valueRows * a.count >= ((long long)1 << 31)) return hipErrorInvalidValue;
    if (a.n < 1 || a.nPad < a.n || a.totalRows < 1 || a.nRanges < 1) return hipErrorInvalidValue;
    const long long across = (a.count + kLanes - 1) / kLanes;
    const dim3 grid((unsigned)(across < kMaxGrid ? across : kMaxGrid));
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_track_scatter, grid, dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fx
