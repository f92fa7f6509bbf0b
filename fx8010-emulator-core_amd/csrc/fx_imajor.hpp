// fx_imajor.hpp — launch interface of the two kernels around the emulation launch of an instance-major block (device code:
// fx_imajor.hip).
//
// The caller holds one interleaved [sample][channel] stream per instance: instance i's block is the run of R = samples * channels
// words at stream + i * stride.  The emulation takes [sample][channel][instance].  With a stream as one run of R words both
// directions are a plain 2-D transposition between the streams and the per-instance scratch [rows][n] of a bus block:
// `gather` fills the scratch, the emulation runs on it in place, `scatter` empties it.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fx {

struct ImajorArgs {
    const float* in;    // gather: the streams (device memory or device-visible host memory), 4-byte aligned, no more
    float* out;         // scatter: the same layout, written
    float* wide;        // [rows][n] per-instance scratch, rows packed (device memory)
    long long stride;   // floats from one instance's stream to the next (>= first + rows)
    long long first;    // the first word of every stream's run that this launch moves (a piece of a block: lo * channels)
    long long rows;     // words of every run that this launch moves: samples * channels of the piece, below 2^31
    long long n;        // instances
};

// wide[r][i] = in[i * stride + first + r] for r < rows, i < n.  Words are moved as 32-bit patterns.  Nothing outside the n runs
// is read, nothing outside [rows][n] is written.
hipError_t launchImajorGather(const ImajorArgs& a, hipStream_t stream);

// out[i * stride + first + r] = wide[r][i]: the reverse.  Nothing outside the n runs is written - the words between two runs
// (a stride above the run) keep what they hold.
hipError_t launchImajorScatter(const ImajorArgs& a, hipStream_t stream);

}  // namespace fx
