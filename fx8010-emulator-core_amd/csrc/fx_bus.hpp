// fx_bus.hpp — launch interface of the two group-bus kernels (device code: fx_bus.hip).
//
// A bus block is a sandwich around the unchanged emulation launch: `expand` writes a per-group input [rows][groups] out to the
// per-instance scratch [rows][n], the emulation runs on the scratch in place, `mix` reduces the scratch to [rows][groups].
// rows = samples * channels; group g holds instances g*K .. min((g+1)*K, n) - 1.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fx {

struct BusArgs {
    const float* narrowIn;   // expand: [rows][narrowPitch] group words (device memory or device-visible host memory)
    float* narrowOut;        // mix: the same layout, written
    float* wide;             // [rows][n] per-instance scratch, rows packed (device memory)
    long long rows;          // samples * channels
    long long n;             // instances
    long long group;         // K, 1 <= K <= n (the caller clamps a larger K: one group either way)
    long long groups;        // G = ceil(n / K)
    long long narrowPitch;   // floats per row of the narrow side (>= groups)
};

// wide[r][i] = narrowIn[r][i / K]: a wavefront loads 64 consecutive group words of a row once and writes their copies
hipError_t launchBusExpand(const BusArgs& a, hipStream_t stream);

// narrowOut[r][g] = sum of wide[r][g*K ...] in the order of the 64-lane shuffle-down tree: p[l] (l = 0..63, +0.0f) takes the
// group's members m = j*64 + l for j ascending, then p[l] += p[l + step] for step = 32 .. 1 (l < step); the result is p[0].
// fp32, round to nearest, never fused, denormals kept.
hipError_t launchBusMix(const BusArgs& a, hipStream_t stream);

}  // namespace fx
