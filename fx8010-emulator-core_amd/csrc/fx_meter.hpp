// fx_meter.hpp — launch interface of the output-meter kernel (device code: fx_meter.hip).
//
// A meter launch follows an emulation launch on the same stream and reads the per-instance output block that launch wrote,
// [samples][channels][pitch] f32, columns 0..n-1.  Per (channel, instance) it carries four accumulators in device memory across
// launches (include/fx8010_amd.h "Output meters" fixes the arithmetic word for word): for every output word y of the column, in
// sample order, fin = |y| < +Inf, w = fin ? |y| : +0.0f; energy = energy + (double)w * (double)w (fp64, one rounding per sample:
// the product of two fp32 values is exact), peak = max(peak, w), full_scale += fin && |y| >= 1.0f, nonfinite += !fin, the two
// counters saturating at 0xFFFFFFFF.  One lane owns one column: no atomics, no cross-lane sums, so blocks of 16 + 17 samples leave
// the bits one block of 33 leaves.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace fx {

// The accumulator rows, instance-fastest like every other buffer of a batch: per channel energy f64 [nPad], then peak f32 [nPad],
// full_scale u32 [nPad], nonfinite u32 [nPad] - kMeterBytesPerColumn * nPad bytes per channel, all zero after a reset (+0.0, +0.0f,
// 0, 0).  A wavefront touches 512 contiguous bytes of the energy row and 256 of each of the others.
constexpr size_t kMeterBytesPerColumn = 20;
constexpr size_t meterChannelBytes(long long nPad) { return kMeterBytesPerColumn * (size_t)nPad; }
constexpr size_t meterEnergyOff(long long) { return 0; }
constexpr size_t meterPeakOff(long long nPad) { return 8 * (size_t)nPad; }
constexpr size_t meterFullScaleOff(long long nPad) { return 12 * (size_t)nPad; }
constexpr size_t meterNonfiniteOff(long long nPad) { return 16 * (size_t)nPad; }

struct MeterArgs {
    const float* y;      // [samples][channels][pitch] output words (device memory or device-visible host memory)
    void* rows;          // [channels] x the accumulator rows above (device memory)
    long long n;         // instances: columns 0..n-1 of y
    long long nPad;      // columns of an accumulator row (>= n)
    long long pitch;     // floats per row of y (>= n); channels * pitch * 4 < 2^32
    int samples;         // >= 1
    int channels;        // 1..4
};

// reads the accumulators once, walks the samples of every column in order, writes them back once
hipError_t launchMeter(const MeterArgs& a, hipStream_t stream);

}  // namespace fx
