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

// Target meters (include/fx8010_amd.h "Target meters"): two further fp64 accumulators per (channel, instance) against a reference
// signal held on the device.  The match rows are a block of their own - per channel err f64 [nPad], then cross f64 [nPad], all
// +0.0 after a reset - so that a handle without a target carries nothing of them.
constexpr size_t kMatchBytesPerColumn = 16;
constexpr size_t matchChannelBytes(long long nPad) { return kMatchBytesPerColumn * (size_t)nPad; }
constexpr size_t matchErrOff(long long) { return 0; }
constexpr size_t matchCrossOff(long long nPad) { return 8 * (size_t)nPad; }

struct MeterTargetArgs {
    MeterArgs m;             // the block and the four accumulators, as for launchMeter
    void* match;             // [channels] x the match rows above (device memory)
    const float* target;     // [tSamples][channels][tCols] (device memory): the target columns this batch's instances use
    long long tSamples;      // >= 1
    long long tCols;         // columns of a target row; channels * tCols * 4 < 2^32
    long long group;         // >= 1: instance i is compared with column (firstGlobal + i) / group - firstColumn
    long long firstGlobal;   // the global number of column 0 of y
    long long firstColumn;   // firstGlobal / group
    long long pos;           // target position of sample 0 of the block, >= 0; with loop below tSamples
    int loop;                // 0: samples at positions >= tSamples change the four only; 1: the position wraps
};

// fx_meter with the two match accumulators beside the four: launched INSTEAD of launchMeter while a target is set, so that the
// block is read once.  The four are taken by the same code (meterTake), for every sample.
hipError_t launchMeterTarget(const MeterTargetArgs& a, hipStream_t stream);

// Level meters (include/fx8010_amd.h "Level meters"): two further accumulators per (channel, instance) that fall as well as rise.
// For every output word, with fin and w as above: d = level * release (ONE fp32 multiply, denormals kept), level = max(w, d) - both
// non-negative and finite, so the larger bit pattern - loud = !fin || w >= floor, quiet = loud ? 0 : quiet + 1, saturating at
// 0xFFFFFFFF.  The level rows are a block of their own - per channel level f32 [nPad], then quiet u32 [nPad], all zero after a
// reset - so that a handle without level meters carries nothing of them.  release and floor travel by value in every launch.
constexpr size_t kLevelBytesPerColumn = 8;
constexpr size_t levelChannelBytes(long long nPad) { return kLevelBytesPerColumn * (size_t)nPad; }
constexpr size_t levelLevelOff(long long) { return 0; }
constexpr size_t levelQuietOff(long long nPad) { return 4 * (size_t)nPad; }

struct LevelParams {
    void* rows;       // [channels] x the level rows above (device memory)
    float release;    // finite, +0.0f <= release <= 1 (never -0.0f: the product must keep a clear sign bit)
    float floor;      // finite, +0.0f <= floor
};
struct MeterLevelArgs {
    MeterArgs m;      // the block and the four accumulators, as for launchMeter
    LevelParams l;
};
struct MeterTargetLevelArgs {
    MeterTargetArgs t;   // the block, the four and the two match accumulators, as for launchMeterTarget
    LevelParams l;
};

// fx_meter_level / fx_meter_target_level: launched INSTEAD of fx_meter / fx_meter_target while level meters are on.  The four
// (and the two of a target) are taken by the same code, for every sample; the two level accumulators by levelTake.
hipError_t launchMeterLevel(const MeterLevelArgs& a, hipStream_t stream);
hipError_t launchMeterTargetLevel(const MeterTargetLevelArgs& a, hipStream_t stream);

}  // namespace fx
