// fx_meter.hip — the output-meter kernel behind an emulation launch (fx_meter.hpp).  gfx950, wave64, workgroups of 256 lanes:
// grid.x walks the instances in chunks of 256, grid.y the channels.  One lane owns one column of one channel: it reads its four
// accumulators once, streams the column's samples in order - eight independent row loads in flight, 256 contiguous bytes per
// wavefront and load - and writes the accumulators back once.  Everything that decides a bit is integer work on the word's
// pattern (|y| and its compares, the maximum of two non-negative finite floats) except the energy: an fp64 add of an exact
// product, one rounding per sample.
//
// fx_meter_target is the same kernel with two more fp64 accumulators per column against a target held on the device
// (fx_meter.hpp MeterTargetArgs); it is launched in place of fx_meter while a target is set and takes the four through the same
// meterTake.  Resource usage (-O3, gfx950, from -Rpass-analysis=kernel-resource-usage), VGPRs / scratch bytes per lane / LDS bytes
// per workgroup: fx_meter 56 / 0 / 0, eight wavefronts per SIMD; fx_meter_target 68 / 0 / 0, seven.
//
// fx_meter_level and fx_meter_target_level are the two bodies again (one template each, the existing kernels are its `false`
// instance and compile to what they were) with the two level accumulators of fx_meter.hpp "Level meters" beside the others: an
// envelope that falls by one fp32 multiply per sample and a count of consecutive samples below a floor, taken by levelTake.  They
// are launched in place of the two while level meters are on; release and floor come by value in the arguments.  Resource usage
// as above: fx_meter_level 63 / 0 / 0, eight wavefronts per SIMD; fx_meter_target_level 74 / 0 / 0, six.
#include <hip/hip_runtime.h>

#include "fx_meter.hpp"

namespace fx {

namespace {

constexpr int kMeterLoads = 8;   // row loads in flight per lane

struct MeterAcc {
    double energy;
    uint32_t peak;   // the bits of a non-negative finite float: ordered like the values
    uint32_t fullScale, nonfinite;
};

__device__ __forceinline__ void meterTake(MeterAcc& m, uint32_t word) {
    const uint32_t mag = word & 0x7fffffffu;       // |y|
    const bool fin = mag < 0x7f800000u;            // |y| < +Inf: false for NaN and +-Inf
    const uint32_t w = fin ? mag : 0u;
    const double wd = (double)__builtin_bit_cast(float, w);
    m.energy = m.energy + wd * wd;
    m.peak = w > m.peak ? w : m.peak;
    m.fullScale += (uint32_t)(fin && mag >= 0x3f800000u && m.fullScale != 0xffffffffu);
    m.nonfinite += (uint32_t)(!fin && m.nonfinite != 0xffffffffu);
}

// the two level accumulators (fx_meter.hpp "Level meters"): integer work on the word's pattern plus the one fp32 multiply.  level
// and release are non-negative and finite, so the product is too (+0.0f where either is zero) and its pattern orders like its
// value, as w's does: the maximum and the compare with the floor are unsigned compares.  The multiply has nothing to fuse with.
struct LevelAcc {
    uint32_t level;   // the bits of a non-negative finite float
    uint32_t quiet;
};

__device__ __forceinline__ void levelTake(LevelAcc& l, uint32_t word, float release, uint32_t floorBits) {
    const uint32_t mag = word & 0x7fffffffu;
    const bool fin = mag < 0x7f800000u;
    const uint32_t w = fin ? mag : 0u;
    const uint32_t d = __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, l.level) * release);
    l.level = w > d ? w : d;
    const bool loud = !fin || w >= floorBits;
    l.quiet = loud ? 0u : l.quiet + (uint32_t)(l.quiet != 0xffffffffu);
}

// the body of fx_meter (kLevel false: `l` is unused and nothing of it is compiled) and of fx_meter_level
template <bool kLevel>
__device__ __forceinline__ void meterBody(const MeterArgs& a, const LevelParams& l) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const unsigned c = blockIdx.y;
    char* rows = static_cast<char*>(a.rows) + (size_t)c * meterChannelBytes(a.nPad);
    double* energy = reinterpret_cast<double*>(rows + meterEnergyOff(a.nPad)) + i;
    uint32_t* peak = reinterpret_cast<uint32_t*>(rows + meterPeakOff(a.nPad)) + i;
    uint32_t* fullScale = reinterpret_cast<uint32_t*>(rows + meterFullScaleOff(a.nPad)) + i;
    uint32_t* nonfinite = reinterpret_cast<uint32_t*>(rows + meterNonfiniteOff(a.nPad)) + i;
    MeterAcc m{*energy, *peak, *fullScale, *nonfinite};
    uint32_t* levelAt = nullptr;
    uint32_t* quietAt = nullptr;
    LevelAcc lv{0u, 0u};
    uint32_t floorBits = 0u;
    if (kLevel) {
        char* lrows = static_cast<char*>(l.rows) + (size_t)c * levelChannelBytes(a.nPad);
        levelAt = reinterpret_cast<uint32_t*>(lrows + levelLevelOff(a.nPad)) + i;
        quietAt = reinterpret_cast<uint32_t*>(lrows + levelQuietOff(a.nPad)) + i;
        lv = LevelAcc{*levelAt, *quietAt};
        floorBits = __builtin_bit_cast(uint32_t, l.floor);
    }
    // a sample period is channels * pitch * 4 bytes further on: below 2^32 (launchMeter), a 32-bit stride
    const uint32_t stride = (uint32_t)a.channels * (uint32_t)a.pitch * 4u;
    const char* p = reinterpret_cast<const char*>(a.y + (size_t)c * (size_t)a.pitch + (size_t)i);
    int s = 0;
    for (; s + kMeterLoads <= a.samples; s += kMeterLoads) {
        uint32_t v[kMeterLoads];
#pragma unroll
        for (int u = 0; u < kMeterLoads; ++u) {
            v[u] = *reinterpret_cast<const uint32_t*>(p);
            p += stride;
        }
#pragma unroll
        for (int u = 0; u < kMeterLoads; ++u) {
            meterTake(m, v[u]);
            if (kLevel) levelTake(lv, v[u], l.release, floorBits);
        }
    }
    for (; s < a.samples; ++s) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
        meterTake(m, v);
        if (kLevel) levelTake(lv, v, l.release, floorBits);
        p += stride;
    }
    *energy = m.energy;
    *peak = m.peak;
    *fullScale = m.fullScale;
    *nonfinite = m.nonfinite;
    if (kLevel) {
        *levelAt = lv.level;
        *quietAt = lv.quiet;
    }
}

__global__ __launch_bounds__(256) void fx_meter(MeterArgs a) { meterBody<false>(a, LevelParams{}); }
__global__ __launch_bounds__(256) void fx_meter_level(MeterLevelArgs a) { meterBody<true>(a.m, a.l); }

// one sample against the target (include/fx8010_amd.h "Target meters"): d, e, the sum and the product are one rounding each -
// the library is built with -ffp-contract=off, nothing here fuses - and the product of two fp32 values is exact in fp64
__device__ __forceinline__ void matchTake(double& err, double& cross, uint32_t yWord, uint32_t tWord) {
    const bool ok = (yWord & 0x7fffffffu) < 0x7f800000u && (tWord & 0x7fffffffu) < 0x7f800000u;
    const double y = (double)__builtin_bit_cast(float, yWord), t = (double)__builtin_bit_cast(float, tWord);
    const double d = y - t;
    const double e = d * d;
    const double yt = y * t;
    err = ok ? err + e : err;
    cross = ok ? cross + yt : cross;
}

// fx_meter plus the two match accumulators: the same geometry, one lane per column, eight y loads and the eight t loads of the
// round in flight together.  The lane's target column is computed once (a 64-bit divide); the target row advances by one per
// sample with a conditional wrap - no `%` in the loop - and a wrap or the end of the target may fall anywhere inside a round.
// Without `loop`, a sample at or beyond the end loads no target word and takes meterTake alone.  With group >= 64 the t loads of a
// wavefront hit one or two addresses.
template <bool kLevel>
__device__ __forceinline__ void targetBody(const MeterTargetArgs& a, const LevelParams& l) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m.n) return;
    const unsigned c = blockIdx.y;
    char* rows = static_cast<char*>(a.m.rows) + (size_t)c * meterChannelBytes(a.m.nPad);
    double* energy = reinterpret_cast<double*>(rows + meterEnergyOff(a.m.nPad)) + i;
    uint32_t* peak = reinterpret_cast<uint32_t*>(rows + meterPeakOff(a.m.nPad)) + i;
    uint32_t* fullScale = reinterpret_cast<uint32_t*>(rows + meterFullScaleOff(a.m.nPad)) + i;
    uint32_t* nonfinite = reinterpret_cast<uint32_t*>(rows + meterNonfiniteOff(a.m.nPad)) + i;
    char* match = static_cast<char*>(a.match) + (size_t)c * matchChannelBytes(a.m.nPad);
    double* errAt = reinterpret_cast<double*>(match + matchErrOff(a.m.nPad)) + i;
    double* crossAt = reinterpret_cast<double*>(match + matchCrossOff(a.m.nPad)) + i;
    MeterAcc m{*energy, *peak, *fullScale, *nonfinite};
    double err = *errAt, cross = *crossAt;
    uint32_t* levelAt = nullptr;
    uint32_t* quietAt = nullptr;
    LevelAcc lv{0u, 0u};
    uint32_t floorBits = 0u;
    if (kLevel) {
        char* lrows = static_cast<char*>(l.rows) + (size_t)c * levelChannelBytes(a.m.nPad);
        levelAt = reinterpret_cast<uint32_t*>(lrows + levelLevelOff(a.m.nPad)) + i;
        quietAt = reinterpret_cast<uint32_t*>(lrows + levelQuietOff(a.m.nPad)) + i;
        lv = LevelAcc{*levelAt, *quietAt};
        floorBits = __builtin_bit_cast(uint32_t, l.floor);
    }
    const uint32_t stride = (uint32_t)a.m.channels * (uint32_t)a.m.pitch * 4u;
    const char* p = reinterpret_cast<const char*>(a.m.y + (size_t)c * (size_t)a.m.pitch + (size_t)i);
    // the lane's column of the target: below tCols for every i < n (launchMeterTarget)
    const long long col = (long long)((unsigned long long)(a.firstGlobal + i) / (unsigned long long)a.group) - a.firstColumn;
    const uint32_t tStride = (uint32_t)a.m.channels * (uint32_t)a.tCols * 4u;
    const char* const tBase = reinterpret_cast<const char*>(a.target + (size_t)c * (size_t)a.tCols + (size_t)col);
    long long q = a.pos;   // the target row of the next sample; without loop it runs on beyond tSamples and is then never used
    const char* tp = q < a.tSamples ? tBase + (size_t)q * tStride : tBase;
    const bool loop = a.loop != 0;
    int s = 0;
    for (; s + kMeterLoads <= a.m.samples; s += kMeterLoads) {
        uint32_t v[kMeterLoads], t[kMeterLoads];
        unsigned has = 0;
#pragma unroll
        for (int u = 0; u < kMeterLoads; ++u) {
            v[u] = *reinterpret_cast<const uint32_t*>(p);
            p += stride;
            const bool in = q < a.tSamples;
            t[u] = in ? *reinterpret_cast<const uint32_t*>(tp) : 0u;
            has |= (unsigned)in << u;
            ++q;
            tp += tStride;
            if (loop && q == a.tSamples) {
                q = 0;
                tp = tBase;
            }
        }
#pragma unroll
        for (int u = 0; u < kMeterLoads; ++u) {
            meterTake(m, v[u]);
            if (kLevel) levelTake(lv, v[u], l.release, floorBits);
            if (has & (1u << u)) matchTake(err, cross, v[u], t[u]);
        }
    }
    for (; s < a.m.samples; ++s) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
        p += stride;
        meterTake(m, v);
        if (kLevel) levelTake(lv, v, l.release, floorBits);
        if (q < a.tSamples) matchTake(err, cross, v, *reinterpret_cast<const uint32_t*>(tp));
        ++q;
        tp += tStride;
        if (loop && q == a.tSamples) {
            q = 0;
            tp = tBase;
        }
    }
    *energy = m.energy;
    *peak = m.peak;
    *fullScale = m.fullScale;
    *nonfinite = m.nonfinite;
    *errAt = err;
    *crossAt = cross;
    if (kLevel) {
        *levelAt = lv.level;
        *quietAt = lv.quiet;
    }
}

__global__ __launch_bounds__(256) void fx_meter_target(MeterTargetArgs a) { targetBody<false>(a, LevelParams{}); }
__global__ __launch_bounds__(256) void fx_meter_target_level(MeterTargetLevelArgs a) { targetBody<true>(a.t, a.l); }

}  // namespace

namespace {

bool badMeterArgs(const MeterArgs& a) {
    if (!a.y || !a.rows || a.n < 1 || a.nPad < a.n || a.pitch < a.n || a.samples < 1 || a.channels < 1 || a.channels > 4) return true;
    if ((unsigned long long)a.channels * (unsigned long long)a.pitch * 4u >= (1ull << 32)) return true;
    return (a.n + 255) / 256 >= ((long long)1 << 31);
}

bool badTargetArgs(const MeterTargetArgs& a) {
    const MeterArgs& m = a.m;
    if (badMeterArgs(m)) return true;
    if (!a.match || !a.target || a.tSamples < 1 || a.tCols < 1 || a.group < 1 || a.firstGlobal < 0 || a.pos < 0 || (a.loop && a.pos >= a.tSamples)) return true;
    // every lane's column lies in the block: the first one is column 0, the last one below tCols
    if (a.firstColumn != a.firstGlobal / a.group || (a.firstGlobal + m.n - 1) / a.group - a.firstColumn >= a.tCols) return true;
    return (unsigned long long)m.channels * (unsigned long long)a.tCols * 4u >= (1ull << 32);
}

// (the sign bit of both must be clear: levelTake compares patterns)
bool badLevelParams(const LevelParams& l) {
    return !l.rows || !(l.release >= 0.0f && l.release <= 1.0f) || !(l.floor >= 0.0f && l.floor < __builtin_inff()) || __builtin_signbit(l.release) || __builtin_signbit(l.floor);
}

}  // namespace

hipError_t launchMeterLevel(const MeterLevelArgs& a, hipStream_t stream) {
    if (badMeterArgs(a.m) || badLevelParams(a.l)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_meter_level, dim3((unsigned)((a.m.n + 255) / 256), (unsigned)a.m.channels), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchMeterTargetLevel(const MeterTargetLevelArgs& a, hipStream_t stream) {
    if (badTargetArgs(a.t) || badLevelParams(a.l)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_meter_target_level, dim3((unsigned)((a.t.m.n + 255) / 256), (unsigned)a.t.m.channels), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchMeterTarget(const MeterTargetArgs& a, hipStream_t stream) {
    if (badTargetArgs(a)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_meter_target, dim3((unsigned)((a.m.n + 255) / 256), (unsigned)a.m.channels), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchMeter(const MeterArgs& a, hipStream_t stream) {
    if (badMeterArgs(a)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_meter, dim3((unsigned)((a.n + 255) / 256), (unsigned)a.channels), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fx
