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

__global__ __launch_bounds__(256) void fx_meter(MeterArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const unsigned c = blockIdx.y;
    char* rows = static_cast<char*>(a.rows) + (size_t)c * meterChannelBytes(a.nPad);
    double* energy = reinterpret_cast<double*>(rows + meterEnergyOff(a.nPad)) + i;
    uint32_t* peak = reinterpret_cast<uint32_t*>(rows + meterPeakOff(a.nPad)) + i;
    uint32_t* fullScale = reinterpret_cast<uint32_t*>(rows + meterFullScaleOff(a.nPad)) + i;
    uint32_t* nonfinite = reinterpret_cast<uint32_t*>(rows + meterNonfiniteOff(a.nPad)) + i;
    MeterAcc m{*energy, *peak, *fullScale, *nonfinite};
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
        for (int u = 0; u < kMeterLoads; ++u) meterTake(m, v[u]);
    }
    for (; s < a.samples; ++s) {
        meterTake(m, *reinterpret_cast<const uint32_t*>(p));
        p += stride;
    }
    *energy = m.energy;
    *peak = m.peak;
    *fullScale = m.fullScale;
    *nonfinite = m.nonfinite;
}

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
__global__ __launch_bounds__(256) void fx_meter_target(MeterTargetArgs a) {
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
            if (has & (1u << u)) matchTake(err, cross, v[u], t[u]);
        }
    }
    for (; s < a.m.samples; ++s) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
        p += stride;
        meterTake(m, v);
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
}

}  // namespace

hipError_t launchMeterTarget(const MeterTargetArgs& a, hipStream_t stream) {
    const MeterArgs& m = a.m;
    if (!m.y || !m.rows || m.n < 1 || m.nPad < m.n || m.pitch < m.n || m.samples < 1 || m.channels < 1 || m.channels > 4) return hipErrorInvalidValue;
    if ((unsigned long long)m.channels * (unsigned long long)m.pitch * 4u >= (1ull << 32)) return hipErrorInvalidValue;
    if (!a.match || !a.target || a.tSamples < 1 || a.tCols < 1 || a.group < 1 || a.firstGlobal < 0 || a.pos < 0 || (a.loop && a.pos >= a.tSamples)) return hipErrorInvalidValue;
    // every lane's column lies in the block: the first one is column 0, the last one below tCols
    if (a.firstColumn != a.firstGlobal / a.group || (a.firstGlobal + m.n - 1) / a.group - a.firstColumn >= a.tCols) return hipErrorInvalidValue;
    if ((unsigned long long)m.channels * (unsigned long long)a.tCols * 4u >= (1ull << 32)) return hipErrorInvalidValue;
    const long long blocks = (m.n + 255) / 256;
    if (blocks >= ((long long)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_meter_target, dim3((unsigned)blocks, (unsigned)m.channels), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchMeter(const MeterArgs& a, hipStream_t stream) {
    if (!a.y || !a.rows || a.n < 1 || a.nPad < a.n || a.pitch < a.n || a.samples < 1 || a.channels < 1 || a.channels > 4) return hipErrorInvalidValue;
    if ((unsigned long long)a.channels * (unsigned long long)a.pitch * 4u >= (1ull << 32)) return hipErrorInvalidValue;
    const long long blocks = (a.n + 255) / 256;
    if (blocks >= ((long long)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_meter, dim3((unsigned)blocks, (unsigned)a.channels), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fx
