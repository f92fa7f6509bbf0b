// fx_meter.hip — the output-meter kernel behind an emulation launch (fx_meter.hpp).  gfx950, wave64, workgroups of 256 lanes:
// grid.x walks the instances in chunks of 256, grid.y the channels.  One lane owns one column of one channel: it reads its four
// accumulators once, streams the column's samples in order - eight independent row loads in flight, 256 contiguous bytes per
// wavefront and load - and writes the accumulators back once.  Everything that decides a bit is integer work on the word's
// pattern (|y| and its compares, the maximum of two non-negative finite floats) except the energy: an fp64 add of an exact
// product, one rounding per sample.
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

}  // namespace

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
