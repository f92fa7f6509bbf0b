// fx_meter_tone.hip — the tone-meter kernels (fx_meter_tone.hpp).  gfx950, wave64, plain HIP C++, vector loads and stores only.
//
// fx_meter_tone<K> has the geometry of fx_meter (fx_meter.hip): workgroups of 256 lanes, grid.x over chunks of 256 instances,
// grid.y over the channels, one lane per column, the 32-bit byte stride, eight independent row loads in flight.  The 2 K fp64
// accumulators of a lane are read once, stay in registers for the whole launch and are written once.  It is a template over the
// tone count - eight kernels, picked by a switch on the host - because every tone is a dependency chain of its own (multiply, add,
// subtract: three dependent fp64 operations per sample) and the compiler needs the count to interleave the K chains.  The
// coefficients come by value in the argument block and live in scalar registers.  No LDS, no atomics, no scratch.
//
// Nothing is fused: p = c * s1 is rounded before q = x + p (-ffp-contract=off, csrc/Makefile; fx_meter_tone.hpp).
//
// Resource usage (-O3, gfx950, from -Rpass-analysis=kernel-resource-usage), VGPRs / SGPRs / scratch bytes per lane / LDS bytes per
// workgroup, wavefronts per SIMD:
//   fx_meter_tone<1>  53 / 32 / 0 / 0, eight      (<2> 63, <3> 53: eight)
//   fx_meter_tone<4>  61 / 30 / 0 / 0, eight      (<5> 69: seven, <6> 77: six, <7> 85: five)
//   fx_meter_tone<8>  93 / 38 / 0 / 0, five
//   fx_tone_gather    24 / 36 / 0 / 0, eight
//   fx_tone_zero       8 / 20 / 0 / 0, eight
// The code object holds no fused multiply-add of fp64 operands for these kernels.
#include <hip/hip_runtime.h>

#include "fx_meter_tone.hpp"

namespace fx {

namespace {

constexpr int kToneLoads = 8;   // row loads in flight per lane
constexpr int kLanes = kMeterSelectChunk;

// one output word into the K chains of a lane
template <int K>
__device__ __forceinline__ void toneTake(double (&s1)[K], double (&s2)[K], const double (&c)[K], uint32_t word) {
    const bool fin = (word & 0x7fffffffu) < 0x7f800000u;   // |y| < +Inf: false for NaN and +-Inf
    const double x = fin ? (double)__builtin_bit_cast(float, word) : 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double p = c[k] * s1[k];
        const double q = x + p;
        const double s0 = q - s2[k];
        s2[k] = s1[k];
        s1[k] = s0;
    }
}

template <int K>
__global__ __launch_bounds__(256) void fx_meter_tone(MeterToneArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const unsigned ch = blockIdx.y;
    double* const rows = reinterpret_cast<double*>(static_cast<char*>(a.block) + toneRowOff(a.nPad, K, (int)ch, 0)) + i;
    double s1[K], s2[K], c[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        c[k] = a.coeff[k];
        s1[k] = rows[(size_t)(2 * k) * (size_t)a.nPad];
        s2[k] = rows[(size_t)(2 * k + 1) * (size_t)a.nPad];
    }
    // a sample period is channels * pitch * 4 bytes further on: below 2^32 (launchMeterTone), a 32-bit stride
    const uint32_t stride = (uint32_t)a.channels * (uint32_t)a.pitch * 4u;
    const char* p = reinterpret_cast<const char*>(a.y + (size_t)ch * (size_t)a.pitch + (size_t)i);
    int s = 0;
    for (; s + kToneLoads <= a.samples; s += kToneLoads) {
        uint32_t v[kToneLoads];
#pragma unroll
        for (int u = 0; u < kToneLoads; ++u) {
            v[u] = *reinterpret_cast<const uint32_t*>(p);
            p += stride;
        }
#pragma unroll
        for (int u = 0; u < kToneLoads; ++u) toneTake<K>(s1, s2, c, v[u]);
    }
    for (; s < a.samples; ++s) {
        toneTake<K>(s1, s2, c, *reinterpret_cast<const uint32_t*>(p));
        p += stride;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        rows[(size_t)(2 * k) * (size_t)a.nPad] = s1[k];
        rows[(size_t)(2 * k + 1) * (size_t)a.nPad] = s2[k];
    }
}

// one lane per list entry: the packed side is s1 [tones][channels][count], then s2, then P
template <bool kGather>
__device__ __forceinline__ void toneColumns(const MeterListArgs& a) {
    const long long k = (long long)blockIdx.x * kLanes + threadIdx.x;
    if (k >= a.count) return;
    const long long inst = a.list[k];
    if (inst < 0 || inst >= a.n) return;
    const char* const head = static_cast<const char*>(a.rows);
    const int tones = (int)*reinterpret_cast<const long long*>(head + kToneCountOff);
    if (tones < 1 || tones > kMeterMaxTones) return;   // (cannot be: the runtime writes the header before the block is in force)
    const size_t part = (size_t)tones * (size_t)a.channels * (size_t)a.count;
    double* const packed = static_cast<double*>(a.packed);
    for (int t = 0; t < tones; ++t) {
        const double c = reinterpret_cast<const double*>(head)[t];
        for (int ch = 0; ch < a.channels; ++ch) {
            double* const s1At = reinterpret_cast<double*>(static_cast<char*>(a.rows) + toneRowOff(a.nPad, tones, ch, t)) + inst;
            double* const s2At = s1At + a.nPad;
            if (kGather) {
                const size_t at = ((size_t)t * (size_t)a.channels + (size_t)ch) * (size_t)a.count + (size_t)k;
                const double s1 = *s1At, s2 = *s2At;
                packed[at] = s1;
                packed[part + at] = s2;
                packed[2 * part + at] = tonePower(c, s1, s2);
            }
            if (!kGather || a.reset) {
                *s1At = 0.0;
                *s2At = 0.0;
            }
        }
    }
}

__global__ __launch_bounds__(kLanes) void fx_tone_gather(MeterListArgs a) { toneColumns<true>(a); }
__global__ __launch_bounds__(kLanes) void fx_tone_zero(MeterListArgs a) { toneColumns<false>(a); }

bool badToneList(const MeterListArgs& a, bool gather) {
    if (!a.rows || !a.list || a.count < 1 || a.count >= ((long long)1 << 31) || a.n < 1 || a.nPad < a.n) return true;
    if (a.channels < 1 || a.channels > 4) return true;
    return gather && !a.packed;
}

template <int K>
hipError_t launchTone(const MeterToneArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(fx_meter_tone<K>, dim3((unsigned)((a.n + 255) / 256), (unsigned)a.channels), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launchMeterTone(const MeterToneArgs& a, hipStream_t stream) {
    if (!a.y || !a.block || a.n < 1 || a.nPad < a.n || a.pitch < a.n || a.samples < 1 || a.channels < 1 || a.channels > 4) return hipErrorInvalidValue;
    if ((unsigned long long)a.channels * (unsigned long long)a.pitch * 4u >= (1ull << 32) || (a.n + 255) / 256 >= ((long long)1 << 31)) return hipErrorInvalidValue;
    if (a.tones < 1 || a.tones > kMeterMaxTones) return hipErrorInvalidValue;
    for (int k = 0; k < a.tones; ++k)
        if (!(a.coeff[k] >= -2.0 && a.coeff[k] <= 2.0) || (a.coeff[k] == 0.0 && __builtin_signbit(a.coeff[k]))) return hipErrorInvalidValue;
    (void)hipGetLastError();
    switch (a.tones) {
        case 1: return launchTone<1>(a, stream);
        case 2: return launchTone<2>(a, stream);
        case 3: return launchTone<3>(a, stream);
        case 4: return launchTone<4>(a, stream);
        case 5: return launchTone<5>(a, stream);
        case 6: return launchTone<6>(a, stream);
        case 7: return launchTone<7>(a, stream);
        default: return launchTone<8>(a, stream);
    }
}

hipError_t launchToneGather(const MeterListArgs& a, hipStream_t stream) {
    if (badToneList(a, true)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_tone_gather, dim3((unsigned)((a.count + kLanes - 1) / kLanes)), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchToneZero(const MeterListArgs& a, hipStream_t stream) {
    if (badToneList(a, false)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_tone_zero, dim3((unsigned)((a.count + kLanes - 1) / kLanes)), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fx
