// fx_meter_value.hpp — V(n), the value of an instance in the meter queries (include/fx8010_amd.h "Meter queries by list", "Target
// meters", "Level meters", "Tone meters", "Meter ranks"), one device function per family.  DEVICE CODE: included by fx_meter_list.hip (the
// selects, fx_meter_best) and fx_meter_rank.hip (the ranks) and by nothing else, so that a select and a rank of the same family take
// V by the same instructions.
//
// Every V is a fixed sequence of IEEE operations in fp64.  The energy is an fp64 word already; a peak or an envelope (the bits of a
// non-negative finite float) and a counter (a uint32) convert to fp64 without rounding; the maximum or minimum of fp64 values is one
// of them.  The match value is the sum over the channels in channel order, starting from v(0,n).  The tone value is tonePower
// (fx_meter_tone.hpp) of two finite words.  No V is ever NaN.
#pragma once

#include <hip/hip_runtime.h>

#include "fx_meter.hpp"
#include "fx_meter_tone.hpp"

namespace fx {

// the four accumulators (stat 0 energy, 1 peak, 2 full_scale, 3 nonfinite): the maximum over the channels
__device__ __forceinline__ double meterValue(const void* rows, long long nPad, int channels, int stat, long long col) {
    const char* ch = static_cast<const char*>(rows);
    double best = 0.0;
    for (int c = 0; c < channels; ++c, ch += meterChannelBytes(nPad)) {
        double v;
        if (stat == 0) v = reinterpret_cast<const double*>(ch + meterEnergyOff(nPad))[col];
        else if (stat == 1) v = (double)reinterpret_cast<const float*>(ch + meterPeakOff(nPad))[col];
        else if (stat == 2) v = (double)reinterpret_cast<const uint32_t*>(ch + meterFullScaleOff(nPad))[col];
        else v = (double)reinterpret_cast<const uint32_t*>(ch + meterNonfiniteOff(nPad))[col];
        best = (c == 0 || v > best) ? v : best;
    }
    return best;
}

// the match rows (stat 0 err, 1 cross): ((v0 + v1) + v2) + v3 in fp64, in channel order, starting from v0
__device__ __forceinline__ double matchValue(const void* rows, long long nPad, int channels, int stat, long long col) {
    const char* ch = static_cast<const char*>(rows) + (stat == 0 ? matchErrOff(nPad) : matchCrossOff(nPad));
    double sum = reinterpret_cast<const double*>(ch)[col];
    for (int c = 1; c < channels; ++c) {
        ch += matchChannelBytes(nPad);
        sum = sum + reinterpret_cast<const double*>(ch)[col];
    }
    return sum;
}

// the level rows: stat 0 the maximum of the envelopes, stat 1 the MINIMUM of the quiet runs
__device__ __forceinline__ double levelValue(const void* rows, long long nPad, int channels, int stat, long long col) {
    const char* ch = static_cast<const char*>(rows);
    double best = 0.0;
    for (int c = 0; c < channels; ++c, ch += levelChannelBytes(nPad)) {
        if (stat == 0) {
            const double v = (double)reinterpret_cast<const float*>(ch + levelLevelOff(nPad))[col];
            best = (c == 0 || v > best) ? v : best;
        } else {
            const double v = (double)reinterpret_cast<const uint32_t*>(ch + levelQuietOff(nPad))[col];
            best = (c == 0 || v < best) ? v : best;
        }
    }
    return best;
}

// the tone rows (rows = the tone block, stat = the tone): the maximum over the channels of P; K and c come from the block's header
__device__ __forceinline__ double toneValue(const void* rows, long long nPad, int channels, int tone, long long col) {
    const char* const head = static_cast<const char*>(rows);
    const int tones = (int)*reinterpret_cast<const long long*>(head + kToneCountOff);
    const double c = reinterpret_cast<const double*>(head)[tone];
    double best = 0.0;
    for (int ch = 0; ch < channels; ++ch) {
        const double* const s1 = reinterpret_cast<const double*>(head + toneRowOff(nPad, tones, ch, tone)) + col;
        const double v = tonePower(c, s1[0], s1[nPad]);
        best = (ch == 0 || v > best) ? v : best;
    }
    return best;
}

}  // namespace fx
