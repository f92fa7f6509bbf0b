// fx_meter_tone.hpp — launch interface of the tone meters (device code: fx_meter_tone.hip; the select's two kernels sit beside
// their siblings in fx_meter_list.hip, the rank goes through fx_meter_rank.hip).
//
// Tone meters (include/fx8010_amd.h "Tone meters"): a Goertzel recurrence per (tone k, channel, instance) - two fp64 words s1, s2,
// +0.0 after a reset.  For every output word y of the column, in sample order, with fin as in fx_meter.hpp: x = fin ? (double)y :
// +0.0 (the SIGNED word), p = c * s1, q = x + p, s0 = q - s2, s2 = s1, s1 = s0 - one fp64 multiply, one add, one subtract, each
// rounded on its own.  NOTHING IS FUSED: the contract depends on -ffp-contract=off (csrc/Makefile FLAGS / HOSTFLAGS); with a
// fused multiply-add p would not be rounded and the words would differ from the definition.  The figure is tonePower below.
//
// Bounds.  With |c| <= 2 the impulse response of the recurrence is bounded by its index (|sin((n + 1)w) / sin(w)| <= n + 1, and
// n + 1 at c = +-2), so after n samples |s1| <= n (n + 1) / 2 * max|y|.  From fp32 inputs (|y| < 2^128) a word could leave fp64 only
// beyond n ~ 2^447 samples: no reachable sample count makes a word non-finite or P a NaN.  The rule of the ranks "no V is ever NaN"
// (fx_meter_value.hpp) rests on this, and it is why coefficients beyond +-2 - a recurrence that grows exponentially - are refused.
//
// The tone block of a batch, one device allocation: a header of kToneHeaderBytes - coeff f64 [kMeterMaxTones], then the tone
// count K as a 64-bit word - followed by the rows [channels][K][2][nPad] f64: for channel c and tone k the row of s1, then the row
// of s2.  With the header in the block toneValue(rows, nPad, channels, tone, col) has the signature of its siblings and the
// argument structs of the selects and the ranks stay as they are.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "fx_meter.hpp"
#include "fx_meter_list.hpp"
#include "fx_meter_rank.hpp"

namespace fx {

constexpr int kMeterMaxTones = 8;   // FXB_METER_MAX_TONES
constexpr size_t kToneHeaderBytes = 128;
constexpr size_t kToneCountOff = 8 * (size_t)kMeterMaxTones;   // byte offset of K in the header
constexpr size_t toneRowsBytes(long long nPad, int channels, int tones) { return (size_t)channels * (size_t)tones * 16 * (size_t)nPad; }
constexpr size_t toneBlockBytes(long long nPad, int channels, int tones) { return kToneHeaderBytes + toneRowsBytes(nPad, channels, tones); }
// byte offset of the s1 row of (channel, tone) in the block; the s2 row follows 8 * nPad bytes further on
constexpr size_t toneRowOff(long long nPad, int tones, int channel, int tone) { return kToneHeaderBytes + ((size_t)channel * (size_t)tones + (size_t)tone) * 16 * (size_t)nPad; }

// P = (s1*s1 + s2*s2) - (c*s1)*s2: five fp64 operations in exactly this order, none fused (-ffp-contract=off).  The one place that
// computes it: the full read calls it on the host, fx_tone_gather, toneValue (the selects and ranks) and the stand-in call it too.
// It may come out a few ulps negative; it is ordered as the real number it is.
__host__ __device__ inline double tonePower(double c, double s1, double s2) {
    const double a = s1 * s1;
    const double b = s2 * s2;
    const double sum = a + b;
    const double p = c * s1;
    const double m = p * s2;
    return sum - m;
}

struct MeterToneArgs {
    const float* y;      // the block fx_meter reads: [samples][channels][pitch]
    void* block;         // the tone block above (device memory); only its rows are touched
    long long n, nPad, pitch;
    int samples;         // >= 1
    int channels;        // 1..4
    int tones;           // 1..kMeterMaxTones
    double coeff[kMeterMaxTones];   // by value: finite, -2 <= c <= 2, never -0.0; entries from `tones` on are unused
};

// fx_meter_tone<K>: a launch of its own behind the meter launch of a block, the geometry of fx_meter.  The 2 K accumulators of a
// lane stay in registers for the whole launch: read once, written once.
hipError_t launchMeterTone(const MeterToneArgs& a, hipStream_t stream);

// bytes of the packed side of a tone gather: s1 f64 [tones][channels][count], then s2, then P
constexpr size_t tonePackedBytes(int tones, int channels, long long count) { return (size_t)tones * (size_t)channels * (size_t)count * 24; }
// fx_tone_gather / fx_tone_zero: one lane per list entry (MeterListArgs with rows = the tone block; K and the coefficients are
// read from its header).  The gather writes s1, s2 and P of every (tone, channel) of the listed column; with `reset` the lane that
// has read a column stores its zeros.  fx_tone_zero stores only.  An entry outside [0, n) is skipped.
hipError_t launchToneGather(const MeterListArgs& a, hipStream_t stream);
hipError_t launchToneZero(const MeterListArgs& a, hipStream_t stream);

// the select over V(n) = the maximum over the channels of P(tone, c, n) (fx_meter_value.hpp toneValue)
struct ToneSelectArgs {
    const void* rows;              // the tone block
    unsigned long long* offsets;   // as MeterSelectArgs
    long long* list;
    long long n, nPad;
    long long first, nRange;
    long long firstGlobal;
    long long cap;
    double threshold;
    int channels;                  // 1..4
    int stat;                      // the tone, 0 .. K - 1 (the runtime checks it against K)
    int below;
};
// the three launches of launchMeterSelect (fx_tone_count / fx_meter_scan / fx_tone_emit) with the predicate above
hipError_t launchToneSelect(const ToneSelectArgs& a, hipStream_t stream);

// launchMeterRank for the family kRankTone (rows = the tone block, stat = the tone), under a name of its own so that a host-only
// stand-in can define it apart from the stand-in of the three other families
hipError_t launchToneRank(const MeterRankArgs& a, hipStream_t stream);

}  // namespace fx
