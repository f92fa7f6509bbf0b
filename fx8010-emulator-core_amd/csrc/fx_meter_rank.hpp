// fx_meter_rank.hpp — launch interface of the kernels behind the meter ranks (fxb_meter_rank, fxb_meter_rank_match,
// fxb_meter_rank_level; device code: fx_meter_rank.hip).
//
// A rank asks for the first k candidates of a range under the total order (V, n): V ascending as real numbers - with `largest`
// descending - and ties to the smaller instance number.  V(n) and the candidates are those of the select of the same family
// (fx_meter_value.hpp; V >= threshold, with `below` V < threshold).  It is a selection, not a sort: a most-significant-digit radix
// select over 64-bit keys finds the key T of the k-th candidate, then the count / scan / emit pattern of the selects writes the
// winners - every candidate with a key below T and the first few, BY INSTANCE NUMBER, of those whose key equals T - as (n, V)
// pairs ascending by instance.  The host puts the pairs into rank order (rankBefore).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "fx_meter_list.hpp"

namespace fx {

constexpr int kMeterRankDigitBits = 8;                             // bits of one radix digit
constexpr int kMeterRankPasses = 64 / kMeterRankDigitBits;         // digits of a key, most significant first
constexpr int kMeterRankBins = 1 << kMeterRankDigitBits;           // = the lanes of a workgroup: one bin per lane in the pick
static_assert(kMeterRankBins == kMeterSelectChunk, "the pick scans the bins with one lane each");

enum { kRankMeter = 0, kRankMatch = 1, kRankLevel = 2, kRankTone = 3 };   // MeterRankArgs::family

// The staging block of one rank, 64-bit words, in this order (the part the host copies back comes first):
//   result   [kRankResultWords]          M (the candidates), R = min(k, M) (the pairs written), T (the key of the R-th), the number
//                                        of candidates with key == T that win
//   pairs    [2 * room]                  room = min(k, nRange): pair i is (instance number, the bits of V), ascending by instance
//   hist     [kMeterRankPasses][kMeterRankBins]   digit counts of pass p among the candidates whose higher digits equal the prefix
//   slots    [kMeterRankPasses][2]       (prefix, remainder) in front of pass p; slot 0 is unused (nothing is in front of pass 0)
//   below    [chunks]                    per chunk: candidates with key < T; after the scan the exclusive scan of the winners
//   equal    [chunks]                    per chunk: candidates with key == T; after the scan the chunk's share of those that win
// hist and slots must be zero when the first kernel starts (launchMeterRank queues the memset).
constexpr size_t kRankResultWords = 4;
constexpr size_t rankPairsOff() { return kRankResultWords; }
constexpr size_t rankHistOff(long long room) { return kRankResultWords + 2 * (size_t)room; }
constexpr size_t rankSlotsOff(long long room) { return rankHistOff(room) + (size_t)kMeterRankPasses * kMeterRankBins; }
constexpr size_t rankBelowOff(long long room) { return rankSlotsOff(room) + (size_t)kMeterRankPasses * 2; }
constexpr size_t rankEqualOff(long long nRange, long long room) { return rankBelowOff(room) + (size_t)meterSelectChunks(nRange); }
constexpr size_t meterRankStageWords(long long nRange, long long room) { return rankEqualOff(nRange, room) + (size_t)meterSelectChunks(nRange); }

struct MeterRankArgs {
    const void* rows;              // [channels] x the rows of the family (device memory): accumulator, match or level rows; the tone block
    unsigned long long* stage;     // device memory, meterRankStageWords(nRange, room) words, laid out as above
    long long n, nPad;             // instances, and the pitch of a row
    long long first, nRange;       // LOCAL columns first .. first + nRange - 1 are looked at; first + nRange <= n
    long long firstGlobal;         // the number written for column `first`
    long long k;                   // pairs wanted, >= 0
    long long room;                // min(k, nRange): pairs the staging has room for
    double threshold;              // not NaN; +-Inf allowed
    int channels;                  // 1..4
    int family;                    // kRankMeter / kRankMatch / kRankLevel / kRankTone
    int stat;                      // the family's: 0..3, 0..1, 0..1, the tone 0..K-1
    int below;                     // 0: V >= threshold is a candidate; 1: V < threshold
    int largest;                   // 0: V ascending; 1: V descending.  Ties go to the smaller instance number either way
};

// kMeterRankPasses + 3 launches behind one memset, whatever nRange, k and the data are: fx_rank_hist once per digit (each
// workgroup first repeats the pick of the digit in front from that pass's histogram: no launch of its own, no workgroup waits for
// another), fx_rank_count (the last pick; below / equal per chunk), fx_rank_scan (one workgroup: the shares of the equals, the
// exclusive scan of the winners), fx_rank_emit (with room == 0 - a count query - not launched).  Reads the rows and writes nothing
// but `stage`.  The only atomics are integer adds into histogram bins, whose sums do not depend on their order: the same bits run
// to run.
hipError_t launchMeterRank(const MeterRankArgs& a, hipStream_t stream);

// the total order of the ranks, for the host: whether (va, na) comes before (vb, nb).  Compares of real numbers: -0.0 == +0.0
inline bool rankBefore(double va, long long na, double vb, long long nb, bool largest) {
    if (va != vb) return largest ? va > vb : va < vb;
    return na < nb;
}

}  // namespace fx
