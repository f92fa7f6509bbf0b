// fx_meter_list.hpp — launch interface of the kernels behind the meter queries by list (fxb_meter_select, fxb_meter_read_list,
// fxb_meter_reset_list; device code: fx_meter_list.hip).
//
// The accumulator rows are those of fx_meter.hpp: per channel energy f64 [nPad], peak f32 [nPad], full_scale u32 [nPad],
// nonfinite u32 [nPad].  A select looks at ONE of the four rows of every channel; the value of an instance is the maximum over the
// channels, taken in fp64 (include/fx8010_amd.h "Meter queries by list").  The packed side of a gather holds, for `count` list
// entries, energy f64 [channels][count], then peak f32 [channels][count], full_scale and nonfinite u32 [channels][count]: every
// row has the pitch `count`, and the 64-bit part comes first so that every part is aligned.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace fx {

constexpr int kMeterSelectChunk = 256;   // instances of one chunk: one workgroup, one count
constexpr int kMeterScanWidth = 256;     // lanes of the scan: above that many chunks a lane owns several counts and loops
constexpr long long meterSelectChunks(long long nRange) { return (nRange + kMeterSelectChunk - 1) / kMeterSelectChunk; }
// bytes of the packed side of a gather
constexpr size_t meterPackedBytes(int channels, long long count) { return (size_t)channels * (size_t)count * 20; }

struct MeterSelectArgs {
    const void* rows;              // [channels] x the accumulator rows (device memory)
    unsigned long long* offsets;   // device memory, meterSelectChunks(nRange) + 1 words: the chunk counts, then their exclusive
                                   // scan in place, the total M in the last word
    long long* list;               // device memory, min(cap, nRange) words (may be null when that is 0)
    long long n, nPad;             // instances, and the pitch of an accumulator row
    long long first, nRange;       // LOCAL columns first .. first + nRange - 1 are looked at; first + nRange <= n
    long long firstGlobal;         // the number written for column `first`
    long long cap;                 // entries of `list` that may be written, >= 0
    double threshold;              // not NaN; +-Inf allowed
    int channels;                  // 1..4
    int stat;                      // 0 energy, 1 peak, 2 full_scale, 3 nonfinite
    int below;                     // 0: V >= threshold matches; 1: V < threshold
};

// three launches on `stream`: fx_meter_count (a count per chunk), fx_meter_scan (one workgroup: the exclusive scan and the
// total), fx_meter_emit (the matching numbers firstGlobal + i at offset + rank, where that is below cap).  Reads the rows and
// writes nothing but offsets[0 .. chunks] and list[0 .. min(M, cap) - 1].  The order is ascending and the same run to run.
hipError_t launchMeterSelect(const MeterSelectArgs& a, hipStream_t stream);

struct MeterListArgs {
    void* rows;               // [channels] x the accumulator rows
    const long long* list;    // device memory: `count` instance numbers, each in [0, n)
    void* packed;             // gather: the packed side (above), device memory; zero: unused
    long long count;          // 1 .. 2^31 - 1
    long long n, nPad;
    int channels;             // 1..4
    int reset;                // gather: zero the accumulators of every listed column behind its read, in the same lane
};

// packed[..][c][k] = the accumulators of channel c of instance list[k], bit for bit.  Repeats are fine without reset.  An entry
// outside [0, n) - the runtime refuses such lists - is skipped: its column of the packed side stays as it is.
hipError_t launchMeterGather(const MeterListArgs& a, hipStream_t stream);
// the four accumulators of every channel of every listed instance = +0.0, +0.0f, 0, 0.  Stores only; repeats are fine.
hipError_t launchMeterZero(const MeterListArgs& a, hipStream_t stream);

// ---- queries over the match rows of a target (fx_meter.hpp; include/fx8010_amd.h "Target meters") -----------------------------
// The value of an instance is V(n) = ((v(0,n) + v(1,n)) + v(2,n)) + v(3,n) over the channels in fp64, in channel order, starting
// from v(0,n): a sum, not the maximum of the select above.  No match accumulator is ever NaN or infinite.

struct MatchSelectArgs {
    const void* rows;              // [channels] x the match rows (device memory)
    unsigned long long* offsets;   // as MeterSelectArgs
    long long* list;
    long long n, nPad;
    long long first, nRange;
    long long firstGlobal;
    long long cap;
    double threshold;
    int channels;                  // 1..4
    int stat;                      // 0 err, 1 cross
    int below;
};
// the three launches of launchMeterSelect with the channel-sum predicate over the match rows
hipError_t launchMatchSelect(const MatchSelectArgs& a, hipStream_t stream);

struct MeterBestArgs {
    const void* rows;         // [channels] x the match rows
    long long* winner;        // device memory, `groups` words: the GLOBAL instance number of the best local member of each group
    double* value;            // device memory, `groups` words: its V
    long long n, nPad;
    long long firstGlobal;    // the global number of local column 0
    long long group;          // >= 1: group g holds the global instances g * group .. (g + 1) * group - 1
    long long firstGroup;     // firstGlobal / group: winner[0] belongs to it
    long long groups;         // (firstGlobal + n - 1) / group - firstGroup + 1: every one of them has a local member
    int channels;             // 1..4
    int stat;                 // 0 err, 1 cross
    int largest;              // 0: the smallest V wins; 1: the largest.  Ties go to the smallest instance number
};
// fx_meter_best: one wavefront per group.  The lanes stride the group's local members keeping the best (V, n) under the total
// order "V, then n"; a 64-lane shuffle reduction of the pair; lane 0 stores.  Only compares decide: the tree shape cannot change
// a bit.  No atomics, no workgroup waits for another.  Groups below 64 leave lanes idle.
hipError_t launchMeterBest(const MeterBestArgs& a, hipStream_t stream);

// err and cross of every channel of every listed instance = +0.0 (MeterListArgs with rows = the match rows; packed, reset
// unused).  Stores only; repeats are fine; an entry outside [0, n) is skipped.
hipError_t launchMatchZero(const MeterListArgs& a, hipStream_t stream);

// ---- queries over the level rows (fx_meter.hpp; include/fx8010_amd.h "Level meters") ------------------------------------------
// The value of an instance: stat 0 (envelope) the MAXIMUM over the channels of (double)level, stat 1 (quiet run) the MINIMUM over
// the channels of (double)quiet - a voice has been quiet for k samples only if every channel has.  Both convert to fp64 without
// rounding and no level is ever NaN, so V >= t and V < t stay complements.

struct LevelSelectArgs {
    const void* rows;              // [channels] x the level rows (device memory)
    unsigned long long* offsets;   // as MeterSelectArgs
    long long* list;
    long long n, nPad;
    long long first, nRange;
    long long firstGlobal;
    long long cap;
    double threshold;
    int channels;                  // 1..4
    int stat;                      // 0 envelope, 1 quiet run
    int below;
};
// the three launches of launchMeterSelect (fx_level_count / fx_meter_scan / fx_level_emit) with the predicate above
hipError_t launchLevelSelect(const LevelSelectArgs& a, hipStream_t stream);

// bytes of the packed side of a level gather: level f32 [channels][count], then quiet u32 [channels][count]
constexpr size_t levelPackedBytes(int channels, long long count) { return (size_t)channels * (size_t)count * 8; }
// fx_level_gather / fx_level_zero: launchMeterGather / launchMeterZero on the two level rows (MeterListArgs with rows = the level
// rows and the packed side above).  One lane per list entry; with `reset` the lane that has read a column stores its zeros.
hipError_t launchLevelGather(const MeterListArgs& a, hipStream_t stream);
hipError_t launchLevelZero(const MeterListArgs& a, hipStream_t stream);

}  // namespace fx
