// fx_bus.hpp — launch interface of the group-bus kernels (device code: fx_bus.hip).
//
// A bus block is a sandwich around the unchanged emulation launch: `expand` writes a per-group input [rows][groups] out to the
// per-instance scratch [rows][n], the emulation runs on the scratch in place, `mix` reduces the scratch to [rows][groups].
// rows = samples * channels; group g holds instances g*K .. min((g+1)*K, n) - 1.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fx {

struct BusArgs {
    const float* narrowIn;   // expand: [rows][narrowPitch] group words (device memory or device-visible host memory)
    float* narrowOut;        // mix: the same layout, written
    float* wide;             // [rows][n] per-instance scratch, rows packed (device memory)
    long long rows;          // samples * channels
    long long n;             // instances
    long long group;         // K, 1 <= K <= n (the caller clamps a larger K: one group either way)
    long long groups;        // G = ceil(n / K)
    long long narrowPitch;   // floats per row of the narrow side (>= groups)
};

// wide[r][i] = narrowIn[r][i / K]: a wavefront loads 64 consecutive group words of a row once and writes their copies
hipError_t launchBusExpand(const BusArgs& a, hipStream_t stream);

// narrowOut[r][g] = sum of wide[r][g*K ...] in the order of the 64-lane shuffle-down tree: p[l] (l = 0..63, +0.0f) takes the
// group's members m = j*64 + l for j ascending, then p[l] += p[l + step] for step = 32 .. 1 (l < step); the result is p[0].
// fp32, round to nearest, never fused, denormals kept.
hipError_t launchBusMix(const BusArgs& a, hipStream_t stream);

// Where the rows of a weighted launch are in the caller's block and on its ramp: the base of the arguments of the gains, the
// sends and the feeds, so that each of them has these fields under these names.
struct BusRampArgs {
    int channels;            // C: row r of the piece is sample r / C + sample0 of the call, channel r % C
    int ramp;                // 1: a ramp is pending, w = a + (b - a) * ((float)(s + 1) * r) and exactly b at s == samples - 1; 0: w = b
    float r;                 // 1.0f / (float)samples, divided once on the host
    int samples;             // S of the caller's block, never a piece's
    int sample0;             // first sample of this piece within the block
};

// The gains of a weighted mix (include/fx8010_amd.h "Bus gains"): two blocks [channels][gainPitch] by instance, device memory.
struct BusGainArgs : BusRampArgs {
    const float* current;    // a: read only while a ramp is pending (may be null otherwise)
    const float* target;     // b
    long long gainPitch;     // floats per channel row of both blocks (>= n)
};

// narrowOut[r][g] = the sum of launchBusMix over the terms (w == 0.0f ? +0.0f : w * wide[r][i]) instead of wide[r][i]: a member
// with a weight of either zero contributes +0.0f whatever it holds.  (b - a), * t, a + and w * y are rounded one by one.
hipError_t launchBusMixGain(const BusArgs& a, const BusGainArgs& g, hipStream_t stream);

// Bus taps (include/fx8010_amd.h "Bus taps"): a handful of columns of the scratch block, gathered into a narrow [rows][tapPitch]
// side beside the mix.  Words move as 32-bit patterns.
struct BusTapArgs {
    const uint32_t* wide;    // [rows][n] per-instance scratch, rows packed (device memory)
    uint32_t* tapOut;        // [rows][tapPitch] (device memory or device-visible host memory)
    const uint32_t* idx;     // [taps] instance numbers of this batch, each below n (device memory; the caller has checked them)
    const uint32_t* col;     // [taps] the column of tapOut each tap goes to, each below tapPitch; null: tap t goes to column t
    long long rows;          // samples * channels
    long long n;             // instances; n * 4 < 2^32
    long long taps;          // T of this batch, 1 <= T <= 65 536
    long long tapPitch;      // words per row of tapOut (>= taps; with `col`, above every column; <= 65 536)
};

// tapOut[r][col ? col[t] : t] = wide[r][idx[t]]: consecutive lanes own consecutive taps, so a row's store is contiguous where the
// columns are (256 bytes per wavefront once T >= 64); the load is a gather
hipError_t launchBusTap(const BusTapArgs& a, hipStream_t stream);

// Bus sends (include/fx8010_amd.h "Bus sends"): aux buses by member list.  Bus j owns `entries` of a CSR structure; the entries
// are cut into chunks of at most kSendChunk positions of ONE bus (the host builds the table), every chunk is summed by one
// wavefront in the order of launchBusMix, and a bus with more than one chunk is the same sum over its chunk sums.
constexpr long long kSendChunk = 1024;   // part of the contract, not a tuning knob
struct BusSendChunk { uint32_t first, count; };          // entries first .. first + count - 1, 1 <= count <= kSendChunk
struct BusSendBus { uint32_t firstChunk, chunks, column; };   // Q = chunks (0: an empty bus); column of auxOut where `columns` is set
struct BusSendArgs : BusRampArgs {
    const float* wide;            // [rows][n] per-instance scratch, rows packed (device memory)
    const uint32_t* idx;          // [entries] instance numbers of this batch, each below n (device memory; the caller has checked them)
    const float* current;         // a: [channels][gainPitch] by entry, read only while a ramp is pending (may be null otherwise)
    const float* target;          // b
    const BusSendChunk* chunk;    // [chunks] (device memory); every first + count <= entries
    const BusSendBus* bus;        // [buses] (device memory); every firstChunk + chunks <= chunks of the launch
    float* partial;               // [rows][chunks] chunk sums (device memory), written by the first kernel, read by the second
    float* auxOut;                // [rows][auxPitch] (device memory or device-visible host memory)
    long long rows;               // samples * channels
    long long n;                  // instances; n * 4 < 2^32
    long long entries;            // E of this batch (may be 0: every bus is empty)
    long long gainPitch;          // floats per channel row of both gain blocks (>= entries)
    long long chunks;             // of the table (0 iff entries == 0)
    long long buses;              // of this batch, 1 <= buses <= 65 536
    long long auxPitch;           // floats per row of auxOut (>= buses; with `columns`, above every column)
    int columns;                  // 1: bus j goes to column bus[j].column; 0: to column j
};

// partial[r][q] = the sum of chunk q's terms (w == 0.0f ? +0.0f : w * wide[r][idx[e]]) in the order of launchBusMix, then
// auxOut[r][column of bus j] = partial[r][firstChunk] for one chunk, that same sum over the bus's chunk sums for more, +0.0f for none
hipError_t launchBusSend(const BusSendArgs& a, hipStream_t stream);

// Bus feeds (include/fx8010_amd.h "Bus feeds"): the scratch block built from per-instance lists of columns of a narrow source
// block [rows][m].  Instance i owns the entries off[i] .. off[i + 1] - 1 (CSR by instance); the MAP form (off null) is the
// structure whose every instance has exactly one entry, entry i being instance i's.  Every table is 32-bit words, 16-byte
// aligned and padded so that a lane reads the words of its four instances with one access whatever n is:
//   off     [ceil4(n) + 1], the words behind off[n] repeating it (instances that do not exist own nothing); null: the map form
//   idx     [entries] source columns, each below m (the map form: [ceil4(n)], padded with columns below m)
//   target  b: [channels][gainPitch] by entry; null: UNWEIGHTED (words move as bit patterns)
//   current a: read only while a ramp is pending
// gainPitch >= entries (the map form: >= ceil4(n) and a multiple of 4).
struct BusFeedArgs : BusRampArgs {   // (unweighted: channels only, ramp 0)
    const uint32_t* src;     // [rows][m] source words, rows packed (device memory: every word is gathered many times)
    uint32_t* wide;          // [rows][n] per-instance scratch, rows packed (device memory)
    const uint32_t* off;
    const uint32_t* idx;
    const float* current;
    const float* target;
    long long rows;          // samples * channels
    long long n;             // instances; n * 4 < 2^32
    long long m;             // source columns, m >= 1; m * 4 < 2^32
    long long entries;       // E of this batch, <= 2^24 (the map form: n)
    long long gainPitch;
};

// wide[r][i] = the word of the definition: +0.0f for no entry, term_0 for one, ((term_0 + term_1) + term_2) + ... in entry order
// for more; term_k = src[r][idx[e]] (unweighted), else (w == 0.0f ? +0.0f : w * src[r][idx[e]]) with w as in launchBusMixGain
hipError_t launchBusFeed(const BusFeedArgs& a, hipStream_t stream);

// A gain set by list (include/fx8010_amd.h "Gain sets by list"): `count` words per channel scattered into one or both of the two
// gain blocks of the bus gains, the sends or the feeds.  Words move as 32-bit patterns.
struct GainScatterArgs {
    const uint32_t* idx;     // [count] positions in a channel row of the blocks, each below pitch and no two alike (device memory; the caller has checked them)
    const uint32_t* val;     // [channels][count] the new words, row pitch exactly count (device memory)
    uint32_t* b;             // [channels][pitch] the block that is b
    uint32_t* a;             // the block that is a, written with the same words (ramp = 0 while a ramp is pending); null: b only
    long long count;         // K >= 1
    long long pitch;         // words per channel row of both blocks: n (bus gains), E of this batch (sends), the quad-padded pitch (feeds)
    int channels;            // C
};

// b[c][idx[k]] = val[c][k] (and a likewise) for every c and k: one lane per list entry, loads of consecutive words, scattered stores
hipError_t launchGainScatter(const GainScatterArgs& a, hipStream_t stream);

}  // namespace fx
