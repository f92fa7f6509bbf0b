// fx_tram.hpp — launch interface of the kernels behind the delay-line windows by list (fxb_set_tram_list, fxb_get_tram_list;
// device code: fx_tram.hip).
//
// One delay line of the batch is line[inst / cols][slot][inst % cols] (cols = 64 * K instances of one wavefront tile, `slots`
// allocated slots per instance: fx_instances.hpp).  A window is nWords words of one instance, word j of it being
//   physical (ringSize == 0):  slot first + j
//   logical  (ringSize == Z):  slot (p - 1 - first - j) mod Z, or with `dane` slot (p + 1 + first + j) mod Z, p being the
//                              instance's position word state[posRow][inst] as the kernel finds it
// (include/fx8010_amd.h "Delay-line windows by list").  On the packed side entry i's window is values + i * valueStride.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fx {

struct TramListArgs {
    uint32_t* line;           // [waves][slots][cols]
    const uint32_t* state;    // [stateRows][nPad]; read in logical mode only (may be null otherwise)
    const long long* list;    // device memory: `count` instance numbers, each in [0, n)
    uint32_t* values;         // device memory: the scatter reads it, the gather writes it
    long long valueStride;    // words between two windows (>= nWords); scatter only: 0 = every listed instance takes values[0 .. nWords)
    long long count;          // list entries, 1 .. 2^31 - 1
    long long n, nPad;        // instances, and the pitch of a state row
    int slots, cols;          // allocated slots of the line (>= 1), 64 / 128 / 256
    int posRow;               // the state row of the line's write position
    int ringSize;             // 0: physical; else Z (1 .. slots)
    int dane;                 // logical mode: the FX_OPT_TRAM_DANE addressing
    int first, nWords;        // physical: first + nWords <= slots; logical: first < Z, nWords <= Z; nWords >= 1
};

// word j of the window of instance list[i] = values[i * valueStride + j].  Words move as 32-bit patterns.  Nothing but the listed
// words is written: no column >= n, no slot outside the line, none of the padding.  An entry outside [0, n), or in logical mode an
// entry whose position word lies outside 0 .. Z - 1, is skipped.  An instance listed twice would be written twice in no defined
// order - the caller refuses such lists.
hipError_t launchTramScatter(const TramListArgs& a, hipStream_t stream);

// values[i * valueStride + j] = word j of the window of instance list[i].  Repeats are fine; a skipped entry's window is left
// as it is.
hipError_t launchTramGather(const TramListArgs& a, hipStream_t stream);

}  // namespace fx
