// fx_tracks.hpp — launch interface of the kernels that expand list schedules into event rows (fxb_set_register_tracks_list;
// device code: fx_tracks.hip).
//
// An event of a per-instance track is one row of nPad words in the track buffer (fx_xlate.hpp TrackEvent, strideBytes = nPad * 4):
// the generated loop loads one word per lane from it.  For a register with list schedules the rows of a block are built on the
// device: fx_track_hold fills every event row of the register with the register's state row - what every voice holds at the head
// of the block - and fx_track_scatter then writes the steps' words at the listed voices, each into the rows from its own event
// up to the same schedule's next one.  `rows` points at the first event row; row r is the nPad words at rows + r * nPad.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fx {

constexpr int kMaxTrackHolds = 16;   // registers with schedules (fx_xlate.hpp kMaxTracks)

struct TrackHoldArgs {
    const uint32_t* state;    // [stateRows][nPad], 16-byte aligned
    uint32_t* rows;           // [totalRows][nPad], 16-byte aligned
    long long nPad;           // a multiple of 256: every row of either block is 16-byte aligned
    long long totalRows;
    int stateRows;
    int nRegs;                // 1 .. kMaxTrackHolds: the wave-uniform table below
    int stateRow[kMaxTrackHolds];   // the register's row of the state block
    int firstRow[kMaxTrackHolds];   // its first event row
    int rowCount[kMaxTrackHolds];   // its event rows: firstRow .. firstRow + rowCount - 1
};

// rows[firstRow[t] + e][i] = state[stateRow[t]][i] for every t < nRegs, e < rowCount[t], i < nPad.  A table entry that points
// outside either block is skipped.
hipError_t launchTrackHold(const TrackHoldArgs& a, hipStream_t stream);

struct TrackRange { int valueRow, rowLo, rowHi, reserved; };   // values[valueRow][entry] goes to the rows rowLo .. rowHi - 1

struct TrackScatterArgs {
    uint32_t* rows;             // [totalRows][nPad]
    const long long* list;      // device memory: `count` instance numbers, each in [0, n)
    const uint32_t* values;     // device memory: [valueRows][count] - the caller's [step][key][entry]
    const TrackRange* ranges;   // device memory: nRanges of them, one per (step inside the block, key)
    long long count;            // 1 .. 2^31 - 1; valueRows * count < 2^31
    long long n, nPad, totalRows;
    int nRanges, valueRows;
};

// rows[r][list[i]] = values[ranges[j].valueRow][i] for every j < nRanges, ranges[j].rowLo <= r < ranges[j].rowHi, i < count.
// Words move as 32-bit patterns; nothing but the named words is written.  An entry outside [0, n) and a range that names a value
// row or an event row outside its block are skipped.  The words of one launch are disjoint (the caller refuses an instance listed
// twice and a register named twice), and so are those of two launches between one hold and the block (no voice of a register
// belongs to two schedules): no atomics.
hipError_t launchTrackScatter(const TrackScatterArgs& a, hipStream_t stream);

}  // namespace fx
