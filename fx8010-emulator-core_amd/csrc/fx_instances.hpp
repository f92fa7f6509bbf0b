// fx_instances.hpp — launch interface of the kernels behind the per-instance state calls (fxb_copy_instances,
// fxb_reset_instances, fxb_save_instances, fxb_load_instances, fxb_load_instances_rotated; device code: fx_instances.hip).
//
// The state of one instance is W = stateRows + iSlots + xSlots 32-bit words, scattered over three transposed blocks:
//   word w < stateRows                    state[w][inst]                          (row pitch nPad)
//   word stateRows + s, s < iSlots        itram[inst / cols][s][inst % cols]      (cols = 64 * K instances of one wavefront tile)
//   word stateRows + iSlots + s           xtram[inst / cols][s][inst % cols]
// A RECORD is those W words packed in that order: what the whole-batch image (fx_batch.hpp SnapshotHeader) holds for the
// instance, column by column.  `gather` pulls the records of a list of instances out of the blocks, `scatter` puts records back.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fx {

struct InstArgs {
    uint32_t* state;          // [stateRows][nPad]
    uint32_t* itram;          // [waves][iSlots][cols]; may be null when iSlots == 0
    uint32_t* xtram;          // [waves][xSlots][cols]; may be null when xSlots == 0
    const long long* list;    // device memory: `count` instance numbers, each in [0, n)
    uint32_t* records;        // device memory: record k at records + k * recStride
    long long count;          // list entries, 1 .. 2^31 - 1
    long long recStride;      // words between two records (>= W); scatter only: 0 = every listed instance takes records[0 .. W)
    long long n, nPad;        // instances, and the pitch of a state row
    int stateRows, iSlots, xSlots;
    int cols;                 // 64, 128 or 256
    int skipLo, skipHi;       // scatter only: the state rows [skipLo, skipHi) keep what they hold (the delay-line positions at a reset)
};

inline long long instanceWords(const InstArgs& a) { return (long long)a.stateRows + a.iSlots + a.xSlots; }

// records[k][w] = word w of instance list[k].  Words move as 32-bit patterns.  Nothing but the listed instances is read, nothing
// but the `count` records is written.
hipError_t launchInstGather(const InstArgs& a, hipStream_t stream);

// word w of instance list[k] = records[k][w] (recStride 0: records[0][w]) for every w outside [skipLo, skipHi).  Nothing but the
// words of the listed instances is written: no column >= n, none of the padding up to nPad.  An instance listed twice would be
// written twice in no defined order - the caller refuses such lists.
hipError_t launchInstScatter(const InstArgs& a, hipStream_t stream);

// The scatter of fxb_load_instances_rotated: InstArgs as they are, and a rotation per record and delay line.
struct InstRotArgs {
    InstArgs base;            // recStride >= W (no broadcast record); skipLo / skipHi as for the scatter
    const int* rot;           // device memory: [count][2], the rotation of record k on iTRAM (rot[2k]) and xTRAM (rot[2k + 1])
    int iSize, xSize;         // slots 0 .. size - 1 of a line are a ring (size <= iSlots / xSlots; 0: the line is copied as it is)
};

// As launchInstScatter, except inside the rings: slot (j + d) mod size of instance list[k] = slot j of records[k], j = 0 .. size - 1,
// with d = that record's rotation on the line.  A rotation outside 0 .. size - 1 - the runtime computes them in that range - is
// taken as 0.  Slots from `size` on are copied as they are.
hipError_t launchInstScatterRot(const InstRotArgs& a, hipStream_t stream);

}  // namespace fx
