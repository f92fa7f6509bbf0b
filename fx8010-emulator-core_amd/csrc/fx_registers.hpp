// fx_registers.hpp — launch interface of the kernels behind the register calls by list (fxb_set_registers_list,
// fxb_get_registers_list; device code: fx_registers.hip).
//
// A register's values live in one row of the state block, state[row][instance] (row pitch nPad), so the words a list call moves
// are the crossing points of a few rows and a list of instances.  On the packed side they are values[key][entry]: the caller's
// [key][entry] order, one contiguous run of `count` words per key.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace fx {

struct RegListArgs {
    uint32_t* state;          // [stateRows][nPad]
    const long long* list;    // device memory: `count` instance numbers, each in [0, n)
    const int* rows;          // device memory: `nKeys` row numbers, each in [0, stateRows)
    uint32_t* values;         // device memory: [nKeys][count]; the scatter reads it, the gather writes it
    long long count;          // list entries, 1 .. 2^31 - 1
    long long n, nPad;        // instances, and the pitch of a state row
    int nKeys;                // 1 .. ; nKeys * count < 2^31
    int stateRows;
};

// state[rows[k]][list[i]] = values[k][i].  Words move as 32-bit patterns.  Nothing but the listed words is written: no column
// >= n, none of the padding up to nPad.  An instance listed twice, or a row listed twice, would be written twice in no defined
// order - the caller refuses such lists.
hipError_t launchRegScatter(const RegListArgs& a, hipStream_t stream);

// values[k][i] = state[rows[k]][list[i]].  Repeats are fine.  A word whose entry or row is out of range is left as it is.
hipError_t launchRegGather(const RegListArgs& a, hipStream_t stream);

}  // namespace fx
