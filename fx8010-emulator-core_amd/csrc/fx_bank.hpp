// fx_bank.hpp — launch interface of the kernels behind the record bank (fxb_bank_store, fxb_bank_recall; device code:
// fx_bank.hip).  A BANK is nSlots packed records of W words (fx_instances.hpp has the record): slot s is bank[s * W .. s * W + W).
// The kernels are those of fx_instances.hip with the packed side addressed through a slot list, and one more that works out the
// rotations of a recall on the device.
//
// A list entry of these calls is a pair of 64-bit words: the instance number, and the SLOT WORD - the slot in its low 32 bits, the
// caller's number of the entry in its high 32 bits (a shard's entries are a part of the caller's list; a refusal names the latter).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "fx_instances.hpp"

namespace fx {

// why the device refused a record of a recall (include/fx8010_amd.h FXB_BANK_*)
enum BankFault { kBankBadPosition = 1, kBankPhase = 2, kBankNoRing = 3 };

// the cells of a bank, 64-bit words in device memory.  kBankCellFaults / kBankCellLowest belong to the call that is running: the
// runtime zeroes both in front of fx_bank_rotations.  The other three are kept from call to call until the host resets them.
enum BankCell {
    kBankCellFaults = 0,    // bad (entry, line) pairs of this call
    kBankCellLowest = 1,    // ~key of the lowest one, raised with atomicMax; key = entry << 3 | line << 2 | BankFault
    kBankCellRefused = 2,   // recalls refused so far
    kBankCellLastKey = 3,   // key of the most recent refused recall
    kBankCellLastCall = 4,  // ... and its serial number (BankRotArgs::serial)
    kBankCells = 8
};

struct BankArgs {
    InstArgs base;                 // list / count: the instances; records and recStride are not used (the bank is the packed side)
    uint32_t* bank;                // [nSlots][W]
    const long long* slots;        // device memory: `count` slot words
    long long nSlots;
};

// bank[slot[k]][w] = word w of instance list[k].  Slots must not repeat (the runtime refuses such lists).
hipError_t launchBankGather(const BankArgs& a, hipStream_t stream);

// a delay line as the rotation rule sees it (Batch::RingLine)
struct BankLine {
    int size;                      // Z
    int slots;                     // allocated slots; 0: the program has no memory on this line
    int ring;                      // slots == size
    int writes, reads;             // which position kinds the program has an instruction of
};

struct BankRotArgs {
    BankArgs bank;
    BankLine line[2];              // iTRAM, xTRAM
    int cursorBase;                // state row of the first of the four position words
    int dane;                      // one counter per line, in the write word
    int* pairs;                    // device memory: [count][2], written by fx_bank_rotations, read by fx_bank_scatter_rot; null: no
                                   // rotation, no gate, no row skipped - the plain scatter of a program without delay-line instructions
    unsigned long long* cells;     // device memory: kBankCells words
    long long serial;              // which recall of the handle this is
};

// pairs[k] = the rotations of the record in slot[k] towards instance list[k] (Batch::recordRotations has the rule), from the
// record's position words in the bank and the position rows of the batch as the kernel finds them.  A record the rule refuses
// gets the pair (0, 0), adds one to cells[kBankCellFaults] and raises cells[kBankCellLowest].
hipError_t launchBankRotations(const BankRotArgs& a, hipStream_t stream);

// launchInstScatterRot with records[k] = bank[slot[k]] and rot = pairs.  With cells[kBankCellFaults] != 0 no workgroup stores a
// word of the batch; the first one notes the refusal in the kept cells.
hipError_t launchBankScatterRot(const BankRotArgs& a, hipStream_t stream);

}  // namespace fx
