// fx_batch_bus_side.hpp — the small state holders the modes of a bus block share (taps, sends, feeds, gains; fx_batch.hpp), and the ones
// the other block paths use with them.  Plain structs: what allocates or can fail is a member of Batch (fx_batch_bus_side.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace fx {

// a device (or pinned) block that is grown on demand and kept: Batch::growBlock
template <class T> struct Block {
    T* p = nullptr;
    size_t cap = 0;   // elements
};

// a caller's buffer that passed its addressability check, and the address the device takes for it: Batch::lookup.  A real-time
// caller pays for the runtime's lookups once
struct CheckedAddr {
    const void* host = nullptr;
    size_t bytes = 0;
    void* dev = nullptr;
    bool holds(const void* p, size_t n) const { return p == host && n <= bytes; }
    void forget() { host = nullptr; }
};

// one narrow side of a bus block beside the mix - the tap rows [S][C][T], the aux rows [S][C][A], 32-bit words either way: the
// staging of a pageable buffer (the compact [rows][entries of this batch] block on the device and, for a shard that places its
// columns on the host, the same block in pinned memory) and the last device-entry buffer that passed its check
struct SideRows {
    Block<uint32_t> dev, pinned;
    CheckedAddr checked;
};
// the texts of a side: what its refusals and its allocations are called
struct SideTexts {
    const char *off, *needsMix, *overlaps, *notAddressable, *devStage, *pinnedStage;
};
// where the kernel of a side stores in one block: the caller's rows as the device addresses them (pitch = the handle's total, at
// the columns of the device list where `columns`), or the compact staging block (`staged`; pitch = mine).  dst null: this batch
// launches nothing.  place: staged rows whose columns the host puts in their places behind the copy-out (null: entry k is column k)
struct Route {
    uint32_t* dst = nullptr;
    int64_t pitch = 0;
    bool columns = false, staged = false;
    size_t mine = 0;
    int64_t total = 0;
    const int64_t* place = nullptr;
};
// another footprint a side's rows must not meet: rows of `width` words at `pitch` (p null: none)
struct Footprint {
    const float* p;
    int64_t width, pitch;
};

// where the feed kernel of one block gathers from (Batch::planFeedRoute): the caller's source rows [rows][M] where they are
// memory of the device, else the device copy the runtime makes of them piece by piece
struct FeedRoute {
    const uint32_t* dev = nullptr;    // gathered in place; null: staged
    const float* host = nullptr;      // ... the caller's rows then
};

// the device block of a set in two steps, so that several shards can be all-or-nothing: Batch::reserveBlock allocates the block
// of the set to come and touches nothing else, releaseBlock drops a reservation that is not taken up, takeUpBlock frees the block
// in force and puts the reserved one in its place
struct ReservedBlock {
    uint32_t* cur = nullptr;
    uint32_t* reserved = nullptr;
    size_t reservedWords = 0;
};

// two gain blocks, one of them the target b, the other the current set a.  a is only meaningful while a ramp is pending: without
// one a counts as equal to b.  A ramp with none pending makes the old b the new a (the blocks swap roles); anything else replaces
// b where it is, and ramp = 0 drops a pending ramp.  A set that has landed assigns {writeTarget(ramp), ramp != 0}.
struct RampPair {
    int target = 0;
    bool pending = false;
    int writeTarget(int ramp) const { return (ramp && !pending) ? target ^ 1 : target; }
    int inForce() const { return pending ? target ^ 1 : target; }   // a while a ramp waits for its block, else b
    void consume() { pending = false; }                             // by a block that was fully queued: a counts as b from here on
};

}  // namespace fx
