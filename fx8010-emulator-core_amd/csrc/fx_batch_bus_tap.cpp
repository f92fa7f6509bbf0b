// fx_batch_bus_tap.cpp — the taps of bus blocks: the state of one batch (fx_batch.hpp "Bus taps", kernel: fx_bus_tap in
// fx_bus.hip, launched by launchTaps from Batch::runBus).
//
// The list lives twice: on the host (tapList_ / tapPos_, what busGetTaps reads) and in one device block of 32-bit words (the
// instance numbers, then - for a shard of a larger handle - the column of the caller's row each of them goes to).  A set is two
// steps so that several shards can be all-or-nothing: busReserveTaps allocates the block of the set to come and touches nothing
// else, busSetTaps waits for everything queued on the handle (a queued block keeps the taps it was queued with), frees the old
// block, takes the reserved one and fills it with a synchronous copy (fx_batch_bus_side.hpp ReservedBlock).  Selections change at
// human rate: no double buffering.  The only other allocations are the staging blocks of a pageable tap_out (planSideRoute on
// tapRows_), made in front of a block's first launch; the route, the copy-out and the placement of the columns are the shared
// side-row path of fx_batch_bus_side.cpp.
#include "fx_batch.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

const SideTexts Batch::kTapTexts = {"bus taps: tap_out given while taps are off (fxb_bus_set_taps)",
                                     "bus taps: tap_out needs FXB_BUS_MIX_OUT (without it `out` holds every column)",
                                     "bus taps: tap_out overlaps the input or the output",
                                     "d_tap_out: not memory of this handle's device or device-visible host memory over the whole block",
                                     "hipMalloc bus tap staging",
                                     "pinned staging of the bus taps"};

const char* Batch::checkTapShape(const float* in, const float* out, const float* tapOut, size_t rows, int64_t total, unsigned flags, int64_t inWidth, int64_t inPitch,
                                 int64_t outWidth, int64_t outPitch) {
    const Footprint others[2] = {{in, inWidth, inPitch}, {out, outWidth, outPitch}};
    return checkSideShape(kTapTexts, tapOut, rows, total, flags, others, in && out ? 2 : 0);
}

int Batch::busReserveTaps(int64_t count) {
    (void)hipSetDevice(device_);
    if (count < 0 || count > kMaxTaps) return fail(FX_E_ARG, "bus taps: count out of range");
    return reserveBlock(tap_, (size_t)count * 2, "hipMalloc bus tap list");   // (room for the columns, whether this set has them or not)
}

void Batch::busReleaseTaps() { releaseBlock(tap_); }

int Batch::busSetTaps(const int64_t* list, const int64_t* pos, int64_t count, int64_t total) {
    (void)hipSetDevice(device_);
    if (count < 0 || total < count || total > kMaxTaps || (count > 0 && !list) || (count > 0 && !pos && total != count)) return fail(FX_E_ARG, "bus taps: count out of range or a null list");
    for (int64_t k = 0; k < count; ++k)
        if (list[k] < 0 || list[k] >= n_ || (pos && (pos[k] < 0 || pos[k] >= total))) return fail(FX_E_ARG, "bus taps: an entry outside 0..N-1");
    if (count > 0 && tap_.reservedWords < (size_t)count * 2) {
        const int rc = busReserveTaps(count);
        if (rc != 0) return rc;
    }
    // the host's copies first: from here on nothing can run out of memory
    std::vector<int64_t> newList(list, list + count), newPos;
    if (pos) newPos.assign(pos, pos + count);
    std::vector<uint32_t> words((size_t)count + newPos.size());
    for (int64_t k = 0; k < count; ++k) words[(size_t)k] = (uint32_t)list[k];
    for (size_t k = 0; k < newPos.size(); ++k) words[(size_t)count + k] = (uint32_t)newPos[k];
    const int rc = sync();   // (blocks queued with the old list still read it)
    if (rc != 0) return rc;
    if (count > 0) {
        const hipError_t e = hipMemcpy(tap_.reserved, words.data(), words.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hipFail(e, "bus taps: copying the list to the device");
    }
    takeUpBlock(tap_, count > 0);
    tapList_.swap(newList);
    tapPos_.swap(newPos);
    tapTotal_ = total;
    if (total == 0) freeSideRows(tapRows_);   // off: the staging of pageable rows goes as well
    return 0;
}

int64_t Batch::busGetTaps(int64_t* list, int64_t cap, int64_t first) const {
    if (list)
        for (size_t k = 0; k < tapList_.size(); ++k) {
            const int64_t column = tapPos_.empty() ? (int64_t)k : tapPos_[k];
            if (column < cap) list[column] = first + tapList_[k];
        }
    return tapTotal_;
}

// the launch of one piece (Batch::runBus): rows [first, first + rows) of the block, read from the scratch where the emulation has
// just written it
hipError_t Batch::launchTaps(const Route& route, size_t first, long long rows, hipStream_t s) {
    BusTapArgs t{};
    t.wide = reinterpret_cast<const uint32_t*>(bus_.p);
    t.tapOut = route.dst + first * (size_t)route.pitch;
    t.idx = tap_.cur;
    t.col = route.columns ? tap_.cur + tapList_.size() : nullptr;
    t.rows = rows;
    t.n = n_;
    t.taps = tapCount();
    t.tapPitch = route.pitch;
    return launchBusTap(t, s);
}

}  // namespace fx
