// fx_batch_bus_side.cpp — what the modes of a bus block share (fx_batch_bus_side.hpp): the growth of a kept block, the reserved
// block of a two-step set, and the ONE path of a narrow side beside the mix - its refusals, its route, its copy-out and the
// placement of its columns.  The taps (fx_batch_bus_tap.cpp) and the sends (fx_batch_bus_send.cpp) each run it with a SideRows, a
// SideTexts and the counts of their list or structure; a further side output would do the same.
#include "fx_batch.hpp"

namespace fx {

// A block of at least `want` elements (of bytesEach bytes), called `name` in the error.  The old block goes first - whoever may
// still be working on it has been waited for by the caller - and FX_E_MEMORY leaves none.
int Batch::growBlock(void** p, size_t* cap, size_t want, size_t bytesEach, bool pinned, const char* name) {
    if (want <= *cap) return 0;
    if (!pinned) (void)hipFree(*p);
    else if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    if ((pinned ? hipHostMalloc(p, want * bytesEach, hipHostMallocDefault) : hipMalloc(p, want * bytesEach)) != hipSuccess) {
        *p = nullptr;
        return hipFail(hipErrorOutOfMemory, name);
    }
    *cap = want;
    return 0;
}

void Batch::freeBlock(void** p, size_t* cap, bool pinned) {
    if (!pinned) (void)hipFree(*p);
    else if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
}

int Batch::reserveBlock(ReservedBlock& b, size_t words, const char* name) {
    releaseBlock(b);
    if (words == 0) return 0;
    if (hipMalloc(reinterpret_cast<void**>(&b.reserved), words * 4) != hipSuccess) {
        b.reserved = nullptr;
        return hipFail(hipErrorOutOfMemory, name);
    }
    b.reservedWords = words;
    return 0;
}

void Batch::releaseBlock(ReservedBlock& b) {
    if (!b.reserved) return;
    (void)hipSetDevice(device_);
    (void)hipFree(b.reserved);
    b.reserved = nullptr;
    b.reservedWords = 0;
}

// any: the set to come has a block (the reserved one); else the batch holds none from here on
void Batch::takeUpBlock(ReservedBlock& b, bool any) {
    (void)hipFree(b.cur);
    b.cur = any ? b.reserved : nullptr;
    if (any) {
        b.reserved = nullptr;
        b.reservedWords = 0;
    } else {
        releaseBlock(b);
    }
}

void Batch::freeSideRows(SideRows& side) {
    freeBlock(side.dev, false);
    freeBlock(side.pinned, true);
}

// What a side's rows add to the refusals of the bus entries that read nothing but the arguments: null, or why not.  total: the
// width of the rows (0: the mode is off).
const char* Batch::checkSideShape(const SideTexts& texts, const float* sideOut, size_t rows, int64_t total, unsigned flags, const Footprint* others, int nOthers) {
    if (!sideOut) return nullptr;
    if (total < 1) return texts.off;
    if (!(flags & kBusMixOut)) return texts.needsMix;
    if (rows == 0) return nullptr;
    const char* a = reinterpret_cast<const char*>(sideOut);
    const size_t bytes = rows * (size_t)total * 4;
    for (int k = 0; k < nOthers; ++k) {
        const char* o = reinterpret_cast<const char*>(others[k].p);
        const size_t otherBytes = ((rows - 1) * (size_t)others[k].pitch + (size_t)others[k].width) * 4;
        if (o && !(a + bytes <= o || o + otherBytes <= a)) return texts.overlaps;
    }
    return nullptr;
}

// Where the kernel of a side stores in this block, decided - and everything it needs allocated - before the block's first launch.
// dev: the caller's rows as the device addresses them, or null (staged).  mine / place: this batch's entries and the column of the
// caller's [..][total] rows each of them goes to (null: entry k is column k)
int Batch::planSideRoute(SideRows& side, const SideTexts& texts, float* out, const void* dev, size_t rows, size_t mine, int64_t total, const int64_t* place, Route* route) {
    *route = Route{};
    if (!out || mine == 0) return 0;   // (a shard that owns none of the entries launches nothing)
    route->mine = mine;
    route->total = total;
    if (dev) {
        route->dst = static_cast<uint32_t*>(const_cast<void*>(dev));
        route->pitch = total;
        route->columns = place != nullptr;
        return 0;
    }
    const size_t words = rows * mine;
    int rc = 0;
    if (words > side.dev.cap) {
        (void)hipStreamSynchronize(stream_);
        if ((rc = growBlock(side.dev, words, false, texts.devStage)) != 0) return rc;
    }
    if (place && (rc = growBlock(side.pinned, words, true, texts.pinnedStage)) != 0) return rc;
    route->dst = side.dev.p;
    route->pitch = (int64_t)mine;
    route->staged = true;
    route->place = place;
    return 0;
}

// the staged rows on their way out, behind the block on its stream: straight into the caller's rows where entry k is column k,
// else into the pinned block from which placeSideColumns puts every column in its place
hipError_t Batch::queueSideCopyOut(const SideRows& side, const Route& route, float* out, size_t rows, hipStream_t stream) {
    if (!route.staged) return hipSuccess;
    return hipMemcpyAsync(route.place ? static_cast<void*>(side.pinned.p) : static_cast<void*>(out), side.dev.p, rows * route.mine * 4, hipMemcpyDeviceToHost, stream);
}

// behind the wait for that copy
void Batch::placeSideColumns(const SideRows& side, const Route& route, float* out, size_t rows) {
    if (!route.staged || !route.place) return;
    uint32_t* dst = reinterpret_cast<uint32_t*>(out);
    for (size_t r = 0; r < rows; ++r)
        for (size_t k = 0; k < route.mine; ++k) dst[r * (size_t)route.total + (size_t)route.place[k]] = side.pinned.p[r * route.mine + k];
}

}  // namespace fx
