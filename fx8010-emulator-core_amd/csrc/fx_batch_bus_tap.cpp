// fx_batch_bus_tap.cpp — the taps of bus blocks: the state of one batch (fx_batch.hpp "Bus taps", kernel: fx_bus_tap in
// fx_bus.hip, where it is launched: Batch::runBus).
//
// The list lives twice: on the host (tapList_ / tapPos_, what busGetTaps reads) and in one device block of 32-bit words (the
// instance numbers, then - for a shard of a larger handle - the column of the caller's row each of them goes to).  A set is two
// steps so that several shards can be all-or-nothing: busReserveTaps allocates the block of the set to come and touches nothing
// else, busSetTaps waits for everything queued on the handle (a queued block keeps the taps it was queued with), frees the old
// block, takes the reserved one and fills it with a synchronous copy.  Selections change at human rate: no double buffering.
// The only other allocations are the staging blocks of a pageable tap_out (planTapRoute), made in front of a block's first launch.
#include "fx_batch.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

const char* Batch::checkTapShape(const float* in, const float* out, const float* tapOut, size_t rows, int64_t total, unsigned flags, int64_t inWidth, int64_t inPitch,
                                 int64_t outWidth, int64_t outPitch) {
    if (!tapOut) return nullptr;
    if (total < 1) return "bus taps: tap_out given while taps are off (fxb_bus_set_taps)";
    if (!(flags & kBusMixOut)) return "bus taps: tap_out needs FXB_BUS_MIX_OUT (without it `out` holds every column)";
    if (rows == 0 || !in || !out) return nullptr;
    const char *t = reinterpret_cast<const char*>(tapOut), *x = reinterpret_cast<const char*>(in), *y = reinterpret_cast<const char*>(out);
    const size_t tapBytes = rows * (size_t)total * 4;
    const size_t inBytes = ((rows - 1) * (size_t)inPitch + (size_t)inWidth) * 4, outBytes = ((rows - 1) * (size_t)outPitch + (size_t)outWidth) * 4;
    if (!(t + tapBytes <= x || x + inBytes <= t) || !(t + tapBytes <= y || y + outBytes <= t)) return "bus taps: tap_out overlaps the input or the output";
    return nullptr;
}

int Batch::busReserveTaps(int64_t count) {
    (void)hipSetDevice(device_);
    if (count < 0 || count > kMaxTaps) return fail(FX_E_ARG, "bus taps: count out of range");
    busReleaseTaps();
    if (count == 0) return 0;
    const size_t words = (size_t)count * 2;   // (room for the columns, whether this set has them or not)
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&dTapReserved_), words * 4);
    if (e != hipSuccess) {
        dTapReserved_ = nullptr;
        return hipFail(hipErrorOutOfMemory, "hipMalloc bus tap list");
    }
    tapReservedWords_ = words;
    return 0;
}

void Batch::busReleaseTaps() {
    if (!dTapReserved_) return;
    (void)hipSetDevice(device_);
    (void)hipFree(dTapReserved_);
    dTapReserved_ = nullptr;
    tapReservedWords_ = 0;
}

int Batch::busSetTaps(const int64_t* list, const int64_t* pos, int64_t count, int64_t total) {
    (void)hipSetDevice(device_);
    if (count < 0 || total < count || total > kMaxTaps || (count > 0 && !list) || (count > 0 && !pos && total != count)) return fail(FX_E_ARG, "bus taps: count out of range or a null list");
    for (int64_t k = 0; k < count; ++k)
        if (list[k] < 0 || list[k] >= n_ || (pos && (pos[k] < 0 || pos[k] >= total))) return fail(FX_E_ARG, "bus taps: an entry outside 0..N-1");
    if (count > 0 && tapReservedWords_ < (size_t)count * 2) {
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
        const hipError_t e = hipMemcpy(dTapReserved_, words.data(), words.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hipFail(e, "bus taps: copying the list to the device");
    }
    (void)hipFree(dTap_);
    dTap_ = count > 0 ? dTapReserved_ : nullptr;
    if (count > 0) {
        dTapReserved_ = nullptr;
        tapReservedWords_ = 0;
    } else {
        busReleaseTaps();
    }
    tapList_.swap(newList);
    tapPos_.swap(newPos);
    tapTotal_ = total;
    if (total == 0) {   // off: the staging of pageable rows goes as well
        (void)hipFree(dTapStage_);
        dTapStage_ = nullptr;
        tapStageCap_ = 0;
        if (hTapStage_) (void)hipHostFree(hTapStage_);
        hTapStage_ = nullptr;
        hTapStageCap_ = 0;
    }
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

// Where the tap kernel of this block stores, decided - and everything it needs allocated - before the block's first launch.
int Batch::planTapRoute(float* tapOut, const void* devTap, size_t rows, TapRoute* route) {
    *route = TapRoute{};
    if (!tapOut || tapList_.empty()) return 0;   // (a shard that owns none of the entries launches nothing)
    if (devTap) {
        route->dst = static_cast<uint32_t*>(const_cast<void*>(devTap));
        route->pitch = tapTotal_;
        route->columns = !tapPos_.empty();
        return 0;
    }
    const size_t words = rows * tapList_.size();
    if (words > tapStageCap_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipFree(dTapStage_);
        dTapStage_ = nullptr;
        tapStageCap_ = 0;
        if (hipMalloc(reinterpret_cast<void**>(&dTapStage_), words * 4) != hipSuccess) {
            dTapStage_ = nullptr;
            return hipFail(hipErrorOutOfMemory, "hipMalloc bus tap staging");
        }
        tapStageCap_ = words;
    }
    if (!tapPos_.empty() && words > hTapStageCap_) {
        if (hTapStage_) (void)hipHostFree(hTapStage_);
        hTapStage_ = nullptr;
        hTapStageCap_ = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&hTapStage_), words * 4, hipHostMallocDefault) != hipSuccess) {
            hTapStage_ = nullptr;
            return hipFail(hipErrorOutOfMemory, "pinned staging of the bus taps");
        }
        hTapStageCap_ = words;
    }
    route->dst = dTapStage_;
    route->pitch = (int64_t)tapList_.size();
    route->columns = false;
    route->staged = true;
    return 0;
}

// the staged rows on their way out, behind the block on its stream: straight into the caller's rows where entry k is column k,
// else into the pinned block from which placeTapColumns puts every column in its place
hipError_t Batch::queueTapCopyOut(const TapRoute& route, float* tapOut, size_t rows, hipStream_t stream) {
    if (!route.staged) return hipSuccess;
    const size_t bytes = rows * tapList_.size() * 4;
    return hipMemcpyAsync(tapPos_.empty() ? static_cast<void*>(tapOut) : static_cast<void*>(hTapStage_), dTapStage_, bytes, hipMemcpyDeviceToHost, stream);
}

void Batch::placeTapColumns(const TapRoute& route, float* tapOut, size_t rows) {
    if (!route.staged || tapPos_.empty()) return;
    const size_t mine = tapList_.size();
    uint32_t* dst = reinterpret_cast<uint32_t*>(tapOut);
    for (size_t r = 0; r < rows; ++r)
        for (size_t k = 0; k < mine; ++k) dst[r * (size_t)tapTotal_ + (size_t)tapPos_[k]] = hTapStage_[r * mine + k];
}

}  // namespace fx
