// fx_batch_bus_send.cpp — the sends of bus blocks: the state of one batch (fx_batch.hpp "Bus sends", kernels: fx_bus_send_chunks
// and fx_bus_send_fold in fx_bus.hip, launched by launchSends from Batch::runBus).
//
// The structure lives twice: on the host (send_, what busGetSends reads - the weights a and b included) and in ONE device block
// of 32-bit words: the member numbers [E], the two gain blocks [C][E] whose roles swap from ramp to ramp like the bus gains'
// (sendRamp_, fx_batch_bus_side.hpp RampPair), the chunk table and the per-bus {first chunk, Q, column} table.  A set is two steps so that several shards can be all-or-nothing:
// busReserveSends allocates the block of the set to come and touches nothing else, busSetSends waits for everything queued on the
// handle (a queued block keeps the sends it was queued with), takes the reserved block and fills it with a synchronous copy.
// busSetSendGains waits the same way and copies into the gain block that becomes b: structures and send levels change at human
// rate, so there is no staging and no event of their own.  The only other allocations are the block of chunk sums and the staging
// of a pageable aux_out (planAuxRoute), both made in front of a block's first launch; the route, the copy-out and the placement of
// the columns are the shared side-row path of fx_batch_bus_side.cpp.
#include "fx_batch.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

const SideTexts Batch::kAuxTexts = {"bus sends: aux_out given while sends are off (fxb_bus_set_sends)",
                                     "bus sends: aux_out needs FXB_BUS_MIX_OUT (without it `out` holds every column)",
                                     "bus sends: aux_out overlaps the input, the output or the tap rows",
                                     "d_aux_out: not memory of this handle's device or device-visible host memory over the whole block",
                                     "hipMalloc bus send staging",
                                     "pinned staging of the bus sends"};

const char* Batch::checkAuxShape(const float* in, const float* out, const float* tapOut, const float* auxOut, size_t rows, int64_t buses, int64_t taps, unsigned flags,
                                 int64_t inWidth, int64_t inPitch, int64_t outWidth, int64_t outPitch) {
    const int64_t tapWidth = std::max<int64_t>(taps, 0);
    const Footprint others[3] = {{in, inWidth, inPitch}, {out, outWidth, outPitch}, {tapOut, tapWidth, tapWidth}};
    return checkSideShape(kAuxTexts, auxOut, rows, buses, flags, others, 3);
}

size_t Batch::SendSet::chunkCount() const {
    size_t chunks = 0;
    for (size_t j = 0; j + 1 < offsets.size(); ++j) chunks += (size_t)((offsets[j + 1] - offsets[j] + kSendChunk - 1) / kSendChunk);
    return chunks;
}

// words of the device block of a structure of `buses` buses, `entries` entries and `chunks` chunks
size_t Batch::sendBlockWords(int64_t buses, int64_t entries, size_t chunks) const {
    return (size_t)entries * (1 + 2 * (size_t)prog_.numChannels) + chunks * 2 + (size_t)buses * 3;
}

int Batch::busReserveSends(int64_t buses, int64_t entries, int64_t chunks) {
    (void)hipSetDevice(device_);
    if (buses < 0 || buses > kMaxSendBuses || entries < 0 || entries > kMaxSendEntries || chunks < 0) return fail(FX_E_ARG, "bus sends: counts out of range");
    return reserveBlock(sendBlock_, buses == 0 ? 0 : sendBlockWords(buses, entries, (size_t)chunks), "hipMalloc bus sends");
}

void Batch::busReleaseSends() { releaseBlock(sendBlock_); }

void Batch::freeSendBlocks() {
    freeBlock(sendPartial_, false);
    freeSideRows(auxRows_);
}

int Batch::busSetSends(SendSet&& set) {
    (void)hipSetDevice(device_);
    const int64_t buses = (int64_t)set.column.size(), entries = (int64_t)set.members.size();
    const size_t ch = (size_t)prog_.numChannels;
    if (set.totalBuses < buses || set.totalBuses > kMaxSendBuses || set.totalEntries < entries || set.totalEntries > kMaxSendEntries ||
        set.offsets.size() != (size_t)buses + 1 || set.first.size() != (size_t)buses || set.offsets.front() != 0 || set.offsets.back() != entries ||
        set.gain[0].size() != ch * (size_t)entries || (set.totalBuses == 0 && buses != 0))
        return fail(FX_E_ARG, "bus sends: a structure that does not hold together");
    for (int64_t j = 0; j < buses; ++j)
        if (set.offsets[(size_t)j + 1] < set.offsets[(size_t)j] || set.column[(size_t)j] < 0 || set.column[(size_t)j] >= set.totalBuses)
            return fail(FX_E_ARG, "bus sends: offsets must not decrease");
    for (int64_t m : set.members)
        if (m < 0 || m >= n_) return fail(FX_E_ARG, "bus sends: a member outside 0..N-1");
    const size_t chunks = set.chunkCount();
    const size_t words = sendBlockWords(buses, entries, chunks);
    if (buses > 0 && sendBlock_.reservedWords < words) {
        const int rc = busReserveSends(buses, entries, (int64_t)chunks);
        if (rc != 0) return rc;
    }
    // the image of the device block, on the host first: from here on nothing can run out of memory but these vectors (bad_alloc
    // leaves the handle as it was: nothing has been touched yet)
    std::vector<uint32_t> image(buses > 0 ? words : 0);
    size_t at = 0;
    const size_t offIdx = at;
    for (int64_t m : set.members) image[at++] = (uint32_t)m;
    const size_t offGain[2] = {at, at + ch * (size_t)entries};
    if (entries > 0) {
        std::memcpy(&image[offGain[0]], set.gain[0].data(), ch * (size_t)entries * 4);
        std::memcpy(&image[offGain[1]], set.gain[0].data(), ch * (size_t)entries * 4);
    }
    at += 2 * ch * (size_t)entries;
    const size_t offChunk = at, offBus = at + chunks * 2;
    size_t q = 0;
    for (int64_t j = 0; j < buses; ++j) {
        const int64_t lo = set.offsets[(size_t)j], hi = set.offsets[(size_t)j + 1];
        const size_t firstChunk = q;
        for (int64_t e = lo; e < hi; e += kSendChunk, ++q) {
            image[offChunk + q * 2] = (uint32_t)e;
            image[offChunk + q * 2 + 1] = (uint32_t)std::min<int64_t>(hi - e, kSendChunk);
        }
        image[offBus + (size_t)j * 3] = (uint32_t)firstChunk;
        image[offBus + (size_t)j * 3 + 1] = (uint32_t)(q - firstChunk);
        image[offBus + (size_t)j * 3 + 2] = (uint32_t)set.column[(size_t)j];
    }
    set.gain[1] = set.gain[0];
    const int rc = sync();   // (blocks queued with the old structure still read it)
    if (rc != 0) return rc;
    if (buses > 0) {
        const hipError_t e = hipMemcpy(sendBlock_.reserved, image.data(), words * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hipFail(e, "bus sends: copying the structure to the device");
    }
    takeUpBlock(sendBlock_, buses > 0);
    sendOff_[0] = offIdx;
    sendOff_[1] = offGain[0];
    sendOff_[2] = offGain[1];
    sendOff_[3] = offChunk;
    sendOff_[4] = offBus;
    sendChunks_ = (int64_t)chunks;
    sendIdentity_ = buses == set.totalBuses;
    for (int64_t j = 0; j < buses && sendIdentity_; ++j) sendIdentity_ = set.column[(size_t)j] == j;
    send_ = std::move(set);
    sendRamp_ = RampPair{};   // a = b, and a ramp that was waiting for its block is gone
    if (send_.totalBuses == 0) {
        send_ = SendSet{};
        freeSendBlocks();
    }
    return 0;
}

int Batch::busSetSendGains(const float* gains, int ramp) {
    (void)hipSetDevice(device_);
    if (ramp != 0 && ramp != 1) return fail(FX_E_ARG, "bus sends: ramp must be 0 or 1");
    if (send_.totalBuses < 1) return fail(FX_E_ARG, "bus sends: sends are off (fxb_bus_set_sends)");
    if (send_.totalEntries > 0 && !gains) return fail(FX_E_ARG, "null buffer");
    const size_t ch = (size_t)prog_.numChannels, mine = send_.members.size(), all = (size_t)send_.totalEntries;
    // this batch's entries of the caller's [C][E]: bus j's run begins at first[j] there and at offsets[j] here
    std::vector<float> next(ch * mine);
    for (size_t c = 0; c < ch; ++c)
        for (size_t j = 0; j < send_.column.size(); ++j) {
            const size_t lo = (size_t)send_.offsets[j], count = (size_t)send_.offsets[j + 1] - lo;
            if (count > 0) std::memcpy(&next[c * mine + lo], gains + c * all + (size_t)send_.first[j], count * 4);
        }
    const int rc = sync();   // (blocks queued with the old weights still read them)
    if (rc != 0) return rc;
    const int target = sendRamp_.writeTarget(ramp);   // (the state machine of the bus gains)
    if (mine > 0) {
        const hipError_t e = hipMemcpy(sendBlock_.cur + sendOff_[1 + target], next.data(), next.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hipFail(e, "bus sends: copying the gains to the device");
    }
    send_.gain[target].swap(next);
    sendRamp_ = RampPair{target, ramp != 0};
    return 0;
}

int64_t Batch::busGetSends(int64_t* offsets, int64_t offCap, int64_t* members, float* gains, int64_t cap, int64_t firstInstance) const {
    const size_t ch = (size_t)prog_.numChannels, mine = send_.members.size(), all = (size_t)send_.totalEntries;
    const std::vector<float>& g = send_.gain[sendRamp_.inForce()];
    for (size_t j = 0; j < send_.column.size(); ++j) {
        const int64_t lo = send_.offsets[j], hi = send_.offsets[j + 1], first = send_.first[j];
        if (offsets && send_.column[j] < offCap) offsets[send_.column[j]] = first;
        for (int64_t e = lo; e < hi && first + (e - lo) < cap; ++e) {
            const size_t to = (size_t)(first + (e - lo));
            if (members) members[to] = firstInstance + send_.members[(size_t)e];
            if (gains)
                for (size_t c = 0; c < ch; ++c) gains[c * all + to] = g[c * mine + (size_t)e];
        }
    }
    if (offsets && send_.totalBuses > 0 && send_.totalBuses < offCap) offsets[send_.totalBuses] = send_.totalEntries;
    return send_.totalEntries;
}

// Everything the sends of a block need, allocated before the block's first launch: the chunk sums of the largest piece, then the
// route of the aux rows (planSideRoute: for a pageable aux_out the compact staging rows).
int Batch::planAuxRoute(float* auxOut, const void* devAux, size_t rows, size_t pieceRows, Route* route) {
    *route = Route{};
    const size_t mine = send_.column.size();
    if (!auxOut || mine == 0) return 0;   // (a shard that owns none of the buses launches nothing)
    const size_t partial = pieceRows * (size_t)sendChunks_;
    if (partial > sendPartial_.cap) {
        if (busLaunched_) (void)hipEventSynchronize(evBus_);   // (a block on the caller's stream may still be working on the old one)
        (void)hipStreamSynchronize(stream_);
        const int rc = growBlock(sendPartial_, partial, false, "hipMalloc bus send chunk sums");
        if (rc != 0) return rc;
    }
    return planSideRoute(auxRows_, kAuxTexts, auxOut, devAux, rows, mine, send_.totalBuses, sendIdentity_ ? nullptr : send_.column.data(), route);
}

// the launch of one piece (Batch::runBus): rows [first, first + rows) of the block, sample0 the piece's first sample
hipError_t Batch::launchSends(const Route& route, size_t first, long long rows, int nSamples, int sample0, hipStream_t s) {
    BusSendArgs a{};
    const uint32_t* words = sendBlock_.cur;
    a.wide = bus_.p;
    a.idx = words + sendOff_[0];
    a.target = reinterpret_cast<const float*>(words + sendOff_[1 + sendRamp_.target]);
    a.current = sendRamp_.pending ? reinterpret_cast<const float*>(words + sendOff_[1 + (sendRamp_.target ^ 1)]) : nullptr;
    a.chunk = reinterpret_cast<const BusSendChunk*>(words + sendOff_[3]);
    a.bus = reinterpret_cast<const BusSendBus*>(words + sendOff_[4]);
    a.partial = sendPartial_.p;
    a.auxOut = reinterpret_cast<float*>(route.dst) + first * (size_t)route.pitch;
    a.rows = rows;
    a.n = n_;
    a.entries = (long long)send_.members.size();
    a.gainPitch = a.entries;
    a.chunks = sendChunks_;
    a.buses = (long long)send_.column.size();
    a.auxPitch = route.pitch;
    a.columns = route.columns ? 1 : 0;
    setRamp(a, sendRamp_, nSamples, sample0);
    return launchBusSend(a, s);
}

}  // namespace fx
