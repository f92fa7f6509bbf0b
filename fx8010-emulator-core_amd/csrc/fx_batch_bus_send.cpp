// fx_batch_bus_send.cpp — the sends of bus blocks: the state of one batch (fx_batch.hpp "Bus sends", kernels: fx_bus_send_chunks
// and fx_bus_send_fold in fx_bus.hip, where they are launched: Batch::runBus).
//
// The structure lives twice: on the host (send_, what busGetSends reads - the weights a and b included) and in ONE device block
// of 32-bit words: the member numbers [E], the two gain blocks [C][E] whose roles swap from ramp to ramp like the bus gains', the
// chunk table and the per-bus {first chunk, Q, column} table.  A set is two steps so that several shards can be all-or-nothing:
// busReserveSends allocates the block of the set to come and touches nothing else, busSetSends waits for everything queued on the
// handle (a queued block keeps the sends it was queued with), takes the reserved block and fills it with a synchronous copy.
// busSetSendGains waits the same way and copies into the gain block that becomes b: structures and send levels change at human
// rate, so there is no staging and no event of their own.  The only other allocations are the block of chunk sums and the staging
// of a pageable aux_out (planAuxRoute), both made in front of a block's first launch.
#include "fx_batch.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

const char* Batch::checkAuxShape(const float* in, const float* out, const float* tapOut, const float* auxOut, size_t rows, int64_t buses, int64_t taps, unsigned flags,
                                 int64_t inWidth, int64_t inPitch, int64_t outWidth, int64_t outPitch) {
    if (!auxOut) return nullptr;
    if (buses < 1) return "bus sends: aux_out given while sends are off (fxb_bus_set_sends)";
    if (!(flags & kBusMixOut)) return "bus sends: aux_out needs FXB_BUS_MIX_OUT (without it `out` holds every column)";
    if (rows == 0) return nullptr;
    const char* a = reinterpret_cast<const char*>(auxOut);
    const size_t auxBytes = rows * (size_t)buses * 4;
    auto meets = [&](const float* other, size_t bytes) {
        const char* o = reinterpret_cast<const char*>(other);
        return other && !(a + auxBytes <= o || o + bytes <= a);
    };
    if (meets(in, ((rows - 1) * (size_t)inPitch + (size_t)inWidth) * 4) || meets(out, ((rows - 1) * (size_t)outPitch + (size_t)outWidth) * 4) ||
        meets(tapOut, rows * (size_t)std::max<int64_t>(taps, 0) * 4))
        return "bus sends: aux_out overlaps the input, the output or the tap rows";
    return nullptr;
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
    busReleaseSends();
    if (buses == 0) return 0;
    const size_t words = sendBlockWords(buses, entries, (size_t)chunks);
    if (hipMalloc(reinterpret_cast<void**>(&dSendReserved_), words * 4) != hipSuccess) {
        dSendReserved_ = nullptr;
        return hipFail(hipErrorOutOfMemory, "hipMalloc bus sends");
    }
    sendReservedWords_ = words;
    return 0;
}

void Batch::busReleaseSends() {
    if (!dSendReserved_) return;
    (void)hipSetDevice(device_);
    (void)hipFree(dSendReserved_);
    dSendReserved_ = nullptr;
    sendReservedWords_ = 0;
}

void Batch::freeSendBlocks() {
    (void)hipFree(dSendPartial_);
    dSendPartial_ = nullptr;
    sendPartialCap_ = 0;
    (void)hipFree(dAuxStage_);
    dAuxStage_ = nullptr;
    auxStageCap_ = 0;
    if (hAuxStage_) (void)hipHostFree(hAuxStage_);
    hAuxStage_ = nullptr;
    hAuxStageCap_ = 0;
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
    if (buses > 0 && sendReservedWords_ < words) {
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
        const hipError_t e = hipMemcpy(dSendReserved_, image.data(), words * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hipFail(e, "bus sends: copying the structure to the device");
    }
    (void)hipFree(dSend_);
    dSend_ = buses > 0 ? dSendReserved_ : nullptr;
    dSendReserved_ = nullptr;
    sendReservedWords_ = 0;
    if (buses == 0) busReleaseSends();
    sendOff_[0] = offIdx;
    sendOff_[1] = offGain[0];
    sendOff_[2] = offGain[1];
    sendOff_[3] = offChunk;
    sendOff_[4] = offBus;
    sendChunks_ = (int64_t)chunks;
    sendIdentity_ = buses == set.totalBuses;
    for (int64_t j = 0; j < buses && sendIdentity_; ++j) sendIdentity_ = set.column[(size_t)j] == j;
    send_ = std::move(set);
    sendTarget_ = 0;
    sendRampPending_ = false;   // a = b, and a ramp that was waiting for its block is gone
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
    for (float g : next)
        if (!std::isfinite(g)) return fail(FX_E_ARG, "bus sends: every gain must be finite");
    const int rc = sync();   // (blocks queued with the old weights still read them)
    if (rc != 0) return rc;
    // the state machine of the bus gains: a ramp with none pending makes the old b the new a (the blocks swap roles); anything
    // else replaces b where it is, and ramp = 0 drops a pending ramp
    const int target = (ramp && !sendRampPending_) ? sendTarget_ ^ 1 : sendTarget_;
    if (mine > 0) {
        const hipError_t e = hipMemcpy(dSend_ + sendOff_[1 + target], next.data(), next.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hipFail(e, "bus sends: copying the gains to the device");
    }
    send_.gain[target].swap(next);
    sendTarget_ = target;
    sendRampPending_ = ramp != 0;
    return 0;
}

int64_t Batch::busGetSends(int64_t* offsets, int64_t offCap, int64_t* members, float* gains, int64_t cap, int64_t firstInstance) const {
    const size_t ch = (size_t)prog_.numChannels, mine = send_.members.size(), all = (size_t)send_.totalEntries;
    // the gains in force: a while a ramp waits for its block, else b
    const std::vector<float>& g = send_.gain[sendRampPending_ ? sendTarget_ ^ 1 : sendTarget_];
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

// Where the fold kernel of this block stores, decided - and everything the sends of the block need allocated - before the block's
// first launch: the chunk sums of the largest piece, and for a pageable aux_out the compact staging rows.
int Batch::planAuxRoute(float* auxOut, const void* devAux, size_t rows, size_t pieceRows, AuxRoute* route) {
    *route = AuxRoute{};
    const size_t mine = send_.column.size();
    if (!auxOut || mine == 0) return 0;   // (a shard that owns none of the buses launches nothing)
    const size_t partial = pieceRows * (size_t)sendChunks_;
    if (partial > sendPartialCap_) {
        if (busLaunched_) (void)hipEventSynchronize(evBus_);   // (a block on the caller's stream may still be working on the old one)
        (void)hipStreamSynchronize(stream_);
        (void)hipFree(dSendPartial_);
        dSendPartial_ = nullptr;
        sendPartialCap_ = 0;
        if (hipMalloc(reinterpret_cast<void**>(&dSendPartial_), partial * 4) != hipSuccess) {
            dSendPartial_ = nullptr;
            return hipFail(hipErrorOutOfMemory, "hipMalloc bus send chunk sums");
        }
        sendPartialCap_ = partial;
    }
    if (devAux) {
        route->dst = static_cast<float*>(const_cast<void*>(devAux));
        route->pitch = send_.totalBuses;
        route->columns = !sendIdentity_;
        return 0;
    }
    const size_t words = rows * mine;
    if (words > auxStageCap_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipFree(dAuxStage_);
        dAuxStage_ = nullptr;
        auxStageCap_ = 0;
        if (hipMalloc(reinterpret_cast<void**>(&dAuxStage_), words * 4) != hipSuccess) {
            dAuxStage_ = nullptr;
            return hipFail(hipErrorOutOfMemory, "hipMalloc bus send staging");
        }
        auxStageCap_ = words;
    }
    if (!sendIdentity_ && words > hAuxStageCap_) {
        if (hAuxStage_) (void)hipHostFree(hAuxStage_);
        hAuxStage_ = nullptr;
        hAuxStageCap_ = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&hAuxStage_), words * 4, hipHostMallocDefault) != hipSuccess) {
            hAuxStage_ = nullptr;
            return hipFail(hipErrorOutOfMemory, "pinned staging of the bus sends");
        }
        hAuxStageCap_ = words;
    }
    route->dst = dAuxStage_;
    route->pitch = (int64_t)mine;
    route->columns = false;
    route->staged = true;
    return 0;
}

// the staged rows on their way out, behind the block on its stream: straight into the caller's rows where bus j is column j,
// else into the pinned block from which placeAuxColumns puts every column in its place
hipError_t Batch::queueAuxCopyOut(const AuxRoute& route, float* auxOut, size_t rows, hipStream_t stream) {
    if (!route.staged) return hipSuccess;
    const size_t bytes = rows * send_.column.size() * 4;
    return hipMemcpyAsync(sendIdentity_ ? static_cast<void*>(auxOut) : static_cast<void*>(hAuxStage_), dAuxStage_, bytes, hipMemcpyDeviceToHost, stream);
}

void Batch::placeAuxColumns(const AuxRoute& route, float* auxOut, size_t rows) {
    if (!route.staged || sendIdentity_) return;
    const size_t mine = send_.column.size();
    for (size_t r = 0; r < rows; ++r)
        for (size_t j = 0; j < mine; ++j) std::memcpy(auxOut + r * (size_t)send_.totalBuses + (size_t)send_.column[j], hAuxStage_ + r * mine + j, 4);
}

// the launch of one piece (Batch::runBus): rows [first, first + rows) of the block, sample0 the piece's first sample
hipError_t Batch::launchSends(const AuxRoute& route, size_t first, long long rows, int nSamples, int sample0, hipStream_t s) {
    BusSendArgs a{};
    const uint32_t* words = dSend_;
    a.wide = dBus_;
    a.idx = words + sendOff_[0];
    a.target = reinterpret_cast<const float*>(words + sendOff_[1 + sendTarget_]);
    a.current = sendRampPending_ ? reinterpret_cast<const float*>(words + sendOff_[1 + (sendTarget_ ^ 1)]) : nullptr;
    a.chunk = reinterpret_cast<const BusSendChunk*>(words + sendOff_[3]);
    a.bus = reinterpret_cast<const BusSendBus*>(words + sendOff_[4]);
    a.partial = dSendPartial_;
    a.auxOut = route.dst + first * (size_t)route.pitch;
    a.rows = rows;
    a.n = n_;
    a.entries = (long long)send_.members.size();
    a.gainPitch = a.entries;
    a.chunks = sendChunks_;
    a.buses = (long long)send_.column.size();
    a.auxPitch = route.pitch;
    a.columns = route.columns ? 1 : 0;
    a.channels = prog_.numChannels;
    a.ramp = sendRampPending_ ? 1 : 0;
    a.r = 1.0f / (float)nSamples;   // the one division of the definition: S is the caller's block, never a piece
    a.samples = nSamples;
    a.sample0 = sample0;
    return launchBusSend(a, s);
}

}  // namespace fx
