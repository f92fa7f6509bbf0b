// fx_batch_bus_gain_list.cpp — gain sets by list: the moved entries of the bus gains, the send gains or the feed gains of one
// batch, scattered on the device (include/fx8010_amd.h "Gain sets by list", kernel: fx_gain_scatter in fx_bus.hip).
//
// One path for the three calls (setGainList), told apart by a GainListTarget: the two device gain blocks, their row pitch, the
// RampPair that keeps their roles, and the host copy where the structure has one (send_.gain / feed_.gain, which busGetSends /
// busGetFeeds read).  A set copies the positions and the caller's columns into pinned staging (the caller's arrays are free on
// return) and queues on the handle's stream, behind evBus_ - every bus block queued so far, on whatever stream, keeps the weights
// it was queued with:
//   ramp, none pending     the blocks swap roles as in a full set; the block that becomes b holds stale words and first takes a
//                          device-to-device copy of the old b ("a := b everywhere"), then the scatter;
//   ramp, one pending      the scatter into b;
//   no ramp                the scatter into b, and into a as well while a ramp is pending (without one a counts as b and is
//                          not read); a pending ramp stays pending.
// Then the event a later block waits for: evGain_ for the bus gains (as behind a full set), evList_ for the sends and the feeds
// (runBus waits for it only while sideListCopied_).  The staging is reused, so a set first waits on the HOST for the previous
// list set's scatter - which waited for the block in front of it: two list sets behind one running block cost the caller the
// rest of that block, as two full gain sets do.  Nothing here allocates outside busReserveGainList.
#include "fx_batch.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

// The refusals that read nothing but the arguments (Sharded asks for the whole handle, before any shard is posted): every index
// in 0..range-1, no index twice (checkList), every value finite.
int Batch::checkGainList(const int64_t* list, int64_t count, int64_t range, const float* gains, int channels, const char* what, std::string* why) {
    const std::string name(what);
    if (count < 0) { *why = name + ": count < 0"; return FX_E_ARG; }
    if (count == 0) return 0;
    if (!list || !gains) { *why = name + ": a null list or null gains"; return FX_E_ARG; }
    const ListFault f = checkList(list, count, range, true);
    if (f.kind == ListFault::kOutside) { *why = listOutside(name, f, range); return FX_E_ARG; }
    if (f) { *why = name + ": index " + std::to_string(list[f.entry]) + " is listed more than once"; return FX_E_ARG; }
    if (!gainsFinite(gains, channels, count, count)) { *why = name + ": every gain must be finite"; return FX_E_ARG; }
    return 0;
}

int Batch::busReserveGainList(int64_t count) {
    (void)hipSetDevice(device_);
    // (the reserve step of the by-list frame, with this file's own event: the sets here are ordered behind evBus_ only)
    const size_t words = (size_t)std::max<int64_t>(count, 0) * ((size_t)prog_.numChannels + 1);
    static const char* const kTexts[3] = {"gain list event", "hipMalloc gain list staging", "pinned staging of the gain list"};
    return reserveListStage(gainList_, hGainList_, words, evList_, listCopied_, true, kTexts);
}

int Batch::setGainList(const GainListTarget& t, const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* gains, int ramp) {
    const size_t ch = (size_t)prog_.numChannels, k = (size_t)count, words = k * (ch + 1);
    if (words > gainList_.cap || words > hGainList_.cap || !evList_) return fail(FX_E_ARG, std::string(t.name) + ": no staging reserved (busReserveGainList)");
    hipError_t e = hipSuccess;
    if (k > 0) {
        if (listCopied_ && (e = hipEventSynchronize(evList_)) != hipSuccess) return hipFail(e, "gain list: waiting for the previous set");
        listCopied_ = false;
        uint32_t* stage = hGainList_.p;
        for (size_t i = 0; i < k; ++i) stage[i] = (uint32_t)list[i];
        for (size_t c = 0; c < ch; ++c) copyColumn(&stage[k * (1 + c)], gains + c * (size_t)total, pos, k, 4, false);
    }
    const bool swap = ramp != 0 && !t.ramp->pending;   // a := b everywhere: the old b becomes a, the other block takes its words and is b
    const int target = t.ramp->writeTarget(ramp);
    const bool both = ramp == 0 && t.ramp->pending;
    const size_t blockWords = ch * t.pitch;
    if (!swap && k == 0) return 0;
    if (busLaunched_ && (e = hipStreamWaitEvent(stream_, evBus_, 0)) != hipSuccess) return hipFail(e, "gain list: ordering behind the queued bus blocks");
    if (swap && blockWords > 0) e = hipMemcpyAsync(t.block[target], t.block[target ^ 1], blockWords * 4, hipMemcpyDeviceToDevice, stream_);
    if (e == hipSuccess && k > 0) e = hipMemcpyAsync(gainList_.p, hGainList_.p, words * 4, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess && k > 0) {
        GainScatterArgs a{};
        a.idx = gainList_.p;
        a.val = gainList_.p + k;
        a.b = t.block[target];
        a.a = both ? t.block[target ^ 1] : nullptr;
        a.count = count;
        a.pitch = (long long)t.pitch;
        a.channels = prog_.numChannels;
        e = launchGainScatter(a, stream_);
    }
    if (e == hipSuccess) e = hipEventRecord(evList_, stream_);
    if (e == hipSuccess && !t.side) e = hipEventRecord(evGain_, stream_);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream_);   // (nothing may still read the staging)
        return hipFail(e, "gain list: queueing the scatter");
    }
    if (k > 0) {
        ++gainListSets_;
        listCopied_ = true;
    }
    if (t.side) sideListCopied_ = true;
    else gainCopied_ = true;
    if (t.mirror) {
        if (swap) t.mirror[target] = t.mirror[target ^ 1];
        for (size_t c = 0; c < ch; ++c)
            for (size_t i = 0; i < k; ++i) {
                const float v = gains[c * (size_t)total + (size_t)(pos ? pos[i] : (int64_t)i)];
                t.mirror[target][c * t.mirrorPitch + (size_t)list[i]] = v;
                if (both) t.mirror[target ^ 1][c * t.mirrorPitch + (size_t)list[i]] = v;
            }
    }
    if (ramp) *t.ramp = RampPair{target, true};
    return 0;
}

int Batch::busSetGainsList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* gains, int ramp) {
    (void)hipSetDevice(device_);
    if (!gainsOn_) return fail(FX_E_ARG, "bus gains by list: gains are off (fxb_bus_set_gains)");
    const GainListTarget t{{reinterpret_cast<uint32_t*>(dGain_[0]), reinterpret_cast<uint32_t*>(dGain_[1])}, (size_t)n_, &gainRamp_, nullptr, 0, false, "bus gains by list"};
    return setGainList(t, list, pos, count, total, gains, ramp);
}

int Batch::busSetSendGainsList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* gains, int ramp) {
    (void)hipSetDevice(device_);
    if (send_.totalBuses < 1) return fail(FX_E_ARG, "bus send gains by list: sends are off (fxb_bus_set_sends)");
    const size_t mine = send_.members.size();
    uint32_t* words = sendBlock_.cur;
    const GainListTarget t{{words + sendOff_[1], words + sendOff_[2]}, mine, &sendRamp_, send_.gain, mine, true, "bus send gains by list"};
    return setGainList(t, list, pos, count, total, gains, ramp);
}

int Batch::busSetFeedGainsList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* gains, int ramp) {
    (void)hipSetDevice(device_);
    if (feed_.sources < 1) return fail(FX_E_ARG, "bus feed gains by list: feeds are off (fxb_bus_set_feeds)");
    // unweighted feeds become weighted first: both blocks hold 1.0f already (busSetFeeds / busSetFeedGains(null)), on the device
    // and on the host, and a block queued earlier keeps the unweighted launch it was queued with
    feed_.weighted = true;
    uint32_t* words = feedBlock_.cur;
    const GainListTarget t{{words + feedOff_[2], words + feedOff_[3]}, feedGainPitch_, &feedRamp_, feed_.gain, feed_.columns.size(), true, "bus feed gains by list"};
    return setGainList(t, list, pos, count, total, gains, ramp);
}

int64_t Batch::busSendLocalEntry(int64_t entry) const {
    // the last of this batch's buses whose run begins at or in front of the entry (the runs ascend with the bus numbers)
    const auto it = std::upper_bound(send_.first.begin(), send_.first.end(), entry);
    if (it == send_.first.begin()) return -1;
    const size_t j = (size_t)(it - send_.first.begin()) - 1;
    const int64_t at = entry - send_.first[j];
    return at < send_.offsets[j + 1] - send_.offsets[j] ? send_.offsets[j] + at : -1;
}

int64_t Batch::busFeedLocalEntry(int64_t entry) const {
    const int64_t at = entry - feed_.first;
    return at >= 0 && at < (int64_t)feed_.columns.size() ? at : -1;
}

}  // namespace fx
