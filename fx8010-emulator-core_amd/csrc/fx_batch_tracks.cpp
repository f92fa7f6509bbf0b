// fx_batch_tracks.cpp — the list schedules of one batch: per-voice changes of program parameters at given samples of the next
// block (include/fx8010_amd.h "Register tracks by list", fx_batch.hpp "Register tracks by list", kernels: fx_tracks.hip).
//
// Arming copies the caller's list, the columns of its values and the state rows of its registers into the pinned half of a staging
// pair and from there to the device on the handle's stream (evTrackCopy_ behind the copy); the caller's arrays are free on
// return.  It waits on the HOST only for the expansion that last read the staging (evTrackList_, recorded behind the last
// fx_track_scatter, not behind the block), and it is the call that allocates: the staging pair and the track buffer for every
// step of everything that is armed.  The listed values never pass through trackStage_.
//
// The translated tier expands the schedules at the head of the block (Batch::uploadTracks plans, expandTrackLists launches):
// header copy -> fx_track_hold -> fx_track_scatter per schedule -> the emulation kernel, all on the block's stream.  The other
// tiers cut the block (processWithTrackFallback) and apply the steps due at a cut through fx_reg_scatter reading the same
// staging (applyTrackListsAt), ordered like a register list set and without a host wait.
#include "fx_batch.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

bool Batch::listScheduled(int reg) const {
    for (const ListSchedule& s : listSchedules_)
        if (std::find(s.regs.begin(), s.regs.end(), reg) != s.regs.end()) return true;
    return false;
}

int Batch::checkTrackList(const std::vector<int>& regs, const int64_t* list, int64_t count, int64_t n, const float* values, int nSteps, int first, int period, std::string* why) {
    const std::string name("set_register_tracks_list");
    if (count < 0) { *why = name + ": count < 0"; return FX_E_ARG; }
    if (nSteps < 1 || period < 1 || first < 0) { *why = name + ": n_steps >= 1, period >= 1 and first >= 0 are required"; return FX_E_ARG; }
    if (count == 0 || regs.empty()) return 0;
    if (!list || !values) { *why = name + ": a null list or null values"; return FX_E_ARG; }
    if ((int64_t)nSteps * (int64_t)regs.size() >= ((int64_t)1 << 31) || count >= ((int64_t)1 << 31) || (int64_t)nSteps * (int64_t)regs.size() * count >= ((int64_t)1 << 31)) {
        *why = name + ": n_steps * n_keys * count must stay below 2^31";
        return FX_E_ARG;
    }
    // the list and the keys: what a register list set refuses
    return checkRegisterList("set_register_tracks_list", regs, list, count, n, values, true, why);
}

int Batch::checkTrackListArm(const std::vector<int>& regs, const int64_t* list, int64_t count, int64_t firstGlobal, std::string* why) {
    const std::string name("set_register_tracks_list");
    if (!dState_) { *why = "no program loaded"; return FX_E_NOTREADY; }
    if (listSchedules_.size() >= (size_t)kMaxListSchedules) { *why = name + ": at most " + std::to_string(kMaxListSchedules) + " list schedules can be armed"; return FX_E_ARG; }
    size_t fresh = 0;
    for (const int r : regs) {
        const std::string& reg = prog_.regs[(size_t)r].name;
        // "the others keep what they have" is a value known at the head of the block only for a register the program never changes
        if (intrinsicLane(r)) { *why = name + ": the program itself changes register '" + reg + "' (an instruction's result, the CCR, an input or an output)"; return FX_E_ARG; }
        const auto at = std::find(trackRegs_.begin(), trackRegs_.end(), r);
        if (at == trackRegs_.end()) ++fresh;
        else if (pendingTracks_[(size_t)(at - trackRegs_.begin())].steps > 0) { *why = name + ": register '" + reg + "' has a schedule armed through set_register_track"; return FX_E_ARG; }
    }
    if (trackRegs_.size() + fresh > (size_t)kMaxTracks) { *why = name + ": at most " + std::to_string(kMaxTracks) + " registers can have schedules"; return FX_E_ARG; }
    // each (register, voice) word belongs to one schedule
    for (const ListSchedule& s : listSchedules_) {
        if (s.list.empty() || count == 0) continue;
        int shared = -1;
        for (const int r : regs)
            if (std::find(s.regs.begin(), s.regs.end(), r) != s.regs.end()) shared = r;
        if (shared < 0) continue;
        std::vector<int64_t> sorted(s.list);
        std::sort(sorted.begin(), sorted.end());
        for (int64_t i = 0; i < count; ++i)
            if (std::binary_search(sorted.begin(), sorted.end(), list[i])) {
                *why = name + ": instance " + std::to_string(firstGlobal + list[i]) + " is already named by an armed list schedule of register '" + prog_.regs[(size_t)shared].name + "'";
                return FX_E_ARG;
            }
    }
    return 0;
}

// what uploadTracks can need at most for everything that is armed (and `moreSteps` steps of each of `moreRegs` on top): every step
// inside the block.  Events, the values of the dense schedules, the ranges, the event rows.
size_t Batch::trackBufferWorstBytes(const std::vector<int>* moreRegs, int moreSteps) const {
    size_t events = 0, denseWords = 0, listSteps = moreRegs ? moreRegs->size() * (size_t)moreSteps : 0;
    for (const PendingTrack& t : pendingTracks_) {
        if (t.steps <= 0) continue;
        events += (size_t)t.steps;
        denseWords += t.perInstance ? (size_t)t.steps * (size_t)nPad_ : (size_t)t.steps;
    }
    for (const ListSchedule& s : listSchedules_) listSteps += s.regs.size() * (size_t)s.steps;
    const size_t header = (((events + listSteps + 1) * 4 + denseWords) + 3) & ~(size_t)3;
    return (header + listSteps * 4 + listSteps * (size_t)nPad_) * 4 + 256;
}

int Batch::growTrackBuffer(size_t bytes) {
    if (bytes <= tracksCap_) return 0;
    // (a TrackEvent names its value by a 32-bit byte offset)
    if (bytes >= ((size_t)1 << 32)) return fail(FX_E_MEMORY, "tracks: the event rows of everything armed would pass 4 GiB");
    uint32_t* grown = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&grown), bytes) != hipSuccess) return hipFail(hipErrorOutOfMemory, "hipMalloc tracks");
    waitLastLaunch();   // (the previous block may still be reading the buffer that goes)
    (void)hipFree(dTracks_);
    dTracks_ = grown;
    tracksCap_ = bytes;
    tracksClear_ = false;   // (no header yet)
    return 0;
}

int Batch::reserveTrackList(const std::vector<int>& regs, int64_t count, int nSteps) {
    (void)hipSetDevice(device_);
    if (regs.empty()) return 0;
    for (hipEvent_t* ev : {&evInst_, &evTrackCopy_, &evTrackList_})
        if (!*ev && hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess) { *ev = nullptr; return hipFail(hipErrorOutOfMemory, "register tracks by list: event"); }
    const size_t need = trackListUsed_ + (count > 0 ? trackListPartWords(regs.size(), count, nSteps) : 0);
    if (need > hTrackList_.cap || need > trackList_.cap) {
        // whoever reads the blocks that go: the last expansion, the copies of the parts armed so far
        if (trackListBusy_ && hipEventSynchronize(evTrackList_) == hipSuccess) trackListBusy_ = false;
        if (trackListUsed_ > 0) (void)hipEventSynchronize(evTrackCopy_);
        const size_t want = need + need / 2;
        // the new pair first: a failure leaves the old one, and what is armed in it, as it is
        uint32_t *host = nullptr, *dev = nullptr;
        if (hipHostMalloc(reinterpret_cast<void**>(&host), want * 4, hipHostMallocDefault) != hipSuccess) return hipFail(hipErrorOutOfMemory, "pinned staging of the register tracks by list");
        if (hipMalloc(reinterpret_cast<void**>(&dev), want * 4) != hipSuccess) {
            (void)hipHostFree(host);
            return hipFail(hipErrorOutOfMemory, "hipMalloc register tracks by list staging");
        }
        if (trackListUsed_ > 0) {
            std::memcpy(host, hTrackList_.p, trackListUsed_ * 4);
            hipError_t e = hipMemcpyAsync(dev, host, trackListUsed_ * 4, hipMemcpyHostToDevice, stream_);
            if (e == hipSuccess) e = hipEventRecord(evTrackCopy_, stream_);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(stream_);
                (void)hipHostFree(host);
                (void)hipFree(dev);
                return hipFail(e, "register tracks by list: moving the staging");
            }
        }
        freeBlock(hTrackList_, true);
        freeBlock(trackList_, false);
        hTrackList_.p = host;
        trackList_.p = dev;
        hTrackList_.cap = trackList_.cap = want;
    }
    return growTrackBuffer(trackBufferWorstBytes(&regs, nSteps));
}

int Batch::armTrackList(const std::vector<int>& regs, const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* values, int nSteps, int first, int period) {
    (void)hipSetDevice(device_);
    if (!dState_) return fail(FX_E_NOTREADY, "no program loaded");
    if (regs.empty()) return 0;
    ListSchedule sch;
    sch.regs = regs;
    sch.steps = nSteps;
    sch.first = first;
    sch.period = period;
    sch.at = trackListUsed_;
    size_t part = 0;
    if (count > 0) {
        const size_t k = (size_t)count, nk = regs.size();
        part = trackListPartWords(nk, count, nSteps);
        if (sch.at + part > hTrackList_.cap || sch.at + part > trackList_.cap || !evTrackCopy_ || !evTrackList_) return fail(FX_E_ARG, "register tracks by list: no staging reserved (reserveTrackList)");
        if (trackListBusy_) {
            const hipError_t e = hipEventSynchronize(evTrackList_);
            if (e != hipSuccess) return hipFail(e, "register tracks by list: waiting for the previous expansion");
            trackListBusy_ = false;
        }
        sch.list.assign(list, list + count);
        uint32_t* stage = hTrackList_.p + sch.at;
        static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == 4, "track list staging");
        std::memcpy(stage, list, k * 8);
        uint32_t* v = stage + k * 2;
        for (size_t row = 0; row < (size_t)nSteps * nk; ++row) copyColumn(&v[row * k], values + row * (size_t)total, pos, k, 4, false);
        std::memcpy(v + (size_t)nSteps * nk * k, regs.data(), nk * 4);   // (a register's row is its number: StateLayout)
        if (part > k * 2 + (size_t)nSteps * nk * k + nk) stage[part - 1] = 0;
        hipError_t e = hipMemcpyAsync(trackList_.p + sch.at, stage, part * 4, hipMemcpyHostToDevice, stream_);
        if (e == hipSuccess) e = hipEventRecord(evTrackCopy_, stream_);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(stream_);   // (nothing may still read the staging)
            return hipFail(e, "register tracks by list: queueing the copy");
        }
    }
    // the first schedule of a register makes it trackable (setRegisterTrack): other code, once
    for (const int r : regs) {
        size_t slot = 0;
        while (slot < trackRegs_.size() && trackRegs_[slot] != r) ++slot;
        if (slot == trackRegs_.size()) {
            coldSetChanged();
            trackRegs_.push_back(r);
            pendingTracks_.resize(trackRegs_.size());
            lowDirty_ = true;
        }
        sch.slots.push_back((int)slot);
    }
    trackListUsed_ += part;
    listSchedules_.push_back(std::move(sch));
    return 0;
}

int Batch::clearTrackLists() {
    // (copies of the parts that go may still be running: they read the pinned half, which stays as it is until the next arming)
    listSchedules_.clear();
    trackListUsed_ = 0;
    return 0;
}

int Batch::finishTrackLists(hipStream_t s, bool launched) {
    listSchedules_.clear();
    trackListUsed_ = 0;
    if (!launched) return 0;
    const hipError_t e = hipEventRecord(evTrackList_, s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);   // (nothing may still read the staging)
        return hipFail(e, "register tracks by list: the event behind the expansion");
    }
    trackListBusy_ = true;
    return 0;
}

int Batch::expandTrackLists(const ListExpansion& x, hipStream_t s) {
    if (x.totalRows == 0) return 0;
    hipError_t e = hipStreamWaitEvent(s, evTrackCopy_, 0);   // the parts armed on the handle's stream
    TrackHoldArgs h = x.hold;
    h.state = dState_;
    h.rows = dTracks_ + x.rowsAt;
    h.nPad = nPad_;
    h.totalRows = (long long)x.totalRows;
    h.stateRows = stateRows_;
    if (e == hipSuccess) e = launchTrackHold(h, s);
    for (size_t j = 0; j < x.launches.size() && e == hipSuccess; ++j) {
        const ListSchedule& sch = listSchedules_[x.launches[j].schedule];
        TrackScatterArgs a{};
        a.rows = h.rows;
        a.list = reinterpret_cast<const long long*>(trackList_.p + sch.at);   // (hipMalloc aligns the block, every part is an even number of words)
        a.values = trackList_.p + sch.valuesAt();
        a.ranges = reinterpret_cast<const TrackRange*>(dTracks_ + x.launches[j].rangesAt);
        a.count = sch.count();
        a.n = n_;
        a.nPad = nPad_;
        a.totalRows = (long long)x.totalRows;
        a.nRanges = x.launches[j].nRanges;
        a.valueRows = sch.steps * (int)sch.regs.size();
        e = launchTrackScatter(a, s);
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        return hipFail(e, "register tracks by list: queueing the expansion");
    }
    ++trackListExpands_;
    return 0;
}

// the steps due at `sample`, in arming order, through the scatter of the register list sets and in their place in the by-list frame
// (setRegistersList; nothing to stage, so no host wait): behind every block queued so far, in front of evInst_
int Batch::applyTrackListsAt(std::vector<ListSchedule>& schedules, int sample) {
    for (const ListSchedule& sch : schedules) {
        if (sch.list.empty() || sample < sch.first || (sample - sch.first) % sch.period != 0 || (sample - sch.first) / sch.period >= sch.steps) continue;
        const size_t q = (size_t)((sample - sch.first) / sch.period), nk = sch.regs.size(), k = sch.list.size();
        RegListArgs a{};
        a.state = dState_;
        a.list = reinterpret_cast<const long long*>(trackList_.p + sch.at);
        a.values = trackList_.p + sch.valuesAt() + q * nk * k;
        a.rows = reinterpret_cast<const int*>(trackList_.p + sch.rowsAt());
        a.count = sch.count();
        a.n = n_;
        a.nPad = nPad_;
        a.nKeys = (int)nk;
        a.stateRows = stateRows_;
        hipError_t e = orderBehindQueuedBlocks();
        if (e == hipSuccess) e = launchRegScatter(a, stream_);
        if (const int failed = closeInstCall(e, "register tracks by list: queueing a step")) return failed;
        noteRegistersWritten(sch.regs);
    }
    return 0;
}

}  // namespace fx
