// fx_batch_meter_list.cpp — the meter queries by list of one batch: the instances whose meter passes a threshold, compacted on
// the device into an ascending list; the accumulators of listed instances gathered, and zeroed (include/fx8010_amd.h "Meter
// queries by list", fx_batch.hpp "Meter queries by list", kernels: fx_meter_list.hip).
//
// The select and the list read are synchronous: they wait as sync() does - which covers a list reset still in flight - launch on
// the handle's stream and wait for it.  The list reset runs inside the by-list frame (fx_batch.hpp "THE BY-LIST
// FRAME", fx_batch_list.cpp): the list is staged, fx_meter_zero is the kernel in front of evInst_.
//
// One staging pair of 64-bit words serves the three calls - none of them can find it in use: the synchronous two have drained
// everything, the reset waits for evInst_ first.  A select lays it out as [chunk counts / offsets][the total][the list], so that
// the total and the head of the list come back in one copy; a list call as [the list][the packed rows].  meterSamples_ and the
// host's view of everything else stay as they are: the list calls touch accumulator words only.
#include "fx_batch.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

namespace {
// entries of a select's list that travel with the total in the first copy
constexpr int64_t kSelectHead = 4096;
size_t selectWords(int64_t nRange, int64_t cap) { return (size_t)meterSelectChunks(nRange) + 1 + (size_t)std::min(cap, nRange); }
size_t listWords(int channels, int64_t count, bool gather) { return (size_t)count + (gather ? (meterPackedBytes(channels, count) + 7) / 8 : 0); }
}  // namespace

int Batch::checkMeterSelect(int stat, double threshold, int64_t first, int64_t nRange, int64_t n, const int64_t* list, int64_t cap, unsigned flags, std::string* why) {
    if (stat < FXB_METER_ENERGY || stat > FXB_METER_NONFINITE) { *why = "meter_select: stat must be 0..3 (FXB_METER_ENERGY .. FXB_METER_NONFINITE)"; return FX_E_ARG; }
    if (flags & ~(unsigned)FXB_METER_BELOW) { *why = "meter_select: flags has an unknown bit"; return FX_E_ARG; }
    if (std::isnan(threshold)) { *why = "meter_select: the threshold is NaN"; return FX_E_ARG; }
    if (first < 0 || nRange < 0 || first > n || nRange > n - first) { *why = "meter_select: first .. first + n_range - 1 must lie in 0.." + std::to_string(n - 1); return FX_E_ARG; }
    if (cap < 0) { *why = "meter_select: cap < 0"; return FX_E_ARG; }
    if (cap > 0 && !list) { *why = "meter_select: a null list with cap > 0"; return FX_E_ARG; }
    return 0;
}

int Batch::checkMeterList(const char* name, const int64_t* list, int64_t count, int64_t n, bool unique, std::string* why) {
    const std::string who(name);
    if (count < 0) { *why = who + ": count < 0"; return FX_E_ARG; }
    if (count == 0) return 0;
    if (!list) { *why = who + ": a null list"; return FX_E_ARG; }
    if (count >= ((int64_t)1 << 31)) { *why = who + ": count must stay below 2^31"; return FX_E_ARG; }
    const ListFault f = checkList(list, count, n, unique);
    if (f.kind == ListFault::kOutside) { *why = listOutside(who, f, n); return FX_E_ARG; }
    if (f) { *why = who + ": instance " + std::to_string(list[f.entry]) + " is listed more than once (reset)"; return FX_E_ARG; }
    return 0;
}

int Batch::reserveMeterStage(size_t words, bool needEvent) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, "meters: metering is off (fxb_meter_enable)");
    if (words == 0) return 0;
    static const char* const kTexts[3] = {"meter list event", "hipMalloc meter list staging", "pinned staging of the meter list"};
    return reserveListStage(meterStage_, hMeterStage_, words, evInst_, instLaunched_, needEvent, kTexts);
}

int Batch::reserveMeterSelect(int64_t nRange, int64_t cap) { return reserveMeterStage(nRange > 0 ? selectWords(nRange, cap) : 0, false); }
int Batch::reserveMeterList(int64_t count, bool gather) { return reserveMeterStage(count > 0 ? listWords(prog_.numChannels, count, gather) : 0, !gather); }

int64_t Batch::meterSelect(int stat, double threshold, bool below, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, int64_t cap) {
    return runSelect(SelectRows::kMeter, stat, threshold, below, first, nRange, firstGlobal, list, cap);
}

// rows: kMatch is the select over the match rows of a target (fx_batch_meter_target.cpp), kLevel the one over the level rows
// (fx_batch_meter_level.cpp), kTone the one over the tone rows (fx_batch_meter_tone.cpp) - the same staging, copies and counts of words, another predicate on the device
int64_t Batch::runSelect(SelectRows rows, int stat, double threshold, bool below, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, int64_t cap) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, "meters: metering is off (fxb_meter_enable)");
    if (rows == SelectRows::kMatch && !dTarget_) return fail(FX_E_ARG, "meter target: no target is set (fxb_meter_set_target)");
    if (rows == SelectRows::kLevel && !dLevel_) return fail(FX_E_ARG, "level meters: the mode is off (fxb_meter_set_level)");
    if (rows == SelectRows::kTone && !dTone_) return fail(FX_E_ARG, "tone meters: the mode is off (fxb_meter_set_tones)");
    if (rows == SelectRows::kTone && (stat < 0 || stat >= toneCount_)) return fail(FX_E_ARG, "meter_select_tone: tone must lie in 0 .. n_tones - 1");
    if (nRange == 0) return 0;
    if (selectWords(nRange, cap) > meterStage_.cap || selectWords(nRange, cap) > hMeterStage_.cap) return fail(FX_E_ARG, "meter_select: no staging reserved (reserveMeterSelect)");
    const int rc = sync();
    if (rc != 0) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(unsigned long long) == 8, "meter list staging");
    const size_t chunks = (size_t)meterSelectChunks(nRange);
    const int64_t room = std::min(cap, nRange);
    MeterSelectArgs a{};
    a.rows = dMeter_;
    a.offsets = meterStage_.p;
    a.list = room > 0 ? reinterpret_cast<long long*>(meterStage_.p + chunks + 1) : nullptr;
    a.n = n_;
    a.nPad = nPad_;
    a.first = first;
    a.nRange = nRange;
    a.firstGlobal = firstGlobal;
    a.cap = room;
    a.threshold = threshold;
    a.channels = prog_.numChannels;
    a.stat = stat;
    a.below = below ? 1 : 0;
    hipError_t e;
    if (rows == SelectRows::kMatch) {
        const MatchSelectArgs b{dMatch_, a.offsets, a.list, a.n, a.nPad, a.first, a.nRange, a.firstGlobal, a.cap, a.threshold, a.channels, a.stat, a.below};
        if ((e = launchMatchSelect(b, stream_)) == hipSuccess) ++matchSelects_;
    } else if (rows == SelectRows::kLevel) {
        const LevelSelectArgs b{dLevel_, a.offsets, a.list, a.n, a.nPad, a.first, a.nRange, a.firstGlobal, a.cap, a.threshold, a.channels, a.stat, a.below};
        if ((e = launchLevelSelect(b, stream_)) == hipSuccess) ++levelSelects_;
    } else if (rows == SelectRows::kTone) {
        const ToneSelectArgs b{dTone_, a.offsets, a.list, a.n, a.nPad, a.first, a.nRange, a.firstGlobal, a.cap, a.threshold, a.channels, a.stat, a.below};
        if ((e = launchToneSelect(b, stream_)) == hipSuccess) ++toneSelects_;
    } else if ((e = launchMeterSelect(a, stream_)) == hipSuccess) {
        ++meterSelects_;
    }
    // the total and the head of the list in one copy; the rest of a long list once the total says how long it is
    const int64_t head = std::min(room, kSelectHead);
    unsigned long long* const hTotal = hMeterStage_.p + chunks;
    if (e == hipSuccess) e = hipMemcpyAsync(hTotal, meterStage_.p + chunks, (size_t)(1 + head) * 8, hipMemcpyDeviceToHost, stream_);
    hipError_t se = hipStreamSynchronize(stream_);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hipFail(e, "meter_select");
    const int64_t m = (int64_t)*hTotal, take = std::min(m, room);
    if (take > head) {
        e = hipMemcpyAsync(hTotal + 1 + head, meterStage_.p + chunks + 1 + head, (size_t)(take - head) * 8, hipMemcpyDeviceToHost, stream_);
        se = hipStreamSynchronize(stream_);
        if (e == hipSuccess) e = se;
        if (e != hipSuccess) return hipFail(e, "meter_select: the list");
    }
    if (take > 0) std::memcpy(list, hTotal + 1, (size_t)take * 8);
    return m;
}

int Batch::meterReadList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, double* energy, float* peak, uint32_t* fullScale, uint32_t* nonfinite, bool reset) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, "meters: metering is off (fxb_meter_enable)");
    if (count == 0) return 0;
    const int channels = prog_.numChannels;
    const size_t k = (size_t)count, words = listWords(channels, count, true);
    if (words > meterStage_.cap || words > hMeterStage_.cap) return fail(FX_E_ARG, "meter_read_list: no staging reserved (reserveMeterList)");
    const int rc = sync();
    if (rc != 0) return rc;
    std::memcpy(hMeterStage_.p, list, k * 8);
    MeterListArgs a{};
    a.rows = dMeter_;
    a.list = reinterpret_cast<const long long*>(meterStage_.p);
    a.packed = meterStage_.p + k;
    a.count = count;
    a.n = n_;
    a.nPad = nPad_;
    a.channels = channels;
    a.reset = reset ? 1 : 0;
    hipError_t e = hipMemcpyAsync(meterStage_.p, hMeterStage_.p, k * 8, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = launchMeterGather(a, stream_);
    if (e == hipSuccess) {
        ++meterListReads_;
        e = hipMemcpyAsync(hMeterStage_.p + k, meterStage_.p + k, meterPackedBytes(channels, count), hipMemcpyDeviceToHost, stream_);
    }
    const hipError_t se = hipStreamSynchronize(stream_);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hipFail(e, "meter_read_list: the gather");
    // the packed side: energy [channels][count], then peak, full_scale, nonfinite (fx_meter_list.hpp)
    const size_t rowWords = (size_t)channels * k;
    const char* packed = reinterpret_cast<const char*>(hMeterStage_.p + k);
    const char* part[4] = {packed, packed + rowWords * 8, packed + rowWords * 12, packed + rowWords * 16};
    char* out[4] = {reinterpret_cast<char*>(energy), reinterpret_cast<char*>(peak), reinterpret_cast<char*>(fullScale), reinterpret_cast<char*>(nonfinite)};
    for (int r = 0; r < 4; ++r) {
        if (!out[r]) continue;
        const size_t bytes = r == 0 ? 8 : 4;
        for (int c = 0; c < channels; ++c) {
            const char* from = part[r] + (size_t)c * k * bytes;
            char* to = out[r] + (size_t)c * (size_t)total * bytes;
            copyColumn(to, from, pos, k, bytes, true);
        }
    }
    return 0;
}

int Batch::meterResetList(const int64_t* list, int64_t count) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, "meters: metering is off (fxb_meter_enable)");
    if (count == 0) return 0;
    const size_t k = (size_t)count;
    if (k > meterStage_.cap || k > hMeterStage_.cap || !evInst_) return fail(FX_E_ARG, "meter_reset_list: no staging reserved (reserveMeterList)");
    if (const int rc = waitPreviousInstCall("meter_reset_list: waiting for the previous call")) return rc;
    std::memcpy(hMeterStage_.p, list, k * 8);
    MeterListArgs a{};
    a.rows = dMeter_;
    a.list = reinterpret_cast<const long long*>(meterStage_.p);
    a.count = count;
    a.n = n_;
    a.nPad = nPad_;
    a.channels = prog_.numChannels;
    hipError_t e = hipMemcpyAsync(meterStage_.p, hMeterStage_.p, k * 8, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = orderBehindQueuedBlocks();   // (a block's meter launch sits in front of its ev1_ record)
    if (e == hipSuccess) e = launchMeterZero(a, stream_);
    // (a slot reused gets fresh meters, all of them: the listed columns of the match rows of a target, inside the same frame)
    if (e == hipSuccess && dMatch_) {
        a.rows = dMatch_;
        e = launchMatchZero(a, stream_);
    }
    // (... and those of the level rows)
    if (e == hipSuccess && dLevel_) {
        a.rows = dLevel_;
        e = launchLevelZero(a, stream_);
    }
    // (... and those of the tone rows: stores only, inside the same frame)
    if (e == hipSuccess && dTone_) {
        a.rows = dTone_;
        e = launchToneZero(a, stream_);
    }
    if (const int failed = closeInstCall(e, "meter_reset_list: queueing the zeroing")) return failed;
    ++meterListResets_;
    return 0;
}

}  // namespace fx
