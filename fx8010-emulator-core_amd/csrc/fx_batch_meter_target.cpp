// fx_batch_meter_target.cpp — the target meters of one batch: a reference signal held on the device, two further fp64
// accumulators per (channel, instance) against it, and the queries that bring back the verdict instead of the signal
// (include/fx8010_amd.h "Target meters", fx_batch.hpp "Target meters", kernels: fx_meter.hip fx_meter_target, fx_meter_list.hip
// fx_match_count / _emit, fx_meter_best, fx_match_zero).
//
// Split check / reserve / act like the list calls (fx_batch_meter_list.cpp), so that a sharded handle can ask every shard before
// any shard changes: checkMeterTarget refuses for the whole handle, reserveMeterTarget is the allocating half - the block of the
// target columns this batch's instances use and, where there are none yet, the match rows - and setMeterTarget waits as sync()
// does, copies the columns, zeroes the match rows and takes the blocks into force.  Everything the feature allocates is allocated
// there; launchBlock (fx_batch_io.cpp) only picks the launch and advances the position.  The match select shares the staging and
// the copies of the meter select (Batch::runSelect); the winners of fxb_meter_best travel through the same staging pair as
// [winner words][value words].  All of the queries are synchronous: they wait as sync() does, which covers a list reset in flight.
#include "fx_batch.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

namespace {
const char* const kNoTarget = "meter target: no target is set (fxb_meter_set_target)";
const char* const kMeterOff = "meters: metering is off (fxb_meter_enable)";
}  // namespace

int Batch::checkMeterTarget(const float* target, int64_t nSamples, int64_t group, unsigned flags, int channels, int64_t nTotal, std::string* why) {
    if (!target) { *why = "meter_set_target: a null target"; return FX_E_ARG; }
    if (nSamples < 1) { *why = "meter_set_target: n_samples must be at least 1"; return FX_E_ARG; }
    if (group < 1) { *why = "meter_set_target: group must be at least 1"; return FX_E_ARG; }
    if (flags & ~(unsigned)FXB_METER_TARGET_LOOP) { *why = "meter_set_target: flags has an unknown bit"; return FX_E_ARG; }
    const int64_t g = std::min(group, nTotal), cols = (nTotal + g - 1) / g;
    // words of the whole target below 2^31: channels <= 4 and cols <= nTotal, so the product on the right cannot overflow
    if (nSamples > (((int64_t)1 << 31) - 1) / ((int64_t)channels * cols)) { *why = "meter_set_target: n_samples * num_channels * G must stay below 2^31 words"; return FX_E_ARG; }
    return 0;
}

int Batch::checkMatchSelect(int stat, double threshold, int64_t first, int64_t nRange, int64_t n, const int64_t* list, int64_t cap, unsigned flags, std::string* why) {
    if (stat < FXB_MATCH_ERROR || stat > FXB_MATCH_CROSS) { *why = "meter_select_match: stat must be 0 or 1 (FXB_MATCH_ERROR, FXB_MATCH_CROSS)"; return FX_E_ARG; }
    if (flags & ~(unsigned)FXB_METER_BELOW) { *why = "meter_select_match: flags has an unknown bit"; return FX_E_ARG; }
    if (std::isnan(threshold)) { *why = "meter_select_match: the threshold is NaN"; return FX_E_ARG; }
    if (first < 0 || nRange < 0 || first > n || nRange > n - first) { *why = "meter_select_match: first .. first + n_range - 1 must lie in 0.." + std::to_string(n - 1); return FX_E_ARG; }
    if (cap < 0) { *why = "meter_select_match: cap < 0"; return FX_E_ARG; }
    if (cap > 0 && !list) { *why = "meter_select_match: a null list with cap > 0"; return FX_E_ARG; }
    return 0;
}

void Batch::releaseMeterTarget() {
    (void)hipSetDevice(device_);
    (void)hipFree(targetNew_);
    (void)hipFree(matchNew_);
    targetNew_ = nullptr;
    matchNew_ = nullptr;
}

// group: at most the instance count of the whole handle (the caller has clamped it: one column for all of them)
int Batch::reserveMeterTarget(int64_t nSamples, int64_t group, int64_t firstGlobal) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    const int channels = prog_.numChannels;
    const int64_t cols = meterBestGroups(group, firstGlobal);   // (the same count: the columns first / group .. last / group)
    if ((unsigned long long)channels * (unsigned long long)cols * 4u >= (1ull << 32)) return fail(FX_E_ARG, "meter_set_target: num_channels * G * 4 of a shard must stay below 2^32 (the kernel's row stride)");
    releaseMeterTarget();
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&targetNew_), (size_t)nSamples * (size_t)channels * (size_t)cols * 4);
    if (e != hipSuccess) { targetNew_ = nullptr; return hipFail(hipErrorOutOfMemory, "hipMalloc meter target"); }
    if (!dMatch_) {
        e = hipMalloc(&matchNew_, matchChannelBytes(nPad_) * (size_t)channels);
        if (e != hipSuccess) {
            matchNew_ = nullptr;
            releaseMeterTarget();
            return hipFail(hipErrorOutOfMemory, "hipMalloc match rows");
        }
    }
    return 0;
}

int Batch::zeroMatchRows() {
    waitLastLaunch();
    hipError_t e = hipMemsetAsync(dMatch_, 0, matchChannelBytes(nPad_) * (size_t)prog_.numChannels, stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    return e == hipSuccess ? 0 : hipFail(e, "zeroing the match rows");
}

// cols: columns of a row of the caller's block (G of the whole handle); this batch takes those from firstGlobal / group on
int Batch::setMeterTarget(const float* target, int64_t nSamples, int64_t group, int64_t firstGlobal, int64_t cols, bool loop) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    if (!targetNew_ || (!dMatch_ && !matchNew_)) return fail(FX_E_ARG, "meter_set_target: nothing reserved (reserveMeterTarget)");
    int rc = sync();   // (queued blocks read the target and the rows that are in force)
    const int64_t mine = meterBestGroups(group, firstGlobal), firstCol = firstGlobal / group;
    if (rc == 0) {
        const hipError_t e = hipMemcpy2D(targetNew_, (size_t)mine * 4, target + firstCol, (size_t)cols * 4, (size_t)mine * 4, (size_t)nSamples * (size_t)prog_.numChannels, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = hipFail(e, "copying the meter target");
    }
    if (rc != 0) {
        releaseMeterTarget();
        return rc;
    }
    (void)hipFree(dTarget_);
    dTarget_ = targetNew_;
    targetNew_ = nullptr;
    if (matchNew_) {
        dMatch_ = matchNew_;
        matchNew_ = nullptr;
    }
    targetSamples_ = nSamples;
    targetCols_ = mine;
    targetGroup_ = group;
    targetFirstGlobal_ = firstGlobal;
    targetLoop_ = loop;
    targetPos_ = 0;
    return zeroMatchRows();
}

int Batch::clearMeterTarget() {
    (void)hipSetDevice(device_);
    releaseMeterTarget();
    if (!dTarget_) return 0;
    waitLastLaunch();
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(dTarget_);
    (void)hipFree(dMatch_);
    dTarget_ = nullptr;
    dMatch_ = nullptr;
    targetSamples_ = targetCols_ = targetPos_ = 0;
    return 0;
}

int Batch::meterTargetSeek(int64_t pos) {
    if (!dTarget_) return fail(FX_E_ARG, kNoTarget);
    if (pos < 0 || pos > targetSamples_ || (targetLoop_ && pos == targetSamples_))
        return fail(FX_E_ARG, "meter_target_seek: pos must lie in 0..n_samples (below n_samples with FXB_METER_TARGET_LOOP)");
    targetPos_ = pos;
    return 0;
}

MeterTargetArgs Batch::meterTargetArgs(const MeterArgs& m) const {
    MeterTargetArgs t{};
    t.m = m;
    t.match = dMatch_;
    t.target = dTarget_;
    t.tSamples = targetSamples_;
    t.tCols = targetCols_;
    t.group = targetGroup_;
    t.firstGlobal = targetFirstGlobal_;
    t.firstColumn = targetFirstGlobal_ / targetGroup_;
    t.pos = targetPos_;
    t.loop = targetLoop_ ? 1 : 0;
    return t;
}

int Batch::meterReadMatch(double* err, double* cross, bool reset, int64_t rowPitch) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    if (!dTarget_) return fail(FX_E_ARG, kNoTarget);
    if (rowPitch <= 0) rowPitch = n_;
    if (rowPitch < n_) return fail(FX_E_ARG, "meters: row pitch below the instance count");
    const int rc = sync();
    if (rc != 0) return rc;
    hipError_t e = hipSuccess;
    for (int c = 0; c < prog_.numChannels && e == hipSuccess; ++c) {
        const char* ch = static_cast<const char*>(dMatch_) + (size_t)c * matchChannelBytes(nPad_);
        const size_t at = (size_t)c * (size_t)rowPitch;
        if (err) e = hipMemcpy(err + at, ch + matchErrOff(nPad_), (size_t)n_ * 8, hipMemcpyDeviceToHost);
        if (cross && e == hipSuccess) e = hipMemcpy(cross + at, ch + matchCrossOff(nPad_), (size_t)n_ * 8, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return hipFail(e, "reading the match rows");
    return reset ? zeroMatchRows() : 0;
}

int64_t Batch::matchSelect(int stat, double threshold, bool below, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, int64_t cap) {
    return runSelect(SelectRows::kMatch, stat, threshold, below, first, nRange, firstGlobal, list, cap);
}

int Batch::reserveMeterBest(int64_t group, int64_t firstGlobal) {
    if (dMeter_ && !dTarget_) return fail(FX_E_ARG, kNoTarget);
    return reserveMeterStage(2 * (size_t)meterBestGroups(group, firstGlobal), false);
}

int Batch::meterBest(int stat, int64_t group, int64_t firstGlobal, bool largest, int64_t* winner, double* value) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    if (!dTarget_) return fail(FX_E_ARG, kNoTarget);
    const size_t groups = (size_t)meterBestGroups(group, firstGlobal);
    if (2 * groups > meterStage_.cap || 2 * groups > hMeterStage_.cap) return fail(FX_E_ARG, "meter_best: no staging reserved (reserveMeterBest)");
    const int rc = sync();
    if (rc != 0) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(double) == 8, "meter list staging");
    MeterBestArgs a{};
    a.rows = dMatch_;
    a.winner = reinterpret_cast<long long*>(meterStage_.p);
    a.value = reinterpret_cast<double*>(meterStage_.p + groups);
    a.n = n_;
    a.nPad = nPad_;
    a.firstGlobal = firstGlobal;
    a.group = group;
    a.firstGroup = firstGlobal / group;
    a.groups = (long long)groups;
    a.channels = prog_.numChannels;
    a.stat = stat;
    a.largest = largest ? 1 : 0;
    hipError_t e = launchMeterBest(a, stream_);
    if (e == hipSuccess) {
        ++matchBests_;
        e = hipMemcpyAsync(hMeterStage_.p, meterStage_.p, 2 * groups * 8, hipMemcpyDeviceToHost, stream_);
    }
    const hipError_t se = hipStreamSynchronize(stream_);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hipFail(e, "meter_best");
    if (winner) std::memcpy(winner, hMeterStage_.p, groups * 8);
    if (value) std::memcpy(value, hMeterStage_.p + groups, groups * 8);
    return 0;
}

}  // namespace fx
