// fx_batch_meter_level.cpp — the level meters of one batch: two further accumulators per (channel, instance) that fall as well as
// rise - an envelope with instant attack and exponential release, and the count of consecutive samples below a floor - and the
// queries that bring them back (include/fx8010_amd.h "Level meters", fx_batch.hpp "Level meters", kernels: fx_meter.hip
// fx_meter_level / fx_meter_target_level, fx_meter_list.hip fx_level_count / _emit / _gather / _zero).
//
// Split check / reserve / act like the target meters (fx_batch_meter_target.cpp), so that a sharded handle can ask every shard
// before any shard changes: checkMeterLevel refuses for the whole handle, reserveMeterLevel is the allocating half - the level
// rows, where there are none yet - and setMeterLevel takes them into force, zeroed, and sets the two parameters.  Everything the
// feature allocates is allocated there; launchBlock (fx_batch_io.cpp) only picks the launch and hands the parameters over by
// value.  The select shares the staging and the copies of the meter select (Batch::runSelect); the list read goes through the same
// staging pair as [the list][the packed rows].  The reads and the select are synchronous: they wait as sync() does, which covers
// a list reset in flight.
#include "fx_batch.hpp"

#include <cmath>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

namespace {
const char* const kLevelOff = "level meters: the mode is off (fxb_meter_set_level)";
const char* const kMeterOff = "meters: metering is off (fxb_meter_enable)";
}  // namespace

int Batch::checkMeterLevel(float* release, float* floor, unsigned flags, std::string* why) {
    if (!(std::isfinite(*release) && *release >= 0.0f && *release <= 1.0f)) { *why = "meter_set_level: release must be finite and lie in 0..1"; return FX_E_ARG; }
    if (!(std::isfinite(*floor) && *floor >= 0.0f)) { *why = "meter_set_level: floor must be finite and not negative"; return FX_E_ARG; }
    if (flags != 0) { *why = "meter_set_level: flags must be 0"; return FX_E_ARG; }
    // (-0.0 is taken as 0: the kernel compares bit patterns and wants the sign bit clear)
    if (*release == 0.0f) *release = 0.0f;
    if (*floor == 0.0f) *floor = 0.0f;
    return 0;
}

int Batch::checkLevelSelect(int stat, double threshold, int64_t first, int64_t nRange, int64_t n, const int64_t* list, int64_t cap, unsigned flags, std::string* why) {
    if (stat < FXB_LEVEL_ENVELOPE || stat > FXB_LEVEL_QUIET) { *why = "meter_select_level: stat must be 0 or 1 (FXB_LEVEL_ENVELOPE, FXB_LEVEL_QUIET)"; return FX_E_ARG; }
    if (flags & ~(unsigned)FXB_METER_BELOW) { *why = "meter_select_level: flags has an unknown bit"; return FX_E_ARG; }
    if (std::isnan(threshold)) { *why = "meter_select_level: the threshold is NaN"; return FX_E_ARG; }
    if (first < 0 || nRange < 0 || first > n || nRange > n - first) { *why = "meter_select_level: first .. first + n_range - 1 must lie in 0.." + std::to_string(n - 1); return FX_E_ARG; }
    if (cap < 0) { *why = "meter_select_level: cap < 0"; return FX_E_ARG; }
    if (cap > 0 && !list) { *why = "meter_select_level: a null list with cap > 0"; return FX_E_ARG; }
    return 0;
}

void Batch::releaseMeterLevel() {
    (void)hipSetDevice(device_);
    (void)hipFree(levelNew_);
    levelNew_ = nullptr;
}

int Batch::reserveMeterLevel() {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    releaseMeterLevel();
    if (dLevel_) return 0;   // (the mode is on: a set changes the parameters only)
    const hipError_t e = hipMalloc(&levelNew_, levelChannelBytes(nPad_) * (size_t)prog_.numChannels);
    if (e != hipSuccess) { levelNew_ = nullptr; return hipFail(hipErrorOutOfMemory, "hipMalloc level rows"); }
    return 0;
}

int Batch::zeroLevelRows() {
    waitLastLaunch();
    hipError_t e = hipMemsetAsync(dLevel_, 0, levelChannelBytes(nPad_) * (size_t)prog_.numChannels, stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    return e == hipSuccess ? 0 : hipFail(e, "zeroing the level rows");
}

// release, floor: checked and canonical (checkMeterLevel)
int Batch::setMeterLevel(float release, float floor) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    if (!dLevel_) {
        if (!levelNew_) return fail(FX_E_ARG, "meter_set_level: nothing reserved (reserveMeterLevel)");
        const int rc = sync();   // (the first call waits as sync() does: the blocks queued so far are metered without the rows)
        if (rc != 0) {
            releaseMeterLevel();
            return rc;
        }
        dLevel_ = levelNew_;
        levelNew_ = nullptr;
        if (const int zr = zeroLevelRows()) {
            (void)hipFree(dLevel_);
            dLevel_ = nullptr;
            return zr;
        }
    }
    // (host-side: the blocks queued so far carry the parameters they were queued with)
    levelRelease_ = release;
    levelFloor_ = floor;
    return 0;
}

int Batch::clearMeterLevel() {
    (void)hipSetDevice(device_);
    releaseMeterLevel();
    if (!dLevel_) return 0;
    waitLastLaunch();
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(dLevel_);
    dLevel_ = nullptr;
    levelRelease_ = levelFloor_ = 0.0f;
    return 0;
}

int Batch::getMeterLevel(float* release, float* floor) {
    if (!dLevel_) return fail(FX_E_ARG, kLevelOff);
    if (release) *release = levelRelease_;
    if (floor) *floor = levelFloor_;
    return 0;
}

int Batch::meterReadLevel(float* level, uint32_t* quiet, bool reset, int64_t rowPitch) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    if (!dLevel_) return fail(FX_E_ARG, kLevelOff);
    if (rowPitch <= 0) rowPitch = n_;
    if (rowPitch < n_) return fail(FX_E_ARG, "meters: row pitch below the instance count");
    const int rc = sync();
    if (rc != 0) return rc;
    hipError_t e = hipSuccess;
    for (int c = 0; c < prog_.numChannels && e == hipSuccess; ++c) {
        const char* ch = static_cast<const char*>(dLevel_) + (size_t)c * levelChannelBytes(nPad_);
        const size_t at = (size_t)c * (size_t)rowPitch;
        if (level) e = hipMemcpy(level + at, ch + levelLevelOff(nPad_), (size_t)n_ * 4, hipMemcpyDeviceToHost);
        if (quiet && e == hipSuccess) e = hipMemcpy(quiet + at, ch + levelQuietOff(nPad_), (size_t)n_ * 4, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return hipFail(e, "reading the level rows");
    return reset ? zeroLevelRows() : 0;
}

// (the staging is that of meterReadList: reserveMeterList(count, true) holds the list and a packed side of 20 bytes per column
// and channel, of which this call uses 8)
int Batch::meterReadLevelList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, float* level, uint32_t* quiet, bool reset) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    if (!dLevel_) return fail(FX_E_ARG, kLevelOff);
    if (count == 0) return 0;
    const int channels = prog_.numChannels;
    const size_t k = (size_t)count, words = k + (levelPackedBytes(channels, count) + 7) / 8;
    if (words > meterStage_.cap || words > hMeterStage_.cap) return fail(FX_E_ARG, "meter_read_level_list: no staging reserved (reserveMeterList)");
    const int rc = sync();
    if (rc != 0) return rc;
    std::memcpy(hMeterStage_.p, list, k * 8);
    MeterListArgs a{};
    a.rows = dLevel_;
    a.list = reinterpret_cast<const long long*>(meterStage_.p);
    a.packed = meterStage_.p + k;
    a.count = count;
    a.n = n_;
    a.nPad = nPad_;
    a.channels = channels;
    a.reset = reset ? 1 : 0;
    hipError_t e = hipMemcpyAsync(meterStage_.p, hMeterStage_.p, k * 8, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = launchLevelGather(a, stream_);
    if (e == hipSuccess) {
        ++levelListReads_;
        e = hipMemcpyAsync(hMeterStage_.p + k, meterStage_.p + k, levelPackedBytes(channels, count), hipMemcpyDeviceToHost, stream_);
    }
    const hipError_t se = hipStreamSynchronize(stream_);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hipFail(e, "meter_read_level_list: the gather");
    // the packed side: level [channels][count], then quiet (fx_meter_list.hpp)
    const size_t rowWords = (size_t)channels * k;
    const char* packed = reinterpret_cast<const char*>(hMeterStage_.p + k);
    const char* part[2] = {packed, packed + rowWords * 4};
    char* out[2] = {reinterpret_cast<char*>(level), reinterpret_cast<char*>(quiet)};
    for (int r = 0; r < 2; ++r) {
        if (!out[r]) continue;
        for (int c = 0; c < channels; ++c) copyColumn(out[r] + (size_t)c * (size_t)total * 4, part[r] + (size_t)c * k * 4, pos, k, 4, true);
    }
    return 0;
}

int64_t Batch::levelSelect(int stat, double threshold, bool below, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, int64_t cap) {
    return runSelect(SelectRows::kLevel, stat, threshold, below, first, nRange, firstGlobal, list, cap);
}

}  // namespace fx
