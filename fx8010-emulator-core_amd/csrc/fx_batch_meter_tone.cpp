// fx_batch_meter_tone.cpp — the tone meters of one batch: a Goertzel recurrence per (tone, channel, instance) - two fp64 words that
// a launch of its own behind the meter launch of every block carries on - and the queries that bring the words and the power
// back (include/fx8010_amd.h "Tone meters", fx_batch.hpp "Tone meters", kernels: fx_meter_tone.hip fx_meter_tone<K> /
// fx_tone_gather / fx_tone_zero, fx_meter_list.hip fx_tone_count / _emit, fx_meter_rank.hip through launchToneRank).
//
// Split check / reserve / act like the level meters (fx_batch_meter_level.cpp), so that a sharded handle can ask every shard
// before any shard changes: checkMeterTones refuses for the whole handle, reserveMeterTones is the allocating half - a tone block
// of the asked size, always a new one - and setMeterTones takes it into force: it waits, writes the header, zeroes the rows and
// frees the block it replaces.  Everything the feature allocates is allocated there; launchBlock (fx_batch_io.cpp) only queues
// the launch and hands the coefficients over by value.  The select shares the staging and the copies of the meter select
// (Batch::runSelect), the rank those of the meter ranks (Batch::meterRank); the list read goes through the same staging pair as
// [the list][the packed rows].  The reads, the select and the rank are synchronous: they wait as sync() does, which covers a list
// reset in flight.
#include "fx_batch.hpp"

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/fx8010_amd.h"

namespace fx {

namespace {
const char* const kTonesOff = "tone meters: the mode is off (fxb_meter_set_tones)";
const char* const kMeterOff = "meters: metering is off (fxb_meter_enable)";
static_assert(kMeterMaxTones == FXB_METER_MAX_TONES, "the header's constant and the kernels' agree");
}  // namespace

int Batch::checkMeterTones(int tones, const double* coeff, unsigned flags, double* canonical, std::string* why) {
    if (tones < 1 || tones > kMeterMaxTones) { *why = "meter_set_tones: n_tones must lie in 1.." + std::to_string(kMeterMaxTones); return FX_E_ARG; }
    if (!coeff) { *why = "meter_set_tones: a null coeff"; return FX_E_ARG; }
    if (flags != 0) { *why = "meter_set_tones: flags must be 0"; return FX_E_ARG; }
    for (int k = 0; k < tones; ++k) {
        if (!(std::isfinite(coeff[k]) && coeff[k] >= -2.0 && coeff[k] <= 2.0)) { *why = "meter_set_tones: coeff[" + std::to_string(k) + "] must be finite and lie in -2..2"; return FX_E_ARG; }
        canonical[k] = coeff[k] == 0.0 ? 0.0 : coeff[k];   // (-0.0 is taken as +0.0)
    }
    return 0;
}

int Batch::checkToneSelect(int tone, double threshold, int64_t first, int64_t nRange, int64_t n, const int64_t* list, int64_t cap, unsigned flags, std::string* why) {
    if (tone < 0 || tone >= kMeterMaxTones) { *why = "meter_select_tone: tone must lie in 0 .. n_tones - 1"; return FX_E_ARG; }
    if (flags & ~(unsigned)FXB_METER_BELOW) { *why = "meter_select_tone: flags has an unknown bit"; return FX_E_ARG; }
    if (std::isnan(threshold)) { *why = "meter_select_tone: the threshold is NaN"; return FX_E_ARG; }
    if (first < 0 || nRange < 0 || first > n || nRange > n - first) { *why = "meter_select_tone: first .. first + n_range - 1 must lie in 0.." + std::to_string(n - 1); return FX_E_ARG; }
    if (cap < 0) { *why = "meter_select_tone: cap < 0"; return FX_E_ARG; }
    if (cap > 0 && !list) { *why = "meter_select_tone: a null list with cap > 0"; return FX_E_ARG; }
    return 0;
}

void Batch::releaseMeterTones() {
    (void)hipSetDevice(device_);
    (void)hipFree(toneNew_);
    toneNew_ = nullptr;
    toneNewCount_ = 0;
}

int Batch::reserveMeterTones(int tones) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    if (tones < 1 || tones > kMeterMaxTones) return fail(FX_E_ARG, "meter_set_tones: n_tones out of range");
    releaseMeterTones();
    const hipError_t e = hipMalloc(&toneNew_, toneBlockBytes(nPad_, prog_.numChannels, tones));
    if (e != hipSuccess) { toneNew_ = nullptr; return hipFail(hipErrorOutOfMemory, "hipMalloc tone rows"); }
    toneNewCount_ = tones;
    return 0;
}

int Batch::zeroToneRows() {
    waitLastLaunch();
    hipError_t e = hipMemsetAsync(static_cast<char*>(dTone_) + kToneHeaderBytes, 0, toneRowsBytes(nPad_, prog_.numChannels, toneCount_), stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    return e == hipSuccess ? 0 : hipFail(e, "zeroing the tone rows");
}

// tones, coeff: checked and canonical (checkMeterTones)
int Batch::setMeterTones(int tones, const double* coeff) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    if (!toneNew_ || toneNewCount_ != tones) return fail(FX_E_ARG, "meter_set_tones: nothing reserved (reserveMeterTones)");
    const int rc = sync();   // (every call waits as sync() does: the blocks queued so far are metered with the mode they were queued with)
    if (rc != 0) {
        releaseMeterTones();
        return rc;
    }
    // the header of the new block: the coefficients, then K
    unsigned char head[kToneHeaderBytes] = {};
    std::memcpy(head, coeff, (size_t)tones * 8);
    const long long count = tones;
    std::memcpy(head + kToneCountOff, &count, 8);
    hipError_t e = hipMemcpy(toneNew_, head, kToneHeaderBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(static_cast<char*>(toneNew_) + kToneHeaderBytes, 0, toneRowsBytes(nPad_, prog_.numChannels, tones), stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    if (e != hipSuccess) {
        releaseMeterTones();
        return hipFail(e, "meter_set_tones: the header and the zeroing");
    }
    (void)hipFree(dTone_);   // (the block of the mode this call replaces, if any: nothing is queued that reads it)
    dTone_ = toneNew_;
    toneNew_ = nullptr;
    toneNewCount_ = 0;
    toneCount_ = tones;
    for (int k = 0; k < kMeterMaxTones; ++k) toneCoeff_[k] = k < tones ? coeff[k] : 0.0;
    return 0;
}

int Batch::clearMeterTones() {
    (void)hipSetDevice(device_);
    releaseMeterTones();
    if (!dTone_) return 0;
    waitLastLaunch();
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(dTone_);
    dTone_ = nullptr;
    toneCount_ = 0;
    for (double& c : toneCoeff_) c = 0.0;
    return 0;
}

int Batch::getMeterTones(int* tones, double* coeff) {
    if (!dTone_) return fail(FX_E_ARG, kTonesOff);
    if (tones) *tones = toneCount_;
    if (coeff) std::memcpy(coeff, toneCoeff_, (size_t)toneCount_ * 8);
    return 0;
}

int Batch::launchToneMeter(const MeterArgs& m, hipStream_t s) {
    MeterToneArgs t{};
    t.y = m.y;
    t.block = dTone_;
    t.n = m.n;
    t.nPad = m.nPad;
    t.pitch = m.pitch;
    t.samples = m.samples;
    t.channels = m.channels;
    t.tones = toneCount_;
    std::memcpy(t.coeff, toneCoeff_, sizeof t.coeff);
    const hipError_t e = launchMeterTone(t, s);
    if (e != hipSuccess) return hipFail(e, "launch fx_meter_tone");
    ++meterToneLaunches_;
    return 0;
}

int Batch::meterReadTones(double* s1, double* s2, double* power, bool reset, int64_t rowPitch) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    if (!dTone_) return fail(FX_E_ARG, kTonesOff);
    if (rowPitch <= 0) rowPitch = n_;
    if (rowPitch < n_) return fail(FX_E_ARG, "meters: row pitch below the instance count");
    const int rc = sync();
    if (rc != 0) return rc;
    const int channels = prog_.numChannels;
    std::vector<double> a((size_t)n_), b((size_t)n_);
    hipError_t e = hipSuccess;
    for (int k = 0; k < toneCount_ && e == hipSuccess; ++k) {
        for (int c = 0; c < channels && e == hipSuccess; ++c) {
            const char* row = static_cast<const char*>(dTone_) + toneRowOff(nPad_, toneCount_, c, k);
            const size_t at = ((size_t)k * (size_t)channels + (size_t)c) * (size_t)rowPitch;
            e = hipMemcpy(a.data(), row, (size_t)n_ * 8, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(b.data(), row + (size_t)nPad_ * 8, (size_t)n_ * 8, hipMemcpyDeviceToHost);
            if (e != hipSuccess) break;
            if (s1) std::memcpy(s1 + at, a.data(), (size_t)n_ * 8);
            if (s2) std::memcpy(s2 + at, b.data(), (size_t)n_ * 8);
            if (power)
                for (int64_t i = 0; i < n_; ++i) power[at + (size_t)i] = tonePower(toneCoeff_[k], a[(size_t)i], b[(size_t)i]);
        }
    }
    if (e != hipSuccess) return hipFail(e, "reading the tone rows");
    return reset ? zeroToneRows() : 0;
}

int Batch::reserveToneList(int64_t count) {
    if (!dTone_) return fail(FX_E_ARG, kTonesOff);
    return reserveMeterStage(count > 0 ? (size_t)count + tonePackedBytes(toneCount_, prog_.numChannels, count) / 8 : 0, false);
}

int Batch::meterReadTonesList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, double* s1, double* s2, double* power, bool reset) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, kMeterOff);
    if (!dTone_) return fail(FX_E_ARG, kTonesOff);
    if (count == 0) return 0;
    const int channels = prog_.numChannels;
    const size_t k = (size_t)count, words = k + tonePackedBytes(toneCount_, channels, count) / 8;
    if (words > meterStage_.cap || words > hMeterStage_.cap) return fail(FX_E_ARG, "meter_read_tones_list: no staging reserved (reserveToneList)");
    const int rc = sync();
    if (rc != 0) return rc;
    std::memcpy(hMeterStage_.p, list, k * 8);
    MeterListArgs a{};
    a.rows = dTone_;
    a.list = reinterpret_cast<const long long*>(meterStage_.p);
    a.packed = meterStage_.p + k;
    a.count = count;
    a.n = n_;
    a.nPad = nPad_;
    a.channels = channels;
    a.reset = reset ? 1 : 0;
    hipError_t e = hipMemcpyAsync(meterStage_.p, hMeterStage_.p, k * 8, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = launchToneGather(a, stream_);
    if (e == hipSuccess) {
        ++toneListReads_;
        e = hipMemcpyAsync(hMeterStage_.p + k, meterStage_.p + k, tonePackedBytes(toneCount_, channels, count), hipMemcpyDeviceToHost, stream_);
    }
    const hipError_t se = hipStreamSynchronize(stream_);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hipFail(e, "meter_read_tones_list: the gather");
    // the packed side: s1 [tones][channels][count], then s2, then P (fx_meter_tone.hpp)
    const size_t rows = (size_t)toneCount_ * (size_t)channels;
    const double* const packed = reinterpret_cast<const double*>(hMeterStage_.p + k);
    double* const out[3] = {s1, s2, power};
    for (int r = 0; r < 3; ++r) {
        if (!out[r]) continue;
        for (size_t row = 0; row < rows; ++row) copyColumn(out[r] + row * (size_t)total, packed + ((size_t)r * rows + row) * k, pos, k, 8, true);
    }
    return 0;
}

int64_t Batch::toneSelect(int tone, double threshold, bool below, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, int64_t cap) {
    return runSelect(SelectRows::kTone, tone, threshold, below, first, nRange, firstGlobal, list, cap);
}

}  // namespace fx
