// fx_batch_meter_rank.cpp — the meter ranks of one batch: the first k candidates of a range under the order (V, n), chosen on the
// device (include/fx8010_amd.h "Meter ranks", fx_batch.hpp "Meter ranks", kernels: fx_meter_rank.hip).  One implementation serves
// the four families - the four accumulators, the match rows of a target, the level rows, the tone rows: the family picks the rows, the range of
// `stat` and the counter.
//
// Split check / reserve / act like the level meters (fx_batch_meter_level.cpp), so that a sharded handle can ask every shard before
// any shard runs: checkMeterRank refuses for the whole handle, reserveMeterRank is the allocating half and meterRank launches.  The
// staging is the pair of the meter queries by list (fx_batch_meter_list.cpp): a synchronous call finds it free.  It is laid out as
// fx_meter_rank.hpp says - the result words and the pairs first - so its size goes by min(k, nRange), the two histogram blocks
// and two words per chunk of 256 instances.  The call waits as sync() does - which covers a list reset still in flight -, queues
// the launches and ONE copy of the result words with the pairs behind them, and waits once.  The pairs come back ascending by
// instance; the host sorts them into rank order (rankBefore), which costs nothing beside the wait at the k a host asks for.
#include "fx_batch.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "../../include/fx8010_amd.h"

namespace fx {

namespace {
const char* const kRankNames[4] = {"meter_rank", "meter_rank_match", "meter_rank_level", "meter_rank_tone"};
// pairs that travel with the result words in the one copy when M is not known to be smaller: all of them up to this many; a
// longer list is fetched in a second copy once R is known
constexpr int64_t kRankHead = 4096;
}  // namespace

int Batch::checkMeterRank(int family, int stat, int64_t k, double threshold, int64_t first, int64_t nRange, int64_t n, const int64_t* list, unsigned flags, std::string* why) {
    const std::string who(kRankNames[family]);
    if (family == kRankMeter && (stat < FXB_METER_ENERGY || stat > FXB_METER_NONFINITE)) { *why = who + ": stat must be 0..3 (FXB_METER_ENERGY .. FXB_METER_NONFINITE)"; return FX_E_ARG; }
    if (family == kRankMatch && (stat < FXB_MATCH_ERROR || stat > FXB_MATCH_CROSS)) { *why = who + ": stat must be 0 or 1 (FXB_MATCH_ERROR, FXB_MATCH_CROSS)"; return FX_E_ARG; }
    if (family == kRankLevel && (stat < FXB_LEVEL_ENVELOPE || stat > FXB_LEVEL_QUIET)) { *why = who + ": stat must be 0 or 1 (FXB_LEVEL_ENVELOPE, FXB_LEVEL_QUIET)"; return FX_E_ARG; }
    if (family == kRankTone && (stat < 0 || stat >= kMeterMaxTones)) { *why = who + ": tone must lie in 0 .. n_tones - 1"; return FX_E_ARG; }
    if (flags & ~(unsigned)(FXB_METER_BELOW | FXB_METER_LARGEST)) { *why = who + ": flags has an unknown bit"; return FX_E_ARG; }
    if (std::isnan(threshold)) { *why = who + ": the threshold is NaN"; return FX_E_ARG; }
    if (first < 0 || nRange < 0 || first > n || nRange > n - first) { *why = who + ": first .. first + n_range - 1 must lie in 0.." + std::to_string(n - 1); return FX_E_ARG; }
    if (k < 0) { *why = who + ": k < 0"; return FX_E_ARG; }
    if (k > 0 && !list) { *why = who + ": a null list with k > 0"; return FX_E_ARG; }
    return 0;
}

int Batch::reserveMeterRank(int64_t nRange, int64_t k) { return reserveMeterStage(nRange > 0 ? meterRankStageWords(nRange, std::min(k, nRange)) : 0, false); }

int64_t Batch::meterRank(int family, int stat, int64_t k, double threshold, bool below, bool largest, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, double* value) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, "meters: metering is off (fxb_meter_enable)");
    if (family == kRankMatch && !dTarget_) return fail(FX_E_ARG, "meter target: no target is set (fxb_meter_set_target)");
    if (family == kRankLevel && !dLevel_) return fail(FX_E_ARG, "level meters: the mode is off (fxb_meter_set_level)");
    if (family == kRankTone && !dTone_) return fail(FX_E_ARG, "tone meters: the mode is off (fxb_meter_set_tones)");
    if (family == kRankTone && (stat < 0 || stat >= toneCount_)) return fail(FX_E_ARG, "meter_rank_tone: tone must lie in 0 .. n_tones - 1");
    if (nRange == 0) return 0;
    const int64_t room = std::min(k, nRange);
    const size_t words = meterRankStageWords(nRange, room);
    if (words > meterStage_.cap || words > hMeterStage_.cap) return fail(FX_E_ARG, std::string(kRankNames[family]) + ": no staging reserved (reserveMeterRank)");
    const int rc = sync();
    if (rc != 0) return rc;
    MeterRankArgs a{};
    a.rows = family == kRankMatch ? dMatch_ : family == kRankLevel ? dLevel_ : family == kRankTone ? dTone_ : dMeter_;
    a.stage = meterStage_.p;
    a.n = n_;
    a.nPad = nPad_;
    a.first = first;
    a.nRange = nRange;
    a.firstGlobal = firstGlobal;
    a.k = k;
    a.room = room;
    a.threshold = threshold;
    a.channels = prog_.numChannels;
    a.family = family;
    a.stat = stat;
    a.below = below ? 1 : 0;
    a.largest = largest ? 1 : 0;
    hipError_t e = family == kRankTone ? launchToneRank(a, stream_) : launchMeterRank(a, stream_);
    if (e == hipSuccess) ++(family == kRankMatch ? matchRanks_ : family == kRankLevel ? levelRanks_ : family == kRankTone ? toneRanks_ : meterRanks_);
    // the result words and the pairs behind them in one copy; the rest of a list above kRankHead once R says how long it is
    const int64_t head = std::min(room, kRankHead);
    unsigned long long* const h = hMeterStage_.p;
    if (e == hipSuccess) e = hipMemcpyAsync(h, meterStage_.p, (kRankResultWords + 2 * (size_t)head) * 8, hipMemcpyDeviceToHost, stream_);
    hipError_t se = hipStreamSynchronize(stream_);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hipFail(e, kRankNames[family]);
    const int64_t m = (int64_t)h[0], r = std::min((int64_t)h[1], room);
    if (r > head) {
        const size_t at = kRankResultWords + 2 * (size_t)head;
        e = hipMemcpyAsync(h + at, meterStage_.p + at, 2 * (size_t)(r - head) * 8, hipMemcpyDeviceToHost, stream_);
        se = hipStreamSynchronize(stream_);
        if (e == hipSuccess) e = se;
        if (e != hipSuccess) return hipFail(e, (std::string(kRankNames[family]) + ": the list").c_str());
    }
    // into rank order: the pairs are ascending by instance, the order is total, so the result does not depend on the sort's ways
    const unsigned long long* const pairs = h + rankPairsOff();
    const auto valueOf = [&](int64_t i) { double v; std::memcpy(&v, &pairs[2 * i + 1], 8); return v; };
    std::vector<int64_t> order((size_t)r);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return rankBefore(valueOf(x), (long long)pairs[2 * x], valueOf(y), (long long)pairs[2 * y], largest); });
    for (int64_t i = 0; i < r; ++i) {
        list[i] = (int64_t)pairs[2 * order[(size_t)i]];
        if (value) std::memcpy(&value[i], &pairs[2 * order[(size_t)i] + 1], 8);
    }
    return m;
}

}  // namespace fx
