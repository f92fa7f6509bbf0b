// fx_shard.cpp — fan-out / fan-in over the shards of a multi-GPU batch (see fx_shard.hpp).
#include "fx_shard.hpp"

#include <cmath>

#include <cstring>

#include <algorithm>
#include <stdexcept>

#include "../../include/fx8010_amd.h"

namespace fx {

namespace {
// restores the calling thread's current HIP device: fx::Batch selects its own device in every call
struct DeviceGuard {
    int prev = -1;
    bool armed = false;
    DeviceGuard() { armed = hipGetDevice(&prev) == hipSuccess; }
    ~DeviceGuard() { if (armed) (void)hipSetDevice(prev); }
};
}  // namespace

std::vector<std::pair<int64_t, int64_t>> Sharded::plan(int64_t nInstances, int nShards) {
    if (nShards < 1) throw std::runtime_error("no device given");
    if (nInstances < (int64_t)nShards) throw std::runtime_error("fewer instances than shards");
    const int64_t k = nShards;
    // contiguous ranges, whole wavefronts (64 instances) per shard: the first (waves mod k) shards get one wavefront more,
    // the last shard ends at nInstances (a ragged last wavefront)
    const int64_t waves = (nInstances + 63) / 64;
    std::vector<std::pair<int64_t, int64_t>> out;
    int64_t first = 0;
    for (int64_t i = 0; i < k; ++i) {
        const int64_t wavesHere = waves / k + (i < waves % k ? 1 : 0);
        const int64_t count = i + 1 == k ? nInstances - first : std::min<int64_t>(wavesHere * 64, nInstances - first);
        if (count < 1) throw std::runtime_error("a shard would be empty: use fewer devices for this few instances");
        out.emplace_back(first, count);
        first += count;
    }
    return out;
}

Sharded::Sharded(int64_t nInstances, int channels, const std::vector<int>& devices) : n_(nInstances) {
    const auto ranges = plan(nInstances, (int)devices.size());
    DeviceGuard guard;  // constructing a Batch selects its device on this (the caller's) thread
    for (size_t i = 0; i < devices.size(); ++i) {
        auto w = std::make_unique<Worker>();
        w->first = ranges[i].first;
        w->count = ranges[i].second;
        w->batch = std::make_unique<Batch>(w->count, channels, devices[i]);
        shards_.push_back(std::move(w));
    }
    if (shards_.size() > 1) {
        try {
            for (auto& w : shards_) w->thread = std::thread(loop, w.get());
        } catch (...) {
            stopThreads();  // a joinable std::thread must not be destroyed: stop the workers that did start, then report
            throw;
        }
    }
}

void Sharded::stopThreads() {
    for (auto& w : shards_) {
        if (!w->thread.joinable()) continue;
        {
            std::lock_guard<std::mutex> lock(w->mu);
            w->quit = true;
        }
        w->cv.notify_all();
        w->thread.join();
    }
}

Sharded::~Sharded() {
    stopThreads();
    // the batches are destroyed on this (the caller's) thread, and a Batch selects its own device to free what it holds: the
    // caller's current device is restored afterwards (found by the stand-in's multi-device scenario, tests/hipstub)
    DeviceGuard guard;
    shards_.clear();
    if (hStage_ && hipHostFree(hStage_) != hipSuccess) (void)hipGetLastError();
}

void Sharded::loop(Worker* w) {
    std::unique_lock<std::mutex> lock(w->mu);
    for (;;) {
        w->cv.wait(lock, [&] { return w->pending || w->quit; });
        if (w->quit) return;
        std::function<int()> task = std::move(w->task);
        w->pending = false;
        lock.unlock();
        int r;
        try {
            r = task();
        } catch (const std::exception& e) {
            w->batch->noteError(e.what());
            r = FX_E_MEMORY;
        }
        lock.lock();
        w->result = r;
        w->done = true;
        w->cv.notify_all();
    }
}

int Sharded::fan(const std::function<int(int, Batch&)>& f) {
    if (shards_.size() == 1) {
        DeviceGuard guard;
        return f(0, *shards_[0]->batch);
    }
    // one post at a time per handle: every worker has ONE mailbox slot, and a second host thread (a UI thread reading a register
    // while the audio thread processes a block) must not overwrite a task that has not been picked up yet - its caller would
    // wait for `done` forever.  (A handle is still not meant for concurrent use: calls are serialised, not made independent.)
    Serial post(api_);
    for (size_t k = 0; k < shards_.size(); ++k) {
        Worker* w = shards_[k].get();
        std::lock_guard<std::mutex> lock(w->mu);
        w->task = [&f, k, w] { return f((int)k, *w->batch); };
        w->pending = true;
        w->done = false;
        w->cv.notify_all();
    }
    int first = 0;
    for (auto& w : shards_) {
        std::unique_lock<std::mutex> lock(w->mu);
        w->cv.wait(lock, [&] { return w->done; });
        if (first == 0 && w->result != 0) {
            first = w->result;
            lastError_ = w->batch->lastError();
        }
    }
    return first;
}

int Sharded::runOn(int k, const std::function<int(Batch&)>& f) {
    Worker* w = shards_[(size_t)k].get();
    if (shards_.size() == 1) {
        DeviceGuard guard;
        return f(*w->batch);
    }
    Serial post(api_);
    {
        std::lock_guard<std::mutex> lock(w->mu);
        w->task = [&f, w] { return f(*w->batch); };
        w->pending = true;
        w->done = false;
        w->cv.notify_all();
    }
    std::unique_lock<std::mutex> lock(w->mu);
    w->cv.wait(lock, [&] { return w->done; });
    if (w->result != 0) lastError_ = w->batch->lastError();
    return w->result;
}

int Sharded::shardOf(int64_t inst) const {
    for (size_t k = 0; k < shards_.size(); ++k)
        if (inst >= shards_[k]->first && inst < shards_[k]->first + shards_[k]->count) return (int)k;
    return -1;
}

const std::string& Sharded::lastError() { return lastError_.empty() ? shards_.front()->batch->lastError() : lastError_; }

bool Sharded::loadFile(const std::string& path) {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int, Batch& b) { return b.loadFile(path) ? 0 : 1; }) == 0;
}
bool Sharded::loadText(const std::string& text) {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int, Batch& b) { return b.loadText(text) ? 0 : 1; }) == 0;
}
int Sharded::setRegister(const std::string& key, float v) {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int, Batch& b) { return b.setRegister(key, v); });
}
void Sharded::setChannels(int c) {
    Serial serial(api_);
    fan([&](int, Batch& b) { b.setChannels(c); return 0; });
}
int Sharded::setOption(unsigned option, bool on) {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int, Batch& b) { return b.setOption(option, on) ? -3 : 0; });
}
int Sharded::setRegisterAt(const std::string& key, int64_t inst, float v) {
    Serial serial(api_);
    lastError_.clear();
    const int k = shardOf(inst);
    if (k < 0) { lastError_ = "instance out of range"; return front().program().findRegister(key) < 0 ? 1 : FX_E_ARG; }
    return runOn(k, [&](Batch& b) { return b.setRegisterAt(key, inst - shards_[(size_t)k]->first, v); });
}
float Sharded::getRegisterAt(const std::string& key, int64_t inst) {
    Serial serial(api_);
    lastError_.clear();
    const int k = shardOf(inst);
    float out = 1.0f;
    runOn(k < 0 ? 0 : k, [&](Batch& b) { out = b.getRegisterAt(key, k < 0 ? -1 : inst - shards_[(size_t)k]->first); return 0; });
    return out;
}
int Sharded::setRegisterArray(const std::string& key, const float* values) {
    Serial serial(api_);
    lastError_.clear();
    if (!values) { lastError_ = "null buffer"; return FX_E_ARG; }
    return fan([&](int k, Batch& b) { return b.setRegisterArray(key, values + shards_[(size_t)k]->first); });
}
int Sharded::getRegisterArray(const std::string& key, float* values) {
    Serial serial(api_);
    lastError_.clear();
    if (!values) { lastError_ = "null buffer"; return FX_E_ARG; }
    return fan([&](int k, Batch& b) { return b.getRegisterArray(key, values + shards_[(size_t)k]->first); });
}
int Sharded::seedNoiseAt(int64_t inst, int32_t x1, int32_t x2) {
    Serial serial(api_);
    lastError_.clear();
    const int k = shardOf(inst);
    if (k < 0) { lastError_ = "instance out of range"; return FX_E_ARG; }
    return runOn(k, [&](Batch& b) { return b.seedNoiseAt(inst - shards_[(size_t)k]->first, x1, x2); });
}

int Sharded::setRegisterTrack(const std::string& key, const float* values, int nSteps, int period, bool perInstance) {
    Serial serial(api_);
    lastError_.clear();
    if (!values) { lastError_ = "null buffer"; return FX_E_ARG; }
    // per-instance schedules are [step][all instances]: a shard takes its columns
    return fan([&](int k, Batch& b) { return b.setRegisterTrack(key, perInstance ? values + shards_[(size_t)k]->first : values, nSteps, period, perInstance, n_); });
}

int Sharded::processHost(const float* in, float* out, int nSamples, int64_t pitch) {
    Serial serial(api_);
    lastError_.clear();
    // what goes by the instance count of the WHOLE batch, before any shard is posted: the default pitch and the refusal of a
    // narrower one (a shard would compare with its own count); every other refusal is the shards' (Batch::checkBlock)
    if (pitch == 0) pitch = n_;
    if (pitch < n_) { lastError_ = "PCM row pitch below the instance count"; return FX_E_ARG; }
    // each shard on its own thread, its device current: in place on its columns when that device can address the buffers, staged
    // copies of its columns otherwise (only that shard)
    return fan([&](int k, Batch& b) {
        const int64_t first = shards_[(size_t)k]->first;
        return b.processHost(in ? in + first : in, out ? out + first : out, nSamples, pitch);
    });
}
int Sharded::processDeviceShards(const float* const* dIn, float* const* dOut, int nSamples) {
    Serial serial(api_);
    lastError_.clear();
    if (nSamples > 0 && (!dIn || !dOut)) { lastError_ = "null buffer table"; return FX_E_ARG; }
    return fan([&](int k, Batch& b) { return b.processDevice(dIn ? dIn[k] : nullptr, dOut ? dOut[k] : nullptr, nSamples, nullptr); });
}
int Sharded::processDevice(const float* dIn, float* dOut, int nSamples, hipStream_t stream) {
    Serial serial(api_);
    lastError_.clear();
    if (shards_.size() != 1) { lastError_ = "a batch of several shards takes one buffer pair per shard: fxb_process_block_dev_shards"; return FX_E_ARG; }
    return runOn(0, [&](Batch& b) { return b.processDevice(dIn, dOut, nSamples, stream); });
}
int Sharded::processDevicePitched(const float* dIn, float* dOut, int nSamples, int64_t pitch, hipStream_t stream) {
    Serial serial(api_);
    lastError_.clear();
    if (shards_.size() != 1) { lastError_ = "a batch of several shards takes one buffer pair per shard: fxb_process_block_dev_shards"; return FX_E_ARG; }
    return runOn(0, [&](Batch& b) { return b.processDeviceChecked(dIn, dOut, nSamples, pitch, stream); });
}
int Sharded::processBus(const float* in, float* out, int nSamples, int64_t group, unsigned flags, bool device, hipStream_t stream, float* tapOut, float* auxOut, bool feed) {
    Serial serial(api_);
    lastError_.clear();
    // the refusals that go by the WHOLE batch, before any shard is posted (a refused call launches nothing on any shard)
    if (group < 1) { lastError_ = "bus: group must be at least 1"; return FX_E_ARG; }
    if (flags & ~(unsigned)Batch::kBusFlags) { lastError_ = "bus: unknown flag bits"; return FX_E_ARG; }
    if (device && shards_.size() != 1) { lastError_ = "the device entry of a bus block is for handles of one shard"; return FX_E_ARG; }
    if (feed && front().busFeedSources() < 1) { lastError_ = "bus feeds: feeds are off (fxb_bus_set_feeds)"; return FX_E_ARG; }
    if (feed && (flags & Batch::kBusSharedIn)) { lastError_ = "bus feeds: FXB_BUS_SHARED_IN does not go with a source block"; return FX_E_ARG; }
    if (tapOut && (front().busTaps() < 1 || !(flags & Batch::kBusMixOut))) {
        lastError_ = Batch::checkTapShape(nullptr, nullptr, tapOut, 0, front().busTaps(), flags, 0, 0, 0, 0);
        return FX_E_ARG;
    }
    if (auxOut && (front().busSendBuses() < 1 || !(flags & Batch::kBusMixOut))) {
        lastError_ = Batch::checkAuxShape(nullptr, nullptr, nullptr, auxOut, 0, front().busSendBuses(), 0, flags, 0, 0, 0, 0);
        return FX_E_ARG;
    }
    if (flags == 0 && !feed) return device ? processDevicePitched(in, out, nSamples, n_, stream) : processHost(in, out, nSamples, 0);
    if (shards_.size() == 1)
        return runOn(0, [&](Batch& b) { return b.processBus(in, out, nSamples, group, flags, 0, 0, device ? Batch::kBusDevice : Batch::kBusHost, stream, tapOut, auxOut, feed); });
    // (the input side of a feed block has no sum across shards: only the groups of a mixed output must not straddle)
    for (auto& w : shards_)
        if ((!feed || (flags & Batch::kBusMixOut)) && w->first % group != 0) { lastError_ = "bus: a group straddles shards (every shard must begin at a multiple of the group size: fxb_shard_plan)"; return FX_E_ARG; }
    const int64_t groups = (n_ + group - 1) / group;
    const int64_t inPitch = feed ? front().busFeedSources() : (flags & Batch::kBusSharedIn) ? groups : n_, outPitch = (flags & Batch::kBusMixOut) ? groups : n_;
    if (feed && nSamples > 0 && in && out && !Batch::feedSourceApart(in, out, (size_t)nSamples * (size_t)front().channels(), inPitch, outPitch, outPitch)) {
        lastError_ = "bus feeds: src overlaps the output (the layouts differ: there is no in-place form)";
        return FX_E_ARG;
    }
    if (!feed && nSamples > 0 && in && out && !Batch::busBuffersApart(in, out, (size_t)nSamples * (size_t)front().channels(), inPitch, inPitch, outPitch, outPitch)) {
        lastError_ = "bus: input and output overlap without being one buffer with one layout";
        return FX_E_ARG;
    }
    // (the tap rows against the footprints of ALL shards' columns; every shard gets the full-width rows and writes its columns)
    if (nSamples > 0)
        if (const char* why = Batch::checkTapShape(in, out, tapOut, (size_t)nSamples * (size_t)front().channels(), front().busTaps(), flags, inPitch, inPitch, outPitch, outPitch)) {
            lastError_ = why;
            return FX_E_ARG;
        }
    // (... and the aux rows against all of that and the tap rows)
    if (nSamples > 0)
        if (const char* why = Batch::checkAuxShape(in, out, tapOut, auxOut, (size_t)nSamples * (size_t)front().channels(), front().busSendBuses(), front().busTaps(), flags, inPitch,
                                                   inPitch, outPitch, outPitch)) {
            lastError_ = why;
            return FX_E_ARG;
        }
    return fan([&](int k, Batch& b) {
        const int64_t first = shards_[(size_t)k]->first;
        // (every shard reads the whole source block of a feed block and stages the rows on its own device)
        const float* shardIn = (in && !feed) ? in + ((flags & Batch::kBusSharedIn) ? first / group : first) : in;
        float* shardOut = out ? out + ((flags & Batch::kBusMixOut) ? first / group : first) : out;
        return b.processBus(shardIn, shardOut, nSamples, group, flags, inPitch, outPitch, Batch::kBusHost, nullptr, tapOut, auxOut, feed);
    });
}
int Sharded::processImajor(const float* in, float* out, int nSamples, int64_t inStride, int64_t outStride, bool device, hipStream_t stream) {
    Serial serial(api_);
    lastError_.clear();
    // the refusals that go by the WHOLE batch, before any shard is posted: the footprints of all instances, the packed stride
    if (device && shards_.size() != 1) { lastError_ = "the device entry of an instance-major block is for handles of one shard"; return FX_E_ARG; }
    const char* why = nullptr;
    if (Batch::checkImajorShape(in, out, nSamples, front().channels(), n_, &inStride, &outStride, &why) != 0) { lastError_ = why; return FX_E_ARG; }
    if (shards_.size() == 1)
        return runOn(0, [&](Batch& b) { return b.processImajor(in, out, nSamples, inStride, outStride, device ? Batch::kBusDevice : Batch::kBusHost, stream); });
    return fan([&](int k, Batch& b) {
        const int64_t first = shards_[(size_t)k]->first;
        return b.processImajor(in ? in + first * inStride : in, out ? out + first * outStride : out, nSamples, inStride, outStride, Batch::kBusHost, nullptr);
    });
}
int Sharded::sync() {
    Serial serial(api_);
    lastError_.clear();
    return fan([](int, Batch& b) { return b.sync(); });
}

// The allocating half of an all-or-nothing set: reserve on every shard; if any of them fails, release on all of them and keep the
// first error - no shard has changed.
int Sharded::reserveOnAll(const std::function<int(int, Batch&)>& reserve, const std::function<void(Batch&)>& release) {
    const int rc = fan(reserve);
    if (rc != 0) {
        const std::string why = lastError();
        fan([&](int, Batch& b) { release(b); return 0; });
        lastError_ = why;
    }
    return rc;
}

int Sharded::meterEnable(bool on) {
    Serial serial(api_);
    lastError_.clear();
    if (!on || front().metering()) return fan([&](int, Batch& b) { return b.meterEnable(on); });
    return reserveOnAll([](int, Batch& b) { return b.meterEnable(true); }, [](Batch& b) { b.meterEnable(false); });
}
int Sharded::meterRead(double* energy, float* peak, uint32_t* fullScale, uint32_t* nonfinite, bool reset) {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int k, Batch& b) {
        const int64_t first = shards_[(size_t)k]->first;
        return b.meterRead(energy ? energy + first : nullptr, peak ? peak + first : nullptr, fullScale ? fullScale + first : nullptr,
                           nonfinite ? nonfinite + first : nullptr, reset, n_);
    });
}
int64_t Sharded::meterSamples() {
    Serial serial(api_);
    lastError_.clear();
    const int64_t s = front().meterSamples();
    if (s < 0) lastError_ = "meters: metering is off (fxb_meter_enable)";
    return s;
}

int64_t Sharded::meterSelect(int stat, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags) {
    return selectRange(SelectRows::kMeter, stat, threshold, first, nRange, list, cap, flags);
}
int64_t Sharded::meterSelectMatch(int stat, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags) {
    return selectRange(SelectRows::kMatch, stat, threshold, first, nRange, list, cap, flags);
}
int64_t Sharded::meterSelectLevel(int stat, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags) {
    return selectRange(SelectRows::kLevel, stat, threshold, first, nRange, list, cap, flags);
}

int64_t Sharded::meterSelectTone(int tone, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags) {
    return selectRange(SelectRows::kTone, tone, threshold, first, nRange, list, cap, flags);
}

// rows: kMatch over the match rows of a target (Batch::matchSelect), kLevel over the level rows (Batch::levelSelect), kTone over
// the tone rows (Batch::toneSelect) - other
// refusals and another predicate, the same ranges and joins
int64_t Sharded::selectRange(SelectRows rows, int stat, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags) {
    Serial serial(api_);
    lastError_.clear();
    const bool match = rows == SelectRows::kMatch, level = rows == SelectRows::kLevel, tone = rows == SelectRows::kTone;
    if ((match ? Batch::checkMatchSelect : level ? Batch::checkLevelSelect : tone ? Batch::checkToneSelect : Batch::checkMeterSelect)(stat, threshold, first, nRange, n_, list, cap, flags, &lastError_) != 0) return FX_E_ARG;
    if (!front().metering()) { lastError_ = "meters: metering is off (fxb_meter_enable)"; return FX_E_ARG; }
    if (match && !front().meterTargetSet()) { lastError_ = "meter target: no target is set (fxb_meter_set_target)"; return FX_E_ARG; }
    if (level && !front().meterLevelOn()) { lastError_ = "level meters: the mode is off (fxb_meter_set_level)"; return FX_E_ARG; }
    if (tone && front().meterTones() == 0) { lastError_ = "tone meters: the mode is off (fxb_meter_set_tones)"; return FX_E_ARG; }
    if (tone && stat >= front().meterTones()) { lastError_ = "meter_select_tone: tone must lie in 0 .. n_tones - 1"; return FX_E_ARG; }
    if (nRange == 0) return 0;
    const bool below = (flags & FXB_METER_BELOW) != 0;
    const auto select = [&](Batch& b, int64_t from, int64_t count, int64_t firstGlobal, int64_t* out) {
        return match ? b.matchSelect(stat, threshold, below, from, count, firstGlobal, out, cap)
                     : level ? b.levelSelect(stat, threshold, below, from, count, firstGlobal, out, cap)
                     : tone  ? b.toneSelect(stat, threshold, below, from, count, firstGlobal, out, cap) : b.meterSelect(stat, threshold, below, from, count, firstGlobal, out, cap);
    };
    if (shards_.size() == 1) {
        if (const int rc = runOn(0, [&](Batch& b) { return b.reserveMeterSelect(nRange, cap); })) return rc;
        int64_t m = 0;
        const int rc = runOn(0, [&](Batch& b) {
            m = select(b, first, nRange, first, list);
            return m < 0 ? (int)m : 0;
        });
        return rc != 0 ? rc : m;
    }
    // the part of the range every shard owns (local numbers), and where its answer goes: a block of its own of min(cap, part)
    // numbers - what a shard finds depends on no other shard, so all of them run side by side and cap is applied as they are joined.
    // (A shard behind the one that fills cap still emits and copies back up to min(cap, part) numbers that are then dropped: the
    // price of not waiting for the shards in front.  Hosts that ask for short lists pay cap x 8 bytes per shard at the most.)
    struct Part { int64_t first = 0, count = 0, m = 0; std::vector<int64_t> found; };
    std::vector<Part> parts(shards_.size());
    for (size_t k = 0; k < shards_.size(); ++k) {
        const int64_t lo = std::max(first, shards_[k]->first), hi = std::min(first + nRange, shards_[k]->first + shards_[k]->count);
        if (hi <= lo) continue;
        parts[k].first = lo - shards_[k]->first;
        parts[k].count = hi - lo;
        parts[k].found.resize((size_t)std::min(cap, parts[k].count));
    }
    if (const int rc = fan([&](int k, Batch& b) { return b.reserveMeterSelect(parts[(size_t)k].count, cap); })) return rc;
    const int rc = fan([&](int k, Batch& b) {
        Part& p = parts[(size_t)k];
        if (p.count == 0) return 0;
        p.m = select(b, p.first, p.count, shards_[(size_t)k]->first + p.first, p.found.data());
        return p.m < 0 ? (int)p.m : 0;
    });
    if (rc != 0) return rc;
    int64_t total = 0, written = 0;
    for (const Part& p : parts) {
        const int64_t take = std::min(std::min(p.m, (int64_t)p.found.size()), cap - written);
        if (take > 0) std::memcpy(list + written, p.found.data(), (size_t)take * 8);
        written += std::max<int64_t>(take, 0);
        total += p.m;
    }
    return total;
}

int64_t Sharded::meterRank(int family, int stat, int64_t k, double threshold, int64_t first, int64_t nRange, int64_t* list, double* value, unsigned flags) {
    Serial serial(api_);
    lastError_.clear();
    if (Batch::checkMeterRank(family, stat, k, threshold, first, nRange, n_, list, flags, &lastError_) != 0) return FX_E_ARG;
    if (!front().metering()) { lastError_ = "meters: metering is off (fxb_meter_enable)"; return FX_E_ARG; }
    if (family == kRankMatch && !front().meterTargetSet()) { lastError_ = "meter target: no target is set (fxb_meter_set_target)"; return FX_E_ARG; }
    if (family == kRankLevel && !front().meterLevelOn()) { lastError_ = "level meters: the mode is off (fxb_meter_set_level)"; return FX_E_ARG; }
    if (family == kRankTone && front().meterTones() == 0) { lastError_ = "tone meters: the mode is off (fxb_meter_set_tones)"; return FX_E_ARG; }
    if (family == kRankTone && stat >= front().meterTones()) { lastError_ = "meter_rank_tone: tone must lie in 0 .. n_tones - 1"; return FX_E_ARG; }
    if (nRange == 0) return 0;
    const bool below = (flags & FXB_METER_BELOW) != 0, largest = (flags & FXB_METER_LARGEST) != 0;
    if (shards_.size() == 1) {
        if (const int rc = runOn(0, [&](Batch& b) { return b.reserveMeterRank(nRange, k); })) return rc;
        int64_t m = 0;
        const int rc = runOn(0, [&](Batch& b) {
            m = b.meterRank(family, stat, k, threshold, below, largest, first, nRange, first, list, value);
            return m < 0 ? (int)m : 0;
        });
        return rc != 0 ? rc : m;
    }
    // the part of the range every shard owns (local numbers) and a block of its own for its min(k, part) pairs: what a shard finds
    // depends on no other shard, so all of them run side by side
    struct Part { int64_t first = 0, count = 0, m = 0; std::vector<int64_t> found; std::vector<double> value; };
    std::vector<Part> parts(shards_.size());
    for (size_t s = 0; s < shards_.size(); ++s) {
        const int64_t lo = std::max(first, shards_[s]->first), hi = std::min(first + nRange, shards_[s]->first + shards_[s]->count);
        if (hi <= lo) continue;
        parts[s].first = lo - shards_[s]->first;
        parts[s].count = hi - lo;
        parts[s].found.resize((size_t)std::min(k, parts[s].count));
        parts[s].value.resize(parts[s].found.size());
    }
    if (const int rc = fan([&](int s, Batch& b) { return b.reserveMeterRank(parts[(size_t)s].count, k); })) return rc;
    const int rc = fan([&](int s, Batch& b) {
        Part& p = parts[(size_t)s];
        if (p.count == 0) return 0;
        p.m = b.meterRank(family, stat, k, threshold, below, largest, p.first, p.count, shards_[(size_t)s]->first + p.first, p.found.data(), p.value.data());
        return p.m < 0 ? (int)p.m : 0;
    });
    if (rc != 0) return rc;
    // the merge: every part is in rank order already; the head of the part that comes first under the order is taken, k times
    int64_t total = 0, written = 0;
    std::vector<size_t> at(parts.size(), 0);
    for (const Part& p : parts) total += p.m;
    while (written < std::min(k, total)) {
        int best = -1;
        for (size_t s = 0; s < parts.size(); ++s) {
            const Part& p = parts[s];
            if (at[s] >= (size_t)std::min(p.m, (int64_t)p.found.size())) continue;
            if (best < 0 || rankBefore(p.value[at[s]], p.found[at[s]], parts[(size_t)best].value[at[(size_t)best]], parts[(size_t)best].found[at[(size_t)best]], largest)) best = (int)s;
        }
        if (best < 0) break;   // (cannot be: the parts hold min(k, M_s) pairs each, together at least min(k, total))
        list[written] = parts[(size_t)best].found[at[(size_t)best]];
        if (value) value[written] = parts[(size_t)best].value[at[(size_t)best]];
        ++at[(size_t)best];
        ++written;
    }
    return total;
}

int Sharded::meterReadList(const int64_t* list, int64_t count, double* energy, float* peak, uint32_t* fullScale, uint32_t* nonfinite, bool reset) {
    Serial serial(api_);
    lastError_.clear();
    if (Batch::checkMeterList("meter_read_list", list, count, n_, reset, &lastError_) != 0) return FX_E_ARG;
    if (!front().metering()) { lastError_ = "meters: metering is off (fxb_meter_enable)"; return FX_E_ARG; }
    if (count == 0) return 0;
    const ShardLists l(*this, list, count);
    // every shard is asked for its staging first: with reset, no shard zeroes a word unless all of them can answer
    if (const int rc = fan([&](int k, Batch& b) { return b.reserveMeterList(l.count(k), true); })) return rc;
    return fan([&](int k, Batch& b) { return b.meterReadList(l.list(k), l.pos(k), l.count(k), count, energy, peak, fullScale, nonfinite, reset); });
}

int Sharded::meterResetList(const int64_t* list, int64_t count) {
    Serial serial(api_);
    lastError_.clear();
    if (Batch::checkMeterList("meter_reset_list", list, count, n_, false, &lastError_) != 0) return FX_E_ARG;
    if (!front().metering()) { lastError_ = "meters: metering is off (fxb_meter_enable)"; return FX_E_ARG; }
    if (count == 0) return 0;
    const ShardLists l(*this, list, count);
    if (const int rc = fan([&](int k, Batch& b) { return b.reserveMeterList(l.count(k), false); })) return rc;
    return fan([&](int k, Batch& b) { return b.meterResetList(l.list(k), l.count(k)); });
}

int Sharded::meterSetLevel(float release, float floor, unsigned flags) {
    Serial serial(api_);
    lastError_.clear();
    if (!front().metering()) { lastError_ = "meters: metering is off (fxb_meter_enable)"; return FX_E_ARG; }
    if (Batch::checkMeterLevel(&release, &floor, flags, &lastError_) != 0) return FX_E_ARG;
    if (const int rc = reserveOnAll([](int, Batch& b) { return b.reserveMeterLevel(); }, [](Batch& b) { b.releaseMeterLevel(); })) return rc;
    return fan([&](int, Batch& b) { return b.setMeterLevel(release, floor); });
}
int Sharded::meterClearLevel() {
    Serial serial(api_);
    lastError_.clear();
    return fan([](int, Batch& b) { return b.clearMeterLevel(); });
}
int Sharded::meterGetLevel(float* release, float* floor) {
    Serial serial(api_);
    lastError_.clear();
    return runOn(0, [&](Batch& b) { return b.getMeterLevel(release, floor); });
}
int Sharded::meterReadLevel(float* level, uint32_t* quiet, bool reset) {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int k, Batch& b) {
        const int64_t first = shards_[(size_t)k]->first;
        return b.meterReadLevel(level ? level + first : nullptr, quiet ? quiet + first : nullptr, reset, n_);
    });
}
int Sharded::meterReadLevelList(const int64_t* list, int64_t count, float* level, uint32_t* quiet, bool reset) {
    Serial serial(api_);
    lastError_.clear();
    if (Batch::checkMeterList("meter_read_level_list", list, count, n_, reset, &lastError_) != 0) return FX_E_ARG;
    if (!front().metering()) { lastError_ = "meters: metering is off (fxb_meter_enable)"; return FX_E_ARG; }
    if (!front().meterLevelOn()) { lastError_ = "level meters: the mode is off (fxb_meter_set_level)"; return FX_E_ARG; }
    if (count == 0) return 0;
    const ShardLists l(*this, list, count);
    // every shard is asked for its staging first: with reset, no shard zeroes a word unless all of them can answer
    if (const int rc = fan([&](int k, Batch& b) { return b.reserveMeterList(l.count(k), true); })) return rc;
    return fan([&](int k, Batch& b) { return b.meterReadLevelList(l.list(k), l.pos(k), l.count(k), count, level, quiet, reset); });
}

int Sharded::meterSetTones(int tones, const double* coeff, unsigned flags) {
    Serial serial(api_);
    lastError_.clear();
    if (!front().metering()) { lastError_ = "meters: metering is off (fxb_meter_enable)"; return FX_E_ARG; }
    double canonical[kMeterMaxTones] = {};
    if (Batch::checkMeterTones(tones, coeff, flags, canonical, &lastError_) != 0) return FX_E_ARG;
    if (const int rc = reserveOnAll([tones](int, Batch& b) { return b.reserveMeterTones(tones); }, [](Batch& b) { b.releaseMeterTones(); })) return rc;
    return fan([&](int, Batch& b) { return b.setMeterTones(tones, canonical); });
}
int Sharded::meterClearTones() {
    Serial serial(api_);
    lastError_.clear();
    return fan([](int, Batch& b) { return b.clearMeterTones(); });
}
int Sharded::meterGetTones(int* tones, double* coeff) {
    Serial serial(api_);
    lastError_.clear();
    return runOn(0, [&](Batch& b) { return b.getMeterTones(tones, coeff); });
}
int Sharded::meterReadTones(double* s1, double* s2, double* power, bool reset) {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int k, Batch& b) {
        const int64_t first = shards_[(size_t)k]->first;
        return b.meterReadTones(s1 ? s1 + first : nullptr, s2 ? s2 + first : nullptr, power ? power + first : nullptr, reset, n_);
    });
}
int Sharded::meterReadTonesList(const int64_t* list, int64_t count, double* s1, double* s2, double* power, bool reset) {
    Serial serial(api_);
    lastError_.clear();
    if (Batch::checkMeterList("meter_read_tones_list", list, count, n_, reset, &lastError_) != 0) return FX_E_ARG;
    if (!front().metering()) { lastError_ = "meters: metering is off (fxb_meter_enable)"; return FX_E_ARG; }
    if (front().meterTones() == 0) { lastError_ = "tone meters: the mode is off (fxb_meter_set_tones)"; return FX_E_ARG; }
    if (count == 0) return 0;
    const ShardLists l(*this, list, count);
    // every shard is asked for its staging first: with reset, no shard zeroes a word unless all of them can answer
    if (const int rc = fan([&](int k, Batch& b) { return b.reserveToneList(l.count(k)); })) return rc;
    return fan([&](int k, Batch& b) { return b.meterReadTonesList(l.list(k), l.pos(k), l.count(k), count, s1, s2, power, reset); });
}

int Sharded::meterSetTarget(const float* target, int64_t nSamples, int64_t group, unsigned flags) {
    Serial serial(api_);
    lastError_.clear();
    if (!front().metering()) { lastError_ = "meters: metering is off (fxb_meter_enable)"; return FX_E_ARG; }
    if (Batch::checkMeterTarget(target, nSamples, group, flags, front().channels(), n_, &lastError_) != 0) return FX_E_ARG;
    // (group >= N is one column for everyone: the same as group = N, which keeps the kernels' products small)
    const int64_t g = std::min(group, n_), cols = (n_ + g - 1) / g;
    const bool loop = (flags & FXB_METER_TARGET_LOOP) != 0;
    if (const int rc = reserveOnAll([&](int k, Batch& b) { return b.reserveMeterTarget(nSamples, g, shards_[(size_t)k]->first); }, [](Batch& b) { b.releaseMeterTarget(); })) return rc;
    return fan([&](int k, Batch& b) { return b.setMeterTarget(target, nSamples, g, shards_[(size_t)k]->first, cols, loop); });
}
int Sharded::meterClearTarget() {
    Serial serial(api_);
    lastError_.clear();
    return fan([](int, Batch& b) { return b.clearMeterTarget(); });
}
int Sharded::meterTargetSeek(int64_t pos) {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int, Batch& b) { return b.meterTargetSeek(pos); });
}
int64_t Sharded::meterTargetPos() {
    Serial serial(api_);
    lastError_.clear();
    const int64_t p = front().meterTargetPos();
    if (p < 0) lastError_ = "meter target: no target is set (fxb_meter_set_target)";
    return p;
}
int Sharded::meterReadMatch(double* err, double* cross, bool reset) {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int k, Batch& b) {
        const int64_t first = shards_[(size_t)k]->first;
        return b.meterReadMatch(err ? err + first : nullptr, cross ? cross + first : nullptr, reset, n_);
    });
}
int Sharded::meterBest(int stat, int64_t group, int64_t* winner, double* value, unsigned flags) {
    Serial serial(api_);
    lastError_.clear();
    if (group < 1) { lastError_ = "meter_best: group must be at least 1"; return FX_E_ARG; }
    if (flags & ~(unsigned)FXB_MATCH_LARGEST) { lastError_ = "meter_best: flags has an unknown bit"; return FX_E_ARG; }
    if (stat < FXB_MATCH_ERROR || stat > FXB_MATCH_CROSS) { lastError_ = "meter_best: stat must be 0 or 1 (FXB_MATCH_ERROR, FXB_MATCH_CROSS)"; return FX_E_ARG; }
    if (!front().metering()) { lastError_ = "meters: metering is off (fxb_meter_enable)"; return FX_E_ARG; }
    if (!front().meterTargetSet()) { lastError_ = "meter target: no target is set (fxb_meter_set_target)"; return FX_E_ARG; }
    const int64_t g = std::min(group, n_);
    const bool largest = (flags & FXB_MATCH_LARGEST) != 0;
    if (const int rc = fan([&](int k, Batch& b) { return b.reserveMeterBest(g, shards_[(size_t)k]->first); })) return rc;
    if (shards_.size() == 1) return runOn(0, [&](Batch& b) { return b.meterBest(stat, g, 0, largest, winner, value); });
    // every shard's partial winners side by side; then the groups in order, a group that straddles joined by (V, then n)
    struct Part { std::vector<int64_t> winner; std::vector<double> value; };
    std::vector<Part> parts(shards_.size());
    for (size_t k = 0; k < shards_.size(); ++k) {
        const size_t groups = (size_t)shards_[k]->batch->meterBestGroups(g, shards_[k]->first);
        parts[k].winner.resize(groups);
        parts[k].value.resize(groups);
    }
    if (const int rc = fan([&](int k, Batch& b) { return b.meterBest(stat, g, shards_[(size_t)k]->first, largest, parts[(size_t)k].winner.data(), parts[(size_t)k].value.data()); })) return rc;
    int64_t done = -1;       // the last group written
    double held = 0.0;       // ... and its value so far
    for (size_t k = 0; k < shards_.size(); ++k) {
        const int64_t firstGroup = shards_[k]->first / g;
        for (size_t i = 0; i < parts[k].winner.size(); ++i) {
            const int64_t at = firstGroup + (int64_t)i, w = parts[k].winner[i];
            const double v = parts[k].value[i];
            if (at > done) {
                if (winner) winner[at] = w;
                if (value) value[at] = v;
                held = v;
                done = at;
                continue;
            }
            // (the group's members on the shards in front have smaller numbers: a tie stays with them)
            const bool better = v != held && (largest ? v > held : v < held);
            if (!better) continue;
            if (winner) winner[at] = w;
            if (value) value[at] = v;
            held = v;
        }
    }
    return 0;
}

int Sharded::busSetGains(const float* gains, int ramp) {
    Serial serial(api_);
    lastError_.clear();
    if (ramp != 0 && ramp != 1) { lastError_ = "bus gains: ramp must be 0 or 1"; return FX_E_ARG; }
    if (!gains) return fan([](int, Batch& b) { return b.busSetGains(nullptr, 0, 0); });
    if (!Batch::gainsFinite(gains, front().channels(), n_, n_)) { lastError_ = "bus gains: every gain must be finite"; return FX_E_ARG; }
    // (the release: a no-op on a shard whose gains are on)
    if (const int rc = reserveOnAll([](int, Batch& b) { return b.busReserveGains(); }, [](Batch& b) { b.busReleaseGains(); })) return rc;
    return fan([&](int k, Batch& b) { return b.busSetGains(gains + shards_[(size_t)k]->first, n_, ramp, true); });
}
int Sharded::busGetGains(float* gains) {
    Serial serial(api_);
    lastError_.clear();
    if (front().busGainsOn() && !gains) { lastError_ = "null buffer"; return FX_E_ARG; }
    return fan([&](int k, Batch& b) { return b.busGetGains(gains ? gains + shards_[(size_t)k]->first : nullptr, n_); });
}

int Sharded::busSetTaps(const int64_t* list, int64_t count) {
    Serial serial(api_);
    lastError_.clear();
    if (count < 0 || count > Batch::kMaxTaps) { lastError_ = "bus taps: count must be 0..65536"; return FX_E_ARG; }
    if (count > 0 && !list) { lastError_ = "bus taps: a null list"; return FX_E_ARG; }
    for (int64_t k = 0; k < count; ++k)
        if (list[k] < 0 || list[k] >= n_) { lastError_ = "bus taps: an entry outside 0..N-1"; return FX_E_ARG; }
    if (count == 0) return fan([](int, Batch& b) { return b.busSetTaps(nullptr, nullptr, 0, 0); });
    if (shards_.size() == 1) return runOn(0, [&](Batch& b) { return b.busSetTaps(list, nullptr, count, count); });
    // every shard reserves the block of its entries first; only when all of them could does any shard's list change
    const ShardLists l(*this, list, count);
    if (const int rc = reserveOnAll([&](int k, Batch& b) { return b.busReserveTaps(l.count(k)); }, [](Batch& b) { b.busReleaseTaps(); })) return rc;
    return fan([&](int k, Batch& b) { return b.busSetTaps(l.list(k), l.pos(k), l.count(k), count); });
}
int64_t Sharded::busGetTaps(int64_t* list, int64_t cap) {
    Serial serial(api_);
    lastError_.clear();
    if (cap < 0 || (cap > 0 && !list)) { lastError_ = "bus taps: a null list with room asked for"; return FX_E_ARG; }
    int64_t total = 0;
    for (auto& w : shards_) total = w->batch->busGetTaps(list, cap, w->first);   // (host state only: no device call)
    return total;
}

int Sharded::busSetSends(int64_t nAux, const int64_t* offsets, const int64_t* members, const float* gains) {
    Serial serial(api_);
    lastError_.clear();
    if (nAux < 0 || nAux > Batch::kMaxSendBuses) { lastError_ = "bus sends: n_aux must be 0..65536"; return FX_E_ARG; }
    if (nAux == 0) return fan([](int, Batch& b) { return b.busSetSends(Batch::SendSet{}); });
    if (!offsets) { lastError_ = "bus sends: null offsets"; return FX_E_ARG; }
    if (offsets[0] != 0) { lastError_ = "bus sends: offsets[0] must be 0"; return FX_E_ARG; }
    for (int64_t b = 0; b < nAux; ++b)
        if (offsets[b + 1] < offsets[b]) { lastError_ = "bus sends: offsets must not decrease"; return FX_E_ARG; }
    const int64_t entries = offsets[nAux];
    if (entries > Batch::kMaxSendEntries) { lastError_ = "bus sends: more than 16 777 216 entries"; return FX_E_ARG; }
    if (entries > 0 && !members) { lastError_ = "bus sends: null members"; return FX_E_ARG; }
    for (int64_t e = 0; e < entries; ++e)
        if (members[e] < 0 || members[e] >= n_) { lastError_ = "bus sends: a member outside 0..N-1"; return FX_E_ARG; }
    const size_t ch = (size_t)front().channels();
    if (gains && !Batch::gainsFinite(gains, (int)ch, entries, entries)) { lastError_ = "bus sends: every gain must be finite"; return FX_E_ARG; }
    // a bus is summed where its members live: no collective on the data path, and no bits that depend on the split
    std::vector<int> owner((size_t)nAux, 0);
    for (int64_t b = 0; b < nAux; ++b)
        for (int64_t e = offsets[b]; e < offsets[b + 1]; ++e) {
            const int s = shardOf(members[e]);
            if (e == offsets[b]) owner[(size_t)b] = s;
            else if (s != owner[(size_t)b]) {
                lastError_ = "bus sends: the members of aux bus " + std::to_string(b) + " fall into more than one shard (fxb_shard_plan tells the boundaries)";
                return FX_E_ARG;
            }
        }
    std::vector<Batch::SendSet> parts(shards_.size());
    for (size_t k = 0; k < parts.size(); ++k) {
        parts[k].totalBuses = nAux;
        parts[k].totalEntries = entries;
    }
    for (int64_t b = 0; b < nAux; ++b) {
        Batch::SendSet& part = parts[(size_t)owner[(size_t)b]];
        const int64_t first = shards_[(size_t)owner[(size_t)b]]->first;
        for (int64_t e = offsets[b]; e < offsets[b + 1]; ++e) part.members.push_back(members[e] - first);
        part.offsets.push_back((int64_t)part.members.size());
        part.column.push_back(b);
        part.first.push_back(offsets[b]);
    }
    for (Batch::SendSet& part : parts) {
        const size_t mine = part.members.size();
        part.gain[0].assign(ch * mine, 1.0f);
        if (gains)
            for (size_t c = 0; c < ch; ++c)
                for (size_t j = 0; j < part.column.size(); ++j) {
                    const size_t lo = (size_t)part.offsets[j], count = (size_t)part.offsets[j + 1] - lo;
                    if (count > 0) std::memcpy(&part.gain[0][c * mine + lo], gains + c * (size_t)entries + (size_t)part.first[j], count * 4);
                }
    }
    // every shard reserves the block of its buses first; only when all of them could does any shard's structure change
    const auto reserve = [&](int k, Batch& b) {
        const Batch::SendSet& part = parts[(size_t)k];
        return b.busReserveSends((int64_t)part.column.size(), (int64_t)part.members.size(), (int64_t)part.chunkCount());
    };
    if (const int rc = reserveOnAll(reserve, [](Batch& b) { b.busReleaseSends(); })) return rc;
    return fan([&](int k, Batch& b) { return b.busSetSends(std::move(parts[(size_t)k])); });
}
int Sharded::busSetSendGains(const float* gains, int ramp) {
    Serial serial(api_);
    lastError_.clear();
    if (ramp != 0 && ramp != 1) { lastError_ = "bus sends: ramp must be 0 or 1"; return FX_E_ARG; }
    if (front().busSendBuses() < 1) { lastError_ = "bus sends: sends are off (fxb_bus_set_sends)"; return FX_E_ARG; }
    const int64_t entries = front().busSendEntries();
    if (entries > 0 && !gains) { lastError_ = "null buffer"; return FX_E_ARG; }
    if (!Batch::gainsFinite(gains, front().channels(), entries, entries)) { lastError_ = "bus sends: every gain must be finite"; return FX_E_ARG; }
    return fan([&](int, Batch& b) { return b.busSetSendGains(gains, ramp); });
}
int64_t Sharded::busGetSends(int64_t* nAux, int64_t* offsets, int64_t offCap, int64_t* members, float* gains, int64_t cap) {
    Serial serial(api_);
    lastError_.clear();
    if (offCap < 0 || cap < 0) { lastError_ = "bus sends: a negative capacity"; return FX_E_ARG; }
    if (nAux) *nAux = front().busSendBuses();
    int64_t total = 0;
    for (auto& w : shards_) total = w->batch->busGetSends(offsets, offCap, members, gains, cap, w->first);   // (host state only: no device call)
    return total;
}

int Sharded::busSetFeeds(int64_t nSrc, const int64_t* offsets, const int64_t* sources, const float* gains) {
    Serial serial(api_);
    lastError_.clear();
    const size_t ch = (size_t)front().channels();
    if (nSrc < 0) { lastError_ = "bus feeds: n_src must not be negative"; return FX_E_ARG; }
    if ((uint64_t)ch * (uint64_t)nSrc * 4u >= ((uint64_t)1 << 32)) { lastError_ = "bus feeds: channels * n_src * 4 must stay below 2^32"; return FX_E_ARG; }
    if (nSrc == 0) return fan([](int, Batch& b) { return b.busSetFeeds(Batch::FeedSet{}); });
    if (!offsets) { lastError_ = "bus feeds: null offsets"; return FX_E_ARG; }
    if (offsets[0] != 0) { lastError_ = "bus feeds: offsets[0] must be 0"; return FX_E_ARG; }
    for (int64_t i = 0; i < n_; ++i)
        if (offsets[i + 1] < offsets[i]) { lastError_ = "bus feeds: offsets must not decrease"; return FX_E_ARG; }
    const int64_t entries = offsets[n_];
    if (entries > Batch::kMaxFeedEntries) { lastError_ = "bus feeds: more than 16 777 216 entries"; return FX_E_ARG; }
    if (entries > 0 && !sources) { lastError_ = "bus feeds: null sources"; return FX_E_ARG; }
    for (int64_t e = 0; e < entries; ++e)
        if (sources[e] < 0 || sources[e] >= nSrc) { lastError_ = "bus feeds: a source outside 0..M-1"; return FX_E_ARG; }
    if (gains && !Batch::gainsFinite(gains, (int)ch, entries, entries)) { lastError_ = "bus feeds: every gain must be finite"; return FX_E_ARG; }
    // a shard's instances own a contiguous run of the entries
    std::vector<Batch::FeedSet> parts(shards_.size());
    for (size_t k = 0; k < parts.size(); ++k) {
        Batch::FeedSet& part = parts[k];
        const int64_t first = shards_[k]->first, count = shards_[k]->batch->instances();
        const int64_t lo = offsets[first], mine = offsets[first + count] - lo;
        part.sources = nSrc;
        part.totalEntries = entries;
        part.first = lo;
        part.weighted = gains != nullptr;
        part.offsets.resize((size_t)count + 1);
        for (int64_t i = 0; i <= count; ++i) part.offsets[(size_t)i] = offsets[first + i] - lo;
        part.columns.assign(sources + lo, sources + lo + mine);
        part.gain[0].assign(ch * (size_t)mine, 1.0f);
        if (gains)
            for (size_t c = 0; c < ch && mine > 0; ++c) std::memcpy(&part.gain[0][c * (size_t)mine], gains + c * (size_t)entries + (size_t)lo, (size_t)mine * 4);
    }
    // every shard reserves the block of its lists first; only when all of them could does any shard's structure change
    const auto reserve = [&](int k, Batch& b) {
        const Batch::FeedSet& part = parts[(size_t)k];
        return b.busReserveFeeds(nSrc, (int64_t)part.columns.size(), part.isMap());
    };
    if (const int rc = reserveOnAll(reserve, [](Batch& b) { b.busReleaseFeeds(); })) return rc;
    return fan([&](int k, Batch& b) { return b.busSetFeeds(std::move(parts[(size_t)k])); });
}
int Sharded::busSetFeedGains(const float* gains, int ramp) {
    Serial serial(api_);
    lastError_.clear();
    if (ramp != 0 && ramp != 1) { lastError_ = "bus feeds: ramp must be 0 or 1"; return FX_E_ARG; }
    if (front().busFeedSources() < 1) { lastError_ = "bus feeds: feeds are off (fxb_bus_set_feeds)"; return FX_E_ARG; }
    if (gains && !Batch::gainsFinite(gains, front().channels(), front().busFeedEntries(), front().busFeedEntries())) { lastError_ = "bus feeds: every gain must be finite"; return FX_E_ARG; }
    return fan([&](int, Batch& b) { return b.busSetFeedGains(gains, ramp); });
}
int64_t Sharded::busGetFeeds(int64_t* nSrc, int64_t* offsets, int64_t offCap, int64_t* sources, float* gains, int64_t cap) {
    Serial serial(api_);
    lastError_.clear();
    if (offCap < 0 || cap < 0) { lastError_ = "bus feeds: a negative capacity"; return FX_E_ARG; }
    if (nSrc) *nSrc = front().busFeedSources();
    for (auto& w : shards_) w->batch->busGetFeeds(offsets, offCap, sources, gains, cap, w->first);   // (host state only: no device call)
    return front().busFeedEntries();
}

int Sharded::busSetGainList(GainListKind kind, const int64_t* list, int64_t count, const float* gains, int ramp) {
    Serial serial(api_);
    lastError_.clear();
    static const char* const kNames[3] = {"bus gains by list", "bus send gains by list", "bus feed gains by list"};
    const char* name = kNames[kind];
    if (ramp != 0 && ramp != 1) { lastError_ = std::string(name) + ": ramp must be 0 or 1"; return FX_E_ARG; }
    if (count < 0) { lastError_ = std::string(name) + ": count < 0"; return FX_E_ARG; }
    int64_t range = 0;
    if (kind == kGainList) {
        if (!front().busGainsOn()) { lastError_ = "bus gains by list: gains are off (fxb_bus_set_gains)"; return FX_E_ARG; }
        range = n_;
    } else if (kind == kSendGainList) {
        if (front().busSendBuses() < 1) { lastError_ = "bus send gains by list: sends are off (fxb_bus_set_sends)"; return FX_E_ARG; }
        range = front().busSendEntries();
    } else {
        if (front().busFeedSources() < 1) { lastError_ = "bus feed gains by list: feeds are off (fxb_bus_set_feeds)"; return FX_E_ARG; }
        range = front().busFeedEntries();
    }
    if (count == 0) return 0;
    if (Batch::checkGainList(list, count, range, gains, front().channels(), name, &lastError_) != 0) return FX_E_ARG;
    const auto set = [&](Batch& b, const int64_t* l, const int64_t* pos, int64_t mine) {
        return kind == kGainList ? b.busSetGainsList(l, pos, mine, count, gains, ramp)
             : kind == kSendGainList ? b.busSetSendGainsList(l, pos, mine, count, gains, ramp)
                                     : b.busSetFeedGainsList(l, pos, mine, count, gains, ramp);
    };
    // (one shard: a global number is a local one - every bus and every list is its own, from entry 0 on)
    if (shards_.size() == 1)
        return runOn(0, [&](Batch& b) {
            const int rc = b.busReserveGainList(count);
            return rc != 0 ? rc : set(b, list, nullptr, count);
        });
    std::vector<ListPart> parts(shards_.size());
    if (kind == kGainList) parts = splitList(list, count);
    else
        for (int64_t k = 0; k < count; ++k) {
            size_t s = 0;
            int64_t local = -1;
            for (; s < shards_.size() && local < 0; ++s) local = kind == kSendGainList ? shards_[s]->batch->busSendLocalEntry(list[k]) : shards_[s]->batch->busFeedLocalEntry(list[k]);
            if (local < 0) { lastError_ = std::string(name) + ": an entry that no shard holds"; return FX_E_ARG; }   // (host state only; never, behind the range check)
            parts[s - 1].list.push_back(local);
            parts[s - 1].pos.push_back(k);
        }
    // every shard reserves its staging first; only when all of them could does any shard's state change (staging that has grown
    // stays: it is no state)
    const ShardLists l(std::move(parts));
    if (const int rc = fan([&](int k, Batch& b) { return b.busReserveGainList(l.count(k)); })) return rc;
    return fan([&](int k, Batch& b) { return set(b, l.list(k), l.pos(k), l.count(k)); });
}

int64_t Sharded::instructionCounter() {
    Serial serial(api_);
    std::vector<int64_t> part(shards_.size(), 0);
    fan([&](int k, Batch& b) { part[(size_t)k] = b.instructionCounter(); return 0; });
    int64_t sum = 0;
    for (int64_t p : part) {
        if (p < 0) return -1;
        sum += p;
    }
    return sum;
}
int64_t Sharded::instructionCounterAt(int64_t inst) {
    Serial serial(api_);
    const int k = shardOf(inst);
    if (k < 0) return 0;
    int64_t out = 0;
    runOn(k, [&](Batch& b) { out = b.instructionCounterAt(inst - shards_[(size_t)k]->first); return 0; });
    return out;
}
uint32_t Sharded::oodFlags() {
    Serial serial(api_);
    std::vector<uint32_t> part(shards_.size(), 0);
    fan([&](int k, Batch& b) { part[(size_t)k] = b.oodFlags(); return 0; });
    uint32_t all = 0;
    for (uint32_t p : part) all |= p;
    return all;
}
float Sharded::lastKernelMs() {
    Serial serial(api_);
    std::vector<float> part(shards_.size(), -1.0f);
    fan([&](int k, Batch& b) { part[(size_t)k] = b.lastKernelMs(); return 0; });  // (a shard's events belong to its thread's device)
    float worst = -1.0f;
    for (float p : part) worst = std::max(worst, p);
    return worst;
}
int64_t Sharded::stateBytes() {
    Serial serial(api_);
    lastError_.clear();
    Batch::SnapshotHeader hdr;
    if (runOn(0, [&](Batch& b) { return b.snapshotShape(&hdr); }) != 0) return -1;
    hdr.n = n_;
    return Batch::snapshotBytes(hdr);
}
int Sharded::saveState(void* buf, int64_t cap) {
    Serial serial(api_);
    lastError_.clear();
    Batch::SnapshotHeader hdr;
    int rc = runOn(0, [&](Batch& b) { return b.snapshotShape(&hdr); });
    if (rc != 0) return rc;
    hdr.n = n_;
    if (!buf || cap < Batch::snapshotBytes(hdr)) { lastError_ = "save_state: buffer smaller than fxb_state_size()"; return FX_E_ARG; }
    std::memcpy(buf, &hdr, sizeof(hdr));
    return fan([&](int k, Batch& b) { return b.saveStateColumns(static_cast<uint8_t*>(buf), hdr, shards_[(size_t)k]->first); });
}
int Sharded::loadState(const void* buf, int64_t bytes) {
    Serial serial(api_);
    lastError_.clear();
    Batch::SnapshotHeader hdr;
    if (!buf || bytes < (int64_t)sizeof(hdr)) { lastError_ = "load_state: no image"; return FX_E_ARG; }
    std::memcpy(&hdr, buf, sizeof(hdr));
    // the header is the caller's (a file that may be damaged): version, every count and the size they imply are checked here,
    // before a shard computes a single address from them
    const Batch::SnapshotHeader ours;
    const int64_t need = Batch::snapshotBytes(hdr);
    if (hdr.magic != ours.magic || hdr.version != ours.version || hdr.n != n_ || need < 0 || bytes < need) {
        lastError_ = "load_state: not a state image of a batch of this many instances (wrong version, damaged header or truncated)";
        return FX_E_ARG;
    }
    return fan([&](int k, Batch& b) { return b.loadStateColumns(static_cast<const uint8_t*>(buf), hdr, shards_[(size_t)k]->first); });
}

// ---- per-instance state calls -----------------------------------------------------------------------------------------------------
std::vector<Sharded::ListPart> Sharded::splitList(const int64_t* list, int64_t count) const {
    std::vector<ListPart> parts(shards_.size());
    for (int64_t k = 0; k < count; ++k) {
        const int s = shardOf(list[k]);   // (the list has been checked: every entry has a shard)
        parts[(size_t)s].list.push_back(list[k] - shards_[(size_t)s]->first);
        parts[(size_t)s].pos.push_back(k);
    }
    return parts;
}

int64_t Sharded::instanceImageBytes(int64_t count) {
    Serial serial(api_);
    lastError_.clear();
    if (count < 0 || count >= ((int64_t)1 << 31)) { lastError_ = "instance image: count out of range"; return FX_E_ARG; }
    Batch::SnapshotHeader hdr;
    const int rc = runOn(0, [&](Batch& b) { return b.instanceShape(&hdr, count); });
    if (rc != 0) return rc;
    return (int64_t)sizeof(hdr) + count * Batch::instanceWords(hdr) * 4;
}

int Sharded::growStage(size_t words, const char* who) {
    if (words <= stageWords_) return 0;
    if (hStage_ && hipHostFree(hStage_) != hipSuccess) (void)hipGetLastError();
    hStage_ = nullptr;
    stageWords_ = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&hStage_), words * 4, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        hStage_ = nullptr;
        lastError_ = who;
        return FX_E_MEMORY;
    }
    stageWords_ = words;
    return 0;
}

int Sharded::copyInstances(const int64_t* src, const int64_t* dst, int64_t count) {
    Serial serial(api_);
    lastError_.clear();
    const char* why = nullptr;
    if (count > 0 && (!src || !dst)) { lastError_ = "instances: a null list"; return FX_E_ARG; }
    if (Batch::checkInstanceLists(src, dst, count, n_, &why) != 0) { lastError_ = why; return FX_E_ARG; }
    if (shards_.size() == 1) return runOn(0, [&](Batch& b) { return b.copyInstances(src, dst, count); });
    // pairs inside a shard: local lists for that shard; the others: (source shard, local source, destination shard, local destination)
    struct Pairs { std::vector<int64_t> src, dst; };
    std::vector<Pairs> inside(shards_.size());
    struct Cross { int from, to; int64_t src, dst; };
    std::vector<Cross> cross;
    for (int64_t k = 0; k < count; ++k) {
        const int f = shardOf(src[k]), t = shardOf(dst[k]);
        const int64_t ls = src[k] - shards_[(size_t)f]->first, ld = dst[k] - shards_[(size_t)t]->first;
        if (f == t) { inside[(size_t)f].src.push_back(ls); inside[(size_t)f].dst.push_back(ld); }
        else cross.push_back({f, t, ls, ld});
    }
    // (by source shard, then by destination shard: a shard's records are runs of the staging block, one copy each)
    std::stable_sort(cross.begin(), cross.end(), [](const Cross& a, const Cross& b) { return a.from != b.from ? a.from < b.from : a.to < b.to; });
    int rc = fan([&](int k, Batch& b) { return b.copyInstances(inside[(size_t)k].src.data(), inside[(size_t)k].dst.data(), (int64_t)inside[(size_t)k].src.size()); });
    if (rc != 0 || cross.empty()) return rc;
    Batch::SnapshotHeader hdr;
    if ((rc = runOn(0, [&](Batch& b) { return b.instanceShape(&hdr, 0); })) != 0) return rc;
    const size_t W = (size_t)Batch::instanceWords(hdr), chunk = std::max<size_t>(kStageBytes / (W * 4), 1);
    if ((rc = growStage(std::min(chunk, cross.size()) * W, "copy_instances: no pinned staging for the pairs that cross shards")) != 0) return rc;
    for (size_t c0 = 0; c0 < cross.size() && rc == 0; c0 += chunk) {
        const size_t m = std::min(chunk, cross.size() - c0);
        std::vector<ListPart> from(shards_.size()), to(shards_.size());
        for (size_t k = 0; k < m; ++k) {
            const Cross& x = cross[c0 + k];
            from[(size_t)x.from].list.push_back(x.src); from[(size_t)x.from].pos.push_back((int64_t)k);
            to[(size_t)x.to].list.push_back(x.dst); to[(size_t)x.to].pos.push_back((int64_t)k);
        }
        // every gather of the chunk has finished (fan waits for all shards) before a scatter starts
        rc = fan([&](int k, Batch& b) { return b.gatherRecords(from[(size_t)k].list.data(), from[(size_t)k].pos.data(), (int64_t)from[(size_t)k].list.size(), hStage_); });
        if (rc == 0) rc = fan([&](int k, Batch& b) { return b.scatterRecords(to[(size_t)k].list.data(), to[(size_t)k].pos.data(), (int64_t)to[(size_t)k].list.size(), hStage_); });
    }
    return rc;
}

int Sharded::resetInstances(const int64_t* list, int64_t count) {
    Serial serial(api_);
    lastError_.clear();
    const char* why = nullptr;
    if (count > 0 && !list) { lastError_ = "instances: a null list"; return FX_E_ARG; }
    if (Batch::checkInstanceLists(nullptr, list, count, n_, &why) != 0) { lastError_ = why; return FX_E_ARG; }
    const ShardLists l(*this, list, count);
    return fan([&](int k, Batch& b) { return b.resetInstances(l.list(k), l.count(k)); });
}

int Sharded::saveInstances(const int64_t* list, int64_t count, void* buf, int64_t cap) {
    Serial serial(api_);
    lastError_.clear();
    const char* why = nullptr;
    if (count > 0 && !list) { lastError_ = "instances: a null list"; return FX_E_ARG; }
    if (Batch::checkInstanceLists(list, nullptr, count, n_, &why) != 0) { lastError_ = why; return FX_E_ARG; }
    Batch::SnapshotHeader hdr;
    int rc = runOn(0, [&](Batch& b) { return b.instanceShape(&hdr, count); });
    if (rc != 0) return rc;
    if (count == 0 && (!buf || cap < (int64_t)sizeof(hdr))) return 0;   // (nothing to save; a buffer that holds a header gets one)
    if (!buf || cap < (int64_t)sizeof(hdr) + count * Batch::instanceWords(hdr) * 4) { lastError_ = "save_instances: buffer smaller than fxb_instance_image_size()"; return FX_E_ARG; }
    std::memcpy(buf, &hdr, sizeof(hdr));
    uint32_t* records = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(buf) + sizeof(hdr));
    const ShardLists l(*this, list, count);
    return fan([&](int k, Batch& b) { return b.gatherRecords(l.list(k), l.pos(k), l.count(k), records); });
}

int Sharded::loadRecords(const int64_t* list, int64_t count, const void* buf, int64_t bytes, bool rotated) {
    Serial serial(api_);
    lastError_.clear();
    const char* why = nullptr;
    if (count > 0 && !list) { lastError_ = "instances: a null list"; return FX_E_ARG; }
    if (Batch::checkInstanceLists(nullptr, list, count, n_, &why) != 0) { lastError_ = why; return FX_E_ARG; }
    Batch::SnapshotHeader hdr;
    if (count == 0) return runOn(0, [&](Batch& b) { return b.instanceShape(&hdr, 0); });   // (nothing to load; FX_E_NOTREADY without a program)
    if (!buf || bytes < (int64_t)sizeof(hdr)) { lastError_ = "load_instances: no image"; return FX_E_ARG; }
    std::memcpy(&hdr, buf, sizeof(hdr));
    int rc = runOn(0, [&](Batch& b) { return b.checkInstanceImage(hdr, count, bytes); });
    if (rc != 0 || count == 0) return rc;
    const uint32_t* records = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(buf) + sizeof(hdr));
    const ShardLists l(*this, list, count);
    // the delay-line rule on every shard before any shard changes a word
    if (rotated) {
        bool applies = false;
        if ((rc = runOn(0, [&](Batch& b) { return b.rotationApplies(&applies); })) != 0) return rc;
        rotated = applies;
    }
    std::vector<std::vector<int32_t>> rot(shards_.size());   // rotated: per shard, [its entries][2]
    rc = fan([&](int k, Batch& b) {
        return rotated ? b.recordRotations(l.list(k), l.pos(k), l.count(k), records, &rot[(size_t)k]) : b.checkRecordCursors(l.list(k), l.pos(k), l.count(k), records);
    });
    if (rc != 0) return rc;
    return fan([&](int k, Batch& b) {
        const int r = rotated ? b.scatterRecordsRotated(l.list(k), l.pos(k), l.count(k), records, rot[(size_t)k].data()) : b.scatterRecords(l.list(k), l.pos(k), l.count(k), records);
        if (r == 0) b.promoteLoaded(records, count);
        return r;
    });
}

// ---- record bank -------------------------------------------------------------------------------------------------------------------
int Sharded::bankCreate(int64_t nSlots) {
    Serial serial(api_);
    lastError_.clear();
    const int rc = reserveOnAll([&](int, Batch& b) { return b.bankReserve(nSlots); }, [](Batch& b) { b.bankRelease(); });
    return rc != 0 ? rc : fan([](int, Batch& b) { b.bankTake(); return 0; });
}

int64_t Sharded::bankSlots() {
    Serial serial(api_);
    return front().bankSlots();   // (every shard holds the same bank)
}

int Sharded::bankChecked(const char* who, const int64_t* slots, const int64_t* list, int64_t count, bool instances, bool uniqueSlots) {
    lastError_.clear();
    if (!front().stateReady()) { lastError_ = "no program loaded"; return FX_E_NOTREADY; }
    std::string why;
    if (Batch::checkBankLists(who, slots, list, count, front().bankSlots(), instances ? n_ : 0, uniqueSlots, &why) != 0) { lastError_ = why; return FX_E_ARG; }
    return 0;
}

int Sharded::bankStore(const int64_t* slots, const int64_t* list, int64_t count) {
    Serial serial(api_);
    int rc = bankChecked("bank_store", slots, list, count, true, true);
    if (rc != 0 || count == 0) return rc;
    const ShardLists l(*this, list, count);
    if ((rc = fan([&](int k, Batch& b) { return b.reserveBankCall(l.count(k)); })) != 0) return rc;
    rc = fan([&](int k, Batch& b) { return b.bankStore(slots, l.list(k), l.pos(k), l.count(k)); });
    if (rc != 0 || shards_.size() == 1) return rc;
    // the other shards' copies: owner -> pinned staging -> every other shard, in chunks of the staging block, with the shadow rows
    Batch::SnapshotHeader hdr;
    if ((rc = runOn(0, [&](Batch& b) { return b.instanceShape(&hdr, 0); })) != 0) return rc;
    const size_t W = (size_t)Batch::instanceWords(hdr), chunk = std::max<size_t>(kStageBytes / (W * 4), 1), regs = (size_t)front().bankShadowRegs();
    if ((rc = growStage(std::min(chunk, (size_t)count) * W, "bank_store: no pinned staging for the copies to the other shards")) != 0) return rc;
    for (size_t k = 0; k < shards_.size() && rc == 0; ++k) {
        std::vector<int64_t> own((size_t)l.count((int)k));
        for (size_t i = 0; i < own.size(); ++i) own[i] = slots[l.pos((int)k)[i]];
        for (size_t c0 = 0; c0 < own.size() && rc == 0; c0 += chunk) {
            const int64_t m = (int64_t)std::min(chunk, own.size() - c0);
            if ((rc = runOn((int)k, [&](Batch& b) { return b.bankGetRecords(own.data() + c0, m, hStage_); })) != 0) break;
            std::vector<uint64_t> shadow((size_t)m * regs);
            for (int64_t i = 0; i < m; ++i) std::copy_n(shard((int)k).bankShadowRow(own[c0 + (size_t)i]), regs, shadow.data() + (size_t)i * regs);
            rc = fan([&](int j, Batch& b) { return j == (int)k ? 0 : b.bankPutRecords(own.data() + c0, m, hStage_, shadow.data()); });
        }
    }
    return rc;
}

int Sharded::bankRecall(const int64_t* slots, const int64_t* list, int64_t count) {
    Serial serial(api_);
    int rc = bankChecked("bank_recall", slots, list, count, true, false);
    if (rc != 0 || count == 0) return rc;
    const ShardLists l(*this, list, count);
    if ((rc = fan([&](int k, Batch& b) { return b.reserveBankCall(l.count(k)); })) != 0) return rc;
    const int64_t call = ++bankSerial_;
    // (every shard ends up with the same register rows: each one follows the whole list, like promoteLoaded)
    return fan([&](int k, Batch& b) {
        const int r = b.bankRecall(slots, l.list(k), l.pos(k), l.count(k), call);
        if (r == 0) b.bankNoteRecalled(slots, count);
        return r;
    });
}

int Sharded::bankPut(const int64_t* slots, int64_t count, const void* image, int64_t bytes) {
    Serial serial(api_);
    int rc = bankChecked("bank_put", slots, nullptr, count, false, true);
    if (rc != 0 || count == 0) return rc;
    Batch::SnapshotHeader hdr;
    if (!image || bytes < (int64_t)sizeof(hdr)) { lastError_ = "bank_put: no image"; return FX_E_ARG; }
    std::memcpy(&hdr, image, sizeof(hdr));
    if ((rc = runOn(0, [&](Batch& b) { return b.checkInstanceImage(hdr, count, bytes); })) != 0) return rc;
    const uint32_t* records = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(image) + sizeof(hdr));
    return fan([&](int, Batch& b) { return b.bankPutRecords(slots, count, records); });
}

int Sharded::bankGet(const int64_t* slots, int64_t count, void* buf, int64_t cap) {
    Serial serial(api_);
    int rc = bankChecked("bank_get", slots, nullptr, count, false, false);
    if (rc != 0) return rc;
    Batch::SnapshotHeader hdr;
    if ((rc = runOn(0, [&](Batch& b) { return b.instanceShape(&hdr, count); })) != 0) return rc;
    if (count == 0 && (!buf || cap < (int64_t)sizeof(hdr))) return 0;   // (nothing to get; a buffer that holds a header gets one)
    if (!buf || cap < (int64_t)sizeof(hdr) + count * Batch::instanceWords(hdr) * 4) { lastError_ = "bank_get: buffer smaller than fxb_instance_image_size()"; return FX_E_ARG; }
    std::memcpy(buf, &hdr, sizeof(hdr));
    uint32_t* records = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(buf) + sizeof(hdr));
    return runOn(0, [&](Batch& b) { return b.bankGetRecords(slots, count, records); });
}

int Sharded::bankStatus(int64_t* refusedCalls, int64_t* entry, int* reason, bool reset) {
    Serial serial(api_);
    lastError_.clear();
    std::vector<uint64_t> part(shards_.size() * 3, 0);
    const int rc = fan([&](int k, Batch& b) { return b.bankStatus(part.data() + (size_t)k * 3, reset); });
    if (rc != 0) return rc;
    uint64_t refused = 0, call = 0, key = ~(uint64_t)0;
    for (size_t k = 0; k < shards_.size(); ++k) {
        const uint64_t* p = part.data() + k * 3;
        if (p[0] == 0) continue;
        refused += p[0];
        if (p[2] > call) { call = p[2]; key = p[1]; }
        else if (p[2] == call) key = std::min(key, p[1]);
    }
    if (refusedCalls) *refusedCalls = (int64_t)refused;
    if (entry) *entry = refused ? (int64_t)(key >> 3) : -1;
    if (reason) *reason = refused ? (int)(key & 3) : 0;
    return 0;
}

int Sharded::registersList(bool set,const char* const* keys, int nKeys, const int64_t* list, int64_t count, const float* in, float* out) {
    Serial serial(api_);
    lastError_.clear();
    const char* name = set ? "set_registers_list" : "get_registers_list";
    if (nKeys < 0 || count < 0) { lastError_ = std::string(name) + ": a negative n_keys or count"; return FX_E_ARG; }
    if (nKeys > 0 && !keys) { lastError_ = std::string(name) + ": null keys"; return FX_E_ARG; }
    if (!front().stateReady()) { lastError_ = "no program loaded"; return FX_E_NOTREADY; }
    // (the program is replicated: the front shard's register numbers are every shard's)
    std::vector<int> regs;
    if (const int rc = front().resolveRegisters(keys, nKeys, &regs)) { lastError_ = front().lastError(); return rc; }
    if (count == 0 || nKeys == 0) return 0;
    const void* values = set ? static_cast<const void*>(in) : static_cast<const void*>(out);
    if (Batch::checkRegisterList(name, regs, list, count, n_, values, set, &lastError_) != 0) return FX_E_ARG;
    const ShardLists l(*this, list, count);
    if (!set) return fan([&](int k, Batch& b) { return b.getRegistersList(regs, l.list(k), l.pos(k), l.count(k), count, out); });
    // every shard reserves its staging first; only when all of them could is anything queued or noted anywhere (staging that has
    // grown stays: it is no state)
    if (const int rc = fan([&](int k, Batch& b) { return b.reserveRegisterList(nKeys, l.count(k)); })) return rc;
    return fan([&](int k, Batch& b) { return b.setRegistersList(regs, l.list(k), l.pos(k), l.count(k), count, in); });
}

int Sharded::setRegisterTracksList(const char* const* keys, int nKeys, const int64_t* list, int64_t count, const float* values, int nSteps, int first, int period) {
    Serial serial(api_);
    lastError_.clear();
    const char* name = "set_register_tracks_list";
    if (nKeys < 0 || count < 0) { lastError_ = std::string(name) + ": a negative n_keys or count"; return FX_E_ARG; }
    if (nKeys > 0 && !keys) { lastError_ = std::string(name) + ": null keys"; return FX_E_ARG; }
    if (!front().stateReady()) { lastError_ = "no program loaded"; return FX_E_NOTREADY; }
    // (the program is replicated: the front shard's register numbers are every shard's)
    std::vector<int> regs;
    if (const int rc = front().resolveRegisters(keys, nKeys, &regs)) { lastError_ = front().lastError(); return rc; }
    // everything that reads nothing but the arguments, for the whole handle and with the caller's indices
    if (Batch::checkTrackList(regs, list, count, n_, values, nSteps, first, period, &lastError_) != 0) return FX_E_ARG;
    if (count == 0 || nKeys == 0) return 0;
    const ShardLists l(*this, list, count);
    // every shard is asked first - what is armed on it, the program, then its staging and its track buffer; only when all of
    // them could is anything armed anywhere (staging that has grown stays: it is no state)
    int rc = fan([&](int k, Batch& b) {
        std::string why;
        const int r = b.checkTrackListArm(regs, l.list(k), l.count(k), shards_[(size_t)k]->first, &why);
        if (r != 0) b.noteError(why);
        return r;
    });
    if (rc == 0) rc = fan([&](int k, Batch& b) { return b.reserveTrackList(regs, l.count(k), nSteps); });
    if (rc != 0) return rc;
    return fan([&](int k, Batch& b) { return b.armTrackList(regs, l.list(k), l.pos(k), l.count(k), count, values, nSteps, first, period); });
}

int Sharded::clearRegisterTracksList() {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int, Batch& b) { return b.clearTrackLists(); });
}

int Sharded::tramList(int which, const int64_t* list, int64_t count, int first, int nWords, const float* in, float* out, unsigned flags, bool set) {
    Serial serial(api_);
    lastError_.clear();
    const void* values = set ? static_cast<const void*>(in) : static_cast<const void*>(out);
    // everything that reads nothing but the arguments, for the whole handle and with the caller's indices
    if (Batch::checkTramList(set, which, list, count, n_, first, nWords, values, flags, &lastError_) != 0) return FX_E_ARG;
    if (!front().stateReady()) { lastError_ = "no program loaded"; return FX_E_NOTREADY; }
    ShardLists l(*this, list, count, count != 0 && nWords != 0);   // (n_words == 0: the list may be null, and no entry moves)
    l.samePos((flags & FXB_TRAM_BROADCAST) != 0);
    // every shard is asked first - the window against its line, its staging; only when all of them could is anything queued
    // anywhere (staging that has grown stays: it is no state)
    if (const int rc = fan([&](int k, Batch& b) { return b.reserveTramList(set, which, l.count(k), first, nWords, flags); })) return rc;
    if (count == 0 || nWords == 0) return 0;
    return fan([&](int k, Batch& b) { return b.tramList(which, l.list(k), l.pos(k), l.count(k), first, nWords, set ? in : nullptr, set ? nullptr : out, flags); });
}

int Sharded::getTramAt(int which, int64_t inst, float* out, int nSlots) {
    Serial serial(api_);
    lastError_.clear();
    const int k = shardOf(inst);
    if (k < 0) { lastError_ = "instance out of range"; return FX_E_ARG; }
    return runOn(k, [&](Batch& b) { return b.getTramAt(which, inst - shards_[(size_t)k]->first, out, nSlots); });
}
int Sharded::getCursorsAt(int64_t inst, int32_t out4[4]) {
    Serial serial(api_);
    lastError_.clear();
    const int k = shardOf(inst);
    if (k < 0) { lastError_ = "instance out of range"; return FX_E_ARG; }
    return runOn(k, [&](Batch& b) { return b.getCursorsAt(inst - shards_[(size_t)k]->first, out4); });
}
int Sharded::prepare(int nSamples, bool wait) {
    Serial serial(api_);
    lastError_.clear();
    return fan([&](int, Batch& b) { return b.prepare(nSamples, wait); });
}
float Sharded::lastKernelMsOf(int k) {
    Serial serial(api_);
    float ms = -1.0f;
    runOn(k, [&](Batch& b) { ms = b.lastKernelMs(); return 0; });
    return ms;
}
int64_t Sharded::info(int what) {
    Serial serial(api_);
    std::vector<int64_t> part(shards_.size(), 0);
    fan([&](int k, Batch& b) { part[(size_t)k] = b.info(what); return 0; });
    if (what == FXB_INFO_GRID || what == FXB_INFO_HOST_STAGED_BLOCKS || what == FXB_INFO_HOST_INPLACE_BLOCKS || what == FXB_INFO_BUS_BLOCKS ||
        what == FXB_INFO_METER_LAUNCHES || what == FXB_INFO_BUS_GAIN_BLOCKS || what == FXB_INFO_BUS_TAP_BLOCKS || what == FXB_INFO_BUS_SEND_BLOCKS || what == FXB_INFO_BUS_FEED_BLOCKS || what == FXB_INFO_IMAJOR_BLOCKS || what == FXB_INFO_INSTANCE_GATHERS || what == FXB_INFO_INSTANCE_SCATTERS || what == FXB_INFO_INSTANCE_ROTATIONS || what == FXB_INFO_GAIN_LIST_SETS ||
        what == FXB_INFO_REGISTER_LIST_SETS || what == FXB_INFO_REGISTER_LIST_GETS || what == FXB_INFO_TRAM_LIST_SETS || what == FXB_INFO_TRAM_LIST_GETS ||
        what == FXB_INFO_METER_SELECTS || what == FXB_INFO_METER_LIST_READS || what == FXB_INFO_METER_LIST_RESETS || what == FXB_INFO_TRACK_LIST_EXPANDS ||
        what == FXB_INFO_METER_TARGET_LAUNCHES || what == FXB_INFO_METER_MATCH_SELECTS || what == FXB_INFO_METER_MATCH_BESTS ||
        what == FXB_INFO_METER_LEVEL_LAUNCHES || what == FXB_INFO_METER_LEVEL_SELECTS || what == FXB_INFO_METER_LEVEL_LIST_READS ||
        what == FXB_INFO_METER_RANKS || what == FXB_INFO_METER_MATCH_RANKS || what == FXB_INFO_METER_LEVEL_RANKS ||
        what == FXB_INFO_METER_TONE_LAUNCHES || what == FXB_INFO_METER_TONE_SELECTS || what == FXB_INFO_METER_TONE_LIST_READS || what == FXB_INFO_METER_TONE_RANKS ||
        what == FXB_INFO_BANK_STORES || what == FXB_INFO_BANK_RECALLS || what == FXB_INFO_BANK_BYTES ||
        what == FXB_INFO_XLATE_QUIET_LEFT || what == FXB_INFO_XLATE_QUIET_REPAIRS) {
        int64_t sum = 0;
        for (int64_t p : part) sum += p;
        return sum;
    }
    return part[0];
}

}  // namespace fx
