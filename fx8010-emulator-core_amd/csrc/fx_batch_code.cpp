// fx_batch_code.cpp — what a batch runs: the lowering of the program into Code (tier, translation, module, record stream), the
// cache of finished Code and its keys, the builder thread that generates code off the caller's thread, the stage ranking and
// its tuner, block-length classes, and the control bookkeeping that decides which variant is wanted (heat, lean variants).
#include "fx_batch.hpp"

#include <cmath>
#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

// Small batches leave SIMDs empty (and a lone wavefront issues an instruction only every ~4 clocks): a program that can be cut
// runs as a pipeline of stages over the wavefronts of a workgroup (fx_xlate.hpp StageInfo).  Beyond two wavefronts of instances
// per SIMD the plain program has always been the faster one.  FX_STAGES pins the number asked for (1 = never).
bool Batch::stagingPossibleGiven(bool stagingOff) const {
    if (stagingOff) return false;
    if (knobs_.stages) return knobs_.stages >= 2;
    return (n_ + 63) / 64 < 2048;
}

// How many stages?  The planner's own costs decide (planStages: cost of every stage, pipeline overhead included, in units of
// ~1.4 per vector instruction), with a model of the machine calibrated on tools/stage_policy_probe.sh (profiles/r04_stage_policy*.txt:
// the filter chain, twelve parallel chains with 13-row packets, a delay line + SKIP + LOG / EXP program; 16 .. 2 048 wavefronts):
//   a wavefront alone:   L = 2.85 clocks x cost of the slowest stage + 165 (loop control, PCM) + 100 per LOG / EXP round trip
//                            + 5 per row its packets carry + the barrier: (100 + 15 K) clocks x 1 / 0.42 / 0.1 / 0 per sample for one
//                            every 1 / 2 / 4 / 8 samples (tools/stage_block_probe.py, profiles/r04_stage_block_probe.txt)
//   the CU's issue slots: G workgroups per CU x 2.4 clocks x the cost of ALL stages / (4 SIMDs x 0.8) - for K < 4 the wavefronts of
//                            the G workgroups can pile up on K SIMDs of the CU (as many as the VGPR build lets a SIMD hold)
//   a sample takes the larger of the two; a block also fills and drains the pipeline: 3 (K - 1) steps of `group` samples.
// The options come back cheapest first.  The model is good to ~ 20 % (how the dispatcher spreads workgroups over the CUs is not
// in it), so options within kTuneBand of the best are MEASURED on the caller's own blocks before one is kept (noteLaunchTime).
std::vector<Batch::StageOption> Batch::rankStages(const std::vector<MicroOp>& steadyRecords, const std::vector<MicroOp>& lastRecords,
                                                  const XlateProgram& xprog, int nRows, int blockClass, int wavesPerSimdCap, bool stagingOff) const {
    std::vector<StageOption> out;
    if (stagingOff) { out.push_back(StageOption()); return out; }
    if (knobs_.stages) {
        StageOption o;
        o.wanted = knobs_.stages;
        out.push_back(o);
        return out;
    }
    const double W = (double)((n_ + 63) / 64);
    const int64_t groupsPerCu = std::max<int64_t>(1, ((n_ + 63) / 64 + 255) / 256);
    const uint32_t ldsBudget = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(144 * 1024, 160 * 1024 / groupsPerCu - 256));
    const int maxGroup = blockClass == 0 ? 1 : (blockClass == 1 ? 2 : kStageGroupMax);
    const double blockSamples = blockClass == 0 ? 32.0 : (blockClass == 1 ? 128.0 : 2048.0);
    const double kClocksPerCost = 2.85, kIssuePerCost = 2.4, kFixed = 165.0, kLut = 100.0, kEta = 0.8;
    StageOption plain;
    bool havePlain = false;
    std::vector<int> seen;
    for (int wanted : {8, 4, 2}) {
        if (!stagingPossibleGiven(stagingOff)) break;
        const StagePlan plan = planStages(steadyRecords, lastRecords, xprog, nRows, wanted);
        if (!havePlain && plan.totalCost > 0) {
            plain.wanted = plain.stages = 1;
            const double lone = kClocksPerCost * plan.totalCost + kFixed + kLut * plan.totalLuts;
            const double shared = std::ceil(W / 1024.0) * kIssuePerCost * plan.totalCost / kEta;
            plain.predicted = std::max(lone, shared);
            havePlain = true;
        }
        if (plan.cuts.empty()) continue;
        const int k = (int)plan.cuts.size() + 1;
        if (std::find(seen.begin(), seen.end(), k) != seen.end()) continue;
        seen.push_back(k);
        StageLds lds;
        if (!stageLdsLayout(xprog, plan, ldsBudget, maxGroup, &lds, knobs_.stagesGroup)) continue;
        int worst = 0, luts = 0, sum = 0;
        for (size_t s = 0; s < plan.stageCost.size(); ++s) {
            worst = std::max(worst, plan.stageCost[s]);
            luts = std::max(luts, plan.stageLuts[s]);
            sum += plan.stageCost[s];
        }
        size_t rows = 0;
        for (size_t c2 = 0; c2 < plan.live.size(); ++c2) rows = std::max(rows, plan.live[c2].size() + (c2 + 1 < plan.live.size() ? plan.live[c2 + 1].size() : 0));
        const double barrier = (100.0 + 15.0 * k) * (lds.group >= 8 ? 0.0 : (lds.group == 4 ? 0.1 : (lds.group == 2 ? 0.42 : 1.0)));
        const double lone = kClocksPerCost * worst + kFixed + kLut * luts + 5.0 * (double)rows + barrier;
        const double G = std::ceil(W / 256.0);
        double shared = G * kIssuePerCost * sum / (4.0 * kEta);
        // (K < 4: measured between an even spread and a pile-up of the G workgroups' wavefronts on K SIMDs - the filter chain and the
        // parallel chains in two stages sit near the pile-up, the delay-line program near the even spread: the geometric mean)
        if (k < 4) {
            const double piled = std::min(G, (double)wavesPerSimdCap) * kIssuePerCost * worst / kEta;
            if (piled > std::max(shared, lone)) shared = std::sqrt(std::max(shared, lone) * piled);
        }
        StageOption o;
        o.wanted = wanted;
        o.stages = k;
        o.group = lds.group;
        o.predicted = std::max(lone, shared) * (1.0 + 3.0 * (k - 1) * lds.group / blockSamples);
        out.push_back(o);
    }
    if (havePlain || out.empty()) out.push_back(plain);
    std::stable_sort(out.begin(), out.end(), [](const StageOption& a, const StageOption& b2) { return a.predicted < b2.predicted; });
    return out;
}

// What the generated code is a function of.  Two calls with equal keys would build the same Code, so a finished one is reused
// (ensureLowered): the program (a load counter: registers and instructions only ever accumulate), the options, which registers
// have rows although no instruction writes them (per-instance values, moving controls, control tracks), the values of all the
// others (they are folded into the code as literals), the block-length class staged code is generated for, whether the
// translation is put off because compiled-in controls keep changing, and the diagnostic knobs of the environment.
std::string Batch::codeKey(int blockClass, bool defer) const { return codeKeyFor(laneForced(), blockClass, defer, pickFor(blockClass)); }

std::string Batch::codeKeyFor(const std::vector<uint8_t>& forced, int blockClass, bool defer, int pick) const {
    std::string k;
    auto word = [&](int64_t v) { k.append(reinterpret_cast<const char*>(&v), 8); };
    word(loadGen_); word((int64_t)prog_.options); word(blockClass); word(pick); word(defer ? 1 : 0);
    word(((iSlotsAlloc_ > 0 || xSlotsAlloc_ > 0) && instPerLane_ != 1) ? instPerLane_ : 0);   // delay lines tiled for K instances per lane pin the HIP C++ kernel
    // (the release knobs are fixed for the life of the handle - fx_knobs.hpp ReleaseKnobs - and so not part of the key)
    for (size_t r = 0; r < hostValue_.size(); ++r) {
        const bool f = r < forced.size() && forced[r];
        // (a register no instruction reads as an operand: its value lives in its state row and cannot reach the code)
        const uint32_t w = f ? 0x7fc0f0f0u : (readByProgram((int)r) ? bitsOf(hostValue_[r]) : 0x7fc0f0f1u);
        k.push_back(f ? 1 : 0);
        k.append(reinterpret_cast<const char*>(&w), 4);
    }
    for (int reg : trackRegs_) word(reg);   // (slot order is part of the code)
    return k;
}

void Batch::releaseCode(Code& c) {
    if (c.module) (void)hipModuleUnload(c.module);
    if (c.dStream) (void)hipFree(c.dStream);
    c.module = nullptr;
    c.fn = nullptr;
    c.dStream = nullptr;
    c.streamCap = 0;
}

void Batch::clearCodeCache() {
    (void)hipSetDevice(device_);
    waitLastLaunch();   // the most recent launch may still run one of them
    releaseCode(c_);
    c_ = Code();
    for (std::unique_ptr<Code>& e : cache_) releaseCode(*e);
    cache_.clear();
}

// c_ -> cache_.  The code that is being replaced may still be running: nothing of it is touched; only when the cache is full
// the least recently used entry goes, behind the most recent launch.
void Batch::stashCode() {
    if (c_.key.empty()) {   // nothing finished (a failed build): drop the pieces
        if (c_.module || c_.dStream) { waitLastLaunch(); releaseCode(c_); }
        c_ = Code();
        return;
    }
    c_.lastUse = ++useClock_;
    cache_.push_back(std::make_unique<Code>(std::move(c_)));
    c_ = Code();
    if (cache_.size() > kCodeCache) {
        const size_t lru = lruVictim();
        waitLastLaunch();
        releaseCode(*cache_[lru]);
        cache_.erase(cache_.begin() + (long)lru);
    }
}

bool Batch::cachedCode(const std::string& key) const {
    for (const std::unique_ptr<Code>& e : cache_)
        if (e->key == key) return true;
    return false;
}

bool Batch::adoptCode(const std::string& key) {
    for (size_t k = 0; k < cache_.size(); ++k)
        if (cache_[k]->key == key) {
            c_ = std::move(*cache_[k]);
            cache_.erase(cache_.begin() + (long)k);
            c_.lastUse = ++useClock_;
            return true;
        }
    return false;
}

// staged code is generated for a class of block lengths - when the batch is small enough to be staged at all
int Batch::keyClass() const {
    if (!stagingPossible()) return -1;
    return wantedClass_ >= 0 ? wantedClass_ : stageBlockClass(std::max(pendingSamples_, 1));
}

bool Batch::deferWanted() const {
    // controls that are compiled into the code keep changing (a set_register within the last few blocks): a translation costs
    // a module load (~1-2 ms), a re-encode for the interpreter ~0.05 ms - interpret until they have been quiet.  (A block of
    // more than ~half a millisecond of translated code pays for its translation at once.)
    const double blockMs = (double)n_ * (double)pendingSamples_ * (double)std::max<size_t>(prog_.instrs.size(), 1) / 1e10;
    return controlHeat_ > 0 && blockMs < 0.5 && !(prog_.options & kOptTramDane) && !knobs_.kernelStartsWith("xlate");
}

int Batch::ensureLowered() {
    if (!loaded_ || !prog_.ready) return fail(FX_E_NOTREADY, "no program loaded");
    if (!lowDirty_) return 0;
    (void)hipSetDevice(device_);
    collectBuilt();
    const int blockClass = keyClass();
    const bool defer = deferWanted();
    const std::string key = codeKey(blockClass, defer);
    if (!c_.key.empty() && c_.key == key) {   // (a register written with the value it had, a schedule armed again: nothing to do)
        lowDirty_ = false;
        return 0;
    }
    stashCode();
    bool have = adoptCode(key);
    if (!have && waitBuild(key)) {   // the builder thread is at it (the control variant, asked for at the first block): shorter than starting over
        collectBuilt();
        have = adoptCode(key);
    }
    if (have) {   // code for this shape exists: a pointer swap
        ++cacheHits_;
        lowDirty_ = false;
        adoptStageOptions();
        prebuildControlVariant();
        return 0;
    }
    std::string err;
    const int rc = buildCodeInto(c_, buildInputs(key, blockClass, defer), false, &err);
    if (rc != 0) return fail(rc, err);
    lowDirty_ = false;
    adoptStageOptions();
    prebuildControlVariant();
    return 0;
}

// The code in force came with the planner's ranking of the stage counts (Code::stageOptions).  The first code of a class of
// block lengths starts that class's tuner: the options the model cannot tell apart (within kTuneBand of the cheapest, three at
// most) are generated on the builder thread and then timed on the caller's own launches, kTuneRuns each (noteLaunchTime); the
// fastest is kept.  FX_STAGES_TUNE=0 (or no builder thread): the model's choice stands.
void Batch::adoptStageOptions() {
    const int cls = c_.blockClass;
    if (cls < 0 || cls >= 3 || !c_.useXlate || keyClass() != cls) return;
    Tuner& t = tune_[cls];
    if (t.init) return;
    t = Tuner();
    t.init = true;
    t.pick = c_.stagePick;
    // (built for "the cheapest": from now on the code goes by the stage count it was built for)
    c_.key = codeKeyFor(laneForced(), cls, c_.deferred, t.pick);
    const bool tuneOff = !knobs_.stagesTune;
    if (c_.stageOptions.empty() || knobs_.stages) { t.done = true; return; }
    const double best = c_.stageOptions.front().predicted;
    for (const StageOption& o : c_.stageOptions)
        if (t.options.size() < 3 && (t.options.empty() || o.predicted <= best * kTuneBand)) t.options.push_back(o);
    bool mine = false;
    for (const StageOption& o : t.options) mine = mine || o.wanted == t.pick;
    if (!mine || t.options.size() < 2 || tuneOff || !builderWanted()) { t.options.clear(); t.done = true; return; }
    t.bestNs.assign(t.options.size(), 0.0f);
    t.runs.assign(t.options.size(), 0);
    for (const StageOption& o : t.options) {
        if (o.wanted == t.pick) continue;
        BuildInputs in = buildInputs(codeKeyFor(laneForced(), cls, false, o.wanted), cls, false);
        in.stagePick = o.wanted;
        requestBuild(std::move(in));
    }
}

// Called at the head of a process call: what the previous launch took goes to the tuner of its class, and the tuner decides what
// the next launch runs - the same option again (kTuneRuns launches each), the next one whose code the builder has finished, or,
// when every option has been timed, the fastest for good.  All options compute the same words: a trial costs time, never bits.
void Batch::noteLaunchTime() {
    const int cls = lastLaunchClass_;
    if (cls < 0 || cls >= 3) return;
    Tuner& t = tune_[cls];
    if (!t.init || t.done) return;
    // (hipErrorNotReady is an answer, not a failure: it must not stay behind as the thread's "last error" for the launch
    // helpers that ask hipGetLastError() after their kernel)
    const hipError_t ready = (lastLaunchTimed_ && launched_) ? hipEventQuery(ev1_) : hipErrorNotReady;
    if (ready != hipSuccess) (void)hipGetLastError();
    if (ready == hipSuccess) {
        lastLaunchTimed_ = false;
        float ms = -1.0f;
        if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess && ms > 0.0f && lastLaunchSamples_ >= kTuneMinSamples)
            for (size_t k = 0; k < t.options.size(); ++k)
                if (t.options[k].wanted == lastLaunchPick_) {
                    const float ns = ms * 1e6f / (float)lastLaunchSamples_;
                    t.bestNs[k] = t.runs[k] == 0 ? ns : std::min(t.bestNs[k], ns);
                    ++t.runs[k];
                    ++t.trials;
                }
    }
    if (lowDirty_ || keyClass() != cls) return;
    size_t cur = 0;
    while (cur < t.options.size() && t.options[cur].wanted != t.pick) ++cur;
    if (cur == t.options.size() || t.runs[cur] < kTuneRuns) return;
    collectBuilt();
    bool waiting = false;
    for (size_t k = 0; k < t.options.size(); ++k) {
        if (t.runs[k] >= kTuneRuns) continue;
        const std::string key = codeKeyFor(laneForced(), cls, false, t.options[k].wanted);
        if (cachedCode(key)) {   // its turn
            t.pick = t.options[k].wanted;
            lowDirty_ = true;
            return;
        }
        if (buildFailed(key)) continue;   // (the builder could not make it: out of the race)
        if (!buildPending(key)) {         // (e.g. the set of registers with rows has changed since the options were asked for)
            BuildInputs in = buildInputs(key, cls, false);
            in.stagePick = t.options[k].wanted;
            requestBuild(std::move(in));
        }
        waiting = waiting || buildPending(key);
    }
    if (waiting) return;
    size_t bestK = cur;
    for (size_t k = 0; k < t.options.size(); ++k)
        if (t.runs[k] >= kTuneRuns && t.bestNs[k] < t.bestNs[bestK]) bestK = k;
    t.done = true;
    if (t.options[bestK].wanted != t.pick) {
        t.pick = t.options[bestK].wanted;
        lowDirty_ = true;
    } else {
        prebuildControlVariant();
    }
}

// ---- the builder thread: code generated off the caller's thread -------------------------------------------------------------
// A translation and its module load take milliseconds; a real-time caller has 667 us per 32-sample block.  Two
// changes of code can be seen coming: the variant in which the declared controls have rows (wanted at the first touch of a
// slider - asked for right after the first build) and the code for another class of block lengths (asked for at the first
// block of that class, while the code in force - correct for every length, only slower - keeps running).  Both are built
// here and handed over through `finished`; the caller's thread picks them up at its next lowering (collectBuilt) as cache
// entries, so what it does then is a pointer swap.  FX_BUILDER=0: no thread, everything on the caller's (diagnostics).

bool Batch::builderWanted() const {
    return knobs_.builder;
}

void Batch::requestBuild(BuildInputs&& in) {
    if (!builderWanted()) return;
    if (!builder_) {
        builder_.reset(new Builder);
        Builder* b = builder_.get();
        b->thread = std::thread([this, b] {
            (void)hipSetDevice(device_);
            if (hipStreamCreateWithFlags(&b->upload, hipStreamNonBlocking) != hipSuccess) { b->upload = nullptr; (void)hipGetLastError(); }
            std::unique_lock<std::mutex> lock(b->mu);
            for (;;) {
                b->cv.wait(lock, [b] { return b->quit || !b->jobs.empty(); });
                if (b->quit) {
                    if (b->upload) (void)hipStreamDestroy(b->upload);
                    b->upload = nullptr;
                    return;
                }
                BuildInputs job = std::move(b->jobs.front());
                b->jobs.pop_front();
                b->running = job.key;
                lock.unlock();
                std::unique_ptr<Code> c(new Code);
                std::string err;
                const int rc = buildCodeInto(*c, job, true, &err);
                if (rc != 0) releaseCode(*c);
                lock.lock();
                b->running.clear();
                if (rc == 0) b->finished.push_back(std::move(c));
                else {
                    b->failed.push_back(job.key);
                    if (b->failed.size() > Builder::kMaxFailed) b->failed.pop_front();
                }
                b->cv.notify_all();
            }
        });
    }
    std::lock_guard<std::mutex> lock(builder_->mu);
    if (builder_->running == in.key) return;
    for (const BuildInputs& j : builder_->jobs) if (j.key == in.key) return;
    for (const std::unique_ptr<Code>& c : builder_->finished) if (c->key == in.key) return;
    for (const std::string& k : builder_->failed) if (k == in.key) return;
    builder_->jobs.push_back(std::move(in));
    builder_->cv.notify_all();
}

void Batch::collectBuilt() {
    if (!builder_) return;
    std::vector<std::unique_ptr<Code>> got;
    {
        std::lock_guard<std::mutex> lock(builder_->mu);
        got.swap(builder_->finished);
    }
    for (std::unique_ptr<Code>& c : got) {
        if (cachedCode(c->key) || c_.key == c->key) { releaseCode(*c); continue; }
        c->lastUse = ++useClock_;
        cache_.push_back(std::move(c));
        if (cache_.size() > kCodeCache) {
            const size_t lru = lruVictim();
            waitLastLaunch();
            releaseCode(*cache_[lru]);
            cache_.erase(cache_.begin() + (long)lru);
        }
    }
}

bool Batch::buildPending(const std::string& key) {
    if (!builder_) return false;
    std::lock_guard<std::mutex> lock(builder_->mu);
    if (builder_->running == key) return true;
    for (const BuildInputs& j : builder_->jobs) if (j.key == key) return true;
    return false;
}

bool Batch::buildFailed(const std::string& key) {
    if (!builder_) return true;
    std::lock_guard<std::mutex> lock(builder_->mu);
    for (const std::string& k : builder_->failed) if (k == key) return true;
    return false;
}

// true: the builder has (or had) this key in hand and is done with it now
bool Batch::waitBuild(const std::string& key) {
    if (!builder_) return false;
    std::unique_lock<std::mutex> lock(builder_->mu);
    auto pending = [&] {
        if (builder_->running == key) return true;
        for (const BuildInputs& j : builder_->jobs) if (j.key == key) return true;
        return false;
    };
    if (!pending()) {
        for (const std::unique_ptr<Code>& c : builder_->finished) if (c->key == key) return true;
        return false;
    }
    builder_->cv.wait(lock, [&] { return !pending(); });
    return true;
}

// before anything a build reads changes (a load, an option) and at the end: no job running, none queued, nothing to pick up
void Batch::drainBuilder(bool stop) {
    if (!builder_) return;
    {
        std::unique_lock<std::mutex> lock(builder_->mu);
        builder_->jobs.clear();
        builder_->cv.wait(lock, [&] { return builder_->running.empty(); });
        for (std::unique_ptr<Code>& c : builder_->finished) releaseCode(*c);
        builder_->finished.clear();
        builder_->failed.clear();
        if (stop) {
            builder_->quit = true;
            builder_->cv.notify_all();
        }
    }
    if (stop) {
        builder_->thread.join();
        builder_.reset();
    }
}

void Batch::prebuildControlVariant() {
    if (controlMode_ || c_.key.empty() || !c_.useXlate || !builderWanted()) return;
    std::vector<uint8_t> forced = laneForced();
    bool any = false;
    for (const std::string& name : prog_.controls) {
        const int r = prog_.findRegister(name);
        if (r < 0 || forced[(size_t)r] || intrinsicLane(r) || !readByProgram(r) || !movableControl(r)) continue;
        forced[(size_t)r] = 1;
        any = true;
    }
    if (!any) return;
    const int blockClass = keyClass();
    // ... for the stage count in force and for every one still on trial: a slider may move while the trials run
    std::vector<int> picks{pickFor(blockClass)};
    if (blockClass >= 0 && blockClass < 3 && tune_[blockClass].init && !tune_[blockClass].done)
        for (const StageOption& o : tune_[blockClass].options)
            if (std::find(picks.begin(), picks.end(), o.wanted) == picks.end()) picks.push_back(o.wanted);
    for (int pick : picks) {
        BuildInputs in = buildInputs(codeKeyFor(forced, blockClass, false, pick), blockClass, false);
        if (cachedCode(in.key)) continue;
        in.forced = forced;
        in.stagePick = pick;
        requestBuild(std::move(in));
    }
}

Batch::BuildInputs Batch::buildInputs(const std::string& key, int blockClass, bool defer) const {
    BuildInputs in;
    in.key = key;
    in.blockClass = blockClass;
    in.defer = defer;
    in.hostValue = hostValue_;
    in.forced = laneForced();
    in.trackRegs = trackRegs_;
    in.stagePick = pickFor(blockClass);
    in.instPerLane = instPerLane_;
    in.iSlotsAlloc = iSlotsAlloc_;
    in.xSlotsAlloc = xSlotsAlloc_;
    in.stateRows = stateRows_;
    in.stagingOff = stagingOff_;
    return in;
}

// The lowering itself, into an empty Code: lower the program for the tier that takes it, translate it where it can be
// translated, load the code object, upload the tables.  offline: on the builder thread, while the batch keeps running other
// code - nothing of the batch's device state may change (no new state rows, no delay-line allocation) and only the translated
// tier qualifies; whatever else the program would need is left to the caller's thread (FX_E_NOTREADY).
namespace {
// errors of a build go to the caller's string: a build may run on the builder thread, where lastError_ is not its to write
int buildFail(std::string* err, int code, const std::string& what) { *err = what; return code; }
int buildHipFail(std::string* err, hipError_t e, const char* where) {
    (void)hipGetLastError();   // (reported here: not again by the next launch helper that asks, Batch::hipFail)
    *err = std::string(where) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? FX_E_MEMORY : FX_E_NODEVICE;
}
}  // namespace

int Batch::buildCodeInto(Code& c, BuildInputs in, bool offline, std::string* err) {
    int rc = chooseTierAndLower(c, in, offline, err);
    if (rc == 0) rc = translateInto(c, in, offline, err);
    if (rc == 0) rc = packStream(c, in, offline, err);
    return rc;
}

// The wavefronts of a SIMD take turns at the top priority (fx_xlate.hpp prioritySlices; the interpreter: AsmArgs::tramDane bit 2)
// wherever a SIMD holds two or more (twoWavesPerSimd) in a build of at most four slots - the priority has four levels, and
// chooseTierAndLower picks such a build for a batch of that size.  FX_XLATE_PRIO=0 / 1 in the environment: never / whenever
// unstaged.
bool Batch::priorityTurns(AsmVariant variant) const {
    if (knobs_.xlatePrio >= 0) return knobs_.xlatePrio != 0;
    return twoWavesPerSimd() && kAsmWavesPerSimd[variant] <= 4;
}

// Step 1: the tier that takes the program and its lowered streams; inline, the state rows and delay lines they need.
int Batch::chooseTierAndLower(Code& c, BuildInputs& in, bool offline, std::string* err) {
    // Preferred: the hand-written gfx950 interpreter (one instance per lane, bookkeeping in VGPRs).
    // Programs it does not cover run on the HIP C++ kernel.  TRAM tiling pins K once allocated.
    Lowered fresh;
    bool asmOk = false;
    const bool tramPinned = in.iSlotsAlloc > 0 || in.xSlotsAlloc > 0;
    const char* forceHip = knobs_.kernel.empty() ? nullptr : knobs_.kernel.c_str();
    const bool wantAsm = !knobs_.kernelIs("hip") && !knobs_.instPerLaneSet;
    if (wantAsm && (!tramPinned || in.instPerLane == 1)) {
        // first choice: register file in VGPRs (row pitch 1 = plain indices), else in LDS
        const bool tryVgpr = !(forceHip && std::strcmp(forceHip, "asm_lds") == 0);
        if (tryVgpr) {
            fresh = lowerProgram(prog_, in.hostValue, in.forced, 1, false, 1);
            asmOk = fresh.error.empty() && asmEligible(fresh, &c.asmWhyNot);
            if (asmOk) {
                // smallest VGPR build that holds the register file = most wavefronts per SIMD
                int v = ASM_V64;
                while (v < ASM_V256 && fresh.nRows > kAsmVgprRows[v]) ++v;
                const int smallest = v;
                // ... and a larger one while that costs no residency this batch can use: the translator keeps the constants of
                // its LOG / EXP index guess and a small cache of products in VGPRs above the register file (fx_xlate.hpp).
                // (The interpreter tier has no use for spare registers, but runs the same build: it is the translator's fallback.)
                {
                    const int wavesPerSimd = (int)((((size_t)n_ + 63) / 64 + 1023) / 1024);  // 256 CUs x 4 SIMDs
                    auto usable = [&](int q) { return std::min(kAsmWavesPerSimd[q], std::max(wavesPerSimd, 1)); };
                    while (v < ASM_V256 && kAsmVgprRows[v] - fresh.nRows < kSpareVgprsWanted && usable(v + 1) >= usable(v)) ++v;
                }
                // a small batch is cut into stages (below): each stage wants spare registers for its packets and its input
                // bursts, and at most 4 wavefronts per SIMD will be resident anyway - the 128-register build costs nothing
                if (stagingPossibleGiven(in.stagingOff))
                    while (v < ASM_V128) ++v;
                // two or more wavefronts per SIMD: they take turns at the top priority in a build of at most four slots
                // (priorityTurns) - and a fifth resident wavefront adds nothing to a SIMD that four keep issuing (measured: config5
                // at 5 per SIMD on the 96-register build = at 4 per SIMD).  So the 128-register build or larger, for batches of
                // any number of rounds (1 048 576 instances, 4 slots with turns against 5-8 without: config5 + 2.0 %, config4
                // + 2.4 %, the memory-bound probe and config3 unchanged).
                if (twoWavesPerSimd())
                    while (v < ASM_V128) ++v;
                const char* pin = forceHip ? std::strstr(forceHip, "_v") : nullptr;
                if (pin && (std::strncmp(forceHip, "asm_v", 5) == 0 || std::strncmp(forceHip, "xlate_v", 7) == 0)) {
                    // diagnostics: pin a (large enough) build of the interpreter (asm_vNN) or of the translator (xlate_vNN)
                    static const char* const tags[ASM_VARIANTS] = {"", "_v64", "_v72", "_v80", "_v96", "_v128", "_v168", "_v256"};
                    for (int q = smallest; q < ASM_VARIANTS; ++q)
                        if (std::strcmp(pin, tags[q]) == 0) v = q;
                }
                c.variant = (AsmVariant)v;
            }
        }
        if (!asmOk) {
            fresh = lowerProgram(prog_, in.hostValue, in.forced, 1, false);
            asmOk = fresh.error.empty() && asmEligible(fresh, &c.asmWhyNot);
            c.variant = ASM_LDS;
        }
    } else {
        c.asmWhyNot = "disabled by FX_KERNEL / FX_INST_PER_LANE";
    }
    if (!asmOk && offline) return buildFail(err, FX_E_NOTREADY, "offline build: not a program for the assembly tiers");
    if (!asmOk) fresh = lowerProgram(prog_, in.hostValue, in.forced, chooseInstPerLane());
    if (!fresh.error.empty()) return buildFail(err, FX_E_PROGRAM, fresh.error);
    if (offline && (fresh.instPerLane != in.instPerLane || fresh.iSlots > in.iSlotsAlloc || fresh.xSlots > in.xSlotsAlloc || makeLayout((int)prog_.regs.size(), prog_.numChannels).totalRows != in.stateRows))
        return buildFail(err, FX_E_NOTREADY, "offline build: the batch's device state would have to change");
    int rc = 0;
    if (!offline) {
        instPerLane_ = fresh.instPerLane;
        rc = ensureState();
        if (rc != 0) { *err = lastError_; return rc; }
    }
    c.useAsm = asmOk;
    // (a register that turns per-instance needs no seeding: the state row of EVERY register holds its current value at all
    // times - ensureState fills new ones, setRegister writes through - and a per-instance write made before the first block
    // must survive the first lowering)
    c.low = std::move(fresh);
    if (!offline) {
        if ((rc = ensureTram(c.low)) != 0) { *err = lastError_; return rc; }
        // the state may just have grown: the steps that follow go by what is allocated now
        in.instPerLane = instPerLane_;
        in.iSlotsAlloc = iSlotsAlloc_;
        in.xSlotsAlloc = xSlotsAlloc_;
        in.stateRows = stateRows_;
    }
    return 0;
}

// Step 2: generated code where the tier and the program allow it - translate, cut into stages where that pays, load the module.
int Batch::translateInto(Code& c, const BuildInputs& in, bool offline, std::string* err) {
    const int blockClass = in.blockClass;
    const char* forceHip = knobs_.kernel.empty() ? nullptr : knobs_.kernel.c_str();
    c.useXlate = false;
    c.stages = 1;
    c.deferred = false;
    c.xlateWhyNot.clear();
    if (c.useAsm && forceHip && std::strncmp(forceHip, "asm", 3) == 0) c.xlateWhyNot = "the interpreter is pinned by FX_KERNEL";
    else if (c.useAsm && c.variant == ASM_LDS) c.xlateWhyNot = "register file in LDS (above 224 rows): no translation template";
    else if (c.useAsm && c.low.multipass) c.xlateWhyNot = "END can be skipped (multi-pass program): the interpreter runs the passes";
    if (c.useAsm && c.low.multipass) {
        // (generated code is one pass over the program; the interpreter's end-of-sample handler starts the next one)
    } else if (c.useAsm && c.variant != ASM_LDS && in.defer) {
        // controls are moving (a set_register within the last few blocks): a translation costs a module load
        // (~1-2 ms), a re-encode for the interpreter ~0.05 ms - interpret until the controls have been quiet
        c.deferred = true;
        c.xlateWhyNot = "deferred: control registers are changing";
    } else if (c.useAsm && c.variant != ASM_LDS && !(forceHip && std::strncmp(forceHip, "asm", 3) == 0)) {
        // first choice for a VGPR build: translate the program into gfx950 code (FX_KERNEL=asm* pins the interpreter)
        const std::vector<MicroOp> steadyRecords = encodeAsmStream(c.low.steady, nullptr, true), lastRecords = encodeAsmStream(c.low.last, nullptr, true);
        std::vector<int> trackRows;
        for (int reg : in.trackRegs) trackRows.push_back(c.low.rowOfReg[(size_t)reg]);
        XlateProgram xprog = xlateProgramOf(steadyRecords, lastRecords, prog_.iTramSize, prog_.xTramSize, c.low.nRows, c.low.inRow, c.low.latchRow, trackRows);
        // 256 bytes per wavefront and slot; the Infinity Cache holds 256 MiB
        xprog.tramStreaming = ((size_t)in.iSlotsAlloc + (size_t)in.xSlotsAlloc) * (((size_t)n_ + 63) / 64) * 256 > ((size_t)512 << 20);
        xprog.prioritySlices = c.prioritySlices = priorityTurns(c.variant);
        XlateImage image;
        const XlateTemplate* tmpl = nullptr;
        bool built = false;
        tmpl = xlateTemplate(c.variant, &c.xlateWhyNot);
        // Small batches leave SIMDs empty (and a lone wavefront issues an instruction every ~4.5 clocks): cut the program
        // into stages run by the wavefronts of one workgroup (fx_xlate.hpp StageInfo) until ~4 wavefronts per SIMD are in
        // flight.  FX_STAGES pins the number asked for (1 = never).
        // how many stages: the caller's pick (a measured one, or an option on trial), else the cheapest by the planner's costs
        c.stageOptions = tmpl ? rankStages(steadyRecords, lastRecords, xprog, c.low.nRows, blockClass, kAsmWavesPerSimd[c.variant], in.stagingOff) : std::vector<StageOption>();
        int wantStages = in.stagePick > 0 ? in.stagePick : (c.stageOptions.empty() ? 1 : c.stageOptions.front().wanted);
        c.stagePick = wantStages;
        // (the wavefronts of a workgroup must be resident together: a CU holds 4 SIMDs x the build's wavefronts per SIMD - a pinned
        // FX_STAGES=16 in the 256-register build would be a launch that cannot start)
        wantStages = std::min(wantStages, 4 * kAsmWavesPerSimd[c.variant]);
        // Measured with config2 at 4 096 instances (profiles/r03b_stage_blocks.txt): a block of 32 samples takes 27 us unstaged, 32 us
        // in 8 stages with a barrier every 8 samples (3 x 7 steps of 8 samples to fill and drain) and 21 us in 4 stages with a
        // barrier per sample; 128 samples 69 / 48 / 40 us (8 stages, every 2 samples); from 256 samples on the long steps win
        // (rankStages charges a block of the class's typical length with the 3 (K - 1) steps of filling and draining)
        const int maxGroup = blockClass == 0 ? 1 : (blockClass == 1 ? 2 : kStageGroupMax);
        c.blockClass = blockClass;
        c.stagesWhyNot.clear();
        if (tmpl && wantStages >= 2) {
            const StagePlan plan = planStages(steadyRecords, lastRecords, xprog, c.low.nRows, wantStages);
            c.stagesWhyNot = plan.why;
            std::string why;
            c.classMatters = !plan.cuts.empty();
            if (!plan.cuts.empty()) {
                // (several workgroups per CU must fit its 160 KiB of LDS together)
                const int64_t groupsPerCu = std::max<int64_t>(1, ((n_ + 63) / 64 + 255) / 256);
                const uint32_t ldsBudget = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(144 * 1024, 160 * 1024 / groupsPerCu - 256));
                built = buildStagedImage(steadyRecords, lastRecords, *tmpl, xprog, plan, &image, nullptr, nullptr, &why, ldsBudget, maxGroup, knobs_.stagesGroup);
                if (!built) { c.stagesWhyNot = why; image = XlateImage(); }
            }
        }
        if (!built) built = tmpl && buildXlateImage(steadyRecords, lastRecords, *tmpl, xprog, &image, &c.xlateWhyNot);
        if (built) {
            hipError_t me = hipModuleLoadData(&c.module, image.elf.data());
            if (me == hipSuccess) me = hipModuleGetFunction(&c.fn, c.module, tmpl->kernelName.c_str());
            if (me != hipSuccess) return buildHipFail(err, me, "loading the translated program");
            c.steady = (uint64_t)image.steadyFastOff | ((uint64_t)image.steadyOff << 32);
            c.last = (uint64_t)image.lastFastOff | ((uint64_t)image.lastOff << 32);
            c.codeBytes = image.codeBytes;
            c.codeHash = imageHash(image);
            c.initOff = image.initOff;
            c.ldsBytes = image.ldsBytes;
            c.wildRow = image.wildRow;
            c.quiet = image.quietOff != 0;
            c.sumGroups = c.quiet && image.sumGroups;
            c.sumGroupCount = c.sumGroups ? (int)image.quietPlan.sumGroups.size() : 0;
            c.sumLinkCount = c.sumGroups ? image.quietPlan.sumLinks : 0;
            const XlateStats& loop = c.quiet ? image.quiet : image.steady;   // the loop that wavefronts start in
            c.unsaturated = loop.unsaturated;
            c.inlined = loop.inlined;
            c.called = loop.called;
            c.valu = loop.valu;
            c.valuSlow = loop.valuSlow;
            c.valuClocks = loop.valuClocks;
            c.vgprConstants = image.vgprConstants;
            if (offline) ++backgroundBuilds_; else ++xlateBuilds_;
            c.stages = image.stages;
            c.stageDesc = image.stageDesc;
            c.stageStoreRows = image.stageStoreRows;
            c.useXlate = true;
        }
    }
    if (offline && !c.useXlate) return buildFail(err, FX_E_NOTREADY, "offline build: the translation failed (" + c.xlateWhyNot + ")");
    return 0;
}

// Step 3: the record stream as the kernel reads it - steady | last | row table | stage descriptors - on the device.
int Batch::packStream(Code& c, const BuildInputs& in, bool offline, std::string* err) {
    if (c.useAsm && !c.useXlate) {
        hipError_t pe = hipSuccess;
        const uint64_t* handlers = asmHandlerTable(c.variant, device_, &pe);
        if (!handlers) return buildHipFail(err, pe, "probe of the assembly interpreter");
        const bool fold = c.variant != ASM_LDS;
        c.low.steady = encodeAsmStream(c.low.steady, handlers, fold);
        c.low.last = encodeAsmStream(c.low.last, handlers, fold);
    }
    const size_t nOps = c.low.steady.size();
    const bool staged = c.useXlate && c.stages > 1;
    const size_t words = nOps * 8 * 2 + c.low.loadRows.size() + c.low.storeRows.size() + c.low.zeroRows.size() + (staged ? (size_t)c.stages * 8 : 0);
    if (words > c.streamCap) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&c.dStream), words * 4 + 256);
        if (e != hipSuccess) return buildHipFail(err, e, "hipMalloc stream");
        c.streamCap = words;
    }
    std::vector<uint32_t> host(words);
    std::memcpy(host.data(), c.low.steady.data(), nOps * 32);
    std::memcpy(host.data() + nOps * 8, c.low.last.data(), nOps * 32);
    size_t p = nOps * 16;
    for (const RowCopy& rcp : c.low.loadRows) {
        // translated programs: bit 15 marks a row of the BOUNDED class (its state value is checked against 1.0)
        const bool bounded = c.useXlate && rcp.ldsRow < c.wildRow.size() && !c.wildRow[rcp.ldsRow];
        host[p++] = rcp.ldsRow | (bounded ? 0x8000u : 0u) | ((uint32_t)rcp.stateRow << 16);
    }
    if (staged) {
        // the store rows grouped by the stage that owns them; each stage's descriptor names its slice
        for (int k = 0; k < c.stages; ++k) {
            c.stageDesc[(size_t)k].storeFirst = (uint32_t)(p - (nOps * 16 + c.low.loadRows.size()));
            uint32_t count = 0;
            for (const RowCopy& rcp : c.low.storeRows) {
                const std::vector<int>& mine = c.stageStoreRows[(size_t)k];
                if (std::find(mine.begin(), mine.end(), (int)rcp.ldsRow) == mine.end()) continue;
                host[p++] = rcp.ldsRow | ((uint32_t)rcp.stateRow << 16);
                ++count;
            }
            c.stageDesc[(size_t)k].storeCount = count;
        }
        if (p != nOps * 16 + c.low.loadRows.size() + c.low.storeRows.size()) return buildFail(err, FX_E_PROGRAM, "internal: a store row without a stage");
    } else {
        for (const RowCopy& rcp : c.low.storeRows) host[p++] = rcp.ldsRow | ((uint32_t)rcp.stateRow << 16);
    }
    for (int zr : c.low.zeroRows) host[p++] = (uint32_t)zr;
    if (staged) {
        static_assert(sizeof(StageDescriptor) == 32, "StageDescriptor layout");
        std::memcpy(host.data() + p, c.stageDesc.data(), (size_t)c.stages * 32);
        p += (size_t)c.stages * 8;
    }
    // (a buffer of its own: no launch reads it yet.  The builder thread copies through a non-blocking stream of its own: a plain
    // hipMemcpy goes through the null stream, which would wait for - and hold up - a caller that launches on a blocking stream)
    hipError_t e;
    if (offline && builder_ && builder_->upload) {
        e = hipMemcpyAsync(c.dStream, host.data(), words * 4, hipMemcpyHostToDevice, builder_->upload);
        if (e == hipSuccess) e = hipStreamSynchronize(builder_->upload);
    } else {
        e = hipMemcpy(c.dStream, host.data(), words * 4, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return buildHipFail(err, e, "stream upload");
    c.key = in.key;
    return 0;
}

// a declared control that has a row only because ANOTHER control moved (markControls): every instance holds hostValue_ of it,
// and nothing but setRegister / setRegisterAt / setRegisterArray / a schedule / a state image can change that - each of which
// calls coldSetChanged() first
bool Batch::coldControl(int reg) const {
    const size_t r = (size_t)reg;
    return controlMode_ && reg >= 0 && r < forcedLane_.size() && r < declared_.size() && r < hotControl_.size() && declared_[r] && forcedLane_[r] && !hotControl_[r] &&
           !laneWritten_[r] && !tracked(reg) && !intrinsicLane(reg);
}

// the controls that could be folded into the code right now
std::vector<uint8_t> Batch::coldControls() const {
    std::vector<uint8_t> cold(forcedLane_.size(), 0);
    for (size_t r = 0; r < cold.size(); ++r) cold[r] = coldControl((int)r);
    return cold;
}

// laneForcedFull() minus a set of folded controls.  (The set is remembered, not the result: rows that other registers get
// meanwhile - a per-instance write, a schedule - must show up in the key of the next lowering; found by the API fuzzer's control
// panel, seed 2600545.)
std::vector<uint8_t> Batch::forcedWithout(const std::vector<uint8_t>& folded) const {
    std::vector<uint8_t> f = laneForcedFull();
    for (size_t r = 0; r < f.size() && r < folded.size(); ++r)
        if (folded[r]) f[r] = 0;
    return f;
}

std::vector<uint8_t> Batch::laneForced() const { return leanActive_ ? forcedWithout(leanFolded_) : laneForcedFull(); }

// Something is about to change that the lean code in force (or on order) may have folded in: back to the full variant (in the
// cache, never evicted while controls have rows: lruVictim) for the next block; a new lean one is asked for then.
void Batch::coldSetChanged() {
    if (!controlMode_) return;
    if (leanActive_) {
        leanActive_ = false;
        lowDirty_ = true;
    }
    leanPending_ = false;
    leanStale_ = true;
}

// a declared control is being written (broadcast): it is hot from now on; lean code that has its old value folded in goes
void Batch::controlWritten(int reg) {
    const size_t r = (size_t)reg;
    if (!controlMode_ || r >= hotControl_.size()) return;
    // a control that starts moving again after it had cooled down rests twice as long before it is folded in the next time (a
    // slider that moves every few hundred milliseconds would otherwise have code built for it, in the background but beside a
    // real-time stream, again and again: tools/realtime_capacity.py with FX_RT_SLIDER_EVERY=300, profiles/r05_rt_slow_slider.txt)
    if (!hotControl_[r] && cooledOnce_[r]) coolAfter_[r] = std::min<int64_t>(coolAfter_[r] * 2, kCoolSamplesMost);
    hotControl_[r] = 1;
    lastControlWrite_[r] = sampleClock_;
    if (leanActive_ && r < leanFolded_.size() && leanFolded_[r]) coldSetChanged();
    else leanStale_ = true;
}

// Head of a block, code in force and clean.  Controls that have not been written for kCoolSamples sample periods cool down (a
// slider is at rest most of the time; a preset recall writes the whole panel once); when the set of controls that could be
// folded differs from what the code in force has folded, the variant for it is asked of the builder thread, and adopted - a
// pointer swap in the lowering that follows - once it has arrived and is still what is wanted.
void Batch::leanStep() {
    if (!controlMode_ || lowDirty_) return;
    if (!builderWanted() || c_.key.empty() || !c_.useXlate || c_.deferred || tracksArmed()) return;
    if (sampleClock_ - lastCoolCheck_ >= kCoolSamples / 8) {
        lastCoolCheck_ = sampleClock_;
        for (size_t r = 0; r < hotControl_.size(); ++r)
            if (hotControl_[r] && sampleClock_ - lastControlWrite_[r] >= coolAfter_[r]) {
                hotControl_[r] = 0;
                cooledOnce_[r] = 1;
                leanStale_ = true;
            }
    }
    if (!leanStale_ && !leanPending_) return;
    const int cls = keyClass();
    const int pick = pickFor(cls);
    if (leanPending_) {
        if (codeKeyFor(forcedWithout(leanWant_), cls, false, pick) != leanKey_) {   // (a folded value, another register's row, the class or the stage count has changed meanwhile)
            leanPending_ = false;
            leanStale_ = true;
        } else {
            collectBuilt();
            if (cachedCode(leanKey_)) {
                leanPending_ = false;
                leanFolded_ = leanWant_;
                leanActive_ = true;
                lowDirty_ = true;
                return;
            }
            if (buildPending(leanKey_)) return;
            leanPending_ = false;   // (the builder could not make it: what runs stays)
        }
    }
    if (!leanStale_) return;
    leanStale_ = false;
    const std::vector<uint8_t> want = coldControls();
    const bool none = std::find(want.begin(), want.end(), (uint8_t)1) == want.end();
    if (leanActive_ ? want == leanFolded_ : none) return;
    if (none) {   // every control with a row is hot again: the full variant is the lean one
        leanActive_ = false;
        lowDirty_ = true;
        return;
    }
    const std::vector<uint8_t> forced = forcedWithout(want);
    const std::string key = codeKeyFor(forced, cls, false, pick);
    if (cachedCode(key)) {
        leanFolded_ = want;
        leanActive_ = true;
        lowDirty_ = true;
        return;
    }
    if (builder_ && buildFailed(key)) return;
    BuildInputs in = buildInputs(key, cls, false);
    in.forced = forced;
    in.stagePick = pick;
    requestBuild(std::move(in));
    leanWant_ = want;
    leanKey_ = key;
    leanPending_ = true;
}

// the cache entry to give up when it is full: the least recently used - but never the full control variant while controls have
// rows (the code every first touch, per-instance write and state image falls back to without a translation)
size_t Batch::lruVictim() const {
    std::string keep;
    if (controlMode_) {
        const int cls = keyClass();
        keep = codeKeyFor(laneForcedFull(), cls, false, pickFor(cls));
    }
    size_t lru = cache_.size();
    for (size_t k = 0; k < cache_.size(); ++k) {
        if (!keep.empty() && cache_[k]->key == keep) continue;
        if (lru == cache_.size() || cache_[k]->lastUse < cache_[lru]->lastUse) lru = k;
    }
    return lru == cache_.size() ? 0 : lru;
}

// Staged code is generated for a class of block lengths (a pipeline fills and drains in 3 (K - 1) steps: short blocks want
// short steps and fewer stages).  The class wanted follows the caller: at once when code for the new class exists already (a
// pointer swap in ensureLowered), after four blocks in a row otherwise - a stray block of another length is not worth a
// translation.  Programs that cannot be cut have one code for every length.
void Batch::noteBlockLength(int nSamples) {
    if (nSamples <= 0) return;
    const int cls = stageBlockClass(nSamples);
    if (wantedClass_ < 0 || c_.key.empty()) {   // the first block after a load (or after a failed build)
        wantedClass_ = cls;
        otherClassBlocks_ = 0;
        // (code that an fxb_info call had generated before the first block is for the shortest class)
        if (!c_.key.empty() && c_.classMatters && c_.blockClass != cls) lowDirty_ = true;
        return;
    }
    if (cls == wantedClass_) { otherClassBlocks_ = 0; return; }
    if (!c_.classMatters) return;   // one code for every block length
    ++otherClassBlocks_;
    const int was = wantedClass_;
    wantedClass_ = cls;
    collectBuilt();
    const int blockClass = keyClass();
    const bool defer = deferWanted();
    const std::string key = codeKey(blockClass, defer);
    if (cachedCode(key)) {
        otherClassBlocks_ = 0;
        lowDirty_ = true;
        return;
    }
    // not there: the builder thread makes it while the code in force (right for every length, only slower) keeps running; a
    // caller without that thread, or whose build cannot be done offline, gets it on its own thread once it has stayed
    if (!lowDirty_) requestBuild(buildInputs(key, blockClass, defer));
    if (otherClassBlocks_ >= 4 && !buildPending(key)) {
        otherClassBlocks_ = 0;
        lowDirty_ = true;
        return;
    }
    wantedClass_ = was;
}

}  // namespace fx
