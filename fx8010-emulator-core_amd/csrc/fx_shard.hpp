// fx_shard.hpp — one batch of instances spread over several GPUs of a node (SURVEY.md section 8 b/e).
//
// Instances share nothing mutable, so the partition is contiguous instance ranges: shard k owns instances
// [first_k, first_k + count_k) on device devices[k]; the program, its LUTs and the control values are replicated.
// There is NO exchange step and no collective: every operation is a fan-out to the shards and a fan-in of their
// results.  Each shard has its own host thread (so that the devices' copies, launches and waits overlap) and its
// own HIP stream (inside fx::Batch).  Every call that reaches a shard's device - broadcast or per instance - is posted
// to that shard's thread (fan / runOn), so the CALLER's current HIP device is never changed by a multi-shard handle; reads of
// replicated host state (program, error list, controls: front()) stay on the caller's thread.  A "sharded" batch with a
// single shard (what fxb_create() makes) runs inline on the caller's thread, under a guard that restores the caller's
// current device afterwards.
#pragma once

#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "fx_batch.hpp"

namespace fx {

class Sharded {
public:
    // devices: HIP ordinals, one shard each (an ordinal may repeat: several shards on one GPU); -1 = the calling thread's
    // current device.  Throws std::runtime_error when a device is unusable or there are more shards than instances.
    Sharded(int64_t nInstances, int channels, const std::vector<int>& devices);
    ~Sharded();
    Sharded(const Sharded&) = delete;
    Sharded& operator=(const Sharded&) = delete;

    // The partition: contiguous ranges of whole wavefronts (64 instances), the remainder in the last shard.  Pure
    // arithmetic (no device): fxb_shard_plan() exposes it, the constructor uses it.  Throws when a shard would be empty.
    static std::vector<std::pair<int64_t, int64_t>> plan(int64_t nInstances, int nShards);

    int shards() const { return (int)shards_.size(); }
    int64_t instances() const { return n_; }
    int64_t firstOf(int k) const { return shards_[(size_t)k]->first; }
    int64_t countOf(int k) const { return shards_[(size_t)k]->count; }
    int deviceOf(int k) const { return shards_[(size_t)k]->batch->device(); }
    Batch& shard(int k) { return *shards_[(size_t)k]->batch; }
    Batch& front() { return *shards_.front()->batch; }  // replicated state (program, errors, controls) reads from here

    bool loadFile(const std::string& path);
    bool loadText(const std::string& text);
    int setRegister(const std::string& key, float v);
    int setRegisterAt(const std::string& key, int64_t inst, float v);
    float getRegisterAt(const std::string& key, int64_t inst);
    int setRegisterArray(const std::string& key, const float* values);
    int getRegisterArray(const std::string& key, float* values);
    int seedNoiseAt(int64_t inst, int32_t x1, int32_t x2);
    int setRegisterTrack(const std::string& key, const float* values, int nSteps, int period, bool perInstance);
    void setChannels(int c);
    int setOption(unsigned option, bool on);

    // host buffers [sample][channel][pitch] (pitch >= all instances; 0 = all of them, a negative one is refused): every shard works on its own columns - in
    // place where the buffers are pinned memory its device can address, else it copies its columns in, runs, copies them out
    int processHost(const float* in, float* out, int nSamples, int64_t pitch = 0);
    // device-resident buffers, one pair per shard: dIn[k] / dOut[k] are [sample][channel][count_k] on shard k's device;
    // asynchronous (pair with sync())
    int processDeviceShards(const float* const* dIn, float* const* dOut, int nSamples);
    // single shard only: the caller's stream
    int processDevice(const float* dIn, float* dOut, int nSamples, hipStream_t stream);
    // ... with a row pitch; the buffers are checked first (Batch::processDeviceChecked)
    int processDevicePitched(const float* dIn, float* dOut, int nSamples, int64_t pitch, hipStream_t stream);
    // group buses (Batch::processBus): `in` / `out` are the caller's full-width buffers, [sample][channel][groups of the whole batch]
    // on a side with its flag.  Every shard must begin at a multiple of `group` (fxb_shard_plan tells the boundaries) and works on
    // its own group columns, on its own thread and device.  device: the caller's stream, single-shard handles only.
    // tapOut (null: none): the caller's full-width [sample][channel][T] rows of the taps in force; a shard writes its entries' columns
    int processBus(const float* in, float* out, int nSamples, int64_t group, unsigned flags, bool device, hipStream_t stream, float* tapOut = nullptr,
                   float* auxOut = nullptr,    // auxOut (null: none): the full-width [sample][channel][A] rows of the sends in force; a shard writes its buses' columns
                   bool feed = false);         // feed: `in` is the source block [sample][channel][M] of the feeds in force; every shard reads all of it
    // instance-major blocks (Batch::processImajor): shard k works on the runs from in + first_k * inStride on, on its own thread
    // and device.  device: the caller's stream, single-shard handles only.
    int processImajor(const float* in, float* out, int nSamples, int64_t inStride, int64_t outStride, bool device, hipStream_t stream);
    int sync();
    // output meters (Batch::meterEnable ...): enable fans out (a shard that cannot allocate leaves metering off on all of them),
    // read gives each shard its columns of the caller's [channels][all instances] arrays, samples is shard 0's
    int meterEnable(bool on);
    int meterRead(double* energy, float* peak, uint32_t* fullScale, uint32_t* nonfinite, bool reset);
    int64_t meterSamples();
    // meter queries by list (Batch "Meter queries by list"): global instance numbers throughout.  The arguments are checked for
    // the whole handle first; then every shard is asked for the staging of its part (of the range, of the list) before any shard
    // launches or changes a word.  select: each shard answers for the part of the range it owns, the parts are concatenated in
    // shard order - ascending - up to cap, the return value is the sum; a shard whose part is empty launches nothing.  read / reset:
    // each shard gets the entries that fall to it with local numbers and their columns; a shard without an entry launches nothing.
    int64_t meterSelect(int stat, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags);
    int meterReadList(const int64_t* list, int64_t count, double* energy, float* peak, uint32_t* fullScale, uint32_t* nonfinite, bool reset);
    int meterResetList(const int64_t* list, int64_t count);
    // target meters (Batch "Target meters"): `target` is the caller's [nSamples][channels][G] block by GLOBAL group column.  The
    // arguments are checked for the whole handle; every shard reserves the block of the columns ITS instances use (shards need
    // no alignment to `group`) and its match rows before any shard changes - FX_E_MEMORY leaves no target anywhere new and the
    // old one in force.  seek fans out, pos is shard 0's.  readMatch gives each shard its columns like meterRead; selectMatch is
    // meterSelect with the other predicate; best: each shard answers for the parts of the groups it owns and the partial
    // winners of a group that straddles shards are joined by the same order (V, then the instance number).
    int meterSetTarget(const float* target, int64_t nSamples, int64_t group, unsigned flags);
    int meterClearTarget();
    int meterTargetSeek(int64_t pos);
    int64_t meterTargetPos();
    int meterReadMatch(double* err, double* cross, bool reset);
    int64_t meterSelectMatch(int stat, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags);
    int meterBest(int stat, int64_t group, int64_t* winner, double* value, unsigned flags);
    // level meters (Batch "Level meters"): the arguments are checked for the whole handle; every shard reserves its level rows
    // before any shard changes - FX_E_MEMORY leaves the mode off everywhere (or, with the mode on, as it was).  get is shard 0's.
    // readLevel gives each shard its columns like meterRead, readLevelList its entries like meterReadList; selectLevel is
    // meterSelect with the level predicate.
    int meterSetLevel(float release, float floor, unsigned flags);
    int meterClearLevel();
    int meterGetLevel(float* release, float* floor);
    int meterReadLevel(float* level, uint32_t* quiet, bool reset);
    int meterReadLevelList(const int64_t* list, int64_t count, float* level, uint32_t* quiet, bool reset);
    int64_t meterSelectLevel(int stat, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags);
    // tone meters (Batch "Tone meters"): the arguments are checked for the whole handle; every shard reserves its tone block
    // before any shard changes - FX_E_MEMORY leaves the mode as it was everywhere.  get is shard 0's.  readTones gives each shard
    // its columns like meterReadLevel, readTonesList its entries like meterReadLevelList; selectTone is meterSelect with the tone
    // predicate; the rank goes through meterRank with the family kRankTone.
    int meterSetTones(int tones, const double* coeff, unsigned flags);
    int meterClearTones();
    int meterGetTones(int* tones, double* coeff);
    int meterReadTones(double* s1, double* s2, double* power, bool reset);
    int meterReadTonesList(const int64_t* list, int64_t count, double* s1, double* s2, double* power, bool reset);
    int64_t meterSelectTone(int tone, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags);
    // meter ranks (Batch "Meter ranks"; family: kRankMeter / kRankMatch / kRankLevel): the arguments are checked for the whole
    // handle; every shard reserves the staging of its part of the range before any shard launches; each shard answers with its own
    // first min(k, M_s) pairs, and the parts are merged under the same total order on global instance numbers - the first k of
    // the whole range are among them.  The return value is the sum of the M_s; a shard whose part is empty launches nothing.
    int64_t meterRank(int family, int stat, int64_t k, double threshold, int64_t first, int64_t nRange, int64_t* list, double* value, unsigned flags);
    // bus gains (Batch::busSetGains ...): `gains` is [channels][all instances] by global instance, checked as a whole (every value
    // finite) before any shard is posted; every shard reserves its blocks first and only when all of them could is any shard's
    // state changed (FX_E_MEMORY leaves the gains as they were everywhere); null turns them off.  get assembles the same layout.
    int busSetGains(const float* gains, int ramp);
    int busGetGains(float* gains);
    // bus taps (Batch::busSetTaps ...): `list` holds GLOBAL instance numbers, checked as a whole before any shard is posted; each
    // shard gets the entries of its range with their positions in the list (splitList) and reserves its device block first, so
    // FX_E_MEMORY leaves the old taps in force everywhere.  count 0 turns them off.  get: T, and the first min(T, cap) entries.
    int busSetTaps(const int64_t* list, int64_t count);
    int64_t busGetTaps(int64_t* list, int64_t cap);
    // bus sends (Batch::busSetSends ...): the CSR structure holds GLOBAL instance numbers and is checked as a whole before any
    // shard is posted; a bus belongs to the shard its members fall into (all into one, else FX_E_ARG naming the bus; an empty bus
    // to the first shard), every shard reserves its device block first, so FX_E_MEMORY leaves the old sends in force everywhere.
    // nAux 0 turns them off.  get: E, and what fits under the caps.
    int busSetSends(int64_t nAux, const int64_t* offsets, const int64_t* members, const float* gains);
    int busSetSendGains(const float* gains, int ramp);
    int64_t busGetSends(int64_t* nAux, int64_t* offsets, int64_t offCap, int64_t* members, float* gains, int64_t cap);
    // bus feeds (Batch::busSetFeeds ...): the CSR structure is by GLOBAL instance and is checked as a whole before any shard is
    // posted; each shard gets the lists of its own instances - a contiguous run of the entries - and reserves its device block
    // first, so FX_E_MEMORY leaves the old feeds in force everywhere.  The input side has no sum across shards: nothing straddles.
    // nSrc 0 turns them off.  get: E, and what fits under the caps.
    int busSetFeeds(int64_t nSrc, const int64_t* offsets, const int64_t* sources, const float* gains);
    int busSetFeedGains(const float* gains, int ramp);
    int64_t busGetFeeds(int64_t* nSrc, int64_t* offsets, int64_t offCap, int64_t* sources, float* gains, int64_t cap);
    // gain sets by list (Batch::busSetGainsList ...): `list` holds GLOBAL instance numbers (bus gains) or GLOBAL entry numbers of the
    // structure in force (sends, feeds), `gains` is [channels][count].  Everything is checked for the whole handle before any shard
    // is posted (range, repeats, finiteness, the mode); each shard gets the entries that fall to it with local numbers and their
    // columns of `gains`, reserves its staging first (FX_E_MEMORY changes nothing anywhere), and a shard without an entry still
    // makes the handle-wide "none pending -> pending" transition.  count 0: nothing happens.
    enum GainListKind { kGainList, kSendGainList, kFeedGainList };
    int busSetGainList(GainListKind kind, const int64_t* list, int64_t count, const float* gains, int ramp);
    int prepare(int nSamples, bool wait);

    // state snapshot of the whole batch, laid out by global instance (fx_batch.hpp SnapshotHeader): an image saved from one
    // partition loads into any other with the same program and instance count
    int64_t stateBytes();
    int saveState(void* buf, int64_t cap);
    int loadState(const void* buf, int64_t bytes);
    // per-instance state calls (Batch "Per-instance state calls"): the lists hold GLOBAL instance numbers and are checked for the
    // whole batch before any shard is posted, then split by shard.  Pairs of a copy inside one shard run on that shard's thread
    // and stream (stream-ordered); a pair that crosses shards goes gather -> pinned staging of the library -> scatter, in chunks
    // of the staging block, every chunk's gathers finished before its scatters start: such a call blocks.
    int64_t instanceImageBytes(int64_t count);
    int copyInstances(const int64_t* src, const int64_t* dst, int64_t count);
    int resetInstances(const int64_t* list, int64_t count);
    int saveInstances(const int64_t* list, int64_t count, void* buf, int64_t cap);
    int loadInstances(const int64_t* list, int64_t count, const void* buf, int64_t bytes) { return loadRecords(list, count, buf, bytes, false); }
    // ... with the delay memory of every record rotated to its destination's positions (Batch::recordRotations); a program that
    // executes no delay-line instruction or has no delay memory goes the way of loadInstances
    int loadInstancesRotated(const int64_t* list, int64_t count, const void* buf, int64_t bytes) { return loadRecords(list, count, buf, bytes, true); }
    // record bank (Batch "Record bank"): EVERY shard holds its own copy of the bank, so any instance recalls any slot without
    // traffic between devices.  create reserves on every shard before any shard changes (FX_E_MEMORY leaves the old bank in force
    // everywhere).  The lists are checked for the whole handle before any shard is posted.  put goes to every shard.  store
    // gathers on the shard that owns the instance (stream-ordered); with several shards the stored slots are then copied to the
    // other shards through the pinned staging of copyInstances, with their register shadow: such a call blocks.  recall splits by
    // ShardLists and stays stream-ordered on every shard; the device gate holds per shard.  status: the refused recalls summed
    // over shards (a call refused on two shards counts twice), and of the most recent refused call - by the handle's serial
    // number - the lowest bad entry on any shard, in the caller's numbering, with its reason.
    int bankCreate(int64_t nSlots);
    int64_t bankSlots();
    int bankStore(const int64_t* slots, const int64_t* list, int64_t count);
    int bankRecall(const int64_t* slots, const int64_t* list, int64_t count);
    int bankPut(const int64_t* slots, int64_t count, const void* image, int64_t bytes);
    int bankGet(const int64_t* slots, int64_t count, void* buf, int64_t cap);
    int bankStatus(int64_t* refusedCalls, int64_t* entry, int* reason, bool reset);
    // register calls by list (Batch "Register calls by list"): `list` holds GLOBAL instance numbers, `values` is [nKeys][count].
    // The keys are resolved and everything is checked for the whole handle before any shard is posted; each shard gets the
    // entries that fall to it with local numbers and their columns of `values` and, for a set, reserves its staging first
    // (FX_E_MEMORY changes nothing anywhere).  A shard without an entry launches nothing and changes nothing.
    int setRegistersList(const char* const* keys, int nKeys, const int64_t* list, int64_t count, const float* values) {
        return registersList(true, keys, nKeys, list, count, values, nullptr);
    }
    // list schedules (include/fx8010_amd.h "Register tracks by list"): keys resolved on the front shard, the whole call checked
    // before any shard is posted, every shard asked (what is armed, its staging, its track buffer) before any arms; a shard takes
    // its entries with their columns of every step - one without entries makes the registers trackable and stages nothing
    int setRegisterTracksList(const char* const* keys, int nKeys, const int64_t* list, int64_t count, const float* values, int nSteps, int first, int period);
    int clearRegisterTracksList();
    int getRegistersList(const char* const* keys, int nKeys, const int64_t* list, int64_t count, float* values) {
        return registersList(false, keys, nKeys, list, count, nullptr, values);
    }
    // delay-line windows by list (Batch "Delay-line windows by list"): `list` holds GLOBAL instance numbers, window i of `values`
    // belongs to list[i].  The whole list is checked first; then every shard is asked for the window and its staging
    // (reserveTramList) before any shard is posted a word; each shard gets the entries that fall to it with local numbers and
    // their windows of `values`.  A shard without an entry launches nothing and changes nothing.
    int setTramList(int which, const int64_t* list, int64_t count, int first, int nWords, const float* values, unsigned flags) {
        return tramList(which, list, count, first, nWords, values, nullptr, flags, true);
    }
    int getTramList(int which, const int64_t* list, int64_t count, int first, int nWords, float* values, unsigned flags) {
        return tramList(which, list, count, first, nWords, nullptr, values, flags, false);
    }
    int getTramAt(int which, int64_t inst, float* out, int nSlots);
    int getCursorsAt(int64_t inst, int32_t out4[4]);

    int64_t instructionCounter();
    int64_t instructionCounterAt(int64_t inst);
    uint32_t oodFlags();
    float lastKernelMs();  // slowest shard
    float lastKernelMsOf(int k);
    int64_t info(int what);
    const std::string& lastError();

private:
    int loadRecords(const int64_t* list, int64_t count, const void* buf, int64_t bytes, bool rotated);
    enum class SelectRows { kMeter, kMatch, kLevel, kTone };
    int64_t selectRange(SelectRows rows, int stat, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags);
    int registersList(bool set, const char* const* keys, int nKeys, const int64_t* list, int64_t count, const float* in, float* out);
    int tramList(int which, const int64_t* list, int64_t count, int first, int nWords, const float* in, float* out, unsigned flags, bool set);
    struct Worker {
        std::unique_ptr<Batch> batch;
        int64_t first = 0, count = 0;
        // a one-slot mailbox: the owner posts a task, the thread runs it, the owner waits for `done`
        std::thread thread;
        std::mutex mu;
        std::condition_variable cv;
        std::function<int()> task;
        bool pending = false, done = false, quit = false;
        int result = 0;
    };
    int shardOf(int64_t inst) const;
    // a global list by shard: per shard the local instance numbers and, for each, its index in the caller's list
    struct ListPart { std::vector<int64_t> list, pos; };
    std::vector<ListPart> splitList(const int64_t* list, int64_t count) const;
    // The list of a by-list call as the shards see it: shard k gets count(k) local numbers list(k), entry i of them column pos(k)[i]
    // of the caller's arrays (null: column i).  A handle of one shard passes the caller's list through - a global number is a local
    // one - with a null pos; several shards hold splitList's parts.  split == false hands no entry to any shard: a call that
    // moves nothing and still asks every shard (tramList).
    class ShardLists {
    public:
        ShardLists(const Sharded& s, const int64_t* list, int64_t count, bool split = true) : whole_(list), count_(count), one_(s.shards_.size() == 1) {
            if (!one_) parts_ = split ? s.splitList(list, count) : std::vector<ListPart>(s.shards_.size());
        }
        explicit ShardLists(std::vector<ListPart>&& parts) : parts_(std::move(parts)) {}   // parts the caller has filled, one per shard
        void samePos(bool on) { samePos_ = on; }   // every entry reads the one column there is (a broadcast): pos(k) is null
        const int64_t* list(int k) const { return one_ ? whole_ : parts_[(size_t)k].list.data(); }
        const int64_t* pos(int k) const { return (one_ || samePos_) ? nullptr : parts_[(size_t)k].pos.data(); }
        int64_t count(int k) const { return one_ ? count_ : (int64_t)parts_[(size_t)k].list.size(); }
    private:
        const int64_t* whole_ = nullptr;
        int64_t count_ = 0;
        bool one_ = false, samePos_ = false;
        std::vector<ListPart> parts_;
    };
    static constexpr size_t kStageBytes = (size_t)64 << 20;
    uint32_t* hStage_ = nullptr;   // pinned (portable) staging of cross-shard copies, allocated on first use and kept
    size_t stageWords_ = 0;
    int growStage(size_t words, const char* who);   // hStage_ of at least `words`; FX_E_MEMORY and why, with the old block gone
    int bankChecked(const char* who, const int64_t* slots, const int64_t* list, int64_t count, bool instances, bool uniqueSlots);
    int64_t bankSerial_ = 0;       // recalls of this handle so far: tells the most recent refused one across shards
    // run f(k, batch) on every shard's thread, wait for all; returns the first non-zero result (shard order)
    int fan(const std::function<int(int, Batch&)>& f);
    // run f(batch) on shard k's thread and wait (a single shard: inline, caller's device restored)
    int runOn(int k, const std::function<int(Batch&)>& f);
    // reserve on every shard; if any fails, release on all of them and keep the first error
    int reserveOnAll(const std::function<int(int, Batch&)>& reserve, const std::function<void(Batch&)>& release);
    void stopThreads();
    static void loop(Worker* w);

    int64_t n_ = 0;
    std::vector<std::unique_ptr<Worker>> shards_;
    std::string lastError_;
    // One call at a time per handle.  A handle is not meant for concurrent use (the reference's objects are not either), but a host
    // with a UI thread that reads a register while its audio thread processes a block must get serialised calls, not corrupted
    // ones: every public call that touches the shards or lastError_ holds this for its whole duration (recursive: fan / runOn
    // take it again for their posts to the one-slot mailboxes).  Found wanting by ThreadSanitizer: lastError_.clear() used to run
    // in front of the lock (tests/hipstub/host_threads.cpp, scenario "shards").
    std::recursive_mutex api_;
    using Serial = std::lock_guard<std::recursive_mutex>;
};

}  // namespace fx
