// fx_batch.hpp — host engine behind the C ABI: N instances of one program on one GPU.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fx_asm.hpp"
#include "fx_batch_bus_side.hpp"
#include "fx_bus.hpp"
#include "fx_imajor.hpp"
#include "fx_instances.hpp"
#include "fx_registers.hpp"
#include "fx_tram.hpp"
#include "fx_tracks.hpp"
#include "fx_xlate.hpp"
#include "fx_decode.hpp"
#include "fx_kernel.hpp"
#include "fx_meter.hpp"
#include "fx_meter_list.hpp"
#include "fx_meter_rank.hpp"
#include "fx_meter_tone.hpp"
#include "fx_knobs.hpp"
#include "fx_model.hpp"

namespace fx {

inline uint32_t bitsOf(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// One column of a by-list call, either way between the caller's array and the staging: element i of the staging is element pos[i]
// of the caller's column (pos null: i), `bytes` each.  toCaller: `to` is the caller's column, else it is the staging.
inline void copyColumn(void* to, const void* from, const int64_t* pos, size_t count, size_t bytes, bool toCaller) {
    if (!pos) { std::memcpy(to, from, count * bytes); return; }
    for (size_t i = 0; i < count; ++i) {
        const size_t theirs = (size_t)pos[i] * bytes, ours = i * bytes;
        std::memcpy(static_cast<char*>(to) + (toCaller ? theirs : ours), static_cast<const char*>(from) + (toCaller ? ours : theirs), bytes);
    }
}

class Batch {
public:
    // throws std::runtime_error when no HIP device is usable (there is no CPU fallback)
    Batch(int64_t nInstances, int channels, int device);
    ~Batch();
    Batch(const Batch&) = delete;
    Batch& operator=(const Batch&) = delete;

    bool loadFile(const std::string& path);
    bool loadText(const std::string& text);

    int setRegister(const std::string& key, float v);                    // 0 found, 1 not found, <0 error
    int setRegisterAt(const std::string& key, int64_t inst, float v);
    float getRegisterAt(const std::string& key, int64_t inst);           // 1.0f when not found
    int setRegisterArray(const std::string& key, const float* values);   // values[n]
    int getRegisterArray(const std::string& key, float* values);
    int seedNoiseAt(int64_t inst, int32_t x1, int32_t x2);
    // A schedule of values for register `key`, applied by the NEXT process call: at sample s of that block, when s is a
    // multiple of `period`, the register takes values[s / period] (perInstance: values[(s / period) * pitch + instance];
    // pitch 0 = n) - what a caller of the reference does with setRegisterValue() between process() calls
    // (source/main.cpp:107-114), without cutting the block.  At most kMaxTracks registers; one-shot.
    int setRegisterTrack(const std::string& key, const float* values, int nSteps, int period, bool perInstance, int64_t pitch = 0);

    int processHost(const float* in, float* out, int nSamples, int64_t pitch = 0);  // synchronous; pitch: instances per host PCM row (0 = n)
    // dIn / dOut: [nSamples][channels][pitch] floats the device can address, this batch's instances are columns 0..n-1 (pitch 0 = n)
    int processDevice(const float* dIn, float* dOut, int nSamples, hipStream_t stream, int64_t pitch = 0);
    // the same for a caller's pointers: refused (FX_E_ARG, no launch) unless both footprints are memory of this handle's device or
    // device-visible host memory, and in == out or the two share no element
    int processDeviceChecked(const float* dIn, float* dOut, int nSamples, int64_t pitch, hipStream_t stream);
    // Group buses (fx_bus.hpp; include/fx8010_amd.h FXB_BUS_*): with kBusSharedIn `in` is [nSamples][channels][inPitch] with one
    // column per group of `group` instances, with kBusMixOut `out` is the same shape and takes every group's sum; a side without
    // its flag is [nSamples][channels][pitch] with one column per instance as in processHost.  Pitch 0: the side's own width.  A
    // shard of a larger batch passes the caller's full-width buffers from its own first column on.  kBusHost: synchronous, in
    // place on pinned buffers or staged; kBusDevice: the buffers are checked like processDeviceChecked's, asynchronous on `stream`.
    enum : unsigned { kBusSharedIn = 1u << 0, kBusMixOut = 1u << 1, kBusFlags = 3u };
    enum BusEntry { kBusHost, kBusDevice };
    // tapOut (null: an untapped block): the caller's [nSamples][channels][T] monitor side of the taps in force, see "Bus taps" below
    // auxOut (null: no sends delivered): the caller's [nSamples][channels][A] rows of the sends in force, see "Bus sends" below
    // feed: `in` is the source block [nSamples][channels][M] of the feeds in force (row pitch exactly M), see "Bus feeds" below
    int processBus(const float* in, float* out, int nSamples, int64_t group, unsigned flags, int64_t inPitch, int64_t outPitch, BusEntry entry, hipStream_t stream,
                   float* tapOut = nullptr, float* auxOut = nullptr, bool feed = false);
    // in == out with one layout, or footprints that share no byte (or no element, where both sides have one layout)
    // a source block of feeds and the output: no shared byte (the layouts differ: there is no in-place form)
    static bool feedSourceApart(const float* src, const float* out, size_t rows, int64_t sources, int64_t outWidth, int64_t outPitch);
    static bool busBuffersApart(const float* in, const float* out, size_t rows, int64_t inWidth, int64_t inPitch, int64_t outWidth, int64_t outPitch);
    // Instance-major blocks (fx_imajor.hpp; include/fx8010_amd.h fxb_process_block_imajor): instance i's input is the run of
    // nSamples * channels floats, [sample][channel], at in + i * inStride, its output the same at out + i * outStride (a stride in
    // floats, 0 = packed).  in == out with one stride, or footprints that share no element.  A shard of a larger batch passes
    // base + first * stride.  Entries as processBus's: kBusHost synchronous, in place on pinned buffers or staged; kBusDevice
    // checked once, asynchronous on `stream`.
    int processImajor(const float* in, float* out, int nSamples, int64_t inStride, int64_t outStride, BusEntry entry, hipStream_t stream);
    // the refusals that read nothing but the arguments (also asked by Sharded, for the whole batch): 0, or why not in *why; a stride
    // of 0 becomes the run
    static int checkImajorShape(const float* in, const float* out, int nSamples, int channels, int64_t n, int64_t* inStride, int64_t* outStride, const char** why);
    int sync();
    // Bus gains (fx_bus.hpp BusGainArgs; include/fx8010_amd.h "Bus gains"): a mode of the handle.  While it is on, the mix of a bus
    // block with kBusMixOut is launchBusMixGain.  `gains` is [channels][rowPitch] with this batch's instances in columns 0..n-1
    // (rowPitch 0 = n), copied through pinned memory of the library; null turns the mode off (waits, frees).  busReserveGains is the
    // allocating half (everything the mode ever needs: FX_E_MEMORY changes nothing), called by busSetGains itself and, for
    // all-or-nothing over shards, by Sharded in front of it; busReleaseGains frees what a failed attempt left on a handle whose
    // gains are off.  checked: the caller has found every value finite.  busGetGains is synchronous like meterRead.  Which of the
    // two gain blocks a set writes and which is in force: RampPair (fx_batch_bus_side.hpp), as for the send gains.
    int busReserveGains();
    void busReleaseGains();
    int busSetGains(const float* gains, int64_t rowPitch, int ramp, bool checked = false);
    int busGetGains(float* gains, int64_t rowPitch = 0);
    bool busGainsOn() const { return gainsOn_; }
    static bool gainsFinite(const float* gains, int channels, int64_t n, int64_t rowPitch);
    // Bus taps (fx_bus.hpp BusTapArgs; include/fx8010_amd.h "Bus taps"): a mode of the handle.  While it is on, a bus block with
    // kBusMixOut and a tapOut gathers the listed columns of the scratch block, pre-fader, into tapOut beside the mix.  `list` holds
    // `count` instance numbers of THIS batch, `pos` the column of the caller's [..][total] rows each of them goes to (null: entry k
    // goes to column k and total == count); total is the T of the whole handle - a shard may own none of the entries (count 0) and
    // still has taps on.  total == 0 turns the mode off (waits, frees).  busReserveTaps is the allocating half (the device list of
    // the set to come: FX_E_MEMORY changes nothing), called by Sharded on every shard in front of any busSetTaps, which then waits
    // for the queued blocks, swaps the lists and cannot run out of memory; busReleaseTaps drops a reservation that is not taken up
    // (ReservedBlock, fx_batch_bus_side.hpp).  The tap rows of a block go the side-row path of fx_batch_bus_side.cpp.
    // busGetTaps: list[pos[k]] = first + local entry k, for the columns below cap; returns total.
    static constexpr int64_t kMaxTaps = 65536;
    int busReserveTaps(int64_t count);
    void busReleaseTaps();
    int busSetTaps(const int64_t* list, const int64_t* pos, int64_t count, int64_t total);
    int64_t busGetTaps(int64_t* list, int64_t cap, int64_t first) const;
    int64_t busTaps() const { return tapTotal_; }
    // what a tapped call adds to the refusals of the bus entries that read nothing but the arguments (also asked by Sharded, for
    // the whole batch): null, or why not.  The footprints of in / out are those of busBuffersApart; with either of them null
    // nothing is compared.  (checkSideShape with the taps' texts.)
    static const char* checkTapShape(const float* in, const float* out, const float* tapOut, size_t rows, int64_t total, unsigned flags, int64_t inWidth, int64_t inPitch,
                                     int64_t outWidth, int64_t outPitch);
    // Bus sends (fx_bus.hpp BusSendArgs; include/fx8010_amd.h "Bus sends"): a mode of the handle.  While it is on, a bus block with
    // kBusMixOut and an auxOut sums the listed columns of the scratch block, pre-fader and each with a weight of its own, onto the
    // aux buses of a CSR structure.  A SendSet is what ONE batch holds of the structure of the whole handle: its buses in the
    // order of their numbers, with local member numbers, the column of the caller's [..][totalBuses] rows each goes to and where
    // its run begins among the caller's totalEntries entries (what fxb_bus_get_sends and the [C][E] of busSetSendGains go by).
    // A shard may own no bus and still has sends on; totalBuses == 0 turns the mode off (waits, frees).  busReserveSends is the
    // allocating half (the device block of the set to come: FX_E_MEMORY changes nothing), called by Sharded on every shard in
    // front of any busSetSends, which then waits for the queued blocks, takes the block, sets a = b and cancels a pending ramp;
    // busReleaseSends drops a reservation that is not taken up.  busSetSendGains(gains = the caller's [C][totalEntries], finite)
    // follows the state machine of busSetGains (RampPair); the next block with an auxOut consumes a pending ramp.  The reserved
    // block and the aux rows of a block are the taps' ReservedBlock and side-row path (fx_batch_bus_side.hpp) over again.
    static constexpr int64_t kMaxSendBuses = 65536, kMaxSendEntries = (int64_t)1 << 24;
    struct SendSet {
        int64_t totalBuses = 0, totalEntries = 0;
        std::vector<int64_t> offsets{0};     // [buses + 1] local CSR
        std::vector<int64_t> members;        // [entries] local instance numbers
        std::vector<int64_t> column, first;  // [buses]
        std::vector<float> gain[2];          // [channels][entries]; busSetSends reads gain[0]
        size_t chunkCount() const;
    };
    int busReserveSends(int64_t buses, int64_t entries, int64_t chunks);
    void busReleaseSends();
    int busSetSends(SendSet&& set);
    int busSetSendGains(const float* gains, int ramp);
    // host state only: this batch's buses into the caller's arrays (offsets[column], members / gains at the bus's global run,
    // below the caps); returns totalEntries
    int64_t busGetSends(int64_t* offsets, int64_t offCap, int64_t* members, float* gains, int64_t cap, int64_t firstInstance) const;
    int64_t busSendBuses() const { return send_.totalBuses; }
    int64_t busSendEntries() const { return send_.totalEntries; }
    // what an auxOut adds to the refusals of the bus entries that read nothing but the arguments (also asked by Sharded, for the
    // whole batch): null, or why not; a null in / out / tapOut is merely not compared.  (checkSideShape with the sends' texts.)
    static const char* checkAuxShape(const float* in, const float* out, const float* tapOut, const float* auxOut, size_t rows, int64_t buses, int64_t taps, unsigned flags,
                                     int64_t inWidth, int64_t inPitch, int64_t outWidth, int64_t outPitch);
    static const char* checkSideShape(const SideTexts& texts, const float* sideOut, size_t rows, int64_t total, unsigned flags, const Footprint* others, int nOthers);
    // Bus feeds (fx_bus.hpp BusFeedArgs; include/fx8010_amd.h "Bus feeds"): a mode of the handle, the sends mirrored on the input
    // side.  While it is on, processBus(..., feed = true) takes `in` as the narrow source block [nSamples][channels][M] and builds
    // the scratch block from per-instance lists of its columns (launchBusFeed) where kBusSharedIn expands it from n / K.  A FeedSet
    // is what ONE batch holds of the CSR-by-instance structure of the whole handle: the lists of its own instances - a contiguous
    // run of the caller's entries that begins at `first` (what fxb_bus_get_feeds and the [C][E] of busSetFeedGains go by).
    // sources == 0 turns the mode off (waits, frees).  weighted = false is the UNWEIGHTED form (words move as bit patterns); its
    // gain blocks hold 1.0f, which is what a ramp out of it starts from.  busReserveFeeds / busReleaseFeeds / busSetFeeds are
    // the two steps of busSetSends over again (ReservedBlock); busSetFeedGains(gains = the caller's [C][totalEntries], finite;
    // null: back to unweighted) follows the state machine of busSetGains (RampPair); the next feed block consumes a pending ramp.
    static constexpr int64_t kMaxFeedEntries = (int64_t)1 << 24;
    struct FeedSet {
        int64_t sources = 0, totalEntries = 0, first = 0;
        bool weighted = false;
        std::vector<int64_t> offsets{0};   // [n + 1] local CSR
        std::vector<int64_t> columns;      // [entries] source columns
        std::vector<float> gain[2];        // [channels][entries]; busSetFeeds reads gain[0]
        bool isMap() const;                // every instance has exactly one entry
    };
    int busReserveFeeds(int64_t sources, int64_t entries, bool map);
    void busReleaseFeeds();
    int busSetFeeds(FeedSet&& set);
    int busSetFeedGains(const float* gains, int ramp);
    // host state only: this batch's lists into the caller's arrays (offsets[firstInstance + i], sources / gains at the global
    // entries, below the caps)
    void busGetFeeds(int64_t* offsets, int64_t offCap, int64_t* sources, float* gains, int64_t cap, int64_t firstInstance) const;
    int64_t busFeedSources() const { return feed_.sources; }
    int64_t busFeedEntries() const { return feed_.totalEntries; }
    // Gain sets by list (fx_bus.hpp GainScatterArgs; include/fx8010_amd.h "Gain sets by list"; fx_batch_bus_gain_list.cpp): the
    // moved entries of the bus gains, the send gains or the feed gains, scattered on the device behind evBus_ like the copy of
    // busSetGains - no wait on the host for the queued blocks.  `list` holds `count` positions of THIS batch (instance numbers;
    // local entry numbers of send_ / feed_), no two alike, `pos` the column of the caller's [channels][total] values each of them
    // takes (null: entry k takes column k and total == count).  count == 0 with total > 0 is a shard that owns none of the entries:
    // it launches nothing and still makes the handle-wide "none pending -> pending" transition.  The caller has checked everything
    // (checkGainList, the modes) and has called busReserveGainList, the allocating half (device and pinned staging of
    // count * (channels + 1) words, the event: FX_E_MEMORY changes nothing).  busSendLocalEntry / busFeedLocalEntry: the local
    // number of a global entry of the structure in force, -1 when it belongs to another shard.
    static int checkGainList(const int64_t* list, int64_t count, int64_t range, const float* gains, int channels, const char* what, std::string* why);
    int busReserveGainList(int64_t count);
    int busSetGainsList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* gains, int ramp);
    int busSetSendGainsList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* gains, int ramp);
    int busSetFeedGainsList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* gains, int ramp);
    int64_t busSendLocalEntry(int64_t entry) const;
    int64_t busFeedLocalEntry(int64_t entry) const;
    // Output meters (fx_meter.hpp; include/fx8010_amd.h "Output meters"): a mode of the handle.  While it is on every emulation
    // launch is followed, on its stream, by a meter launch over the block it wrote.  meterEnable allocates and zeroes (on) or frees
    // (off) the accumulator rows - the only device allocation of metering; on twice keeps the values.  meterRead is synchronous:
    // every array is [channels][rowPitch] with this batch's instances in columns 0..n-1 (rowPitch 0 = n), any pointer may be null.
    int meterEnable(bool on);
    int meterRead(double* energy, float* peak, uint32_t* fullScale, uint32_t* nonfinite, bool reset, int64_t rowPitch = 0);
    int64_t meterSamples() const { return dMeter_ ? meterSamples_ : (int64_t)-3; }   // (FX_E_ARG while metering is off)
    bool metering() const { return dMeter_ != nullptr; }
    int prepare(int nSamples, bool wait);   // generate the code for blocks of this length now (and wait for the builder thread)

    // State snapshot (the reference keeps all DSP state in plain members, include/FX8010.h:162-217, 288-291: registers, output
    // latches, delay memory and its four positions, the LFSR words, the instruction counter).  The image is laid out by GLOBAL
    // instance, so a batch saved from one partition can be loaded into another: this batch's instances are columns
    // [first, first + n) of an image of nTotal instances.  Sections behind the header: state rows [stateRows][nTotal] u32,
    // iTRAM [nTotal][iSlots] f32, xTRAM [nTotal][xSlots] f32.
    struct SnapshotHeader {
        uint32_t magic = 0x54535846u, version = 1;   // "FXST"
        int64_t n = 0;
        int32_t channels = 0, nRegs = 0, stateRows = 0, iSlots = 0, xSlots = 0, reserved[7] = {};
    };
    static_assert(sizeof(SnapshotHeader) == 64, "SnapshotHeader layout");
    int snapshotShape(SnapshotHeader* hdr);   // what this batch would save (lowers the program first); n = this batch's instances
    // bytes of an image with this header; -1 for a header no batch could have written (a damaged file: negative or absurd
    // counts - nothing of it may enter an address computation)
    static int64_t snapshotBytes(const SnapshotHeader& hdr) {
        constexpr int64_t kMaxRows = 1 << 20, kMaxSlots = 1 << 20, kMaxInstances = (int64_t)1 << 40;
        if (hdr.n < 1 || hdr.n > kMaxInstances || hdr.stateRows < 1 || hdr.stateRows > kMaxRows || hdr.nRegs < 0 || hdr.nRegs > hdr.stateRows ||
            hdr.channels < 1 || hdr.channels > 4 || hdr.iSlots < 0 || hdr.iSlots > kMaxSlots || hdr.xSlots < 0 || hdr.xSlots > kMaxSlots)
            return -1;
        const uint64_t words = (uint64_t)hdr.stateRows + (uint64_t)hdr.iSlots + (uint64_t)hdr.xSlots;   // <= 2^20 + 2^21
        return (int64_t)(sizeof(SnapshotHeader) + (uint64_t)hdr.n * 4u * words);                            // < 2^40 * 2^24: no overflow
    }
    int saveStateColumns(uint8_t* image, const SnapshotHeader& hdr, int64_t first);
    int loadStateColumns(const uint8_t* image, const SnapshotHeader& hdr, int64_t first);
    // THE BY-LIST FRAME (fx_batch_list.cpp) - what every call below that changes device state by a list of instances has in common:
    //   check    the refusals that read nothing but the arguments, for the whole handle and with the caller's indices (the static
    //            check... functions, on checkList; Sharded asks before any shard is posted);
    //   reserve  the allocating half, on every shard before any shard changes a word (the reserve... functions, on
    //            reserveListStage: the event, the device block, the pinned block - FX_E_MEMORY changes nothing);
    //   stage    the host waits for the previous instance call or list set only (waitPreviousInstCall: its lists are in the staging
    //            this one is about to fill - between two sets of a real-time host lies a block, so that wait is over before it
    //            starts) and copies the list and the caller's columns into pinned staging: the caller's arrays are free on return;
    //   order    the handle's stream waits for every block queued so far on whatever stream (orderBehindQueuedBlocks: ev1_, evBus_);
    //   fence    the kernels run on the handle's stream and evInst_ is recorded behind them (closeInstCall): a block on another
    //            stream (launchBlock), the host in waitLastLaunch - every register call, every state access - and sync are ordered
    //            behind it.  A failure on the way waits for the stream first: nothing may still read the staging.
    // checkList: what is wrong with `list` and at which entry - the first one in list order outside 0..range-1, else (unique) the
    // first one in list order that repeats an earlier one.  Repeats are found in a bitmap over the range where that is the cheaper
    // one to clear (a real-time list of a thousand entries out of half a million: 56 KiB), else in a sorted copy (a few entries
    // out of millions); both name the same entry.
    struct ListFault {
        enum Kind { kNone, kOutside, kRepeat } kind = kNone;
        int64_t entry = -1;
        explicit operator bool() const { return kind != kNone; }
    };
    static ListFault checkList(const int64_t* list, int64_t count, int64_t range, bool unique);
    static std::string listOutside(const std::string& name, const ListFault& f, int64_t range);   // "<name>: entry i of the list is outside 0..range-1"
    // Per-instance state calls (fx_instances.hpp; include/fx8010_amd.h "Per-instance state").  A RECORD is the W = stateRows +
    // iSlots + xSlots words of one instance, packed: the state rows in the order of the whole-batch image, then the iTRAM slots, then
    // the xTRAM slots.  An instance image is a SnapshotHeader with kInstanceMagic and n = the number of records, then the records.
    // Every list here holds instance numbers of THIS batch; Sharded splits the caller's global lists.  All of them lower the program
    // first and run inside the by-list frame (above).
    static constexpr uint32_t kInstanceMagic = 0x49535846u;   // "FXSI"
    // the refusals that read nothing but the lists (Sharded asks for the whole batch): 0, or FX_E_ARG and why.  dst null: one list
    // whose entries must be distinct; else src may repeat, dst may not and may not appear in src
    static int checkInstanceLists(const int64_t* src, const int64_t* dst, int64_t count, int64_t n, const char** why);
    int instanceShape(SnapshotHeader* hdr, int64_t count);   // the header of an image of `count` records of this batch
    static int64_t instanceWords(const SnapshotHeader& hdr) { return (int64_t)hdr.stateRows + hdr.iSlots + hdr.xSlots; }
    // 0 when `hdr` (validated field by field) heads an instance image of `count` records this batch can take and `bytes` holds it
    int checkInstanceImage(const SnapshotHeader& hdr, int64_t count, int64_t bytes);
    int copyInstances(const int64_t* src, const int64_t* dst, int64_t count);   // stream-ordered
    int resetInstances(const int64_t* list, int64_t count);                     // stream-ordered
    // records to / from host memory, synchronous: the record of list[k] is the W words at buf + pos[k] * W (pos null: k)
    int gatherRecords(const int64_t* list, const int64_t* pos, int64_t count, uint32_t* buf);
    int scatterRecords(const int64_t* list, const int64_t* pos, int64_t count, const uint32_t* buf);
    // the delay-line rule of a load: FX_E_ARG unless the program executes no delay-line instruction or the four position words of
    // every record equal those the destination instance holds now.  Changes nothing.
    int checkRecordCursors(const int64_t* list, const int64_t* pos, int64_t count, const uint32_t* buf);
    // fxb_load_instances_rotated (include/fx8010_amd.h has the definition).  rotationApplies: the program has delay memory and
    // executes delay-line instructions - otherwise such a load goes the way of the plain one.  recordRotations: the rule of that
    // call - FX_E_ARG naming the line and the list entry, or rot = [count][2], the rotation of every record on iTRAM and xTRAM
    // from its position words and those its destination holds now.  Changes nothing.  scatterRecordsRotated: scatterRecords
    // through fx_inst_scatter_rot; the four position rows keep what they hold.
    int rotationApplies(bool* applies);
    int recordRotations(const int64_t* list, const int64_t* pos, int64_t count, const uint32_t* buf, std::vector<int32_t>* rot);
    int scatterRecordsRotated(const int64_t* list, const int64_t* pos, int64_t count, const uint32_t* buf, const int32_t* rot);
    // what the host knows about the registers follows a load of these `total` records (of all shards: every shard ends up with
    // the same rows): a register with a value other than hostValue_ in any record becomes per-instance, as after setRegisterAt
    void promoteLoaded(const uint32_t* buf, int64_t total);
    // Record bank (fx_bank.hpp; include/fx8010_amd.h "Record banks"; fx_batch_bank.cpp): nSlots packed records in device memory
    // of this batch's GPU.  store and recall run inside the by-list frame on the instance calls' staging (the two 64-bit lists and
    // nothing else: instance numbers, and slot words - the slot, and in the high half the caller's number of the entry, pos[i] or
    // i); put and get are synchronous copies.  `list` holds instance numbers of THIS batch; entry i has the slot slots[pos[i]]
    // (pos null: slots[i]).  Sharded has checked the lists for the whole handle (checkBankLists) and reserved on every shard.
    static int checkBankLists(const char* who, const int64_t* slots, const int64_t* list, int64_t count, int64_t nSlots, int64_t n, bool uniqueSlots,
                              std::string* why);
    // the allocating half of a create: the new bank, zero-filled, beside the one in force (FX_E_MEMORY changes nothing); take
    // makes it the bank and frees the old one behind everything queued, release frees it unused.  nSlots 0 reserves nothing and
    // take then leaves the batch without a bank.
    int bankReserve(int64_t nSlots);
    void bankTake();
    void bankRelease();
    int64_t bankSlots() const { return bankSlots_; }
    int reserveBankCall(int64_t count);   // the event, the two lists and the pairs of a call of `count` entries
    int bankStore(const int64_t* slots, const int64_t* list, const int64_t* pos, int64_t count);                     // stream-ordered
    int bankRecall(const int64_t* slots, const int64_t* list, const int64_t* pos, int64_t count, int64_t serial);    // stream-ordered
    // what the host knows about the registers follows a recall of these slots (of all shards, like promoteLoaded): a register is
    // noted as written per instance unless the shadow of every one of the slots holds a known word for it that equals hostValue_'s
    void bankNoteRecalled(const int64_t* slots, int64_t count);
    // slot slots[k] <- / -> the W words at records + k * W, synchronous, behind everything queued.  shadow (put): the shadow rows
    // that go with the records, [count][bankShadowRegs()]; null: every register's word is known, from the record
    int bankPutRecords(const int64_t* slots, int64_t count, const uint32_t* records, const uint64_t* shadow = nullptr);
    int bankGetRecords(const int64_t* slots, int64_t count, uint32_t* records);
    int bankShadowRegs() const { return bankRegs_; }
    const uint64_t* bankShadowRow(int64_t slot) const { return bankShadow_.data() + (size_t)slot * (size_t)bankRegs_; }
    // waits for the queued bank calls; out = { recalls refused since the last reset, the key of the most recent refused one
    // (fx_bank.hpp BankCell), its serial }; reset zeroes the three
    int bankStatus(uint64_t out[3], bool reset);
    // Register calls by list (fx_registers.hpp; include/fx8010_amd.h "Register sets by list"; fx_batch_registers.cpp).  `regs` holds
    // nKeys register numbers of the program (resolveRegisters), `list` holds `count` instance numbers of THIS batch, `pos` the column
    // of the caller's [nKeys][total] values each of them has (null: entry i has column i and total == count).  The caller has checked
    // everything (checkRegisterList) and, for a set, has called reserveRegisterList - the allocating half (device and pinned staging,
    // the event: FX_E_MEMORY changes nothing).  count == 0 is a shard that owns none of the entries: nothing is launched and nothing
    // changes.  setRegistersList leaves the batch as count * nKeys calls of setRegisterAt would, without their wait: the words are
    // scattered inside the by-list frame.  getRegistersList is synchronous and equals getRegisterAt word for word: a register that
    // lives on the host only is answered from hostValue_, the others by one gather.
    bool stateReady() const { return dState_ != nullptr; }
    int resolveRegisters(const char* const* keys, int nKeys, std::vector<int>* regs);   // 0, or 1 and lastError names the key
    // the refusals that read nothing but the arguments (Sharded asks for the whole handle), in the name of the call `name`: every
    // instance in 0..n-1 and, unique (a set), no instance and no register twice
    static int checkRegisterList(const char* name, const std::vector<int>& regs, const int64_t* list, int64_t count, int64_t n, const void* values, bool unique, std::string* why);
    int reserveRegisterList(int nKeys, int64_t count);
    int setRegistersList(const std::vector<int>& regs, const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* values);
    int getRegistersList(const std::vector<int>& regs, const int64_t* list, const int64_t* pos, int64_t count, int64_t total, float* values);
    // Register tracks by list (fx_tracks.hpp; include/fx8010_amd.h "Register tracks by list"; fx_batch_tracks.cpp): one call arms one
    // LIST SCHEDULE for the next block - step q falls due at sample first + q * period, where register regs[k] of instance list[i]
    // takes values[(q * nKeys + k) * total + pos[i]] (pos null: i, total == count).  `list` holds `count` instance numbers of THIS
    // batch.  checkTrackList holds the refusals that read nothing but the arguments (Sharded asks for the whole handle);
    // checkTrackListArm those that read what is armed and the program, and changes nothing; reserveTrackList is the allocating
    // half (the staging pair, the events, the track buffer for every step of everything armed: FX_E_MEMORY changes nothing);
    // armTrackList then cannot fail for want of memory.  count == 0 is a shard that owns none of the entries: its registers become
    // trackable all the same (every shard runs the same code) and the schedule counts towards kMaxListSchedules, but nothing is
    // staged and nothing will be launched for it.  Arming waits on the HOST only for the expansion that last read the staging
    // (evTrackList_, behind the last fx_track_scatter), never for a block.
    static constexpr int kMaxListSchedules = 64;
    static int checkTrackList(const std::vector<int>& regs, const int64_t* list, int64_t count, int64_t n, const float* values, int nSteps, int first, int period, std::string* why);
    int checkTrackListArm(const std::vector<int>& regs, const int64_t* list, int64_t count, int64_t firstGlobal, std::string* why);
    int reserveTrackList(const std::vector<int>& regs, int64_t count, int nSteps);
    int armTrackList(const std::vector<int>& regs, const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* values, int nSteps, int first, int period);
    int clearTrackLists();
    bool listScheduled(int reg) const;   // an armed list schedule names the register
    // Delay-line windows by list (fx_tram.hpp; include/fx8010_amd.h "Delay-line windows by list"; fx_batch_tram.cpp).  `list` holds
    // `count` instance numbers of THIS batch, `pos` the window of the caller's values each of them has (null: entry i has window
    // i); `in` is a set (stride 0: one window for all, FXB_TRAM_BROADCAST), `out` a get.  checkTramList holds the refusals that read
    // nothing but the arguments (Sharded asks for the whole handle); reserveTramList lowers the program, refuses a window the line
    // does not have, and is the allocating half (staging, the event: FX_E_MEMORY changes nothing) - count == 0 there still checks
    // the window, so that every shard is asked before any shard changes a word.  tramList with count == 0 is a shard that owns
    // none of the entries: nothing is launched and nothing changes.  A set runs inside the by-list frame, once per piece: a call of
    // several pieces blocks between them (the staging is reused).  A get is synchronous.  There is no host mirror of delay memory:
    // nothing else changes.
    static int checkTramList(bool set, int which, const int64_t* list, int64_t count, int64_t n, int first, int nWords, const void* values, unsigned flags, std::string* why);
    int reserveTramList(bool set, int which, int64_t count, int first, int nWords, unsigned flags);
    int tramList(int which, const int64_t* list, const int64_t* pos, int64_t count, int first, int nWords, const float* in, float* out, unsigned flags);
    // Meter queries by list (fx_meter_list.hpp; include/fx8010_amd.h "Meter queries by list"; fx_batch_meter_list.cpp).  The
    // check... functions hold the refusals that read nothing but the arguments (Sharded asks for the whole handle); the reserve...
    // functions are the allocating half (staging, the event: FX_E_MEMORY changes nothing; FX_E_ARG while metering is off) and take
    // what falls to THIS batch - nothing to do there reserves nothing.  meterSelect looks at the local columns first .. first +
    // nRange - 1, writes the min(M, cap) smallest matching numbers firstGlobal + (column - first) to `list`, ascending, and returns
    // M; nothing beyond min(M, cap) is touched.  meterReadList writes column pos[i] (null: i) of the caller's [channels][total]
    // arrays for list[i].  Both are synchronous.  meterResetList runs inside the by-list frame.  With count == 0 (a shard that owns
    // no entry) nothing is launched and nothing changes.  None of them touches meterSamples_.
    static int checkMeterSelect(int stat, double threshold, int64_t first, int64_t nRange, int64_t n, const int64_t* list, int64_t cap, unsigned flags, std::string* why);
    static int checkMeterList(const char* name, const int64_t* list, int64_t count, int64_t n, bool unique, std::string* why);
    int reserveMeterSelect(int64_t nRange, int64_t cap);
    int reserveMeterList(int64_t count, bool gather);
    int64_t meterSelect(int stat, double threshold, bool below, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, int64_t cap);
    int meterReadList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, double* energy, float* peak, uint32_t* fullScale, uint32_t* nonfinite, bool reset);
    int meterResetList(const int64_t* list, int64_t count);
    // Target meters (fx_meter.hpp MeterTargetArgs; include/fx8010_amd.h "Target meters"; fx_batch_meter_target.cpp).  Split
    // check / reserve / act like the list calls.  checkMeterTarget is the refusal of the whole handle's arguments (nTotal:
    // instances of the whole handle).  reserveMeterTarget allocates what a set needs for THIS batch - the block of the target
    // columns its instances firstGlobal .. firstGlobal + n - 1 use, the match rows where there are none - and keeps it aside;
    // FX_E_MEMORY or FX_E_ARG (metering off, the 32-bit row stride) changes nothing.  releaseMeterTarget frees what was kept
    // aside.  setMeterTarget waits as sync() does, copies this batch's columns out of the caller's [nSamples][channels][cols]
    // block, zeroes the match rows, takes the reserved blocks into force and sets the position to 0.  While a target is set
    // launchBlock launches fx_meter_target in place of fx_meter and advances the position, per launch.
    static int checkMeterTarget(const float* target, int64_t nSamples, int64_t group, unsigned flags, int channels, int64_t nTotal, std::string* why);
    int reserveMeterTarget(int64_t nSamples, int64_t group, int64_t firstGlobal);
    void releaseMeterTarget();
    int setMeterTarget(const float* target, int64_t nSamples, int64_t group, int64_t firstGlobal, int64_t cols, bool loop);
    int clearMeterTarget();
    bool meterTargetSet() const { return dTarget_ != nullptr; }
    int meterTargetSeek(int64_t pos);
    int64_t meterTargetPos() const { return dTarget_ ? targetPos_ : (int64_t)-3; }
    int meterReadMatch(double* err, double* cross, bool reset, int64_t rowPitch = 0);
    // select over V = the channel sum of match row `stat`: everything else as meterSelect, whose staging it shares
    static int checkMatchSelect(int stat, double threshold, int64_t first, int64_t nRange, int64_t n, const int64_t* list, int64_t cap, unsigned flags, std::string* why);
    int64_t matchSelect(int stat, double threshold, bool below, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, int64_t cap);
    // the best member of every group this batch has a part of: groups firstGlobal / group .. (firstGlobal + n - 1) / group, their
    // count is meterBestGroups; winner / value get one entry each (global instance numbers).  Synchronous.
    int64_t meterBestGroups(int64_t group, int64_t firstGlobal) const { return (firstGlobal + n_ - 1) / group - firstGlobal / group + 1; }
    int reserveMeterBest(int64_t group, int64_t firstGlobal);
    int meterBest(int stat, int64_t group, int64_t firstGlobal, bool largest, int64_t* winner, double* value);
    // Level meters (fx_meter.hpp LevelParams; include/fx8010_amd.h "Level meters"; fx_batch_meter_level.cpp).  Split check /
    // reserve / act like the target meters.  checkMeterLevel refuses for the whole handle and canonicalises -0.0 to +0.0.
    // reserveMeterLevel is the allocating half - the level rows, where there are none - and keeps them aside; FX_E_MEMORY or
    // FX_E_ARG (metering off) changes nothing.  setMeterLevel takes them into force zeroed - the first call waits as sync() does -
    // and sets the two parameters, which travel by value with every launch queued from then on; a call while the mode is on
    // changes only them.  While the mode is on launchBlock launches fx_meter_level / fx_meter_target_level in place of fx_meter /
    // fx_meter_target.  The reads and the select are synchronous and share the staging of the meter queries by list.
    static int checkMeterLevel(float* release, float* floor, unsigned flags, std::string* why);
    int reserveMeterLevel();
    void releaseMeterLevel();
    int setMeterLevel(float release, float floor);
    int clearMeterLevel();
    bool meterLevelOn() const { return dLevel_ != nullptr; }
    int getMeterLevel(float* release, float* floor);
    int meterReadLevel(float* level, uint32_t* quiet, bool reset, int64_t rowPitch = 0);
    int meterReadLevelList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, float* level, uint32_t* quiet, bool reset);
    // select over V = the channel maximum of `level` (stat 0) or the channel MINIMUM of `quiet` (stat 1): everything else as meterSelect
    static int checkLevelSelect(int stat, double threshold, int64_t first, int64_t nRange, int64_t n, const int64_t* list, int64_t cap, unsigned flags, std::string* why);
    int64_t levelSelect(int stat, double threshold, bool below, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, int64_t cap);
    // Meter ranks (fx_meter_rank.hpp; include/fx8010_amd.h "Meter ranks"; fx_batch_meter_rank.cpp).  Split check / reserve / act
    // like the selects.  family: kRankMeter / kRankMatch / kRankLevel - the rows, the range of `stat`, the counter.  checkMeterRank
    // holds the refusals that read nothing but the arguments.  reserveMeterRank grows the staging of the meter queries by list to
    // what this batch's part needs (FX_E_MEMORY changes nothing; FX_E_ARG while metering is off).  meterRank looks at the local
    // columns first .. first + nRange - 1 and writes the first R = min(M, k) candidates under the order (V, n) - V descending with
    // `largest`, ties to the smaller number - as firstGlobal + (column - first) to `list` and their V to `value` (may be null), in
    // rank order; nothing beyond R is touched; it returns M.  Synchronous; changes nothing on the device but the staging.
    static int checkMeterRank(int family, int stat, int64_t k, double threshold, int64_t first, int64_t nRange, int64_t n, const int64_t* list, unsigned flags, std::string* why);
    int reserveMeterRank(int64_t nRange, int64_t k);
    int64_t meterRank(int family, int stat, int64_t k, double threshold, bool below, bool largest, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, double* value);
    // Tone meters (fx_meter_tone.hpp; include/fx8010_amd.h "Tone meters"; fx_batch_meter_tone.cpp).  Split check / reserve / act
    // like the level meters.  checkMeterTones refuses for the whole handle and canonicalises -0.0 to +0.0.  reserveMeterTones is
    // the allocating half - a tone block for `tones` tones, kept aside; FX_E_MEMORY or FX_E_ARG (metering off) changes nothing.
    // setMeterTones waits as sync() does, takes the block into force with its header written and its rows zeroed and frees the
    // block it replaces: the accumulators of other coefficients mean nothing.  While the mode is on launchBlock queues
    // fx_meter_tone<K> behind the meter launch of the block, with the coefficients by value.  The reads, the select and the rank
    // are synchronous and share the staging of the meter queries by list (reserveToneList: a packed side of 24 bytes per tone,
    // channel and entry).
    static int checkMeterTones(int tones, const double* coeff, unsigned flags, double* canonical, std::string* why);
    int reserveMeterTones(int tones);
    void releaseMeterTones();
    int setMeterTones(int tones, const double* coeff);
    int clearMeterTones();
    int meterTones() const { return dTone_ ? toneCount_ : 0; }   // 0: the mode is off
    int getMeterTones(int* tones, double* coeff);
    int meterReadTones(double* s1, double* s2, double* power, bool reset, int64_t rowPitch = 0);
    int reserveToneList(int64_t count);
    int meterReadTonesList(const int64_t* list, const int64_t* pos, int64_t count, int64_t total, double* s1, double* s2, double* power, bool reset);
    // select over V = the channel maximum of P(tone): everything else as meterSelect.  (the tone is checked against K by the caller
    // that knows it: Sharded for the handle, runSelect for this batch)
    static int checkToneSelect(int tone, double threshold, int64_t first, int64_t nRange, int64_t n, const int64_t* list, int64_t cap, unsigned flags, std::string* why);
    int64_t toneSelect(int tone, double threshold, bool below, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, int64_t cap);
    // one instance's delay memory as the reference holds it (which: 0 smallDelayBuffer, 1 largeDelayBuffer), and its positions
    int getTramAt(int which, int64_t inst, float* out, int nSlots);
    int getCursorsAt(int64_t inst, int32_t out4[4]);

    int64_t instructionCounter();
    int64_t instructionCounterAt(int64_t inst);
    uint32_t oodFlags();
    float lastKernelMs();
    int64_t info(int what);
    std::string tierNote() const;   // which tier runs the program as it stands, and why not a faster one (fxb_tier_note)

    const Program& program() const { return prog_; }
    int64_t instances() const { return n_; }
    int device() const { return device_; }
    const std::string& lastError() const { return lastError_; }
    int channels() const { return prog_.numChannels; }        // fixed at construction: PCM layout of process()
    int loaderChannels() const { return prog_.loaderChannels; }  // reference getChannels()
    // reference setChannels(): only the loader's I/O-index bound changes (include/FX8010.h:73, source/FX8010.cpp:447)
    void setChannels(int c) { prog_.loaderChannels = c; }
    void noteError(const std::string& what) { lastError_ = what; }
    // behaviour beyond the reference (fx_model.hpp kOpt*): takes effect for programs loaded afterwards
    int setOption(unsigned option, bool on);

private:
    // ---- device state, registers, control tracks, snapshot, counters (fx_batch.cpp) -----------------------------------------------
    std::string tierNotePlain() const;
    int fail(int code, const std::string& what);
    int hipFail(hipError_t e, const char* where);
    int afterLoad(bool ok);
    int ensureState();            // allocate / grow the state block for the current register count
    int ensureTram(const Lowered& low);
    int uploadTracks(int nSamples, hipStream_t s);   // translated tier: header + values -> dTracks_
    bool tracked(int reg) const;
    std::vector<uint8_t> laneForcedFull() const;  // forcedLane_ plus the trackable registers
    int fillRows(const std::vector<uint32_t>& rows, const std::vector<uint32_t>& values);
    bool laneResident(int reg) const;
    bool intrinsicLane(int reg) const;
    int chooseInstPerLane() const;
    hipStream_t pick(hipStream_t s) const { return s ? s : stream_; }
    void waitLastLaunch();        // host waits for the most recent kernel (an event of ours, not the caller's stream handle)
    bool readByProgram(int reg) const;
    bool declaredControl(int reg) const;
    void markControls();
    bool movableControl(int reg) const;

    Program prog_;
    const ReleaseKnobs knobs_;          // the environment's release knobs as they were when the handle was created (fx_knobs.hpp)
    std::vector<float> hostValue_;      // current value of every register as the host knows it
    std::vector<uint8_t> forcedLane_;   // registers that live in a row of the register file although no instruction writes them:
                                        // per-instance values (setRegisterAt / setRegisterArray / a per-instance schedule) or a moving control
    std::vector<uint8_t> laneWritten_;  // ... of those, the ones whose instances may really hold different values (a broadcast write clears it)
    bool lowDirty_ = true;
    bool loaded_ = false;

    int64_t n_ = 0, nPad_ = 0;
    int device_ = 0;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    bool launched_ = false;  // ev1_ marks the end of the most recent launch (on whatever stream it ran)
    bool timed_ = false;

    uint32_t* dState_ = nullptr;
    StateLayout stateLayout_;
    int stateRows_ = 0;
    float* dITram_ = nullptr;
    float* dXTram_ = nullptr;
    int iSlotsAlloc_ = 0, xSlotsAlloc_ = 0;
    int instPerLane_ = 1;
    std::vector<uint8_t> intrinsicLane_, readByProgram_;   // per register, as of the last load
    double* dLut_ = nullptr;
    // control tracks (fx_xlate.hpp TrackEvent): registers the generated loop can re-load by itself, and what is armed
    struct PendingTrack { int period = 0, steps = 0; bool perInstance = false; std::vector<float> values; };
    std::vector<int> trackRegs_;           // register of slot t
    std::vector<PendingTrack> pendingTracks_;  // per slot; steps == 0: not armed
    uint32_t* dTracks_ = nullptr;
    // the quiet loop's exit words, one per wavefront (fx_xlate.hpp QuietPlan): 0xFFFFFFFF before a launch, then the sample at which
    // the wavefront left the loop, or the block length
    uint32_t* dQuietLeft_ = nullptr;
    size_t quietLeftWords_ = 0;
    bool lastLaunchQuiet_ = false;
    bool lastLaunchSums_ = false;    // ... in a loop with sum groups: the words are pairs {exit sample, repairs}
    int64_t quietRepairs();          // FXB_INFO_XLATE_QUIET_REPAIRS
    int ensureQuietLeft();
    int64_t quietLeft();             // FXB_INFO_XLATE_QUIET_LEFT
    size_t tracksCap_ = 0;                 // bytes
    bool tracksClear_ = false;             // the device header holds no armed schedule
    std::vector<uint32_t> trackStage_;     // host image of dTracks_ for the block being launched
    bool tracksArmed() const { if (!listSchedules_.empty()) return true; for (const PendingTrack& t : pendingTracks_) if (t.steps > 0) return true; return false; }
    // list schedules (fx_batch_tracks.cpp): what is armed for the next block, in arming order.  The lists, the values and the rows
    // of all of them lie in ONE staging pair of 32-bit words (pinned hTrackList_, the master copy; device trackList_), each
    // schedule's part at `at`: [count] instance numbers (64-bit), [steps][keys][count] values, [keys] state rows; a part is
    // copied to the device on stream_ when it is armed (evTrackCopy_ behind the copy).  A block expands them (expandTrackLists,
    // called by uploadTracks) or applies them at its cuts (applyTrackListsAt, the tiers without in-kernel tracks), records
    // evTrackList_ behind the last kernel that reads the staging and drops them: the next arming starts at word 0 behind a host
    // wait for that event.
    struct ListSchedule {
        std::vector<int> regs, slots;    // registers and their track slots
        std::vector<int64_t> list;       // local instance numbers (the refusal of a voice named twice for one register)
        int steps = 0, first = 0, period = 1;
        size_t at = 0;                   // word offset of its part of the staging
        int64_t count() const { return (int64_t)list.size(); }
        size_t valuesAt() const { return at + list.size() * 2; }
        size_t rowsAt() const { return valuesAt() + (size_t)steps * regs.size() * list.size(); }
        int stepsInside(int nSamples) const { return first >= nSamples ? 0 : (int)std::min<int64_t>(steps, ((int64_t)nSamples - 1 - first) / period + 1); }
    };
    std::vector<ListSchedule> listSchedules_;
    Block<uint32_t> trackList_, hTrackList_;
    size_t trackListUsed_ = 0;             // words of the staging that armed schedules occupy
    hipEvent_t evTrackCopy_ = nullptr;     // behind the most recent copy of a part to the device (stream_)
    hipEvent_t evTrackList_ = nullptr;     // behind the last kernel that read the staging
    bool trackListBusy_ = false;           // ... which may still be running
    int64_t trackListExpands_ = 0;         // FXB_INFO_TRACK_LIST_EXPANDS
    static size_t trackListPartWords(size_t nKeys, int64_t count, int nSteps) { return (((size_t)count * 2 + (size_t)nSteps * nKeys * (size_t)count + nKeys) + 1) & ~(size_t)1; }
    size_t trackBufferWorstBytes(const std::vector<int>* moreRegs, int moreSteps) const;
    int growTrackBuffer(size_t bytes);
    // the list part of uploadTracks: hold and scatter on the block's stream behind the header copy; `rowsAt` is the word of dTracks_
    // where the first event row lies, `tabAt` where the ranges of the schedules lie (in the header image, built by uploadTracks)
    struct ListExpansion {
        TrackHoldArgs hold{};
        struct Launch { size_t schedule, rangesAt; int nRanges; };
        std::vector<Launch> launches;
        size_t rowsAt = 0, totalRows = 0;
    };
    int expandTrackLists(const ListExpansion& x, hipStream_t s);
    int applyTrackListsAt(std::vector<ListSchedule>& schedules, int sample);   // a cut of processWithTrackFallback
    int finishTrackLists(hipStream_t s, bool launched);                        // evTrackList_ behind what was launched; the staging starts over
    uint32_t* dScratch_ = nullptr;  // small device scratch: fill lists, reductions
    // output meters: the accumulator rows (fx_meter.hpp), null while metering is off
    void* dMeter_ = nullptr;
    int64_t meterSamples_ = 0;      // sample periods metered since the last reset
    int64_t meterLaunches_ = 0;     // FXB_INFO_METER_LAUNCHES
    int meterReset();               // waits for what has been queued, zeroes the rows
#ifdef FX_DIAGNOSTICS
  public:
    // diagnostics build (fx_knobs.hpp): one word per wavefront, written by generated code behind its last sample when
    // FX_XLATE_ENDSTAMP is set (fx_xlate.cpp) - the low word of the 100 MHz clock at which the wavefront finished
    int readEndStamps(uint32_t* out, int64_t nWords);
  private:
    uint32_t* dStamps_ = nullptr;
    size_t stampWords_ = 0;
#endif
    std::string lastError_;

    // ---- what runs: lowering, code cache, builder thread, stage tuner, control variants (fx_batch_code.cpp) ------------------------
    int ensureLowered();          // (re)lower + upload the stream when dirty
    std::vector<uint8_t> laneForced() const;      // the registers with rows in the code that is wanted now: laneForcedFull(), minus the controls a lean variant in force has folded in
    std::vector<uint8_t> coldControls() const;    // the declared controls that have a row only for company and could be folded into the code (coldControl)
    std::vector<uint8_t> forcedWithout(const std::vector<uint8_t>& folded) const;   // laneForcedFull() minus those
    struct StageOption { int wanted = 1, stages = 1, group = 0; double predicted = 0.0; };   // wanted: what planStages is asked for (1: the plain program)
    // Everything a lowering produces - the lowered streams, the tier that runs them, the loaded code object of a translated
    // program and the device copy of its tables.  It is a pure function of a KEY (codeKey(): the program, the values folded
    // into the code, which registers have rows, the number of stages and the block-length class), so finished ones are
    // kept: a caller that comes back to a shape it has used before - a block length, a set of moving controls - gets a
    // pointer swap, not a translation and a module load.
    struct Code {
        std::string key;               // empty: nothing built
        Lowered low;
        bool useAsm = false;           // runs on the hand-written gfx950 kernel
        AsmVariant variant = ASM_LDS;
        std::string asmWhyNot;
        // translated program (fx_xlate.hpp): a code object of its own
        bool useXlate = false;
        hipModule_t module = nullptr;
        hipFunction_t fn = nullptr;
        uint64_t steady = 0, last = 0;  // {fast, exact} stream offsets as the kernel takes them
        uint32_t codeBytes = 0, initOff = 0, ldsBytes = 0;
        uint64_t codeHash = 0;          // imageHash() of the code object
        int stages = 1;                 // wavefronts per workgroup of the translated program (fx_xlate.hpp StageInfo)
        int blockClass = -1;            // the class of block lengths the staged code was generated for
        bool classMatters = false;      // the program can be cut: code for another class of block lengths would differ
        std::vector<StageDescriptor> stageDesc;
        std::vector<std::vector<int>> stageStoreRows;
        std::string stagesWhyNot;
        std::vector<StageOption> stageOptions;   // what rankStages made of the program (cheapest first)
        int stagePick = 1;                       // ... and the one this code was built for
        int inlined = 0, called = 0, unsaturated = 0, valu = 0, valuSlow = 0, valuClocks = 0, vgprConstants = 0;
        std::vector<uint8_t> wildRow;
        std::string xlateWhyNot;
        bool prioritySlices = false;   // generated code: the wavefronts of a SIMD take turns at the top priority (fx_xlate.hpp)
        bool quiet = false;            // generated code with a quiet loop (fx_xlate.hpp QuietPlan): wavefronts start there
        bool sumGroups = false;        // ... with sum groups (fx_xlate.hpp SumGroup)
        int sumGroupCount = 0, sumLinkCount = 0;
        bool deferred = false;          // the interpreter runs this one because controls were moving when it was built
        uint32_t* dStream = nullptr;    // records / row table / stage descriptors on the device
        size_t streamCap = 0;
        uint64_t lastUse = 0;
    };
    Code c_;                                     // the code in force
    std::vector<std::unique_ptr<Code>> cache_;   // finished ones that are not (at most kCodeCache)
    static constexpr size_t kCodeCache = 8;
    uint64_t useClock_ = 0;
    int loadGen_ = 0;
    int cacheHits_ = 0;
    std::string codeKey(int blockClass, bool defer) const;
    std::string codeKeyFor(const std::vector<uint8_t>& forced, int blockClass, bool defer, int pick) const;
    struct BuildInputs {                         // what a build reads of the batch's changing state (a snapshot: builds also run on the builder thread)
        std::string key;
        int blockClass = -1;
        bool defer = false;
        std::vector<float> hostValue;
        std::vector<uint8_t> forced;             // laneForced()
        std::vector<int> trackRegs;
        int stagePick = 0;                       // stages to ask the planner for; 0: the cheapest by its costs (rankStages)
        // the batch's device state as it was when the build was asked for: a build on the builder thread must not change any of
        // it and reads only this copy (the caller's thread may be growing the state or the delay lines meanwhile)
        int instPerLane = 1, iSlotsAlloc = 0, xSlotsAlloc = 0, stateRows = 0;
        bool stagingOff = false;
    };
    BuildInputs buildInputs(const std::string& key, int blockClass, bool defer) const;
    // the thread that generates code off the caller's thread (fx_batch_code.cpp: requestBuild and what follows it)
    struct Builder {
        std::thread thread;
        std::mutex mu;
        std::condition_variable cv;
        std::deque<BuildInputs> jobs;
        std::string running;                          // key being built
        std::vector<std::unique_ptr<Code>> finished;
        std::deque<std::string> failed;               // keys the offline path could not build (left to the caller's thread); the most recent kMaxFailed
        static constexpr size_t kMaxFailed = 32;      // (a forgotten one is merely asked for again)
        hipStream_t upload = nullptr;                 // the thread's own copy stream (created and destroyed by it; read by it only)
        bool quit = false;
    };
    std::unique_ptr<Builder> builder_;
    bool builderWanted() const;
    void requestBuild(BuildInputs&& in);
    void collectBuilt();                         // what the builder has finished -> cache_
    bool buildPending(const std::string& key);
    bool buildFailed(const std::string& key);
    bool waitBuild(const std::string& key);
    void drainBuilder(bool stop);
    void prebuildControlVariant();
    int keyClass() const;
    void noteBlockLength(int nSamples);
    bool deferWanted() const;
    bool cachedCode(const std::string& key) const;
    void stashCode();                            // c_ -> cache_ (evicting the least recently used), c_ = empty
    bool adoptCode(const std::string& key);      // cache_ -> c_
    void releaseCode(Code& c);                   // unload / free what a Code holds on the device
    void clearCodeCache();
    // the lowering, into an empty Code, in three steps.  `in` is the build's own copy: inline, the first step brings it up to date
    // with the device state it has just grown, so that the later steps read nothing but `in` on either thread
    int buildCodeInto(Code& c, BuildInputs in, bool offline, std::string* err);
    int chooseTierAndLower(Code& c, BuildInputs& in, bool offline, std::string* err);   // tier, lowered streams, state rows and delay lines
    int translateInto(Code& c, const BuildInputs& in, bool offline, std::string* err);  // generated code where the tier has it: image -> loaded module
    int packStream(Code& c, const BuildInputs& in, bool offline, std::string* err);     // records, row table, stage descriptors -> the device
    bool twoWavesPerSimd() const { return (n_ + 63) / 64 >= 2048; }   // 256 CUs x 4 SIMDs x 2
    bool priorityTurns(AsmVariant variant) const;
    int wantedClass_ = -1;                       // block-length class the code should be for (sticky: see processDevice)
    bool controlMode_ = false;                   // the declared controls have rows (the host has moved one)
    // Control mode puts EVERY declared control in a row at the first touch of one (one change of code for the panel, built ahead:
    // no stall).  A row costs what the value folded into the code saves - config5 with `damp` in a row: 100 INTERPs that convert X
    // and form 1 - X every sample and keep their saturation, +33 % per block - so the controls that actually move ("hot": written
    // since the load) keep their rows and the others go back into the code: the LEAN variant, built on the builder thread while
    // the full one runs, adopted at a block boundary (a pointer swap), dropped for the full one (cached, never evicted) the moment
    // a folded control moves.  Same words either way (tests: the knob / control-variant parity tests, tests/hipstub controls scenario).
    // A control is hot from a write until it has been left alone for kCoolSamples sample periods (a slider rests most of the
    // time; a preset recall writes the whole panel once): then its value is folded back in as well.
    std::vector<uint8_t> declared_;              // per register: a declared control (as of the last load)
    std::vector<uint8_t> hotControl_;            // ... that the host has written lately
    std::vector<int64_t> lastControlWrite_;      // sampleClock_ of that write
    int64_t sampleClock_ = 0, lastCoolCheck_ = 0;   // sample periods processed by this handle
    static constexpr int64_t kCoolSamples = 8192;   // 171 ms at 48 kHz: the first rest after which a control is folded in again
    static constexpr int64_t kCoolSamplesMost = int64_t(1) << 24;   // ... doubled every time it moved again after cooling, up to 5.8 minutes
    std::vector<int64_t> coolAfter_;             // per control: the rest it needs now
    std::vector<uint8_t> cooledOnce_;            // ... it has cooled down before
    bool leanActive_ = false;                    // a lean variant is the code wanted now: laneForced() == forcedWithout(leanFolded_)
    std::vector<uint8_t> leanFolded_;            // the controls it has folded in
    bool leanPending_ = false;                   // a lean variant has been asked of the builder thread: leanWant_ folded, leanKey_
    std::vector<uint8_t> leanWant_;
    std::string leanKey_;
    bool leanStale_ = false;                     // the set of hot controls may differ from the rows of the code in force / on order
    bool coldControl(int reg) const;
    void coldSetChanged();
    void controlWritten(int reg);
    void leanStep();                             // head of a block: cool controls down, ask for / adopt the lean variant
    size_t lruVictim() const;

    // ---- how many stages (rankStages: the planner's costs; noteLaunchTime: options the model cannot tell apart are measured)
    bool stagingPossible() const { return stagingPossibleGiven(stagingOff_); }
    bool stagingPossibleGiven(bool stagingOff) const;
    bool stagingOff_ = false;                    // a staged launch failed to start on this device: the plain program from then on
    std::vector<StageOption> rankStages(const std::vector<MicroOp>& steadyRecords, const std::vector<MicroOp>& lastRecords, const XlateProgram& xprog,
                                        int nRows, int blockClass, int wavesPerSimdCap, bool stagingOff) const;
    static constexpr double kTuneBand = 1.6;     // options predicted within this factor of the cheapest are tried
    static constexpr int kTuneRuns = 3, kTuneMinSamples = 8;
    struct Tuner {
        bool init = false, done = false;
        std::vector<StageOption> options;        // on trial (the model's cheapest first)
        std::vector<float> bestNs;               // per option: the fastest launch seen, ns per sample
        std::vector<int> runs;
        int pick = 0;                            // StageOption::wanted in force; 0: nothing built yet (the build picks the model's cheapest)
        int trials = 0;
    };
    Tuner tune_[3];                              // per block-length class
    int pickFor(int blockClass) const { return (blockClass >= 0 && blockClass < 3) ? tune_[blockClass].pick : 0; }
    void adoptStageOptions();                    // after a build / an adoption: the options the code came with start the class's tuner
    void noteLaunchTime();                       // the previous launch's time -> the tuner; move to the next option / settle
    int xlateBuilds_ = 0;                    // translations on the caller's thread since the handle was created
    std::atomic<int> backgroundBuilds_{0};   // ... and on the builder thread
    // a pipeline fills and drains in 3 (K - 1) steps: short blocks get short steps and fewer stages (stageBlockClass); the code is
    // generated for the class of the block that triggered the translation and again when the blocks stay in another class
    int otherClassBlocks_ = 0;
    static int stageBlockClass(int nSamples) { return nSamples <= 48 ? 0 : (nSamples <= 256 ? 1 : 2); }
    // control changes re-lower; while they keep coming the interpreter tier is used (see ensureLowered)
    static constexpr int kHeatPerChange = 8;  // blocks a change keeps the translation deferred
    int controlHeat_ = 0;
    int pendingSamples_ = 0;  // block length of the call that triggered the lowering
    bool everLowered_ = false;

    // ---- a block's path from the C ABI to the kernel launch (fx_batch_io.cpp) -----------------------------------------------------
    int checkBlock(const float* in, const float* out, int nSamples, int64_t* pitch);   // the argument refusals of every entry point; *pitch <= 0 becomes n
    void beginBlock(int nSamples, int pieces = 1);   // head of a caller-visible block: control heat, tuner, block-length class, lean variants, sample clock
    // how launchBlock is called: for a block of its own, for a piece of a pipelined host block (never timed by the stage tuner), or
    // without the event pair, by a caller that waits for the stream right behind the launch (last_kernel_ms: -1)
    enum LaunchMode : unsigned { kWholeBlock = 0, kPiece = 1, kUntimed = 2 };
    int launchBlock(const float* dIn, float* dOut, int nSamples, hipStream_t stream, int64_t pitch, unsigned mode);
    KernelArgs kernelArgs(const float* dIn, float* dOut, int nSamples, int64_t pitch) const;
    AsmArgs asmArgs(const KernelArgs& a) const;
    static hipError_t copyRows(void* dst, size_t dstPitch, const void* src, size_t srcPitch, size_t width, size_t rows, hipMemcpyKind kind, hipStream_t stream);
    int processWithTrackFallback(const float* dIn, float* dOut, int nSamples, hipStream_t stream, int64_t pitch);  // other tiers: cut the block
    int lastLaunchPick_ = 0, lastLaunchSamples_ = 0, lastLaunchClass_ = -1;
    bool lastLaunchTimed_ = false;
    float* dIn_ = nullptr;
    float* dOut_ = nullptr;
    size_t ioCap_ = 0;
    // small blocks (the reference's one process() per sample): pinned host buffers the kernel reads and writes directly
    float* hPinIn_ = nullptr;
    float* hPinOut_ = nullptr;
    bool pinTried_ = false;
    // large host blocks: pieces of the block are copied in, processed and copied out concurrently
    static constexpr int kHostPieces = 8;
    hipStream_t copyIn_ = nullptr, copyOut_ = nullptr;
    hipEvent_t evIn_[kHostPieces] = {}, evDone_[kHostPieces] = {};
    int processHostPipelined(const float* in, float* out, int nSamples, int64_t pitch, int pieces);
    unsigned lastGrid_ = 0;
    int64_t hostStagedBlocks_ = 0, hostInplaceBlocks_ = 0;   // host blocks by route (FXB_INFO_HOST_STAGED_BLOCKS / _INPLACE_BLOCKS)
    // processDeviceChecked: the last buffer pair that passed its checks (a real-time caller pays for the lookups once)
    CheckedAddr checkedIn_, checkedOut_;
    // `c` holds [p, p + bytes) when this returns 0; else FX_E_ARG with `what`, and c holds nothing
    int lookup(CheckedAddr& c, const void* p, size_t bytes, const char* what);
    // an input / output pair, checked together: a miss of either looks both up again, a refusal of either leaves neither cached
    int lookupPair(CheckedAddr& cIn, const void* in, size_t inBytes, CheckedAddr& cOut, const void* out, size_t outBytes);
    // bus blocks: expand -> the ordinary launch in place on the scratch -> mix, piece by piece on one stream
    struct BusShape { int64_t group = 1, groups = 1, inWidth = 0, outWidth = 0, inPitch = 0, outPitch = 0; };
    static constexpr size_t kBusScratchBytes = (size_t)64 << 20;   // 32 samples of 524 288 instances: real-time blocks are never cut
    int checkBus(const float* in, const float* out, const float* tapOut, const float* auxOut, int nSamples, int64_t group, unsigned flags, int64_t inPitch, int64_t outPitch, BusShape* shape,
                 bool feed = false);
    int ensureBusScratch(size_t floats);
    int ensureBusStage(size_t floats);
    // tap / aux: the routes of the two narrow sides beside the mix (fx_batch_bus_side.hpp Route; null: the caller gave no rows)
    int runBus(const float* in, float* out, const float* narrowIn, int64_t narrowInPitch, float* narrowOut, int64_t narrowOutPitch, int nSamples, unsigned flags,
               const BusShape& shape, hipStream_t stream, const Route* tap = nullptr, const Route* aux = nullptr, const FeedRoute* feed = nullptr);
    int busPieceSamples(int nSamples) const;   // the samples of the largest piece runBus cuts a block of nSamples into
    Block<float> bus_;              // the per-instance scratch [samples of a piece][channels][n]
    Block<float> busStage_;         // pageable host buffers: the [samples][channels][groups] sides of a block
    hipEvent_t evBus_ = nullptr;    // behind the last kernel of the most recent bus block
    bool busLaunched_ = false;
    int64_t busBlocks_ = 0;         // FXB_INFO_BUS_BLOCKS
    // bus gains (fx_batch_bus_gain.cpp): two blocks [channels][n] whose roles gainRamp_ keeps (fx_batch_bus_side.hpp RampPair): a
    // holds stale words unless a ramp is pending, so consuming a ramp costs nothing on the device.
    // Every write of a block is a copy on the handle's stream behind evBus_ (a block queued on whatever stream keeps the gains it
    // was queued with) and in front of evGain_ (a later block on whatever stream waits for it).
    float* dGain_[2] = {nullptr, nullptr};
    RampPair gainRamp_;
    // where a piece of a block is on the ramp of its gains, sends or feeds: the BusRampArgs base of the launch's arguments
    // (fx_bus.hpp); r is the one division of the definition: S is the caller's block, never a piece
    void setRamp(BusRampArgs& a, const RampPair& pair, int nSamples, int sample0) const {
        a = BusRampArgs{prog_.numChannels, pair.pending ? 1 : 0, 1.0f / (float)nSamples, nSamples, sample0};
    }
    bool gainsOn_ = false;
    float* hGain_ = nullptr;        // pinned staging: the caller's columns, and the 1.0f block of a ramp out of "off"
    hipEvent_t evGain_ = nullptr;   // behind the most recent copy into a gain block
    bool gainCopied_ = false;       // ... which may still be running
    int64_t busGainBlocks_ = 0;     // FXB_INFO_BUS_GAIN_BLOCKS
    size_t gainFloats() const { return (size_t)prog_.numChannels * (size_t)n_; }
    // gain sets by list (fx_batch_bus_gain_list.cpp): one staging pair for the three calls - [count] positions, then
    // [channels][count] values - grown on demand in the call (busReserveGainList), never inside a block, and reused: a set first
    // waits on the HOST for the previous list set's scatter (evList_, listCopied_).  The bus gains' set is also in front of evGain_
    // (runBus waits for it as for a full set); runBus waits for evList_ itself in front of a block with sends or feeds while a
    // list set of theirs is outstanding (sideListCopied_).  sync() clears both flags.
    struct GainListTarget {
        uint32_t* block[2];               // the two device gain blocks, [channels][pitch] words each
        size_t pitch;
        RampPair* ramp;
        std::vector<float>* mirror;       // the host copies gain[2] of a structure ([channels][mirrorPitch]); null: none (bus gains)
        size_t mirrorPitch;
        bool side;                        // sends / feeds: runBus waits for evList_
        const char* name;
    };
    int setGainList(const GainListTarget& t, const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* gains, int ramp);
    Block<uint32_t> gainList_, hGainList_;
    hipEvent_t evList_ = nullptr;        // behind the most recent list set
    bool listCopied_ = false;            // ... which may still be running (the staging is in use)
    bool sideListCopied_ = false;        // ... and was one of the send or feed gains
    int64_t gainListSets_ = 0;           // FXB_INFO_GAIN_LIST_SETS
    // the pieces every mode of a bus block is made of (fx_batch_bus_side.cpp)
    int growBlock(void** p, size_t* cap, size_t want, size_t bytesEach, bool pinned, const char* name);
    void freeBlock(void** p, size_t* cap, bool pinned);
    template <class T> int growBlock(Block<T>& b, size_t want, bool pinned, const char* name, size_t bytesEach = sizeof(T)) {
        return growBlock(reinterpret_cast<void**>(&b.p), &b.cap, want, bytesEach, pinned, name);
    }
    template <class T> void freeBlock(Block<T>& b, bool pinned) { freeBlock(reinterpret_cast<void**>(&b.p), &b.cap, pinned); }
    int reserveBlock(ReservedBlock& b, size_t words, const char* name);
    void releaseBlock(ReservedBlock& b);
    void takeUpBlock(ReservedBlock& b, bool any);
    void freeSideRows(SideRows& side);
    int planSideRoute(SideRows& side, const SideTexts& texts, float* out, const void* dev, size_t rows, size_t mine, int64_t total, const int64_t* place, Route* route);
    hipError_t queueSideCopyOut(const SideRows& side, const Route& route, float* out, size_t rows, hipStream_t stream);
    void placeSideColumns(const SideRows& side, const Route& route, float* out, size_t rows);
    // bus taps (fx_batch_bus_tap.cpp): the list as the host holds it and as the kernel reads it - one device block (tap_.cur),
    // tapCount() instance numbers and, where the entries have columns of their own (a shard), as many columns behind them.  Only
    // busSetTaps writes it, behind a wait for everything queued, so a queued block keeps the taps it was queued with.
    std::vector<int64_t> tapList_, tapPos_;   // this batch's entries (local numbers) and their columns (empty: identity)
    int64_t tapTotal_ = 0;          // T of the whole handle; 0: taps are off
    ReservedBlock tap_;             // cur: [tapList_.size()] idx, then [tapPos_.size()] col; busReserveTaps: the block of the set to come
    SideRows tapRows_;              // the caller's [S][C][T] side
    static const SideTexts kTapTexts;
    int64_t busTapBlocks_ = 0;      // FXB_INFO_BUS_TAP_BLOCKS
    int64_t tapCount() const { return (int64_t)tapList_.size(); }
    const int64_t* tapPlace() const { return tapPos_.empty() ? nullptr : tapPos_.data(); }
    hipError_t launchTaps(const Route& route, size_t first, long long rows, hipStream_t s);
    // bus sends (fx_batch_bus_send.cpp): the structure as the host holds it and one device block of 32-bit words (sendBlock_.cur) -
    // members, gain block 0, gain block 1, chunk table, bus table, at sendOff_[0..4]; sendRamp_ keeps the roles of the two gain
    // blocks.  Only busSetSends / busSetSendGains write it, behind a wait for everything queued.
    SendSet send_;
    ReservedBlock sendBlock_;            // busReserveSends: the block of the set to come
    size_t sendOff_[5] = {0, 0, 0, 0, 0};
    int64_t sendChunks_ = 0;
    bool sendIdentity_ = true;           // bus j is column j of the caller's rows (a handle of one shard)
    RampPair sendRamp_;
    Block<float> sendPartial_;           // [rows of a piece][sendChunks_] chunk sums, grown on demand in front of a block
    SideRows auxRows_;                   // the caller's [S][C][A] side
    static const SideTexts kAuxTexts;
    int64_t busSendBlocks_ = 0;          // FXB_INFO_BUS_SEND_BLOCKS
    size_t sendBlockWords(int64_t buses, int64_t entries, size_t chunks) const;
    void freeSendBlocks();
    int planAuxRoute(float* auxOut, const void* devAux, size_t rows, size_t pieceRows, Route* route);   // the chunk sums of the largest piece, then planSideRoute
    hipError_t launchSends(const Route& route, size_t first, long long rows, int nSamples, int sample0, hipStream_t s);
    // bus feeds (fx_batch_bus_feed.cpp): the structure as the host holds it and one device block of 32-bit words (feedBlock_.cur) -
    // offsets (CSR form only), source columns, gain block 0, gain block 1, at feedOff_[0..3], every table padded as BusFeedArgs
    // wants it; feedRamp_ keeps the roles of the two gain blocks.  Only busSetFeeds / busSetFeedGains write it, behind a wait for
    // everything queued.  feedSrc_: the device copy [rows][M] of a source block that is not device memory, grown on demand in
    // front of a block's first launch.
    FeedSet feed_;
    ReservedBlock feedBlock_;            // busReserveFeeds: the block of the set to come
    size_t feedOff_[4] = {0, 0, 0, 0};
    size_t feedGainPitch_ = 0;
    bool feedMap_ = false;
    RampPair feedRamp_;
    Block<uint32_t> feedSrc_;
    int64_t busFeedBlocks_ = 0;          // FXB_INFO_BUS_FEED_BLOCKS
    size_t feedBlockWords(int64_t entries, bool map, size_t* off4) const;
    int planFeedRoute(const float* src, const void* devSrc, size_t rows, FeedRoute* route);
    hipError_t launchFeed(const FeedRoute& route, size_t first, long long rows, int nSamples, int sample0, hipStream_t s);
    CheckedAddr busIn_, busOut_;   // kBusDevice: the last pair that passed its checks, as processDeviceChecked keeps one (the last d_tap_out / d_aux_out: tapRows_ / auxRows_)
    // instance-major blocks: gather -> the ordinary launch in place on the bus scratch -> scatter (the scratch, evBus_ and
    // busLaunched_ are shared with bus blocks: the two kinds may alternate, on different streams)
    int runImajor(const float* in, int64_t inStride, float* out, int64_t outStride, int nSamples, hipStream_t stream);
    int64_t imajorBlocks_ = 0;      // FXB_INFO_IMAJOR_BLOCKS
    CheckedAddr imajorIn_, imajorOut_;   // kBusDevice: the last pair that passed its checks
    // per-instance state calls (fx_batch_instances.cpp): a device list and a record scratch of their own, allocated on first use,
    // grown on demand and kept - the records up to kInstScratchBytes, the size of the bus scratch (not shared with it: a bus block
    // on a caller's stream and a copy on the handle's stream then never wait for each other's scratch); a call whose records exceed
    // it runs in pieces.  The lists go through pinned memory of the library, so the caller's arrays are free on return.
    static constexpr size_t kInstScratchBytes = (size_t)64 << 20;
    InstArgs instArgs() const;
    // lower, range check, lists -> device, order behind the blocks; `pairs` (without a list b): [count][2] words that travel in b's place
    int beginInstanceCall(const int64_t* a, const int64_t* b, int64_t count, size_t recordWords, const int32_t* pairs = nullptr);
    int endInstanceCall(bool wait);                           // evInst_ behind what was queued
    int64_t recordsPerPiece() const;
    Block<long long> instList_;          // [2][cap]: cap counts list entries
    Block<long long> hInstList_;         // pinned, same shape
    Block<uint32_t> instRec_;            // words
    Block<uint32_t> hInstRec_;           // pinned: the one record of a reset
    hipEvent_t evInst_ = nullptr;        // behind the last kernel or copy of the most recent instance call
    bool instLaunched_ = false;          // ... which may still be running
    int64_t instGathers_ = 0, instScatters_ = 0;   // FXB_INFO_INSTANCE_GATHERS / _SCATTERS
    int64_t instRotations_ = 0;                    // FXB_INFO_INSTANCE_ROTATIONS
    // record bank (fx_batch_bank.cpp): the slots, the cells of the gate (fx_bank.hpp BankCell) and the pairs of a recall - device
    // memory; bankWords_ is W as it was at the create (a call under another W is refused: the slots would not fit the records).
    // bankShadow_: per slot and register either the word the host knows the record to hold there, or kBankUnknown.
    static constexpr uint64_t kBankUnknown = (uint64_t)1 << 32;
    uint32_t* bank_ = nullptr;
    uint32_t* bankNew_ = nullptr;
    unsigned long long* bankCells_ = nullptr;
    Block<int> bankPairs_;
    int64_t bankSlots_ = 0, bankNewSlots_ = 0, bankWords_ = 0;
    int bankRegs_ = 0;
    std::vector<uint64_t> bankShadow_, bankNewShadow_;
    int64_t bankStores_ = 0, bankRecalls_ = 0;     // FXB_INFO_BANK_STORES / _RECALLS
    void freeBank();                               // behind everything queued; a program load and the destructor
    int bankReady(const char* who);                // lowered, a bank, and W as at the create
    int beginBankCall(const char* who, const int64_t* slots, const int64_t* list, const int64_t* pos, int64_t count);
    bool shadowed(int r) const { return !tracked(r) && !intrinsicLane(r); }
    // the by-list frame (fx_batch_list.cpp; "THE BY-LIST FRAME" above), shared by the instance calls and the list sets.
    // reserveListStage: `ev` on first use where wanted (texts[0] names it in FX_E_MEMORY), the capacity test, a wait for the call
    // that may still be reading the blocks that go (`ev` / `busy`), then the device block (texts[1]), then the pinned one (texts[2]).
    template <class T> int reserveListStage(Block<T>& dev, Block<T>& host, size_t words, hipEvent_t& ev, bool& busy, bool needEvent, const char* const (&texts)[3]) {
        if (needEvent && !ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ev = nullptr; return hipFail(hipErrorOutOfMemory, texts[0]); }
        if (words <= dev.cap && words <= host.cap) return 0;
        // (the previous list set may still be reading the blocks that go)
        if (busy && hipEventSynchronize(ev) == hipSuccess) busy = false;
        const int rc = growBlock(dev, words, false, texts[1]);
        return rc != 0 ? rc : growBlock(host, words, true, texts[2]);
    }
    int waitPreviousInstCall(const char* what);       // the host wait on evInst_ while instLaunched_
    hipError_t orderBehindQueuedBlocks();             // stream_ waits for ev1_ and evBus_: every block queued so far, on whichever stream
    int closeInstCall(hipError_t e, const char* what);   // evInst_ behind what was queued; any failure: wait for stream_, then hipFail(what)
    // what the host knows after a per-instance write to register r, as after setRegisterAt (the row stays valid for every other
    // instance: setRegister's invariant): the first such write to a register the code in force has folded in asks for other code
    void noteRegisterWritten(int r);
    void noteRegistersWritten(const std::vector<int>& regs) { for (const int r : regs) noteRegisterWritten(r); }
    // register calls by list (fx_batch_registers.cpp): one staging pair of 32-bit words, [count] instance numbers (64-bit), then
    // [nKeys][count] values, then [nKeys] rows - grown by reserveRegisterList and reused inside the frame
    Block<uint32_t> regList_, hRegList_;
    static size_t regListWords(int nKeys, int64_t count) { return (size_t)count * 2 + (size_t)nKeys * (size_t)count + (size_t)nKeys; }
    int stageRegisterList(const std::vector<int>& regs, const int64_t* list, int64_t count, RegListArgs* a);
    int64_t regListSets_ = 0, regListGets_ = 0;    // FXB_INFO_REGISTER_LIST_SETS / _GETS
    // delay-line windows by list (fx_batch_tram.cpp): a staging pair of 32-bit words of its own - [entries] instance numbers
    // (64-bit), then the windows of a piece, at most kInstScratchBytes of them - grown by reserveTramList and reused inside the
    // frame, piece by piece
    Block<uint32_t> tramStage_, hTramStage_;
    int64_t tramEntriesPerPiece(int nWords) const { return (int64_t)std::max<size_t>(kInstScratchBytes / ((size_t)nWords * 4), 1); }
    int64_t tramListSets_ = 0, tramListGets_ = 0;  // FXB_INFO_TRAM_LIST_SETS / _GETS
    // meter queries by list (fx_batch_meter_list.cpp): one staging pair of 64-bit words for the three calls - a select's chunk
    // offsets, total and list; a list call's list and packed rows - grown by the reserve... functions and reused: the synchronous
    // calls have drained everything, a reset runs inside the frame
    Block<unsigned long long> meterStage_, hMeterStage_;
    int reserveMeterStage(size_t words, bool needEvent);
    int64_t meterSelects_ = 0, meterListReads_ = 0, meterListResets_ = 0;   // FXB_INFO_METER_SELECTS / _LIST_READS / _LIST_RESETS
    enum class SelectRows { kMeter, kMatch, kLevel, kTone };   // which rows a select looks at, and with which predicate
    int64_t runSelect(SelectRows rows, int stat, double threshold, bool below, int64_t first, int64_t nRange, int64_t firstGlobal, int64_t* list, int64_t cap);
    // target meters (fx_batch_meter_target.cpp): the target block and the match rows in force (null: no target), the blocks a
    // set has reserved and not yet taken, the shape of the target, and the position of the next queued block
    float* dTarget_ = nullptr;
    void* dMatch_ = nullptr;
    float* targetNew_ = nullptr;
    void* matchNew_ = nullptr;
    int64_t targetSamples_ = 0, targetCols_ = 0, targetGroup_ = 1, targetFirstGlobal_ = 0, targetPos_ = 0;
    bool targetLoop_ = false;
    int zeroMatchRows();   // queued on stream_ and waited for
    MeterTargetArgs meterTargetArgs(const MeterArgs& m) const;   // of the block that is about to be queued
    int64_t meterTargetLaunches_ = 0, matchSelects_ = 0, matchBests_ = 0;   // FXB_INFO_METER_TARGET_LAUNCHES / _MATCH_SELECTS / _MATCH_BESTS
    // level meters (fx_batch_meter_level.cpp): the level rows in force (null: the mode is off), the block a set has reserved and
    // not yet taken, and the two parameters of the launches queued from now on
    void* dLevel_ = nullptr;
    void* levelNew_ = nullptr;
    float levelRelease_ = 0.0f, levelFloor_ = 0.0f;
    int zeroLevelRows();   // queued on stream_ and waited for
    LevelParams levelParams() const { return LevelParams{dLevel_, levelRelease_, levelFloor_}; }
    int64_t meterLevelLaunches_ = 0, levelSelects_ = 0, levelListReads_ = 0;   // FXB_INFO_METER_LEVEL_LAUNCHES / _LEVEL_SELECTS / _LEVEL_LIST_READS
    int64_t meterRanks_ = 0, matchRanks_ = 0, levelRanks_ = 0;   // FXB_INFO_METER_RANKS / _MATCH_RANKS / _LEVEL_RANKS (fx_batch_meter_rank.cpp)
    // tone meters (fx_batch_meter_tone.cpp): the tone block in force (null: the mode is off), the block a set has reserved and not
    // yet taken with the tone count it was sized for, and the mode: K and the coefficients of the launches queued from now on
    void* dTone_ = nullptr;
    void* toneNew_ = nullptr;
    int toneNewCount_ = 0;
    int toneCount_ = 0;
    double toneCoeff_[kMeterMaxTones] = {};
    int zeroToneRows();   // queued on stream_ and waited for
    int launchToneMeter(const MeterArgs& m, hipStream_t s);   // of the block that is about to be metered
    int64_t meterToneLaunches_ = 0, toneSelects_ = 0, toneListReads_ = 0, toneRanks_ = 0;   // FXB_INFO_METER_TONE_LAUNCHES / _TONE_SELECTS / _TONE_LIST_READS / _TONE_RANKS
    // a delay line as fxb_load_instances_rotated sees it: size Z, allocated slots, and which position kinds the program has an
    // instruction of (whether or not it is ever executed: a kind whose only instruction sits in a SKIP shadow that is always taken
    // counts, so such a record is compared - and may be refused - rather than loaded unseen)
    bool tramWrites_[2] = {false, false}, tramReads_[2] = {false, false};   // set by ensureTram
    struct RingLine { int size = 0, slots = 0; bool writes = false, reads = false; bool ring() const { return slots > 0 && slots == size; } };
    RingLine ringLine(int which) const;
#ifdef FX_DIAGNOSTICS
    int ensureEndStamps();   // the end stamps' buffer (dStamps_), one word per wavefront
#endif
};

}  // namespace fx
