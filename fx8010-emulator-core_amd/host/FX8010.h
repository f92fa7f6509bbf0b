// FX8010.h — host-side mirror of the reference's public header, over the C ABI of libfx8010_amd.so.
//
// Same namespace, class name, member names, argument meaning and return conventions as the
// reference (include/FX8010.h:47-75), plus everything else that header hands to a translation unit
// that includes it (include/FX8010.h:12-25 the standard headers and `using namespace std`, :33-42 the
// macros E, PI, SAMPLERATE, AUDIOBLOCKSIZE, DEBUG, PRINT_REGISTERS, MAX_IDELAY_SIZE, MAX_XDELAY_SIZE,
// :50 the default constructor), so that a caller written against the reference - its console harness
// source/main.cpp, or the VST block loop it is meant for - compiles unchanged against this header and
// runs the instruction loop on an MI355X instead of the host CPU.  tests/test_dropin_harness.py compiles
// and links the reference's own source/main.cpp + source/helpers.cpp, where they lie, against it:
//     g++ -std=c++17 -DFX8010_REFERENCE_COMPAT -include fx8010-emulator-core_amd/host/FX8010.h -I include \
//         /root/reference/source/main.cpp /root/reference/source/helpers.cpp -L fx8010-emulator-core_amd -lfx8010_amd
// (with FX8010_REFERENCE_COMPAT this header defines the reference's include guard FX8010_H, so main.cpp's own
// #include "../include/FX8010.h" contributes nothing; without it only the classes below are declared).
//
//   Klangraum::FX8010         one emulated DSP, one process() call per sample period
//   Klangraum::FX8010Batch    N independent DSPs stepping one program on one GPU (the data-parallel path) or, built
//                             with a device list / mask, over several GPUs of one node (contiguous instance
//                             ranges, one host thread + stream per device, no collective)
//
// Header-only; link with -lfx8010_amd.  Differences that remain, by design:
//   * construction prints no banner (the reference prints ~7 lines, source/FX8010.cpp:18-24);
//   * when no HIP device is usable the constructor throws std::runtime_error - there is no CPU path;
//   * getInstructionCounter() is computed in 64 bits and truncated to int like the reference's field;
//   * the default constructor, declared but never defined by the reference (include/FX8010.h:50), makes a
//     one-channel DSP.
#ifndef FX8010_AMD_HOST_FX8010_H
#define FX8010_AMD_HOST_FX8010_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "fx8010_amd.h"

// ---- opt-in: everything ELSE the reference header hands its includers (define FX8010_REFERENCE_COMPAT before including, or
// pass -DFX8010_REFERENCE_COMPAT).  The reference's own callers need it - source/main.cpp relies on `using namespace std`, PI,
// DEBUG, AUDIOBLOCKSIZE and on <iostream> / <chrono> / <math.h> coming with the header - but a new includer (a plug-in host)
// should not get a namespace dump and macros called E and DEBUG, so the class below is available without it.
#ifdef FX8010_REFERENCE_COMPAT
// the reference header's own guard: whoever includes this file has "included FX8010.h" (a later #include of the reference's
// include/FX8010.h contributes nothing)
#ifndef FX8010_H
#define FX8010_H
#endif

// what include/FX8010.h:12-24 pulls in for its includers
#include <stdio.h>
#include <iostream>
#include <chrono>
#include <math.h>
#include <fstream>
#include <iomanip>
#include <sstream>
#include <regex>
#include <map>
#include <array>
#include <unordered_map>

using namespace std;  // include/FX8010.h:25 - part of what the reference header exports (main.cpp relies on it)

// the reference's compile-time settings (include/FX8010.h:33-42)
#ifndef E
#define E 2.71828182845
#endif
#ifndef PI
#define PI 3.14159265359
#endif
#ifndef SAMPLERATE
#define SAMPLERATE 48000
#endif
#ifndef AUDIOBLOCKSIZE
#define AUDIOBLOCKSIZE 32
#endif
#ifndef DEBUG
#define DEBUG 0
#endif
#ifndef PRINT_REGISTERS
#define PRINT_REGISTERS 0
#endif
#ifndef MAX_IDELAY_SIZE
#define MAX_IDELAY_SIZE 8192
#endif
#ifndef MAX_XDELAY_SIZE
#define MAX_XDELAY_SIZE 1048576
#endif
#endif  // FX8010_REFERENCE_COMPAT

namespace Klangraum {

// the reference's settings as constants (include/FX8010.h:35-36, :41-42), whether or not the macros are exported
constexpr int kSampleRate = 48000, kAudioBlockSize = 32, kMaxIDelaySize = 8192, kMaxXDelaySize = 1048576;

class FX8010 {
public:
    // reference: FX8010(), include/FX8010.h:50 (declared only there)
    FX8010() : FX8010(1) {}
    // reference: FX8010(int numChannels), include/FX8010.h:51
    FX8010(int numChannels) : channels_(numChannels), h_(fx_create(numChannels)) {
        if (!h_) throw std::runtime_error(std::string("FX8010: ") + fx_last_create_error());
    }
    ~FX8010() { fx_destroy(h_); }
    FX8010(const FX8010&) = delete;
    FX8010& operator=(const FX8010&) = delete;

    // reference: initialize() builds the LOG/EXP tables; here they are built when the library loads
    void initialize() {}

    // reference: std::vector<float> process(const std::vector<float>&), include/FX8010.h:57
    std::vector<float> process(const std::vector<float>& inputSamples) {
        std::vector<float> out((size_t)channels_, 0.0f);  // the reference's outputBuffer keeps its constructed size (FX8010.cpp:122)
        if (fx_process(h_, inputSamples.data(), out.data()) < 0) throw std::runtime_error(std::string("FX8010::process: ") + fx_last_error(h_));
        return out;
    }
    // extension: nSamples consecutive sample periods in one launch; in/out are [nSamples][channels]
    std::vector<float> processBlock(const std::vector<float>& in, int nSamples) {
        std::vector<float> out((size_t)nSamples * (size_t)channels_, 0.0f);
        if (fx_process_block(h_, in.data(), out.data(), nSamples) < 0) throw std::runtime_error(std::string("FX8010::processBlock: ") + fx_last_error(h_));
        return out;
    }

    int getInstructionCounter() { return (int)fx_instruction_counter(h_); }
    bool loadFile(const std::string& path) { return fx_load_file(h_, path.c_str()) == 1; }
    bool load(const std::string& path) { return loadFile(path); }  // alias (the reference's member is loadFile, include/FX8010.h:62)

    struct MyError {
        std::string errorDescription = "";
        int errorRow = 1;
    };
    std::vector<MyError> getErrorList() {
        std::vector<MyError> v;
        for (int i = 0, n = fx_error_count(h_); i < n; ++i) v.push_back({fx_error_desc(h_, i), fx_error_row(h_, i)});
        return v;
    }
    int setRegisterValue(const std::string& key, float value) { return fx_set_register(h_, key.c_str(), value); }
    float getRegisterValue(const std::string& key) { return fx_get_register(h_, key.c_str()); }
    std::vector<std::string> getControlRegisters() {
        std::vector<std::string> v;
        for (int i = 0, n = fx_control_count(h_); i < n; ++i) v.emplace_back(fx_control_at(h_, i));
        return v;
    }
    std::unordered_map<std::string, std::string> getMetaData() {
        std::unordered_map<std::string, std::string> m;
        static const char* const keys[] = {"name", "copyright", "created", "engine", "comment", "guid"};
        char buf[1024];
        for (const char* k : keys)
            if (fx_meta_get(h_, k, buf, (int)sizeof buf)) m[k] = buf;
        return m;
    }
    inline void setChannels(int numChannels_) { fx_set_channels(h_, numChannels_); }
    inline int getChannels() { return fx_get_channels(h_); }
    bool getReadyStatus() { return fx_ready(h_) != 0; }

private:
    int channels_;
    fx_handle* h_;
};

// N instances of one program on one GPU - or, with a device list / mask, spread over several GPUs of the node
// (contiguous instance ranges, one host thread + stream per device inside the library, no exchange between them).
// PCM layout: buf[(sample * channels + channel) * N + instance].
class FX8010Batch {
public:
    FX8010Batch(int64_t nInstances, int numChannels, int device = -1) : n_(nInstances), ch_(numChannels), h_(fxb_create(nInstances, numChannels, device)) {
        if (!h_) throw std::runtime_error(std::string("FX8010Batch: ") + fx_last_create_error());
    }
    // one shard per entry of `devices` (HIP ordinals; an ordinal may repeat)
    FX8010Batch(int64_t nInstances, int numChannels, const std::vector<int>& devices)
        : n_(nInstances), ch_(numChannels), h_(fxb_create_on_devices(nInstances, numChannels, devices.data(), (int)devices.size())) {
        if (!h_) throw std::runtime_error(std::string("FX8010Batch: ") + fx_last_create_error());
    }
    // one shard per set bit of deviceMask (bit d = HIP ordinal d): SURVEY.md section 8b's fxb_create(nInstances, ch, deviceMask)
    static FX8010Batch* sharded(int64_t nInstances, int numChannels, uint64_t deviceMask) {
        std::vector<int> devices;
        for (int d = 0; d < 64; ++d)
            if (deviceMask & (1ull << d)) devices.push_back(d);
        return new FX8010Batch(nInstances, numChannels, devices);
    }
    int shardCount() { return fxb_shard_count(h_); }
    // device-resident buffers of a sharded batch: dIn[k] / dOut[k] live on shard k's device, [nSamples][channels][instances of shard k]
    void processDeviceShards(const float* const* dIn, float* const* dOut, int nSamples) {
        if (fxb_process_block_dev_shards(h_, dIn, dOut, nSamples) < 0) throw std::runtime_error(std::string("FX8010Batch::processDeviceShards: ") + fxb_last_error(h_));
    }
    ~FX8010Batch() { fxb_destroy(h_); }
    FX8010Batch(const FX8010Batch&) = delete;
    FX8010Batch& operator=(const FX8010Batch&) = delete;

    bool loadFile(const std::string& path) { return fxb_load_file(h_, path.c_str()) == 1; }
    bool load(const std::string& path) { return loadFile(path); }
    bool loadText(const std::string& text) { return fxb_load_text(h_, text.c_str()) == 1; }
    int setRegisterValue(const std::string& key, float value) { return fxb_set_register(h_, key.c_str(), value); }
    int setRegisterValue(const std::string& key, int64_t instance, float value) { return fxb_set_register_i(h_, key.c_str(), instance, value); }
    float getRegisterValue(const std::string& key, int64_t instance) { return fxb_get_register_i(h_, key.c_str(), instance); }
    // one value per instance (values.size() == instances): per-instance control automation between blocks
    int setRegisterValues(const std::string& key, const std::vector<float>& values) { return fxb_set_register_array(h_, key.c_str(), values.data()); }
    // a schedule for the next process call: at its sample s, s % period == 0, the register takes values[s / period]
    // (perInstance: values[(s / period) * instances + instance]); the slider of source/main.cpp:107-114 without cutting the block
    int setRegisterTrack(const std::string& key, const std::vector<float>& values, int period, bool perInstance = false) {
        const int steps = (int)(perInstance ? values.size() / (size_t)n_ : values.size());
        return fxb_set_register_track(h_, key.c_str(), values.data(), steps, period, perInstance ? 1 : 0);
    }
    // nSamples sample periods for every instance (host buffers, synchronous)
    void process(const float* in, float* out, int nSamples) {
        if (fxb_process_block(h_, in, out, nSamples) < 0) throw std::runtime_error(std::string("FX8010Batch::process: ") + fxb_last_error(h_));
    }
    // a shared input (in: [nSamples][channels][busGroups(group)], instance n hears column n / group) and / or a mixed output
    // (out: the same shape, every group's sum in the order include/fx8010_amd.h fixes) per group of `group` instances; a side
    // whose flag is false is [nSamples][channels][instances] as in process().  Host buffers, synchronous.
    int64_t busGroups(int64_t group) { return fxb_bus_groups(h_, group); }
    void processBlockBus(const float* in, float* out, int nSamples, int64_t group, bool sharedIn = true, bool mixOut = true) {
        const unsigned flags = (sharedIn ? FXB_BUS_SHARED_IN : 0u) | (mixOut ? FXB_BUS_MIX_OUT : 0u);
        if (fxb_process_block_bus(h_, in, out, nSamples, group, flags) < 0) throw std::runtime_error(std::string("FX8010Batch::processBlockBus: ") + fxb_last_error(h_));
    }
    // bus taps (include/fx8010_amd.h "Bus taps"): the instances (global numbers, any order, repeats allowed, at most 65 536) whose own
    // output words, pre-fader, a tapped block delivers beside the mix; an empty list turns taps off.  processBlockBusTap is
    // processBlockBus with tapOut = [nSamples][channels][busTaps().size()]; it needs mixOut.
    void busSetTaps(const std::vector<int64_t>& instances) {
        if (fxb_bus_set_taps(h_, instances.empty() ? nullptr : instances.data(), (int64_t)instances.size()) < 0)
            throw std::runtime_error(std::string("FX8010Batch::busSetTaps: ") + fxb_last_error(h_));
    }
    std::vector<int64_t> busTaps() {
        const int64_t count = fxb_bus_get_taps(h_, nullptr, 0);
        if (count < 0) throw std::runtime_error(std::string("FX8010Batch::busTaps: ") + fxb_last_error(h_));
        std::vector<int64_t> list((size_t)count);
        if (count > 0) fxb_bus_get_taps(h_, list.data(), count);
        return list;
    }
    void processBlockBusTap(const float* in, float* out, float* tapOut, int nSamples, int64_t group, bool sharedIn = true, bool mixOut = true) {
        const unsigned flags = (sharedIn ? FXB_BUS_SHARED_IN : 0u) | (mixOut ? FXB_BUS_MIX_OUT : 0u);
        if (fxb_process_block_bus_tap(h_, in, out, tapOut, nSamples, group, flags) < 0)
            throw std::runtime_error(std::string("FX8010Batch::processBlockBusTap: ") + fxb_last_error(h_));
    }
    // bus sends (include/fx8010_amd.h "Bus sends"): aux buses by member list, CSR - bus b owns members[offsets[b] .. offsets[b+1]),
    // global instance numbers in any order, repeats allowed; gains is [channels][E] or empty for 1.0f everywhere; an offsets of
    // at most one value turns sends off.  busSetSendGains replaces the weights, with ramp over the next block that is given aux
    // rows.  processBlockBusAux is processBlockBusTap (tapOut may be nullptr) with auxOut = [nSamples][channels][A]: pre-fader
    // sums in the order the header fixes; it needs mixOut.
    void busSetSends(const std::vector<int64_t>& offsets, const std::vector<int64_t>& members, const std::vector<float>& gains = {}) {
        const int64_t buses = offsets.empty() ? 0 : (int64_t)offsets.size() - 1;
        if (fxb_bus_set_sends(h_, buses, offsets.empty() ? nullptr : offsets.data(), members.empty() ? nullptr : members.data(), gains.empty() ? nullptr : gains.data()) < 0)
            throw std::runtime_error(std::string("FX8010Batch::busSetSends: ") + fxb_last_error(h_));
    }
    void busSetSendGains(const std::vector<float>& gains, bool ramp = false) {
        if (fxb_bus_set_send_gains(h_, gains.data(), ramp ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::busSetSendGains: ") + fxb_last_error(h_));
    }
    struct BusSends { std::vector<int64_t> offsets, members; std::vector<float> gains; };   // gains: the ones in force ([channels][E])
    BusSends busSends(int channels) {
        int64_t buses = 0;
        const int64_t entries = fxb_bus_get_sends(h_, &buses, nullptr, 0, nullptr, nullptr, 0);
        if (entries < 0) throw std::runtime_error(std::string("FX8010Batch::busSends: ") + fxb_last_error(h_));
        BusSends s{std::vector<int64_t>((size_t)buses + 1, 0), std::vector<int64_t>((size_t)entries), std::vector<float>((size_t)channels * (size_t)entries)};
        if (buses > 0) fxb_bus_get_sends(h_, nullptr, s.offsets.data(), buses + 1, s.members.data(), s.gains.data(), entries);
        return s;
    }
    void processBlockBusAux(const float* in, float* out, float* tapOut, float* auxOut, int nSamples, int64_t group, bool sharedIn = true, bool mixOut = true) {
        const unsigned flags = (sharedIn ? FXB_BUS_SHARED_IN : 0u) | (mixOut ? FXB_BUS_MIX_OUT : 0u);
        if (fxb_process_block_bus_aux(h_, in, out, tapOut, auxOut, nSamples, group, flags) < 0)
            throw std::runtime_error(std::string("FX8010Batch::processBlockBusAux: ") + fxb_last_error(h_));
    }
    // bus feeds (include/fx8010_amd.h "Bus feeds"): per-instance input by source list, CSR by instance - instance n hears
    // sources[offsets[n] .. offsets[n+1]), columns of a source block [nSamples][channels][nSrc], in any order, repeats allowed;
    // gains is [channels][E] or empty for unweighted (one entry then moves its word as a bit pattern); nSrc == 0 turns feeds off.
    // setFeedGains replaces the weights, with ramp over the next feed block; an empty vector returns to unweighted.
    // processBlockBusFeed is processBlockBusAux (tapOut / auxOut may be nullptr) with src in the place of `in`; src may also be
    // device memory of the handle's device - the aux rows of another handle - and is then gathered where it lies.
    void setFeeds(int64_t nSrc, const std::vector<int64_t>& offsets, const std::vector<int64_t>& sources, const std::vector<float>& gains = {}) {
        if (fxb_bus_set_feeds(h_, nSrc, offsets.empty() ? nullptr : offsets.data(), sources.empty() ? nullptr : sources.data(), gains.empty() ? nullptr : gains.data()) < 0)
            throw std::runtime_error(std::string("FX8010Batch::setFeeds: ") + fxb_last_error(h_));
    }
    void setFeedGains(const std::vector<float>& gains, bool ramp = false) {
        if (fxb_bus_set_feed_gains(h_, gains.empty() ? nullptr : gains.data(), ramp ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::setFeedGains: ") + fxb_last_error(h_));
    }
    void processBlockBusFeed(const float* src, float* out, float* tapOut, float* auxOut, int nSamples, int64_t group = 1, bool mixOut = false) {
        if (fxb_process_block_bus_feed(h_, src, out, tapOut, auxOut, nSamples, group, mixOut ? FXB_BUS_MIX_OUT : 0u) < 0)
            throw std::runtime_error(std::string("FX8010Batch::processBlockBusFeed: ") + fxb_last_error(h_));
    }
    // per-instance gains of the mixed output (include/fx8010_amd.h "Bus gains"): gains is [channels][instances], every value finite,
    // or nullptr for gains off (the unweighted sum); with ramp the next mixing block moves every weight linearly from the gains in
    // force to these and ends exactly on them.  A gain of zero mutes: that instance adds +0.0f whatever it holds.  busGetGains
    // fills [channels][instances] with the gains in force and throws while gains are off.
    void busSetGains(const float* gains, bool ramp = false) {
        if (fxb_bus_set_gains(h_, gains, ramp ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::busSetGains: ") + fxb_last_error(h_));
    }
    void busGetGains(float* gains) {
        if (fxb_bus_get_gains(h_, gains) < 0) throw std::runtime_error(std::string("FX8010Batch::busGetGains: ") + fxb_last_error(h_));
    }
    // one interleaved stream per instance (include/fx8010_amd.h fxb_process_block_imajor): instance n's nSamples * channels floats,
    // [sample][channel], at in + n * inStride, its output the same way at out + n * outStride (strides in floats, 0 = packed; a
    // larger one walks a whole file or ring per instance in place).  Host buffers, synchronous; in == out with one stride is fine.
    void processStreams(const float* in, float* out, int nSamples, int64_t inStride = 0, int64_t outStride = 0) {
        if (fxb_process_block_imajor(h_, in, out, nSamples, inStride, outStride) < 0) throw std::runtime_error(std::string("FX8010Batch::processStreams: ") + fxb_last_error(h_));
    }
    // device-resident buffers, asynchronous on `stream` (hipStream_t)
    void processDevice(const float* dIn, float* dOut, int nSamples, void* stream = nullptr) {
        if (fxb_process_block_dev(h_, dIn, dOut, nSamples, stream) < 0) throw std::runtime_error(std::string("FX8010Batch::processDevice: ") + fxb_last_error(h_));
    }
    void sync() { fxb_sync(h_); }
    // Output meters (include/fx8010_amd.h "Output meters"): per instance and channel the energy, the peak, the samples at the +-1
    // rail and the non-finite ones, accumulated on the device over the blocks processed while metering is on.  meterRead fills
    // [channels][instances] arrays (a null pointer skips one) and, with reset, zeroes the meters afterwards.
    void meterEnable(bool on = true) {
        if (fxb_meter_enable(h_, on ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::meterEnable: ") + fxb_last_error(h_));
    }
    void meterRead(double* energy, float* peak, uint32_t* fullScale, uint32_t* nonfinite, bool reset = false) {
        if (fxb_meter_read(h_, energy, peak, fullScale, nonfinite, reset ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::meterRead: ") + fxb_last_error(h_));
    }
    int64_t meterSamples() {
        const int64_t s = fxb_meter_samples(h_);
        if (s < 0) throw std::runtime_error(std::string("FX8010Batch::meterSamples: ") + fxb_last_error(h_));
        return s;
    }
    // Meter queries by list (include/fx8010_amd.h "Meter queries by list"): meterSelect returns the global instances of first ..
    // first + nRange - 1 (nRange < 0: up to the last) whose meter `stat` (FXB_METER_ENERGY ...), the maximum over the channels, is
    // >= threshold - with FXB_METER_BELOW: < threshold - ascending, at most `cap` of them (cap < 0: all); *matches, when given,
    // gets their number M, which may exceed cap.  meterReadList fills [channels][list.size()] arrays (a null pointer skips one)
    // and, with reset, zeroes the listed columns.  Both are synchronous.  meterResetList is stream-ordered behind the queued
    // blocks (sync() covers it); meterSamples() is not changed by either.
    std::vector<int64_t> meterSelect(int stat, double threshold, unsigned flags = 0, int64_t first = 0, int64_t nRange = -1, int64_t cap = -1, int64_t* matches = nullptr) {
        if (nRange < 0) nRange = n_ - first;
        if (cap < 0) cap = nRange > 0 ? nRange : 0;
        std::vector<int64_t> list((size_t)(cap < nRange ? cap : (nRange > 0 ? nRange : 0)));
        const int64_t m = fxb_meter_select(h_, stat, threshold, first, nRange, list.empty() ? nullptr : list.data(), (int64_t)list.size(), flags);
        if (m < 0) throw std::runtime_error(std::string("FX8010Batch::meterSelect: ") + fxb_last_error(h_));
        if (matches) *matches = m;
        if ((size_t)m < list.size()) list.resize((size_t)m);
        return list;
    }
    void meterReadList(const std::vector<int64_t>& list, double* energy, float* peak, uint32_t* fullScale, uint32_t* nonfinite, bool reset = false) {
        if (fxb_meter_read_list(h_, list.data(), (int64_t)list.size(), energy, peak, fullScale, nonfinite, reset ? 1 : 0) < 0)
            throw std::runtime_error(std::string("FX8010Batch::meterReadList: ") + fxb_last_error(h_));
    }
    void meterResetList(const std::vector<int64_t>& list) {
        if (fxb_meter_reset_list(h_, list.data(), (int64_t)list.size()) < 0) throw std::runtime_error(std::string("FX8010Batch::meterResetList: ") + fxb_last_error(h_));
    }
    // Target meters (include/fx8010_amd.h "Target meters"): target is [nSamples][channels][ceil(N / group)]; while one is set the
    // meters also accumulate the squared error against it and the cross product with it.  meterReadMatch fills
    // [channels][instances] arrays; meterSelectMatch is meterSelect over the channel SUM of FXB_MATCH_ERROR / FXB_MATCH_CROSS;
    // meterBest fills [ceil(N / group)] winners and values (a null pointer skips one).
    void meterSetTarget(const float* target, int64_t nSamples, int64_t group = 1, unsigned flags = 0) {
        if (fxb_meter_set_target(h_, target, nSamples, group, flags) < 0) throw std::runtime_error(std::string("FX8010Batch::meterSetTarget: ") + fxb_last_error(h_));
    }
    void meterClearTarget() {
        if (fxb_meter_clear_target(h_) < 0) throw std::runtime_error(std::string("FX8010Batch::meterClearTarget: ") + fxb_last_error(h_));
    }
    void meterTargetSeek(int64_t pos) {
        if (fxb_meter_target_seek(h_, pos) < 0) throw std::runtime_error(std::string("FX8010Batch::meterTargetSeek: ") + fxb_last_error(h_));
    }
    int64_t meterTargetPos() {
        const int64_t p = fxb_meter_target_pos(h_);
        if (p < 0) throw std::runtime_error(std::string("FX8010Batch::meterTargetPos: ") + fxb_last_error(h_));
        return p;
    }
    void meterReadMatch(double* err, double* cross, bool reset = false) {
        if (fxb_meter_read_match(h_, err, cross, reset ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::meterReadMatch: ") + fxb_last_error(h_));
    }
    int64_t meterSelectMatch(int stat, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags = 0) {
        const int64_t m = fxb_meter_select_match(h_, stat, threshold, first, nRange, list, cap, flags);
        if (m < 0) throw std::runtime_error(std::string("FX8010Batch::meterSelectMatch: ") + fxb_last_error(h_));
        return m;
    }
    void meterBest(int stat, int64_t group, int64_t* winner, double* value, unsigned flags = 0) {
        if (fxb_meter_best(h_, stat, group, winner, value, flags) < 0) throw std::runtime_error(std::string("FX8010Batch::meterBest: ") + fxb_last_error(h_));
    }
    // Level meters (include/fx8010_amd.h "Level meters"): an envelope with instant attack and exponential release and the count of
    // consecutive samples below `floor`, per channel and instance.  meterReadLevel fills [channels][instances] arrays,
    // meterReadLevelList [channels][list.size()]; meterSelectLevel is meterSelect over the channel maximum of FXB_LEVEL_ENVELOPE or
    // the channel minimum of FXB_LEVEL_QUIET.
    void meterSetLevel(float release, float floor = 0.0f) {
        if (fxb_meter_set_level(h_, release, floor, 0) < 0) throw std::runtime_error(std::string("FX8010Batch::meterSetLevel: ") + fxb_last_error(h_));
    }
    void meterClearLevel() {
        if (fxb_meter_clear_level(h_) < 0) throw std::runtime_error(std::string("FX8010Batch::meterClearLevel: ") + fxb_last_error(h_));
    }
    void meterReadLevel(float* level, uint32_t* quiet, bool reset = false) {
        if (fxb_meter_read_level(h_, level, quiet, reset ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::meterReadLevel: ") + fxb_last_error(h_));
    }
    void meterReadLevelList(const std::vector<int64_t>& list, float* level, uint32_t* quiet, bool reset = false) {
        if (fxb_meter_read_level_list(h_, list.data(), (int64_t)list.size(), level, quiet, reset ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::meterReadLevelList: ") + fxb_last_error(h_));
    }
    int64_t meterSelectLevel(int stat, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags = 0) {
        const int64_t m = fxb_meter_select_level(h_, stat, threshold, first, nRange, list, cap, flags);
        if (m < 0) throw std::runtime_error(std::string("FX8010Batch::meterSelectLevel: ") + fxb_last_error(h_));
        return m;
    }
    // Meter ranks (include/fx8010_amd.h "Meter ranks"): the first min(M, k) candidates of first .. first + nRange - 1 under the order
    // (V, n) - V descending with FXB_METER_LARGEST, ties to the smaller instance number - into list (and their V into value, which
    // may be null), in rank order; returns M.  meterRank over the four accumulators, meterRankMatch over the match rows of a target,
    // meterRankLevel over the level rows.
    int64_t meterRank(int stat, int64_t k, double threshold, int64_t first, int64_t nRange, int64_t* list, double* value, unsigned flags = 0) {
        const int64_t m = fxb_meter_rank(h_, stat, k, threshold, first, nRange, list, value, flags);
        if (m < 0) throw std::runtime_error(std::string("FX8010Batch::meterRank: ") + fxb_last_error(h_));
        return m;
    }
    int64_t meterRankMatch(int stat, int64_t k, double threshold, int64_t first, int64_t nRange, int64_t* list, double* value, unsigned flags = 0) {
        const int64_t m = fxb_meter_rank_match(h_, stat, k, threshold, first, nRange, list, value, flags);
        if (m < 0) throw std::runtime_error(std::string("FX8010Batch::meterRankMatch: ") + fxb_last_error(h_));
        return m;
    }
    int64_t meterRankLevel(int stat, int64_t k, double threshold, int64_t first, int64_t nRange, int64_t* list, double* value, unsigned flags = 0) {
        const int64_t m = fxb_meter_rank_level(h_, stat, k, threshold, first, nRange, list, value, flags);
        if (m < 0) throw std::runtime_error(std::string("FX8010Batch::meterRankLevel: ") + fxb_last_error(h_));
        return m;
    }
    // Tone meters (include/fx8010_amd.h "Tone meters"): a Goertzel recurrence per probe frequency, channel and instance; each
    // coefficient is c = 2 cos(2 pi f / fs).  meterReadTones fills [tones][channels][instances] arrays of doubles (any may be
    // null), meterReadTonesList [tones][channels][list.size()]; meterSelectTone / meterRankTone are meterSelect / fxb_meter_rank
    // over the channel maximum of the power at `tone`.
    void meterSetTones(const std::vector<double>& coeff) {
        if (fxb_meter_set_tones(h_, (int)coeff.size(), coeff.data(), 0) < 0) throw std::runtime_error(std::string("FX8010Batch::meterSetTones: ") + fxb_last_error(h_));
    }
    std::vector<double> meterGetTones() {
        int n = 0;
        std::vector<double> coeff(FXB_METER_MAX_TONES);
        if (fxb_meter_get_tones(h_, &n, coeff.data()) < 0) throw std::runtime_error(std::string("FX8010Batch::meterGetTones: ") + fxb_last_error(h_));
        coeff.resize((size_t)n);
        return coeff;
    }
    void meterClearTones() {
        if (fxb_meter_clear_tones(h_) < 0) throw std::runtime_error(std::string("FX8010Batch::meterClearTones: ") + fxb_last_error(h_));
    }
    void meterReadTones(double* s1, double* s2, double* power, bool reset = false) {
        if (fxb_meter_read_tones(h_, s1, s2, power, reset ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::meterReadTones: ") + fxb_last_error(h_));
    }
    void meterReadTonesList(const std::vector<int64_t>& list, double* s1, double* s2, double* power, bool reset = false) {
        if (fxb_meter_read_tones_list(h_, list.data(), (int64_t)list.size(), s1, s2, power, reset ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::meterReadTonesList: ") + fxb_last_error(h_));
    }
    int64_t meterSelectTone(int tone, double threshold, int64_t first, int64_t nRange, int64_t* list, int64_t cap, unsigned flags = 0) {
        const int64_t m = fxb_meter_select_tone(h_, tone, threshold, first, nRange, list, cap, flags);
        if (m < 0) throw std::runtime_error(std::string("FX8010Batch::meterSelectTone: ") + fxb_last_error(h_));
        return m;
    }
    int64_t meterRankTone(int tone, int64_t k, double threshold, int64_t first, int64_t nRange, int64_t* list, double* value, unsigned flags = 0) {
        const int64_t m = fxb_meter_rank_tone(h_, tone, k, threshold, first, nRange, list, value, flags);
        if (m < 0) throw std::runtime_error(std::string("FX8010Batch::meterRankTone: ") + fxb_last_error(h_));
        return m;
    }
    // Per-instance state by list (include/fx8010_amd.h "Per-instance state"): dst[k] becomes a copy of src[k]; the listed instances
    // become fresh ones (registers as last broadcast, delay memory cleared, delay-line positions kept); their records to an image
    // of fxb_instance_image_size bytes and back into any batch with the same program that has run as many samples.  Copy and
    // reset are stream-ordered (sync() covers them), save and load synchronous.
    void copyInstances(const std::vector<int64_t>& src, const std::vector<int64_t>& dst) {
        if (src.size() != dst.size()) throw std::runtime_error("FX8010Batch::copyInstances: lists of different length");
        if (fxb_copy_instances(h_, src.data(), dst.data(), (int64_t)src.size()) < 0) throw std::runtime_error(std::string("FX8010Batch::copyInstances: ") + fxb_last_error(h_));
    }
    // Registers by list (include/fx8010_amd.h "Register sets by list"): values[k * list.size() + i] is register keys[k] of instance
    // list[i].  The set leaves the batch as one setRegisterValue per word would and is stream-ordered behind the queued blocks
    // (sync() covers it); the get is synchronous.  Both throw when a key is no register.
    void setRegistersList(const std::vector<std::string>& keys, const std::vector<int64_t>& list, const std::vector<float>& values) {
        if (values.size() != keys.size() * list.size()) throw std::runtime_error("FX8010Batch::setRegistersList: values must hold keys x list words");
        std::vector<const char*> names;
        for (const std::string& k : keys) names.push_back(k.c_str());
        if (fxb_set_registers_list(h_, names.data(), (int)names.size(), list.data(), (int64_t)list.size(), values.data()) != 0)
            throw std::runtime_error(std::string("FX8010Batch::setRegistersList: ") + fxb_last_error(h_));
    }
    // Register tracks by list (include/fx8010_amd.h "Register tracks by list"): arms one list schedule for the next process call.
    // values[(q * keys.size() + k) * list.size() + i] is what register keys[k] of instance list[i] takes at sample
    // first + q * period; the number of steps follows from values.size().  The other voices keep what they hold.
    void setRegisterTracksList(const std::vector<std::string>& keys, const std::vector<int64_t>& list, const std::vector<float>& values, int first = 0, int period = 1) {
        const size_t perStep = keys.size() * list.size();
        if (perStep == 0 || values.empty() || values.size() % perStep != 0) throw std::runtime_error("FX8010Batch::setRegisterTracksList: values must hold steps x keys x list words");
        std::vector<const char*> names;
        for (const std::string& k : keys) names.push_back(k.c_str());
        if (fxb_set_register_tracks_list(h_, names.data(), (int)names.size(), list.data(), (int64_t)list.size(), values.data(), (int)(values.size() / perStep), first, period) != 0)
            throw std::runtime_error(std::string("FX8010Batch::setRegisterTracksList: ") + fxb_last_error(h_));
    }
    void clearRegisterTracksList() { fxb_clear_register_tracks_list(h_); }
    std::vector<float> getRegistersList(const std::vector<std::string>& keys, const std::vector<int64_t>& list) {
        std::vector<const char*> names;
        for (const std::string& k : keys) names.push_back(k.c_str());
        std::vector<float> values(keys.size() * list.size());
        if (fxb_get_registers_list(h_, names.data(), (int)names.size(), list.data(), (int64_t)list.size(), values.data()) != 0)
            throw std::runtime_error(std::string("FX8010Batch::getRegistersList: ") + fxb_last_error(h_));
        return values;
    }
    // Delay-line windows by list (include/fx8010_amd.h "Delay-line windows by list"): values[i * nWords + j] is word first + j of
    // delay line `which` (0 iTRAM, 1 xTRAM) of instance list[i]; flags: FXB_TRAM_LOGICAL (the index is the age in the ring),
    // FXB_TRAM_BROADCAST (set only: values is one window of nWords for every listed instance).  The set is stream-ordered behind
    // the queued blocks (sync() covers it); the get is synchronous.
    void setTramList(int which, const std::vector<int64_t>& list, int first, int nWords, const std::vector<float>& values, unsigned flags = 0) {
        const size_t windows = (flags & FXB_TRAM_BROADCAST) ? 1 : list.size();
        if (nWords < 0 || values.size() != windows * (size_t)nWords) throw std::runtime_error("FX8010Batch::setTramList: values must hold one window of nWords per listed instance (one in all with FXB_TRAM_BROADCAST)");
        if (fxb_set_tram_list(h_, which, list.data(), (int64_t)list.size(), first, nWords, values.data(), flags) != 0)
            throw std::runtime_error(std::string("FX8010Batch::setTramList: ") + fxb_last_error(h_));
    }
    std::vector<float> getTramList(int which, const std::vector<int64_t>& list, int first, int nWords, unsigned flags = 0) {
        std::vector<float> values(list.size() * (size_t)(nWords > 0 ? nWords : 0));
        if (fxb_get_tram_list(h_, which, list.data(), (int64_t)list.size(), first, nWords, values.data(), flags) != 0)
            throw std::runtime_error(std::string("FX8010Batch::getTramList: ") + fxb_last_error(h_));
        return values;
    }
    void resetInstances(const std::vector<int64_t>& list) {
        if (fxb_reset_instances(h_, list.data(), (int64_t)list.size()) < 0) throw std::runtime_error(std::string("FX8010Batch::resetInstances: ") + fxb_last_error(h_));
    }
    std::vector<uint8_t> saveInstances(const std::vector<int64_t>& list) {
        const int64_t bytes = fxb_instance_image_size(h_, (int64_t)list.size());
        if (bytes < 0) throw std::runtime_error(std::string("FX8010Batch::saveInstances: ") + fxb_last_error(h_));
        std::vector<uint8_t> image((size_t)bytes);
        if (fxb_save_instances(h_, list.data(), (int64_t)list.size(), image.data(), bytes) < 0) throw std::runtime_error(std::string("FX8010Batch::saveInstances: ") + fxb_last_error(h_));
        return image;
    }
    void loadInstances(const std::vector<int64_t>& list, const std::vector<uint8_t>& image) {
        if (fxb_load_instances(h_, list.data(), (int64_t)list.size(), image.data(), (int64_t)image.size()) < 0) throw std::runtime_error(std::string("FX8010Batch::loadInstances: ") + fxb_last_error(h_));
    }
    // ... at any delay-line position: the delay memory of every record is rotated to its destination's positions (fxb_load_instances_rotated)
    void loadInstancesRotated(const std::vector<int64_t>& list, const std::vector<uint8_t>& image) {
        if (fxb_load_instances_rotated(h_, list.data(), (int64_t)list.size(), image.data(), (int64_t)image.size()) < 0) throw std::runtime_error(std::string("FX8010Batch::loadInstancesRotated: ") + fxb_last_error(h_));
    }
    // the record bank (include/fx8010_amd.h "Record banks"): instance records kept on the GPU; store and recall are queued behind the
    // blocks, the rotations of a recall are worked out on the device, what it refuses shows in bankStatus
    void bankCreate(int64_t nSlots) {
        if (fxb_bank_create(h_, nSlots) < 0) throw std::runtime_error(std::string("FX8010Batch::bankCreate: ") + fxb_last_error(h_));
    }
    int64_t bankSlots() const { return fxb_bank_slots(h_); }
    void bankStore(const std::vector<int64_t>& slots, const std::vector<int64_t>& list) {
        if (slots.size() != list.size()) throw std::invalid_argument("FX8010Batch::bankStore: slots and list must have the same length");
        if (fxb_bank_store(h_, slots.data(), list.data(), (int64_t)list.size()) < 0) throw std::runtime_error(std::string("FX8010Batch::bankStore: ") + fxb_last_error(h_));
    }
    void bankRecall(const std::vector<int64_t>& slots, const std::vector<int64_t>& list) {
        if (slots.size() != list.size()) throw std::invalid_argument("FX8010Batch::bankRecall: slots and list must have the same length");
        if (fxb_bank_recall(h_, slots.data(), list.data(), (int64_t)list.size()) < 0) throw std::runtime_error(std::string("FX8010Batch::bankRecall: ") + fxb_last_error(h_));
    }
    void bankPut(const std::vector<int64_t>& slots, const std::vector<uint8_t>& image) {
        if (fxb_bank_put(h_, slots.data(), (int64_t)slots.size(), image.data(), (int64_t)image.size()) < 0) throw std::runtime_error(std::string("FX8010Batch::bankPut: ") + fxb_last_error(h_));
    }
    std::vector<uint8_t> bankGet(const std::vector<int64_t>& slots) {
        const int64_t bytes = fxb_instance_image_size(h_, (int64_t)slots.size());
        if (bytes < 0) throw std::runtime_error(std::string("FX8010Batch::bankGet: ") + fxb_last_error(h_));
        std::vector<uint8_t> image((size_t)bytes);
        if (fxb_bank_get(h_, slots.data(), (int64_t)slots.size(), image.data(), bytes) < 0) throw std::runtime_error(std::string("FX8010Batch::bankGet: ") + fxb_last_error(h_));
        return image;
    }
    struct BankStatus { int64_t refusedCalls = 0, entry = -1; int reason = 0; };   // reason: FXB_BANK_*
    BankStatus bankStatus(bool reset = false) {
        BankStatus s;
        if (fxb_bank_status(h_, &s.refusedCalls, &s.entry, &s.reason, reset ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::bankStatus: ") + fxb_last_error(h_));
        return s;
    }
    // generate the code for blocks of nSamples samples now, not in the first process call (callers with a deadline per block)
    void prepare(int nSamples, bool wait = true) {
        if (fxb_prepare(h_, nSamples, wait ? 1 : 0) < 0) throw std::runtime_error(std::string("FX8010Batch::prepare: ") + fxb_last_error(h_));
    }
    // the whole batch's DSP state (the reference: plain members, include/FX8010.h:162-217, 288-291) as one image, laid out by global
    // instance: it loads into any batch of the same size with the same program, whatever its partition into shards
    std::vector<unsigned char> saveState() {
        const int64_t bytes = fxb_state_size(h_);
        if (bytes < 0) throw std::runtime_error(std::string("FX8010Batch::saveState: ") + fxb_last_error(h_));
        std::vector<unsigned char> image((size_t)bytes);
        if (fxb_save_state(h_, image.data(), bytes) < 0) throw std::runtime_error(std::string("FX8010Batch::saveState: ") + fxb_last_error(h_));
        return image;
    }
    void loadState(const std::vector<unsigned char>& image) {
        if (fxb_load_state(h_, image.data(), (int64_t)image.size()) < 0) throw std::runtime_error(std::string("FX8010Batch::loadState: ") + fxb_last_error(h_));
    }
    int64_t getInstructionCounter() { return fxb_instruction_counter(h_); }
    int64_t getInstructionCounter(int64_t instance) { return fxb_instruction_counter_i(h_, instance); }
    float lastKernelMs() { return fxb_last_kernel_ms(h_); }
    // which tier runs the program as it stands, and why not a faster one (text for the host's log)
    std::string tierNote() {
        char buf[512] = {0};
        fxb_tier_note(h_, buf, (int)sizeof buf);
        return buf;
    }
    int64_t instances() const { return n_; }
    int channels() const { return ch_; }
    fxb_handle* handle() { return h_; }

    // A PCM buffer [nSamples][channels][instances] in pinned host memory (fxb_host_alloc): process() on such buffers runs in place -
    // no staging copies - which is what a host with a deadline per block wants.  Owns its memory; movable, not copyable.
    class PcmBuffer {
    public:
        PcmBuffer() = default;
        PcmBuffer(int64_t instances, int channels, int nSamples)
            : floats_((size_t)instances * (size_t)channels * (size_t)nSamples), p_(static_cast<float*>(fxb_host_alloc((int64_t)floats_ * 4))) {
            if (!p_) throw std::runtime_error(std::string("FX8010Batch::PcmBuffer: ") + fx_last_create_error());
        }
        ~PcmBuffer() { fxb_host_free(p_); }
        PcmBuffer(PcmBuffer&& o) noexcept : floats_(o.floats_), p_(o.p_) { o.p_ = nullptr; o.floats_ = 0; }
        PcmBuffer& operator=(PcmBuffer&& o) noexcept { if (this != &o) { fxb_host_free(p_); p_ = o.p_; floats_ = o.floats_; o.p_ = nullptr; o.floats_ = 0; } return *this; }
        PcmBuffer(const PcmBuffer&) = delete;
        PcmBuffer& operator=(const PcmBuffer&) = delete;
        float* data() { return p_; }
        const float* data() const { return p_; }
        size_t size() const { return floats_; }
    private:
        size_t floats_ = 0;
        float* p_ = nullptr;
    };
    PcmBuffer pcmBuffer(int nSamples) const { return PcmBuffer(n_, ch_, nSamples); }

private:
    int64_t n_;
    int ch_;
    fxb_handle* h_;
};

}  // namespace Klangraum

#endif
