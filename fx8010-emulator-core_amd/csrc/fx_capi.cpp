// fx_capi.cpp — extern "C" surface declared in include/fx8010_amd.h.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>
#include <string>

#include "../../include/fx8010_amd.h"
#include <vector>

#include "fx_batch.hpp"
#include "fx_knobs.hpp"
#include "fx_shard.hpp"
#include "fx_xlate.hpp"

// a batch is one shard (fxb_create) or several (fxb_create_sharded / fxb_create_on_devices)
struct fxb_handle {
    fx::Sharded batch;
    fxb_handle(int64_t n, int ch, const std::vector<int>& devices) : batch(n, ch, devices) {}
};
struct fx_handle {
    fx::Batch batch;
    explicit fx_handle(int ch) : batch(1, ch, -1) {}
};

struct fxp_handle {
    fx::Program prog;
    fx::Lowered low;
    bool lowered = false;
    std::string err;
    std::vector<int> tracked;  // registers fxp_translate treats as trackable (fxp_track_register)
    explicit fxp_handle(int ch) : prog(ch) {}
    void noteError(const std::string& what) { err = what; }
};

namespace {
thread_local std::string g_createError;

template <class H, class... A>
H* create(A... args) {
    try {
        g_createError.clear();
        return new H(args...);
    } catch (const std::exception& e) {
        g_createError = e.what();
    } catch (...) {
        g_createError = "unknown error";
    }
    return nullptr;
}

int errorCount(fx::Batch& b) { return (int)b.program().errors.size(); }
const char* errorDesc(fx::Batch& b, int i) {
    const auto& e = b.program().errors;
    return (i < 0 || i >= (int)e.size()) ? "" : e[i].description.c_str();
}
int errorRow(fx::Batch& b, int i) {
    const auto& e = b.program().errors;
    return (i < 0 || i >= (int)e.size()) ? -1 : e[i].row;
}
int controlCount(fx::Batch& b) { return (int)b.program().controls.size(); }
const char* controlAt(fx::Batch& b, int i) {
    const auto& c = b.program().controls;
    return (i < 0 || i >= (int)c.size()) ? "" : c[i].c_str();
}
int metaGet(fx::Batch& b, const char* key, char* buf, int buflen) {
    if (!key) return 0;
    for (const auto& kv : b.program().meta)
        if (kv.first == key) {
            if (buf && buflen > 0) std::snprintf(buf, (size_t)buflen, "%s", kv.second.c_str());
            return 1;
        }
    return 0;
}


// No exception may cross the C boundary (the caller may be C, ctypes or a DAW host): every entry point runs its body
// through one of these; the message lands where fx*_last_error() finds it.
int codeOf(const std::exception& e) { return dynamic_cast<const std::bad_alloc*>(&e) ? FX_E_MEMORY : FX_E_PROGRAM; }
template <class H, class F>
auto guard(H* h, decltype(std::declval<F>()()) onError, F f) -> decltype(f()) {
    try {
        return f();
    } catch (const std::exception& e) {
        if (h) h->noteError(e.what());
    } catch (...) {
        if (h) h->noteError("unknown error");
    }
    return onError;
}
template <class H, class F>
int guardCode(H* h, F f) {
    try {
        return f();
    } catch (const std::exception& e) {
        if (h) h->noteError(e.what());
        return codeOf(e);
    } catch (...) {
        if (h) h->noteError("unknown error");
        return FX_E_PROGRAM;
    }
}
}  // namespace

extern "C" {

const char* fx_last_create_error(void) { return g_createError.c_str(); }
const char* fxb_version(void) { return "fx8010_amd 0.1 (gfx950)"; }
int fxb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* ---- single instance ---- */
fx_handle* fx_create(int num_channels) { return create<fx_handle>(num_channels); }
void fx_destroy(fx_handle* h) { delete h; }
int fx_load_file(fx_handle* h, const char* path) { return (h && path) ? guard(&h->batch, 0, [&] { return h->batch.loadFile(path) ? 1 : 0; }) : 0; }
int fx_process(fx_handle* h, const float* in, float* out) { return h ? guardCode(&h->batch, [&] { return h->batch.processHost(in, out, 1); }) : FX_E_ARG; }
int fx_process_block(fx_handle* h, const float* in, float* out, int n) { return h ? guardCode(&h->batch, [&] { return h->batch.processHost(in, out, n); }) : FX_E_ARG; }
int fx_set_register(fx_handle* h, const char* key, float v) { return (h && key) ? guardCode(&h->batch, [&] { return h->batch.setRegister(key, v); }) : 1; }
float fx_get_register(fx_handle* h, const char* key) { return (h && key) ? guard(&h->batch, 1.0f, [&] { return h->batch.getRegisterAt(key, 0); }) : 1.0f; }
int64_t fx_instruction_counter(fx_handle* h) { return h ? guard(&h->batch, (int64_t)0, [&] { return h->batch.instructionCounterAt(0); }) : 0; }
int fx_error_count(fx_handle* h) { return h ? errorCount(h->batch) : 0; }
const char* fx_error_desc(fx_handle* h, int i) { return h ? errorDesc(h->batch, i) : ""; }
int fx_error_row(fx_handle* h, int i) { return h ? errorRow(h->batch, i) : -1; }
int fx_control_count(fx_handle* h) { return h ? controlCount(h->batch) : 0; }
const char* fx_control_at(fx_handle* h, int i) { return h ? controlAt(h->batch, i) : ""; }
int fx_meta_get(fx_handle* h, const char* key, char* buf, int buflen) { return h ? guard(&h->batch, 0, [&] { return metaGet(h->batch, key, buf, buflen); }) : 0; }
void fx_set_channels(fx_handle* h, int c) { if (h) h->batch.setChannels(c); }
int fx_set_option(fx_handle* h, unsigned option, int on) { return h ? h->batch.setOption(option, on != 0) : FX_E_ARG; }
int fx_get_channels(fx_handle* h) { return h ? h->batch.loaderChannels() : 0; }
int fx_ready(fx_handle* h) { return (h && h->batch.program().ready) ? 1 : 0; }
const char* fx_last_error(fx_handle* h) { return h ? h->batch.lastError().c_str() : "null handle"; }

#ifdef FX_DIAGNOSTICS
/* ---- diagnostics build only (fx_diag.h) ---- */
extern "C" int fxb_diag_build(void) { return 1; }
extern "C" int fxb_diag_read_end_stamps(void* handle, uint32_t* out, int64_t n_words) {
    fxb_handle* h = static_cast<fxb_handle*>(handle);
    if (!h || h->batch.shards() != 1) return FX_E_ARG;
    return guard(&h->batch.front(), FX_E_PROGRAM, [&] { return h->batch.front().readEndStamps(out, n_words); });
}
#endif

/* ---- batch ---- */
fxb_handle* fxb_create(int64_t n, int ch, int device) { return create<fxb_handle>(n, ch, std::vector<int>{device}); }
fxb_handle* fxb_create_on_devices(int64_t n, int ch, const int* devices, int n_devices) {
    if (!devices || n_devices < 1) { g_createError = "no device given"; return nullptr; }
    return create<fxb_handle>(n, ch, std::vector<int>(devices, devices + n_devices));
}
fxb_handle* fxb_create_sharded(int64_t n, int ch, uint64_t device_mask) {
    std::vector<int> devices;
    for (int d = 0; d < 64; ++d)
        if (device_mask & (1ull << d)) devices.push_back(d);
    if (devices.empty()) { g_createError = "empty device mask"; return nullptr; }
    return create<fxb_handle>(n, ch, devices);
}
int fxb_shard_count(fxb_handle* h) { return h ? h->batch.shards() : 0; }
int fxb_shard_info(fxb_handle* h, int shard, int* device, int64_t* first_instance, int64_t* n_instances) {
    if (!h || shard < 0 || shard >= h->batch.shards()) return FX_E_ARG;
    if (device) *device = h->batch.deviceOf(shard);
    if (first_instance) *first_instance = h->batch.firstOf(shard);
    if (n_instances) *n_instances = h->batch.countOf(shard);
    return 0;
}
float fxb_shard_kernel_ms(fxb_handle* h, int shard) {
    if (!h || shard < 0 || shard >= h->batch.shards()) return -1.0f;
    return guard(&h->batch.front(), -1.0f, [&] { return h->batch.lastKernelMsOf(shard); });
}
int fxb_shard_plan(int64_t n, int n_shards, int64_t* first_instance, int64_t* n_instances_out) {
    if (n_shards < 1 || !first_instance || !n_instances_out) return FX_E_ARG;
    try {
        const auto ranges = fx::Sharded::plan(n, n_shards);
        for (int k = 0; k < n_shards; ++k) { first_instance[k] = ranges[(size_t)k].first; n_instances_out[k] = ranges[(size_t)k].second; }
        return 0;
    } catch (...) {
        return FX_E_ARG;
    }
}
void fxb_destroy(fxb_handle* h) { delete h; }
int fxb_set_option(fxb_handle* h, unsigned option, int on) { return h ? h->batch.setOption(option, on != 0) : FX_E_ARG; }
int fxb_load_file(fxb_handle* h, const char* path) { return (h && path) ? guard(&h->batch.front(), 0, [&] { return h->batch.loadFile(path) ? 1 : 0; }) : 0; }
int fxb_load_text(fxb_handle* h, const char* text) { return (h && text) ? guard(&h->batch.front(), 0, [&] { return h->batch.loadText(text) ? 1 : 0; }) : 0; }
int fxb_set_register(fxb_handle* h, const char* key, float v) { return (h && key) ? guardCode(&h->batch.front(), [&] { return h->batch.setRegister(key, v); }) : 1; }
int fxb_set_register_i(fxb_handle* h, const char* key, int64_t inst, float v) { return (h && key) ? guardCode(&h->batch.front(), [&] { return h->batch.setRegisterAt(key, inst, v); }) : 1; }
float fxb_get_register_i(fxb_handle* h, const char* key, int64_t inst) { return (h && key) ? guard(&h->batch.front(), 1.0f, [&] { return h->batch.getRegisterAt(key, inst); }) : 1.0f; }
int fxb_set_register_array(fxb_handle* h, const char* key, const float* values) { return (h && key) ? guardCode(&h->batch.front(), [&] { return h->batch.setRegisterArray(key, values); }) : 1; }
int fxb_get_register_array(fxb_handle* h, const char* key, float* values) { return (h && key) ? guardCode(&h->batch.front(), [&] { return h->batch.getRegisterArray(key, values); }) : 1; }
int fxb_set_register_track(fxb_handle* h, const char* key, const float* values, int n_steps, int period, int per_instance) {
    return (h && key) ? guardCode(&h->batch.front(), [&] { return h->batch.setRegisterTrack(key, values, n_steps, period, per_instance != 0); }) : 1;
}
int fxb_seed_noise_i(fxb_handle* h, int64_t inst, int32_t x1, int32_t x2) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.seedNoiseAt(inst, x1, x2); }) : FX_E_ARG; }
void* fxb_host_alloc(int64_t bytes) {
    if (bytes <= 0) { g_createError = "fxb_host_alloc: bytes must be positive"; return nullptr; }
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, (size_t)bytes, hipHostMallocPortable);   // (one buffer for every shard's device)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g_createError = std::string("fxb_host_alloc: ") + hipGetErrorString(e);
        return nullptr;
    }
    return p;
}
void fxb_host_free(void* p) {
    if (p && hipHostFree(p) != hipSuccess) (void)hipGetLastError();
}
int fxb_process_block(fxb_handle* h, const float* in, float* out, int n) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.processHost(in, out, n); }) : FX_E_ARG; }
int fxb_process_block_dev(fxb_handle* h, const float* d_in, float* d_out, int n, void* stream) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processDevice(d_in, d_out, n, static_cast<hipStream_t>(stream)); }) : FX_E_ARG;
}
int fxb_process_block_pitched(fxb_handle* h, const float* in, float* out, int n, int64_t pitch) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processHost(in, out, n, pitch > 0 ? pitch : -1); }) : FX_E_ARG;
}
int fxb_process_block_dev_pitched(fxb_handle* h, const float* d_in, float* d_out, int n, int64_t pitch, void* stream) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processDevicePitched(d_in, d_out, n, pitch, static_cast<hipStream_t>(stream)); }) : FX_E_ARG;
}
int fxb_process_block_dev_shards(fxb_handle* h, const float* const* d_in, float* const* d_out, int n) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processDeviceShards(d_in, d_out, n); }) : FX_E_ARG;
}
int64_t fxb_bus_groups(fxb_handle* h, int64_t group) { 
    if (!h || group < 1) return FX_E_ARG;
    const int64_t n = h->batch.instances(), k = std::min(group, n);   // (a larger group is the one group of everything; no overflow)
    return (n + k - 1) / k;
}
int fxb_process_block_bus(fxb_handle* h, const float* in, float* out, int n, int64_t group, unsigned flags) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processBus(in, out, n, group, flags, false, nullptr); }) : FX_E_ARG;
}
int fxb_process_block_bus_dev(fxb_handle* h, const float* d_in, float* d_out, int n, int64_t group, unsigned flags, void* stream) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processBus(d_in, d_out, n, group, flags, true, static_cast<hipStream_t>(stream)); }) : FX_E_ARG;
}
int fxb_process_block_bus_tap(fxb_handle* h, const float* in, float* out, float* tap_out, int n, int64_t group, unsigned flags) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processBus(in, out, n, group, flags, false, nullptr, tap_out); }) : FX_E_ARG;
}
int fxb_process_block_bus_tap_dev(fxb_handle* h, const float* d_in, float* d_out, float* d_tap_out, int n, int64_t group, unsigned flags, void* stream) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processBus(d_in, d_out, n, group, flags, true, static_cast<hipStream_t>(stream), d_tap_out); }) : FX_E_ARG;
}
int fxb_bus_set_taps(fxb_handle* h, const int64_t* list, int64_t count) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.busSetTaps(list, count); }) : FX_E_ARG; }
int64_t fxb_bus_get_taps(fxb_handle* h, int64_t* list, int64_t cap) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.busGetTaps(list, cap); }) : (int64_t)FX_E_ARG;
}
int fxb_process_block_bus_aux(fxb_handle* h, const float* in, float* out, float* tap_out, float* aux_out, int n, int64_t group, unsigned flags) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processBus(in, out, n, group, flags, false, nullptr, tap_out, aux_out); }) : FX_E_ARG;
}
int fxb_process_block_bus_aux_dev(fxb_handle* h, const float* d_in, float* d_out, float* d_tap_out, float* d_aux_out, int n, int64_t group, unsigned flags, void* stream) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processBus(d_in, d_out, n, group, flags, true, static_cast<hipStream_t>(stream), d_tap_out, d_aux_out); }) : FX_E_ARG;
}
int fxb_process_block_bus_feed(fxb_handle* h, const float* src, float* out, float* tap_out, float* aux_out, int n, int64_t group, unsigned flags) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processBus(src, out, n, group, flags, false, nullptr, tap_out, aux_out, true); }) : FX_E_ARG;
}
int fxb_process_block_bus_feed_dev(fxb_handle* h, const float* d_src, float* d_out, float* d_tap_out, float* d_aux_out, int n, int64_t group, unsigned flags, void* stream) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processBus(d_src, d_out, n, group, flags, true, static_cast<hipStream_t>(stream), d_tap_out, d_aux_out, true); }) : FX_E_ARG;
}
int fxb_bus_set_feeds(fxb_handle* h, int64_t n_src, const int64_t* offsets, const int64_t* sources, const float* gains) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.busSetFeeds(n_src, offsets, sources, gains); }) : FX_E_ARG;
}
int fxb_bus_set_feed_gains(fxb_handle* h, const float* gains, int ramp) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.busSetFeedGains(gains, ramp); }) : FX_E_ARG; }
int64_t fxb_bus_get_feeds(fxb_handle* h, int64_t* n_src, int64_t* offsets, int64_t off_cap, int64_t* sources, float* gains, int64_t cap) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.busGetFeeds(n_src, offsets, off_cap, sources, gains, cap); }) : (int64_t)FX_E_ARG;
}
int fxb_bus_set_sends(fxb_handle* h, int64_t n_aux, const int64_t* offsets, const int64_t* members, const float* gains) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.busSetSends(n_aux, offsets, members, gains); }) : FX_E_ARG;
}
int fxb_bus_set_send_gains(fxb_handle* h, const float* gains, int ramp) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.busSetSendGains(gains, ramp); }) : FX_E_ARG; }
int64_t fxb_bus_get_sends(fxb_handle* h, int64_t* n_aux, int64_t* offsets, int64_t off_cap, int64_t* members, float* gains, int64_t cap) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.busGetSends(n_aux, offsets, off_cap, members, gains, cap); }) : (int64_t)FX_E_ARG;
}
int fxb_bus_set_gains_list(fxb_handle* h, const int64_t* list, int64_t count, const float* gains, int ramp) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.busSetGainList(fx::Sharded::kGainList, list, count, gains, ramp); }) : FX_E_ARG;
}
int fxb_bus_set_send_gains_list(fxb_handle* h, const int64_t* entries, int64_t count, const float* gains, int ramp) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.busSetGainList(fx::Sharded::kSendGainList, entries, count, gains, ramp); }) : FX_E_ARG;
}
int fxb_bus_set_feed_gains_list(fxb_handle* h, const int64_t* entries, int64_t count, const float* gains, int ramp) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.busSetGainList(fx::Sharded::kFeedGainList, entries, count, gains, ramp); }) : FX_E_ARG;
}
int fxb_bus_set_gains(fxb_handle* h, const float* gains, int ramp) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.busSetGains(gains, ramp); }) : FX_E_ARG; }
int fxb_bus_get_gains(fxb_handle* h, float* gains) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.busGetGains(gains); }) : FX_E_ARG; }
int fxb_process_block_imajor(fxb_handle* h, const float* in, float* out, int n, int64_t in_stride, int64_t out_stride) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processImajor(in, out, n, in_stride, out_stride, false, nullptr); }) : FX_E_ARG;
}
int fxb_process_block_imajor_dev(fxb_handle* h, const float* d_in, float* d_out, int n, int64_t in_stride, int64_t out_stride, void* stream) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.processImajor(d_in, d_out, n, in_stride, out_stride, true, static_cast<hipStream_t>(stream)); }) : FX_E_ARG;
}
int fxb_meter_enable(fxb_handle* h, int on) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterEnable(on != 0); }) : FX_E_ARG; }
int fxb_meter_read(fxb_handle* h, double* energy, float* peak, uint32_t* full_scale, uint32_t* nonfinite, int reset) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterRead(energy, peak, full_scale, nonfinite, reset != 0); }) : FX_E_ARG;
}
int64_t fxb_meter_select(fxb_handle* h, int stat, double threshold, int64_t first, int64_t n_range, int64_t* list, int64_t cap, unsigned flags) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.meterSelect(stat, threshold, first, n_range, list, cap, flags); }) : (int64_t)FX_E_ARG;
}
int fxb_meter_read_list(fxb_handle* h, const int64_t* list, int64_t count, double* energy, float* peak, uint32_t* full_scale, uint32_t* nonfinite, int reset) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterReadList(list, count, energy, peak, full_scale, nonfinite, reset != 0); }) : FX_E_ARG;
}
int fxb_meter_reset_list(fxb_handle* h, const int64_t* list, int64_t count) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterResetList(list, count); }) : FX_E_ARG;
}
int fxb_meter_set_target(fxb_handle* h, const float* target, int64_t n_samples, int64_t group, unsigned flags) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterSetTarget(target, n_samples, group, flags); }) : FX_E_ARG;
}
int fxb_meter_clear_target(fxb_handle* h) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterClearTarget(); }) : FX_E_ARG; }
int fxb_meter_target_seek(fxb_handle* h, int64_t pos) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterTargetSeek(pos); }) : FX_E_ARG; }
int64_t fxb_meter_target_pos(fxb_handle* h) { return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.meterTargetPos(); }) : FX_E_ARG; }
int fxb_meter_read_match(fxb_handle* h, double* err, double* cross, int reset) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterReadMatch(err, cross, reset != 0); }) : FX_E_ARG;
}
int64_t fxb_meter_rank(fxb_handle* h, int stat, int64_t k, double threshold, int64_t first, int64_t n_range, int64_t* list, double* value, unsigned flags) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.meterRank(fx::kRankMeter, stat, k, threshold, first, n_range, list, value, flags); }) : (int64_t)FX_E_ARG;
}
int64_t fxb_meter_rank_match(fxb_handle* h, int stat, int64_t k, double threshold, int64_t first, int64_t n_range, int64_t* list, double* value, unsigned flags) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.meterRank(fx::kRankMatch, stat, k, threshold, first, n_range, list, value, flags); }) : (int64_t)FX_E_ARG;
}
int64_t fxb_meter_rank_level(fxb_handle* h, int stat, int64_t k, double threshold, int64_t first, int64_t n_range, int64_t* list, double* value, unsigned flags) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.meterRank(fx::kRankLevel, stat, k, threshold, first, n_range, list, value, flags); }) : (int64_t)FX_E_ARG;
}
int64_t fxb_meter_select_match(fxb_handle* h, int stat, double threshold, int64_t first, int64_t n_range, int64_t* list, int64_t cap, unsigned flags) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.meterSelectMatch(stat, threshold, first, n_range, list, cap, flags); }) : (int64_t)FX_E_ARG;
}
int fxb_meter_best(fxb_handle* h, int stat, int64_t group, int64_t* winner, double* value, unsigned flags) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterBest(stat, group, winner, value, flags); }) : FX_E_ARG;
}
int fxb_meter_set_level(fxb_handle* h, float release, float floor, unsigned flags) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterSetLevel(release, floor, flags); }) : FX_E_ARG;
}
int fxb_meter_clear_level(fxb_handle* h) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterClearLevel(); }) : FX_E_ARG; }
int fxb_meter_get_level(fxb_handle* h, float* release, float* floor) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterGetLevel(release, floor); }) : FX_E_ARG;
}
int fxb_meter_read_level(fxb_handle* h, float* level, uint32_t* quiet, int reset) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterReadLevel(level, quiet, reset != 0); }) : FX_E_ARG;
}
int fxb_meter_read_level_list(fxb_handle* h, const int64_t* list, int64_t count, float* level, uint32_t* quiet, int reset) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterReadLevelList(list, count, level, quiet, reset != 0); }) : FX_E_ARG;
}
int64_t fxb_meter_select_level(fxb_handle* h, int stat, double threshold, int64_t first, int64_t n_range, int64_t* list, int64_t cap, unsigned flags) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.meterSelectLevel(stat, threshold, first, n_range, list, cap, flags); }) : (int64_t)FX_E_ARG;
}
int fxb_meter_set_tones(fxb_handle* h, int n_tones, const double* coeff, unsigned flags) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterSetTones(n_tones, coeff, flags); }) : FX_E_ARG;
}
int fxb_meter_clear_tones(fxb_handle* h) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterClearTones(); }) : FX_E_ARG; }
int fxb_meter_get_tones(fxb_handle* h, int* n_tones, double* coeff) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterGetTones(n_tones, coeff); }) : FX_E_ARG;
}
int fxb_meter_read_tones(fxb_handle* h, double* s1, double* s2, double* power, int reset) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterReadTones(s1, s2, power, reset != 0); }) : FX_E_ARG;
}
int fxb_meter_read_tones_list(fxb_handle* h, const int64_t* list, int64_t n_list, double* s1, double* s2, double* power, int reset) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.meterReadTonesList(list, n_list, s1, s2, power, reset != 0); }) : FX_E_ARG;
}
int64_t fxb_meter_select_tone(fxb_handle* h, int tone, double threshold, int64_t first, int64_t n_range, int64_t* list, int64_t cap, unsigned flags) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.meterSelectTone(tone, threshold, first, n_range, list, cap, flags); }) : (int64_t)FX_E_ARG;
}
int64_t fxb_meter_rank_tone(fxb_handle* h, int tone, int64_t k, double threshold, int64_t first, int64_t n_range, int64_t* list, double* value, unsigned flags) {
    return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.meterRank(fx::kRankTone, tone, k, threshold, first, n_range, list, value, flags); }) : (int64_t)FX_E_ARG;
}
int64_t fxb_meter_samples(fxb_handle* h) { return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.meterSamples(); }) : FX_E_ARG; }
int fxb_sync(fxb_handle* h) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.sync(); }) : FX_E_ARG; }
int fxb_prepare(fxb_handle* h, int n_samples, int wait) { return h ? guard(&h->batch.front(), FX_E_PROGRAM, [&] { return h->batch.prepare(n_samples, wait != 0); }) : FX_E_ARG; }
int64_t fxb_state_size(fxb_handle* h) { return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.stateBytes(); }) : FX_E_ARG; }
int fxb_save_state(fxb_handle* h, void* buf, int64_t cap) { return h ? guard(&h->batch.front(), FX_E_PROGRAM, [&] { return h->batch.saveState(buf, cap); }) : FX_E_ARG; }
int fxb_load_state(fxb_handle* h, const void* buf, int64_t bytes) { return h ? guard(&h->batch.front(), FX_E_PROGRAM, [&] { return h->batch.loadState(buf, bytes); }) : FX_E_ARG; }
int64_t fxb_instance_image_size(fxb_handle* h, int64_t count) { return h ? guard(&h->batch.front(), (int64_t)FX_E_PROGRAM, [&] { return h->batch.instanceImageBytes(count); }) : FX_E_ARG; }
int fxb_copy_instances(fxb_handle* h, const int64_t* src, const int64_t* dst, int64_t count) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.copyInstances(src, dst, count); }) : FX_E_ARG;
}
int fxb_reset_instances(fxb_handle* h, const int64_t* list, int64_t count) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.resetInstances(list, count); }) : FX_E_ARG; }
int fxb_save_instances(fxb_handle* h, const int64_t* list, int64_t count, void* buf, int64_t cap) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.saveInstances(list, count, buf, cap); }) : FX_E_ARG;
}
int fxb_load_instances(fxb_handle* h, const int64_t* list, int64_t count, const void* buf, int64_t bytes) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.loadInstances(list, count, buf, bytes); }) : FX_E_ARG;
}
int fxb_load_instances_rotated(fxb_handle* h, const int64_t* list, int64_t count, const void* buf, int64_t bytes) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.loadInstancesRotated(list, count, buf, bytes); }) : FX_E_ARG;
}
int fxb_bank_create(fxb_handle* h, int64_t n_slots) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.bankCreate(n_slots); }) : FX_E_ARG; }
int64_t fxb_bank_slots(fxb_handle* h) { return h ? h->batch.bankSlots() : 0; }
int fxb_bank_store(fxb_handle* h, const int64_t* slots, const int64_t* list, int64_t count) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.bankStore(slots, list, count); }) : FX_E_ARG;
}
int fxb_bank_recall(fxb_handle* h, const int64_t* slots, const int64_t* list, int64_t count) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.bankRecall(slots, list, count); }) : FX_E_ARG;
}
int fxb_bank_put(fxb_handle* h, const int64_t* slots, int64_t count, const void* image, int64_t bytes) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.bankPut(slots, count, image, bytes); }) : FX_E_ARG;
}
int fxb_bank_get(fxb_handle* h, const int64_t* slots, int64_t count, void* buf, int64_t cap) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.bankGet(slots, count, buf, cap); }) : FX_E_ARG;
}
int fxb_bank_status(fxb_handle* h, int64_t* refused_calls, int64_t* entry, int* reason, int reset) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.bankStatus(refused_calls, entry, reason, reset != 0); }) : FX_E_ARG;
}
int fxb_set_registers_list(fxb_handle* h, const char* const* keys, int n_keys, const int64_t* list, int64_t count, const float* values) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.setRegistersList(keys, n_keys, list, count, values); }) : FX_E_ARG;
}
int fxb_get_registers_list(fxb_handle* h, const char* const* keys, int n_keys, const int64_t* list, int64_t count, float* values) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.getRegistersList(keys, n_keys, list, count, values); }) : FX_E_ARG;
}
int fxb_set_register_tracks_list(fxb_handle* h, const char* const* keys, int n_keys, const int64_t* list, int64_t count, const float* values, int n_steps, int first, int period) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.setRegisterTracksList(keys, n_keys, list, count, values, n_steps, first, period); }) : FX_E_ARG;
}
int fxb_clear_register_tracks_list(fxb_handle* h) { return h ? guardCode(&h->batch.front(), [&] { return h->batch.clearRegisterTracksList(); }) : FX_E_ARG; }
int fxb_set_tram_list(fxb_handle* h, int which, const int64_t* list, int64_t count, int first, int n_words, const float* values, unsigned flags) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.setTramList(which, list, count, first, n_words, values, flags); }) : FX_E_ARG;
}
int fxb_get_tram_list(fxb_handle* h, int which, const int64_t* list, int64_t count, int first, int n_words, float* values, unsigned flags) {
    return h ? guardCode(&h->batch.front(), [&] { return h->batch.getTramList(which, list, count, first, n_words, values, flags); }) : FX_E_ARG;
}
int fxb_get_tram_i(fxb_handle* h, int which, int64_t inst, float* out, int n_slots) {
    return h ? guard(&h->batch.front(), FX_E_PROGRAM, [&] { return h->batch.getTramAt(which, inst, out, n_slots); }) : FX_E_ARG;
}
int fxb_get_cursors_i(fxb_handle* h, int64_t inst, int32_t* out4) {
    return h ? guard(&h->batch.front(), FX_E_PROGRAM, [&] { return h->batch.getCursorsAt(inst, out4); }) : FX_E_ARG;
}
int64_t fxb_instruction_counter(fxb_handle* h) { return h ? guard(&h->batch.front(), (int64_t)-1, [&] { return h->batch.instructionCounter(); }) : 0; }
int64_t fxb_instruction_counter_i(fxb_handle* h, int64_t inst) { return h ? guard(&h->batch.front(), (int64_t)0, [&] { return h->batch.instructionCounterAt(inst); }) : 0; }
uint32_t fxb_ood_flags(fxb_handle* h) { return h ? guard(&h->batch.front(), ~0u, [&] { return h->batch.oodFlags(); }) : 0; }
int fxb_error_count(fxb_handle* h) { return h ? errorCount(h->batch.front()) : 0; }
const char* fxb_error_desc(fxb_handle* h, int i) { return h ? errorDesc(h->batch.front(), i) : ""; }
int fxb_error_row(fxb_handle* h, int i) { return h ? errorRow(h->batch.front(), i) : -1; }
int fxb_control_count(fxb_handle* h) { return h ? controlCount(h->batch.front()) : 0; }
const char* fxb_control_at(fxb_handle* h, int i) { return h ? controlAt(h->batch.front(), i) : ""; }
int fxb_meta_get(fxb_handle* h, const char* key, char* buf, int buflen) { return h ? guard(&h->batch.front(), 0, [&] { return metaGet(h->batch.front(), key, buf, buflen); }) : 0; }
int fxb_ready(fxb_handle* h) { return (h && h->batch.front().program().ready) ? 1 : 0; }
const char* fxb_last_error(fxb_handle* h) { return h ? h->batch.lastError().c_str() : "null handle"; }
float fxb_last_kernel_ms(fxb_handle* h) { return h ? guard(&h->batch.front(), -1.0f, [&] { return h->batch.lastKernelMs(); }) : -1.0f; }
int fxb_tier_note(fxb_handle* h, char* buf, int buflen) {
    if (!h) return FX_E_ARG;
    return guard(&h->batch.front(), (int)FX_E_PROGRAM, [&] {
        const std::string note = h->batch.front().tierNote();
        if (buf && buflen > 0) std::snprintf(buf, (size_t)buflen, "%s", note.c_str());
        return (int)note.size();
    });
}
int64_t fxb_info(fxb_handle* h, int what) { return h ? guard(&h->batch.front(), (int64_t)-1, [&] { return h->batch.info(what); }) : -1; }


/* ---- front-end only ---- */
fxp_handle* fxp_create(int ch) { return create<fxp_handle>(ch); }
void fxp_destroy(fxp_handle* h) { delete h; }
int fxp_set_option(fxp_handle* h, unsigned option, int on) {
    if (!h || (option & ~fx::kOptAll)) return FX_E_ARG;
    h->prog.options = on ? (h->prog.options | option) : (h->prog.options & ~option);
    return 0;
}
int fxp_load_file(fxp_handle* h, const char* path) { if (!h || !path) return 0; h->lowered = false; return guard(h, 0, [&] { return h->prog.loadFile(path) ? 1 : 0; }); }
int fxp_load_text(fxp_handle* h, const char* text) { if (!h || !text) return 0; h->lowered = false; return guard(h, 0, [&] { return h->prog.loadText(text) ? 1 : 0; }); }
int fxp_num_registers(fxp_handle* h) { return h ? (int)h->prog.regs.size() : 0; }
const char* fxp_register_name(fxp_handle* h, int i) { return (h && i >= 0 && i < (int)h->prog.regs.size()) ? h->prog.regs[i].name.c_str() : ""; }
int fxp_register_type(fxp_handle* h, int i) { return (h && i >= 0 && i < (int)h->prog.regs.size()) ? h->prog.regs[i].type : -1; }
int fxp_register_ioindex(fxp_handle* h, int i) { return (h && i >= 0 && i < (int)h->prog.regs.size()) ? h->prog.regs[i].io : -1; }
float fxp_register_value(fxp_handle* h, int i) { return (h && i >= 0 && i < (int)h->prog.regs.size()) ? h->prog.regs[i].value : 0.0f; }
int fxp_num_instructions(fxp_handle* h) { return h ? (int)h->prog.instrs.size() : 0; }
void fxp_instruction(fxp_handle* h, int i, int o[8]) {
    if (!h || !o || i < 0 || i >= (int)h->prog.instrs.size()) return;
    const fx::Instr& I = h->prog.instrs[i];
    o[0] = I.op; o[1] = I.r; o[2] = I.a; o[3] = I.x; o[4] = I.y; o[5] = I.hasInput; o[6] = I.hasOutput; o[7] = I.hasNoise;
}
int fxp_itram_size(fxp_handle* h) { return h ? h->prog.iTramSize : 0; }
int fxp_xtram_size(fxp_handle* h) { return h ? h->prog.xTramSize : 0; }
int fxp_error_count(fxp_handle* h) { return h ? (int)h->prog.errors.size() : 0; }
const char* fxp_error_desc(fxp_handle* h, int i) { return (h && i >= 0 && i < (int)h->prog.errors.size()) ? h->prog.errors[i].description.c_str() : ""; }
int fxp_error_row(fxp_handle* h, int i) { return (h && i >= 0 && i < (int)h->prog.errors.size()) ? h->prog.errors[i].row : -1; }
int fxp_control_count(fxp_handle* h) { return h ? (int)h->prog.controls.size() : 0; }
const char* fxp_control_at(fxp_handle* h, int i) { return (h && i >= 0 && i < (int)h->prog.controls.size()) ? h->prog.controls[i].c_str() : ""; }
int fxp_meta_get(fxp_handle* h, const char* key, char* buf, int buflen) {
    if (!h || !key) return 0;
    for (const auto& kv : h->prog.meta)
        if (kv.first == key) { if (buf && buflen > 0) std::snprintf(buf, (size_t)buflen, "%s", kv.second.c_str()); return 1; }
    return 0;
}
int fxp_ready(fxp_handle* h) { return (h && h->prog.ready) ? 1 : 0; }
const double* fxp_lut(int kind, int exponent) {
    static const fx::Luts luts;
    return kind ? luts.exp_[exponent & 31] : luts.log_[exponent & 31];
}
static int lowerImpl(fxp_handle* h);
int fxp_lower(fxp_handle* h) {
    if (!h) return FX_E_ARG;
    return guardCode(h, [&] { return lowerImpl(h); });
}
static int lowerImpl(fxp_handle* h) {
    if (!h->prog.ready) { h->err = "no program loaded"; return FX_E_NOTREADY; }
    std::vector<float> values(h->prog.regs.size());
    for (size_t r = 0; r < values.size(); ++r) values[r] = h->prog.regs[r].value;
    h->low = fx::lowerProgram(h->prog, values, std::vector<uint8_t>(values.size(), 0), 1);
    h->lowered = h->low.error.empty();
    h->err = h->low.error;
    return h->lowered ? 0 : FX_E_PROGRAM;
}
int64_t fxp_lower_info(fxp_handle* h, int what) {
    if (!h || !h->lowered) return -1;
    switch (what) {
        case FXB_INFO_NUM_INSTRUCTIONS: return (int64_t)h->prog.instrs.size();
        case FXB_INFO_NUM_REGISTERS: return (int64_t)h->prog.regs.size();
        case FXB_INFO_NUM_LANE_REGS: return h->low.nLaneRegs;
        case FXB_INFO_NUM_UNIFORM_REGS: return h->low.nUniformRegs;
        case FXB_INFO_LDS_BYTES_PER_WG: return (int64_t)h->low.nRows * 256;
        case FXB_INFO_NUM_MICROOPS: return (int64_t)h->low.steady.size();
        case FXB_INFO_ITRAM_SLOTS: return h->low.iSlots;
        case FXB_INFO_XTRAM_SLOTS: return h->low.xSlots;
        case FXB_INFO_TRAM_OPS: return h->low.tramOpsPerSample;
        case FXB_INFO_MULTIPASS: return h->low.multipass ? 1 : 0;
        case FXB_INFO_NUM_SHADOWED: return h->low.nShadowed;
        case FXB_INFO_NUM_CCR_LIVE: return h->low.nCcrLive;
        default: return -1;
    }
}
static int64_t translateImpl(fxp_handle* h, int vgprs, int stream, void* code, int64_t cap, char* listing, int64_t listing_cap, int stages, int stage,
                             int* stagesOut, int* info, int infoCap, std::vector<int32_t>* quietOut = nullptr);
int fxp_track_register(fxp_handle* h, const char* key) {
    if (!h || !key) return FX_E_ARG;
    const int r = h->prog.findRegister(key);
    if (r < 0) return 1;
    if (std::find(h->tracked.begin(), h->tracked.end(), r) != h->tracked.end()) return 0;
    if (h->tracked.size() >= (size_t)fx::kMaxTracks) { h->err = "at most " + std::to_string(fx::kMaxTracks) + " registers can have schedules"; return FX_E_ARG; }
    h->tracked.push_back(r);
    return 0;
}
int64_t fxp_translate(fxp_handle* h, int vgprs, int stream, void* code, int64_t cap, char* listing, int64_t listing_cap) {
    if (!h) return FX_E_ARG;
    try {
        return translateImpl(h, vgprs, stream, code, cap, listing, listing_cap, 1, 0, nullptr, nullptr, 0);
    } catch (const std::exception& e) {
        h->err = e.what();
        return codeOf(e);
    } catch (...) {
        h->err = "unknown error";
        return FX_E_PROGRAM;
    }
}
int64_t fxp_quiet_plan(fxp_handle* h, int vgprs, int32_t* out, int64_t cap) {
    if (!h) return FX_E_ARG;
    try {
        std::vector<int32_t> words;
        const int64_t rc = translateImpl(h, vgprs, 0, nullptr, 0, nullptr, 0, 1, 0, nullptr, nullptr, 0, &words);
        if (rc < 0) return rc;
        if (out && cap > 0) std::memcpy(out, words.data(), (size_t)std::min<int64_t>(cap, (int64_t)words.size()) * 4);
        return (int64_t)words.size();
    } catch (const std::exception& e) {
        h->err = e.what();
        return codeOf(e);
    } catch (...) {
        h->err = "unknown error";
        return FX_E_PROGRAM;
    }
}
static int64_t translateImpl(fxp_handle* h, int vgprs, int stream, void* code, int64_t cap, char* listing, int64_t listing_cap, int stages, int stage,
                             int* stagesOut, int* info, int infoCap, std::vector<int32_t>* quietOut) {
    if (!h->prog.ready) { h->err = "no program loaded"; return FX_E_NOTREADY; }
    if (listing && listing_cap > 0) listing[0] = 0;
    std::vector<float> values(h->prog.regs.size());
    for (size_t r = 0; r < values.size(); ++r) values[r] = h->prog.regs[r].value;
    // the lowering of the VGPR builds: one instance per lane, bookkeeping in VGPRs, rows are plain indices
    std::vector<uint8_t> perLane(values.size(), 0);
    for (int r : h->tracked) perLane[(size_t)r] = 1;   // (a register with a schedule has a row of its own, as in Batch::laneForced)
    fx::Lowered low = fx::lowerProgram(h->prog, values, perLane, 1, false, 1);
    if (!low.error.empty()) { h->err = low.error; return FX_E_PROGRAM; }
    std::string why;
    if (!fx::asmEligible(low, &why)) { h->err = "not eligible: " + why; return FX_E_PROGRAM; }
    if (low.multipass) { h->err = "not eligible: END can be skipped (multi-pass program: the interpreter runs the passes)"; return FX_E_PROGRAM; }
    int v = fx::ASM_V64;
    while (v < fx::ASM_V256 && low.nRows > fx::kAsmVgprRows[v]) ++v;
    if (vgprs != 0) {
        int want = -1;
        for (int q = fx::ASM_V64; q < fx::ASM_VARIANTS; ++q)
            if (fx::kAsmVgprRows[q] + 32 == vgprs) want = q;
        if (want < v) { h->err = "no such VGPR build, or too small for the program"; return FX_E_ARG; }
        v = want;
    }
    const fx::XlateTemplate* tmpl = fx::xlateTemplate((fx::AsmVariant)v, &h->err);
    if (!tmpl) return FX_E_PROGRAM;
    if (stream < 0 || stream > 6 || (stream >= 5 && stages >= 2)) { h->err = "stream: 0 steady fast, 1 steady exact, 2 last fast, 3 last exact, 4 run-once, 5 steady quiet, 6 steady quiet with sum groups (5, 6: unstaged)"; return FX_E_ARG; }
    std::vector<uint32_t> code4[5];
    std::string text4[5];
    fx::XlateImage plan;
    const std::vector<fx::MicroOp> steadyRecords = fx::encodeAsmStream(low.steady, nullptr, true), lastRecords = fx::encodeAsmStream(low.last, nullptr, true);
    std::vector<int> trackRows;
    for (int r : h->tracked) trackRows.push_back(low.rowOfReg[(size_t)r]);
    fx::XlateProgram xprog = fx::xlateProgramOf(steadyRecords, lastRecords, h->prog.iTramSize, h->prog.xTramSize, low.nRows, low.inRow, low.latchRow, trackRows);
    if (const int prio = fx::ReleaseKnobs::fromEnvironment().xlatePrio; prio >= 0) xprog.prioritySlices = prio != 0;   // (what a batch with that knob generates: tests)
    std::vector<std::vector<uint32_t>> stagedCode;
    std::vector<std::string> stagedText;
    if (stagesOut) *stagesOut = 1;
    bool staged = false;
    if (stages >= 2) {
        const fx::StagePlan sp = fx::planStages(steadyRecords, lastRecords, xprog, low.nRows, stages);
        if (!sp.cuts.empty()) {
            if (!fx::buildStagedImage(steadyRecords, lastRecords, *tmpl, xprog, sp, &plan, &stagedCode, &stagedText, &h->err, 144u * 1024u, fx::kStageGroupMax,
                                      fx::ReleaseKnobs::fromEnvironment().stagesGroup)) return FX_E_PROGRAM;
            staged = true;
            if (stagesOut) *stagesOut = plan.stages;
            // info: per cut its record index and the number of rows handed over, then the LDS bytes of a workgroup
            int q = 0;
            for (size_t c = 0; c < sp.cuts.size() && info && q + 2 <= infoCap; ++c) { info[q++] = sp.cuts[c]; info[q++] = (int)sp.live[c].size(); }
            if (info && q < infoCap) info[q++] = (int)plan.ldsBytes;
            // ... then the number of register-file rows and the stage that stores each of them
            if (info && q < infoCap) info[q++] = (int)sp.storeStage.size();
            for (size_t r = 0; r < sp.storeStage.size() && info && q < infoCap; ++r) info[q++] = sp.storeStage[r];
        } else {
            h->err = "not cut into stages: " + sp.why;
        }
    }
    if (staged && (stage < 0 || stage >= plan.stages)) { h->err = "no such stage"; return FX_E_ARG; }
    if (!staged && !fx::planXlate(steadyRecords, lastRecords, *tmpl, xprog, &plan, code4, text4, &h->err)) return FX_E_PROGRAM;
    if (quietOut) {
        // [0] a quiet loop is generated, [1] eligible, [2] saturation sites, [3] dropped by the fast stream, [4] by the quiet loop,
        // [5] vector instructions of the head check, [6] checked rows, [7] dropped records, [8] records; then per checked row
        // {register-file row, register index (-1: none), bound bits}, the dropped record indices, the steady records (8 words each)
        const fx::QuietPlan& q = plan.quietPlan;
        std::vector<int32_t>& w = *quietOut;
        w = {q.inForce && plan.quietOff ? 1 : 0, q.eligible ? 1 : 0, q.sites, q.fastDropped, q.quietDropped, q.checkInstructions,
             (int32_t)q.checkedRows.size(), (int32_t)q.dropped.size(), (int32_t)steadyRecords.size()};
        for (size_t k = 0; k < q.checkedRows.size(); ++k) {
            int reg = -1;
            for (size_t r = 0; r < low.rowOfReg.size(); ++r)
                if (low.rowOfReg[r] == q.checkedRows[k]) reg = (int)r;
            int32_t bits;
            std::memcpy(&bits, &q.checkedBound[k], 4);
            w.push_back(q.checkedRows[k]);
            w.push_back(reg);
            w.push_back(bits);
        }
        for (int i : q.dropped) w.push_back(i);
        for (const fx::MicroOp& r : steadyRecords)
            for (int k = 0; k < 8; ++k) w.push_back((int32_t)r.w[k]);
        // ... and behind the records: the number of adds of +0 the quiet loop does not emit, then their record indices
        w.push_back((int32_t)q.zeroAddsDropped.size());
        for (int i : q.zeroAddsDropped) w.push_back(i);
        // ... then the sum groups (fx_xlate.hpp SumGroup): their number, the links in them; per group {row, T bits, links, flags
        // (1 first, 2 last of its chain, 4 the start is watched), start VGPR, bits of the running bound of the value in front of
        // the group's chain} and per link {record, watched, negate, addend row (-1: a product), addend VGPR (-1: the row itself),
        // sum VGPR, bits of the addend's running bound}
        w.push_back((int32_t)q.sumGroups.size());
        w.push_back(q.sumLinks);
        for (const fx::SumGroup& g : q.sumGroups) {
            int32_t bits;
            std::memcpy(&bits, &g.threshold, 4);
            auto bitsOf = [](float f) { int32_t b; std::memcpy(&b, &f, 4); return b; };
            w.insert(w.end(), {g.row, bits, (int32_t)g.links.size(), (g.first ? 1 : 0) | (g.last ? 2 : 0) | (g.watchStart ? 4 : 0), g.startReg, bitsOf(g.startBound)});
            for (size_t k = 0; k < g.links.size(); ++k)
                w.insert(w.end(), {g.links[k], g.watched[k], g.negate[k], g.addendRow[k], g.addendReg[k], g.dstReg[k], bitsOf(q.addendBound[(size_t)g.links[k]])});
        }
        h->err = q.why;
        return 0;
    }
    if (stream >= 5 && staged) { h->err = "a program cut into stages has no quiet loop"; return FX_E_ARG; }
    // (stream 5 = the quiet loop without sum groups whatever the image carries; stream 6 = the loop with them, empty where the plan has none)
    static const std::vector<uint32_t> noWords;
    static const std::string noText;
    const std::vector<uint32_t>& quietWords = stream == 6 ? (plan.sumGroups ? plan.quietCode : noWords) : (plan.sumGroups ? plan.plainQuietCode : plan.quietCode);
    const std::string& quietText = stream == 6 ? (plan.sumGroups ? plan.quietListing : noText) : (plan.sumGroups ? plan.plainQuietListing : plan.quietListing);
    const std::vector<uint32_t>& words = stream >= 5 ? quietWords : staged ? stagedCode[stream == 4 ? (size_t)plan.stages * 4 : (size_t)stage * 4 + (size_t)stream] : code4[stream];
    const std::string& text = stream >= 5 ? quietText : staged ? stagedText[stream == 4 ? (size_t)plan.stages * 4 : (size_t)stage * 4 + (size_t)stream] : text4[stream];
    const int64_t bytes = (int64_t)words.size() * 4;
    if (code && cap > 0 && bytes > 0) std::memcpy(code, words.data(), (size_t)std::min<int64_t>(cap, bytes));   // (an empty stream has no data())
    if (listing && listing_cap > 0) {
        const size_t n = std::min<size_t>(text.size(), (size_t)listing_cap - 1);
        std::memcpy(listing, text.data(), n);
        listing[n] = 0;
    }
    return bytes;
}
int64_t fxp_translate_staged(fxp_handle* h, int vgprs, int stages, int stage, int stream, void* code, int64_t cap, char* listing, int64_t listing_cap,
                             int* stages_out, int* info, int info_cap) {
    if (!h) return FX_E_ARG;
    try {
        return translateImpl(h, vgprs, stream, code, cap, listing, listing_cap, stages, stage, stages_out, info, info_cap);
    } catch (const std::exception& e) {
        h->err = e.what();
        return codeOf(e);
    } catch (...) {
        h->err = "unknown error";
        return FX_E_PROGRAM;
    }
}
int64_t fxp_code_hash(fxp_handle* h, int vgprs, int stages, unsigned flags) {
    if (!h) return FX_E_ARG;
    try {
        if (!h->prog.ready) { h->err = "no program loaded"; return FX_E_NOTREADY; }
        std::vector<float> values(h->prog.regs.size());
        for (size_t r = 0; r < values.size(); ++r) values[r] = h->prog.regs[r].value;
        std::vector<uint8_t> perLane(values.size(), 0);
        for (int r : h->tracked) perLane[(size_t)r] = 1;
        fx::Lowered low = fx::lowerProgram(h->prog, values, perLane, 1, false, 1);
        if (!low.error.empty()) { h->err = low.error; return FX_E_PROGRAM; }
        std::string why;
        if (!fx::asmEligible(low, &why)) { h->err = "not eligible: " + why; return FX_E_PROGRAM; }
        if (low.multipass) { h->err = "not eligible: END can be skipped (multi-pass program: the interpreter runs the passes)"; return FX_E_PROGRAM; }
        int want = -1;
        for (int q = fx::ASM_V64; q < fx::ASM_VARIANTS; ++q)
            if (fx::kAsmVgprRows[q] + 32 == vgprs && low.nRows <= fx::kAsmVgprRows[q]) want = q;
        if (want < 0) { h->err = "no such VGPR build, or too small for the program"; return FX_E_ARG; }
        const fx::XlateTemplate* tmpl = fx::xlateTemplate((fx::AsmVariant)want, &h->err);
        if (!tmpl) return FX_E_PROGRAM;
        const std::vector<fx::MicroOp> steadyRecords = fx::encodeAsmStream(low.steady, nullptr, true), lastRecords = fx::encodeAsmStream(low.last, nullptr, true);
        std::vector<int> trackRows;
        for (int r : h->tracked) trackRows.push_back(low.rowOfReg[(size_t)r]);
        fx::XlateProgram xprog = fx::xlateProgramOf(steadyRecords, lastRecords, h->prog.iTramSize, h->prog.xTramSize, low.nRows, low.inRow, low.latchRow, trackRows);
        xprog.tramStreaming = (flags & 1u) != 0;
        xprog.prioritySlices = (flags & 2u) != 0 && stages < 2;
        fx::XlateImage image;
        bool built = false;
        if (stages >= 2) {
            const fx::StagePlan sp = fx::planStages(steadyRecords, lastRecords, xprog, low.nRows, stages);
            if (!sp.cuts.empty()) built = fx::buildStagedImage(steadyRecords, lastRecords, *tmpl, xprog, sp, &image, nullptr, nullptr, &h->err, 144u * 1024u, fx::kStageGroupMax,
                                                              fx::ReleaseKnobs::fromEnvironment().stagesGroup);
            if (!built) image = fx::XlateImage();
        }
        if (!built && !fx::buildXlateImage(steadyRecords, lastRecords, *tmpl, xprog, &image, &h->err)) return FX_E_PROGRAM;
        return (int64_t)fx::imageHash(image);
    } catch (const std::exception& e) {
        h->err = e.what();
        return codeOf(e);
    } catch (...) {
        h->err = "unknown error";
        return FX_E_PROGRAM;
    }
}
const char* fxp_last_error(fxp_handle* h) { return h ? h->err.c_str() : "null handle"; }

}  // extern "C"
