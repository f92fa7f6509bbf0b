// fx_meter_list_stub.cpp — host stand-ins for the launch functions of csrc/fx_meter_list.hip (TEST INFRASTRUCTURE, see
// hip_stub.cpp).  They do the real work in stream order on the stand-in's "device" memory, written from the definition in
// include/fx8010_amd.h ("Meter queries by list") with a formulation of their own: the select is ONE loop over the range that
// appends what matches - no chunks, no counts, no scan (the offsets block only gets the total, where the runtime reads it) - and
// it compares in long double, into which every accumulator format and the threshold convert exactly.  The gather and the zero
// walk the list entry by entry; words move with memcpy: bit patterns.  An entry outside the batch is counted and never followed.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_meter.hpp"
#include "../../fx8010-emulator-core_amd/csrc/fx_meter_list.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_selects{0}, g_gathers{0}, g_zeros{0}, g_strays{0};

size_t rowOff(int stat, long long nPad) {
    return stat == 0 ? fx::meterEnergyOff(nPad) : stat == 1 ? fx::meterPeakOff(nPad) : stat == 2 ? fx::meterFullScaleOff(nPad) : fx::meterNonfiniteOff(nPad);
}
long double valueOf(const void* rows, long long nPad, int c, int stat, long long col) {
    const char* row = static_cast<const char*>(rows) + (size_t)c * fx::meterChannelBytes(nPad) + rowOff(stat, nPad);
    if (stat == 0) { double v; std::memcpy(&v, row + col * 8, 8); return v; }
    if (stat == 1) { float v; std::memcpy(&v, row + col * 4, 4); return v; }
    uint32_t v;
    std::memcpy(&v, row + col * 4, 4);
    return v;
}
bool badList(const fx::MeterListArgs& a, bool gather) {
    if (!a.rows || !a.list || a.count < 1 || a.count >= ((long long)1 << 31) || a.n < 1 || a.nPad < a.n || a.channels < 1 || a.channels > 4) return true;
    return gather && !a.packed;
}
void columns(const fx::MeterListArgs& a, bool gather) {
    const size_t rowWords = (size_t)a.channels * (size_t)a.count;
    char* packed = static_cast<char*>(a.packed);
    for (long long k = 0; k < a.count; ++k) {
        const long long inst = a.list[k];
        if (inst < 0 || inst >= a.n) { g_strays.fetch_add(1); continue; }
        for (int c = 0; c < a.channels; ++c) {
            char* ch = static_cast<char*>(a.rows) + (size_t)c * fx::meterChannelBytes(a.nPad);
            const size_t at = (size_t)c * (size_t)a.count + (size_t)k;
            for (int stat = 0; stat < 4; ++stat) {
                const size_t bytes = stat == 0 ? 8 : 4;
                char* word = ch + rowOff(stat, a.nPad) + (size_t)inst * bytes;
                if (gather) std::memcpy(packed + rowWords * (stat == 0 ? 0 : 4 + 4 * (size_t)stat) + at * bytes, word, bytes);
                if (!gather || a.reset) std::memset(word, 0, bytes);
            }
        }
    }
}
}  // namespace

extern "C" long fxstub_meter_selects(void) { return g_selects.load(); }   // launches
extern "C" long fxstub_meter_gathers(void) { return g_gathers.load(); }
extern "C" long fxstub_meter_zeros(void) { return g_zeros.load(); }
extern "C" long fxstub_meter_list_strays(void) { return g_strays.load(); }   // list entries out of range that a launch met (none is ever followed)

namespace fx {

hipError_t launchMeterSelect(const MeterSelectArgs& args, hipStream_t stream) {
    if (!args.rows || !args.offsets || args.n < 1 || args.nPad < args.n || args.channels < 1 || args.channels > 4 || args.stat < 0 || args.stat > 3) return hipErrorInvalidValue;
    if (args.first < 0 || args.nRange < 1 || args.first > args.n - args.nRange || args.cap < 0 || (args.cap > 0 && !args.list) || args.threshold != args.threshold) return hipErrorInvalidValue;
    const MeterSelectArgs a = args;
    fxstubEnqueue(stream, [a] {
        unsigned long long found = 0;
        const long double t = a.threshold;
        for (long long col = a.first; col < a.first + a.nRange; ++col) {
            long double best = valueOf(a.rows, a.nPad, 0, a.stat, col);
            for (int c = 1; c < a.channels; ++c) {
                const long double v = valueOf(a.rows, a.nPad, c, a.stat, col);
                if (v > best) best = v;
            }
            if (a.below ? !(best < t) : !(best >= t)) continue;
            if (found < (unsigned long long)a.cap) a.list[found] = a.firstGlobal + (col - a.first);
            ++found;
        }
        a.offsets[meterSelectChunks(a.nRange)] = found;
        g_selects.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

hipError_t launchMeterGather(const MeterListArgs& args, hipStream_t stream) {
    if (badList(args, true)) return hipErrorInvalidValue;
    const MeterListArgs a = args;
    fxstubEnqueue(stream, [a] {
        columns(a, true);
        g_gathers.fetch_add(1);
    });
    return hipGetLastError();
}

hipError_t launchMeterZero(const MeterListArgs& args, hipStream_t stream) {
    if (badList(args, false)) return hipErrorInvalidValue;
    const MeterListArgs a = args;
    fxstubEnqueue(stream, [a] {
        columns(a, false);
        g_zeros.fetch_add(1);
    });
    return hipGetLastError();
}

}  // namespace fx
