// fx_bus_feed_stub.cpp — host stand-in for launchBusFeed of csrc/fx_bus.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).
// It does the real arithmetic in stream order on the stand-in's "device" memory, written from the definition in
// include/fx8010_amd.h ("Bus feeds") with an addressing of its own: instance by instance, entry by entry.  The host's tables are
// checked against the structure they must describe first - the padding behind the offsets, the order of the offsets, every source
// column, the alignment and the pitch a lane's 16-byte accesses rely on, a source block that is device memory - and a launch that
// fails a check counts as a stray and writes nothing.
// Compiled with -ffp-contract=off like everything else; the volatiles round every intermediate to fp32 where the definition does.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_bus.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_feeds{0}, g_feedRamps{0}, g_feedMaps{0}, g_badFeeds{0};
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
}  // namespace

extern "C" long fxstub_bus_feeds(void) { return g_feeds.load(); }             // launches, ramping ones included
extern "C" long fxstub_bus_feed_ramps(void) { return g_feedRamps.load(); }    // ... of those, the ones with a ramp pending
extern "C" long fxstub_bus_feed_maps(void) { return g_feedMaps.load(); }      // ... and the ones of the map form
extern "C" long fxstub_bus_feed_strays(void) { return g_badFeeds.load(); }    // launches whose tables or source block failed a check (nothing of them is used)

namespace fx {

hipError_t launchBusFeed(const BusFeedArgs& args, hipStream_t stream) {
    const bool map = !args.off;
    const long long n4 = (args.n + 3) / 4 * 4;
    if (!args.src || !args.wide || args.rows < 1 || args.n < 1 || args.n >= ((long long)1 << 30) || args.m < 1 || args.m >= ((long long)1 << 30) || args.entries < 0 ||
        args.entries > ((long long)1 << 24) || (map && args.entries != args.n) || (args.entries > 0 && !args.idx) || !aligned16(args.off) || !aligned16(args.idx) ||
        args.channels < 1 || args.rows % args.channels != 0)
        return hipErrorInvalidValue;
    if (args.target) {
        if ((args.ramp && !args.current) || args.gainPitch < args.entries || args.samples < 1 || args.sample0 < 0 ||
            (long long)args.sample0 + args.rows / args.channels > (long long)args.samples)
            return hipErrorInvalidValue;
        if (map && (args.gainPitch < n4 || args.gainPitch % 4 != 0 || !aligned16(args.target) || !aligned16(args.current))) return hipErrorInvalidValue;
    } else if (args.ramp) {
        return hipErrorInvalidValue;
    }
    const BusFeedArgs a = args;
    fxstubEnqueue(stream, [a, map, n4] {
        // the tables against the structure they must describe
        bool sound = true;
        hipPointerAttribute_t attr;
        std::memset(&attr, 0, sizeof(attr));
        if (hipPointerGetAttributes(&attr, a.src) != hipSuccess || attr.type != hipMemoryTypeDevice) sound = false;   // (never gathered over PCIe)
        (void)hipGetLastError();
        if (!map) {
            sound = sound && a.off[0] == 0u && a.off[a.n] == (uint32_t)a.entries;
            for (long long i = 0; i < a.n && sound; ++i) sound = a.off[i] <= a.off[i + 1];
            for (long long i = a.n; i <= n4 && sound; ++i) sound = a.off[i] == (uint32_t)a.entries;
        }
        for (long long e = 0; e < (map ? n4 : a.entries) && sound; ++e) sound = a.idx[e] < (uint32_t)a.m;
        if (!sound) {
            g_badFeeds.fetch_add(1);
            return;
        }
        for (long long row = 0; row < a.rows; ++row) {
            const long long s = row / a.channels + a.sample0;   // sample of the call
            const int c = (int)(row % a.channels);
            const uint32_t* x = a.src + row * a.m;
            for (long long i = 0; i < a.n; ++i) {
                const long long lo = map ? i : (long long)a.off[i], hi = map ? i + 1 : (long long)a.off[i + 1];
                uint32_t word = 0u;   // no entry: +0.0f
                volatile float sum = 0.0f;
                for (long long e = lo; e < hi; ++e) {
                    uint32_t termBits = x[a.idx[e]];   // unweighted: the word itself
                    if (a.target) {
                        const float gb = a.target[(long long)c * a.gainPitch + e];
                        volatile float w = gb;
                        if (a.ramp && s != (long long)a.samples - 1) {
                            const float ga = a.current[(long long)c * a.gainPitch + e];
                            volatile float t = (float)(s + 1) * a.r;
                            volatile float d = gb - ga;
                            volatile float mul = d * t;
                            w = ga + mul;
                        }
                        float xf;
                        std::memcpy(&xf, &termBits, 4);
                        volatile float term = 0.0f;
                        if (w != 0.0f) term = w * xf;   // (either zero: +0.0f, whatever the source holds)
                        const float tv = term;
                        std::memcpy(&termBits, &tv, 4);
                    }
                    if (e == lo) {
                        word = termBits;   // the sum starts from term_0, not from zero
                    } else {
                        float prev, tf;
                        std::memcpy(&prev, &word, 4);
                        std::memcpy(&tf, &termBits, 4);
                        sum = prev + tf;
                        const float sv = sum;
                        std::memcpy(&word, &sv, 4);
                    }
                }
                std::memcpy(a.wide + row * a.n + i, &word, 4);
            }
        }
        g_feeds.fetch_add(1);
        if (a.ramp) g_feedRamps.fetch_add(1);
        if (map) g_feedMaps.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

}  // namespace fx
