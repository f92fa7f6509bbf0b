// fx_gain_scatter_stub.cpp — host stand-in for launchGainScatter of csrc/fx_bus.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).
// The scatter in stream order on the stand-in's "device" memory, written from the definition in include/fx8010_amd.h ("Gain sets
// by list") channel by channel, entry by entry - an addressing of its own, not the kernel's lane per entry.  Words move with
// memcpy: bit patterns.  A position outside the row is counted and never stored.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_bus.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_scatters{0}, g_strays{0};
}  // namespace

extern "C" long fxstub_gain_scatters(void) { return g_scatters.load(); }        // launches
extern "C" long fxstub_gain_scatter_strays(void) { return g_strays.load(); }   // positions out of range that a launch met (none is ever stored)

namespace fx {

hipError_t launchGainScatter(const GainScatterArgs& args, hipStream_t stream) {
    if (!args.idx || !args.val || !args.b || args.count < 1 || args.pitch < 1 || args.count > args.pitch || args.pitch >= ((long long)1 << 32) || args.channels < 1)
        return hipErrorInvalidValue;
    const GainScatterArgs g = args;
    fxstubEnqueue(stream, [g] {
        for (int c = 0; c < g.channels; ++c) {
            const uint32_t* from = g.val + (long long)c * g.count;
            for (long long k = 0; k < g.count; ++k) {
                const long long at = g.idx[k];
                if (at >= g.pitch) {
                    if (c == 0) g_strays.fetch_add(1);
                    continue;
                }
                std::memcpy(g.b + (long long)c * g.pitch + at, from + k, 4);
                if (g.a) std::memcpy(g.a + (long long)c * g.pitch + at, from + k, 4);
            }
        }
        g_scatters.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

}  // namespace fx
