// fx_bus_tap_stub.cpp — host stand-in for launchBusTap of csrc/fx_bus.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).
// The gather in stream order on the stand-in's "device" memory, written from the definition in include/fx8010_amd.h ("Bus
// taps") tap by tap, row by row - an addressing of its own, not the kernel's chunks of rows.  Words move with memcpy: bit patterns.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_bus.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_taps{0}, g_badTaps{0};
}  // namespace

extern "C" long fxstub_bus_taps(void) { return g_taps.load(); }          // launches
extern "C" long fxstub_bus_tap_strays(void) { return g_badTaps.load(); } // entries or columns out of range that a launch met (none is ever stored)

namespace fx {

hipError_t launchBusTap(const BusTapArgs& args, hipStream_t stream) {
    if (!args.wide || !args.tapOut || !args.idx || args.rows < 1 || args.n < 1 || args.n >= ((long long)1 << 30) || args.taps < 1 || args.taps > 65536 ||
        args.tapPitch < args.taps || args.tapPitch > 65536)
        return hipErrorInvalidValue;
    const BusTapArgs a = args;
    fxstubEnqueue(stream, [a] {
        for (long long t = 0; t < a.taps; ++t) {
            const long long inst = a.idx[t], column = a.col ? (long long)a.col[t] : t;
            if (inst >= a.n || column >= a.tapPitch) {
                g_badTaps.fetch_add(1);
                continue;
            }
            for (long long r = 0; r < a.rows; ++r) std::memcpy(a.tapOut + r * a.tapPitch + column, a.wide + r * a.n + inst, 4);
        }
        g_taps.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

}  // namespace fx
