// fx_bus_stub.cpp — host stand-ins for the launch functions of csrc/fx_bus.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).
// Both do their real work, in stream order, on the stand-in's "device" memory, like launchFillRows in fx_kernel_stub.cpp: the
// expand copies every group word to its instances, the mix adds in the order fx_bus.hpp fixes (64 partial sums taking the
// members j * 64 + l for j ascending, then the shuffle-down tree).  Compiled with -ffp-contract=off like everything else.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_bus.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_expands{0}, g_mixes{0};
bool bad(const fx::BusArgs& a) { return a.rows < 1 || a.n < 1 || a.group < 1 || a.group > a.n || a.groups != (a.n + a.group - 1) / a.group || a.narrowPitch < a.groups || !a.wide; }
}  // namespace

extern "C" long fxstub_bus_expands(void) { return g_expands.load(); }
extern "C" long fxstub_bus_mixes(void) { return g_mixes.load(); }

namespace fx {

hipError_t launchBusExpand(const BusArgs& args, hipStream_t stream) {
    if (bad(args) || !args.narrowIn) return hipErrorInvalidValue;
    const BusArgs a = args;
    fxstubEnqueue(stream, [a] {
        for (long long r = 0; r < a.rows; ++r)
            for (long long i = 0; i < a.n; ++i) std::memcpy(a.wide + r * a.n + i, a.narrowIn + r * a.narrowPitch + i / a.group, 4);
        g_expands.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

hipError_t launchBusMix(const BusArgs& args, hipStream_t stream) {
    if (bad(args) || !args.narrowOut) return hipErrorInvalidValue;
    const BusArgs a = args;
    fxstubEnqueue(stream, [a] {
        for (long long r = 0; r < a.rows; ++r)
            for (long long g = 0; g < a.groups; ++g) {
                const float* y = a.wide + r * a.n + g * a.group;
                const long long count = a.n - g * a.group < a.group ? a.n - g * a.group : a.group;
                volatile float p[64];   // (volatile: every partial sum is rounded to fp32 where the order says so)
                for (int l = 0; l < 64; ++l) p[l] = 0.0f;
                for (long long m = 0; m < count; ++m) p[m % 64] = p[m % 64] + y[m];
                for (int step = 32; step > 0; step >>= 1)
                    for (int l = 0; l < step; ++l) p[l] = p[l] + p[l + step];
                a.narrowOut[r * a.narrowPitch + g] = p[0];
            }
        g_mixes.fetch_add(1);
    });
    return hipGetLastError();
}

}  // namespace fx
