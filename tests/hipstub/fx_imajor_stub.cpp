// fx_imajor_stub.cpp — host stand-ins for the launch functions of csrc/fx_imajor.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).
// Both do the real transposition, in stream order, on the stand-in's "device" memory, like the bus stand-ins in fx_bus_stub.cpp:
// word by word as 32-bit patterns, touching nothing outside the n runs and the [rows][n] scratch.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_imajor.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_gathers{0}, g_scatters{0};
bool bad(const fx::ImajorArgs& a) {
    return !a.wide || a.n < 1 || a.rows < 1 || a.rows >= ((long long)1 << 31) || a.first < 0 || a.first >= ((long long)1 << 31) || a.stride < a.first + a.rows ||
           a.n >= ((long long)1 << 31) || a.stride > (((long long)1 << 60) / a.n);
}
}  // namespace

extern "C" long fxstub_imajor_gathers(void) { return g_gathers.load(); }
extern "C" long fxstub_imajor_scatters(void) { return g_scatters.load(); }

namespace fx {

hipError_t launchImajorGather(const ImajorArgs& args, hipStream_t stream) {
    if (bad(args) || !args.in) return hipErrorInvalidValue;
    const ImajorArgs a = args;
    fxstubEnqueue(stream, [a] {
        for (long long i = 0; i < a.n; ++i)
            for (long long r = 0; r < a.rows; ++r) std::memcpy(a.wide + r * a.n + i, a.in + i * a.stride + a.first + r, 4);
        g_gathers.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

hipError_t launchImajorScatter(const ImajorArgs& args, hipStream_t stream) {
    if (bad(args) || !args.out) return hipErrorInvalidValue;
    const ImajorArgs a = args;
    fxstubEnqueue(stream, [a] {
        for (long long i = 0; i < a.n; ++i)
            for (long long r = 0; r < a.rows; ++r) std::memcpy(a.out + i * a.stride + a.first + r, a.wide + r * a.n + i, 4);
        g_scatters.fetch_add(1);
    });
    return hipGetLastError();
}

}  // namespace fx
