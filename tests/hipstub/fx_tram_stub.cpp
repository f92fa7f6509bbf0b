// fx_tram_stub.cpp — host stand-ins for the launch functions of csrc/fx_tram.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).
// Both do the real moves in stream order on the stand-in's "device" memory, written from the definition in include/fx8010_amd.h
// ("Delay-line windows by list") entry by entry, word by word - an addressing of its own, not the kernel's origin-and-walk: the
// slot of every word is computed from the entry's position word with `%`, and the word of instance inst at slot s is
// line + (inst / cols) * slots * cols + s * cols + inst % cols.  Words move with memcpy: bit patterns.  An entry outside the
// batch, a position word outside the ring or a slot outside the line is counted and never followed.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_tram.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_scatters{0}, g_gathers{0}, g_strays{0};
bool bad(const fx::TramListArgs& a, bool gather) {
    if (!a.line || !a.list || !a.values || a.count < 1 || a.count >= ((long long)1 << 31) || a.n < 1 || a.nPad < a.n) return true;
    if (a.slots < 1 || (a.cols != 64 && a.cols != 128 && a.cols != 256) || a.first < 0 || a.nWords < 1) return true;
    if (a.ringSize == 0 && (long long)a.first + a.nWords > a.slots) return true;
    if (a.ringSize != 0 && (a.ringSize < 1 || a.ringSize > a.slots || !a.state || a.posRow < 0 || a.first >= a.ringSize || a.nWords > a.ringSize)) return true;
    return a.valueStride == 0 ? gather : a.valueStride < a.nWords;
}
void move(const fx::TramListArgs& a, bool gather) {
    for (long long i = 0; i < a.count; ++i) {
        const long long inst = a.list[i];
        if (inst < 0 || inst >= a.n) { g_strays.fetch_add(1); continue; }
        long long p = 0;
        if (a.ringSize > 0) {
            p = a.state[(long long)a.posRow * a.nPad + inst];
            if (p >= a.ringSize) { g_strays.fetch_add(1); continue; }
        }
        uint32_t* packed = a.values + i * a.valueStride;
        uint32_t* column = a.line + (inst / a.cols) * (long long)a.slots * a.cols + inst % a.cols;
        for (long long j = 0; j < a.nWords; ++j) {
            const long long age = (long long)a.first + j, Z = a.ringSize;
            long long slot = age;
            if (Z > 0) slot = a.dane ? (p + 1 + age) % Z : (((p - 1 - age) % Z) + Z) % Z;
            if (slot < 0 || slot >= a.slots) { g_strays.fetch_add(1); continue; }
            if (gather) std::memcpy(packed + j, column + slot * a.cols, 4);
            else std::memcpy(column + slot * a.cols, packed + j, 4);
        }
    }
}
}  // namespace

extern "C" long fxstub_tram_scatters(void) { return g_scatters.load(); }   // launches
extern "C" long fxstub_tram_gathers(void) { return g_gathers.load(); }
extern "C" long fxstub_tram_strays(void) { return g_strays.load(); }       // entries, positions and slots out of range that a launch met (none is ever followed)

namespace fx {

hipError_t launchTramScatter(const TramListArgs& args, hipStream_t stream) {
    if (bad(args, false)) return hipErrorInvalidValue;
    const TramListArgs a = args;
    fxstubEnqueue(stream, [a] {
        move(a, false);
        g_scatters.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

hipError_t launchTramGather(const TramListArgs& args, hipStream_t stream) {
    if (bad(args, true)) return hipErrorInvalidValue;
    const TramListArgs a = args;
    fxstubEnqueue(stream, [a] {
        move(a, true);
        g_gathers.fetch_add(1);
    });
    return hipGetLastError();
}

}  // namespace fx
