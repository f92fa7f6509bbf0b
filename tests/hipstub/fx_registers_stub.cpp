// fx_registers_stub.cpp — host stand-ins for the launch functions of csrc/fx_registers.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).
// Both do the real moves in stream order on the stand-in's "device" memory, written from the definition in include/fx8010_amd.h
// ("Register sets by list") key by key, entry by entry - an addressing of its own, not the kernel's lane per entry: the word of
// key k and entry i is values[k * count + i] on the packed side and state + rows[k] * nPad + list[i] on the batch side.  Words
// move with memcpy: bit patterns.  An entry outside the batch or a row outside the state block is counted and never followed.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_registers.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_scatters{0}, g_gathers{0}, g_strays{0};
bool bad(const fx::RegListArgs& a) {
    if (!a.state || !a.list || !a.rows || !a.values) return true;
    if (a.count < 1 || a.count >= ((long long)1 << 31) || a.nKeys < 1 || (long long)a.nKeys * a.count >= ((long long)1 << 31)) return true;
    return a.n < 1 || a.nPad < a.n || a.stateRows < 1;
}
void move(const fx::RegListArgs& a, bool gather) {
    for (int k = 0; k < a.nKeys; ++k) {
        const long long row = a.rows[k];
        if (row < 0 || row >= a.stateRows) { g_strays.fetch_add(1); continue; }
        uint32_t* packed = a.values + (long long)k * a.count;
        uint32_t* batch = a.state + row * a.nPad;
        for (long long i = 0; i < a.count; ++i) {
            const long long inst = a.list[i];
            if (inst < 0 || inst >= a.n) {
                if (k == 0) g_strays.fetch_add(1);
                continue;
            }
            if (gather) std::memcpy(packed + i, batch + inst, 4);
            else std::memcpy(batch + inst, packed + i, 4);
        }
    }
}
}  // namespace

extern "C" long fxstub_reg_scatters(void) { return g_scatters.load(); }   // launches
extern "C" long fxstub_reg_gathers(void) { return g_gathers.load(); }
extern "C" long fxstub_reg_strays(void) { return g_strays.load(); }       // entries and rows out of range that a launch met (none is ever followed)

namespace fx {

hipError_t launchRegScatter(const RegListArgs& args, hipStream_t stream) {
    if (bad(args)) return hipErrorInvalidValue;
    const RegListArgs a = args;
    fxstubEnqueue(stream, [a] {
        move(a, false);
        g_scatters.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

hipError_t launchRegGather(const RegListArgs& args, hipStream_t stream) {
    if (bad(args)) return hipErrorInvalidValue;
    const RegListArgs a = args;
    fxstubEnqueue(stream, [a] {
        move(a, true);
        g_gathers.fetch_add(1);
    });
    return hipGetLastError();
}

}  // namespace fx
