// fx_instances_rot_stub.cpp — host stand-in for launchInstScatterRot of csrc/fx_instances.hip (TEST INFRASTRUCTURE, see
// hip_stub.cpp; the other two launch functions: fx_instances_stub.cpp).  It does the real move, in stream order, on the stand-in's
// "device" memory, word by word as 32-bit patterns.  The addressing is written out on its own here, from the RECORD's side (it
// walks the record's slots j and stores each to its destination slot) and not shared with the kernel (which walks the
// destination's words and computes the record word each comes from): state row w of instance i is state[w][i]; slot s of a delay
// line is at [i / cols][s][i % cols]; the record's slot j of a ring of Z slots lands in slot (j + d) mod Z.  Anything the launch
// would touch outside the listed instances' words or the `count` records and rotation pairs counts as a stray.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_instances.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_rotations{0}, g_strays{0};

bool bad(const fx::InstRotArgs& r) {
    const fx::InstArgs& a = r.base;
    if (!a.state || !a.list || !a.records || !r.rot || a.count < 1 || a.count >= ((long long)1 << 31) || a.n < 1 || a.nPad < a.n) return true;
    if (a.stateRows < 1 || a.iSlots < 0 || a.xSlots < 0 || (a.iSlots > 0 && !a.itram) || (a.xSlots > 0 && !a.xtram)) return true;
    if (a.cols != 64 && a.cols != 128 && a.cols != 256) return true;
    if (a.recStride < fx::instanceWords(a) || a.recStride > (((long long)1 << 60) / a.count)) return true;
    if (a.skipLo < 0 || a.skipHi < a.skipLo || a.skipHi > a.stateRows) return true;
    return r.iSize < 0 || r.iSize > a.iSlots || r.xSize < 0 || r.xSize > a.xSlots;
}

// one delay line of one instance: `slots` words of the record at `rec` into the column of `inst` in the block `tram`
void putLine(uint32_t* tram, const uint32_t* rec, long long inst, int cols, int slots, int ring, int d) {
    uint32_t* column = tram + (inst / cols) * (long long)slots * cols + inst % cols;
    if (d < 0 || d >= ring) {
        if (d != 0) g_strays.fetch_add(1);   // (the runtime never sends one; the kernel takes it as 0)
        d = 0;
    }
    for (int j = 0; j < slots; ++j) {
        const int to = j < ring ? (j + d) % ring : j;
        std::memcpy(column + (long long)to * cols, rec + j, 4);
    }
}
}  // namespace

extern "C" long fxstub_inst_rotations(void) { return g_rotations.load(); }
extern "C" long fxstub_inst_rotation_strays(void) { return g_strays.load(); }

namespace fx {

hipError_t launchInstScatterRot(const InstRotArgs& args, hipStream_t stream) {
    if (bad(args)) return hipErrorInvalidValue;
    const InstRotArgs r = args;
    fxstubEnqueue(stream, [r] {
        const InstArgs& a = r.base;
        for (long long k = 0; k < a.count; ++k) {
            const long long inst = a.list[k];
            if (inst < 0 || inst >= a.n) { g_strays.fetch_add(1); continue; }
            const uint32_t* rec = a.records + k * a.recStride;
            for (int w = 0; w < a.stateRows; ++w)
                if (w < a.skipLo || w >= a.skipHi) std::memcpy(a.state + (long long)w * a.nPad + inst, rec + w, 4);
            if (a.iSlots > 0) putLine(a.itram, rec + a.stateRows, inst, a.cols, a.iSlots, r.iSize, r.rot[2 * k]);
            if (a.xSlots > 0) putLine(a.xtram, rec + a.stateRows + a.iSlots, inst, a.cols, a.xSlots, r.xSize, r.rot[2 * k + 1]);
        }
        g_rotations.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

}  // namespace fx
