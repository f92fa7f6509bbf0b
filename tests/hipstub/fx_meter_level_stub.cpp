// fx_meter_level_stub.cpp — host stand-ins for the launch functions of the level meters (csrc/fx_meter.hip launchMeterLevel /
// launchMeterTargetLevel, csrc/fx_meter_list.hip launchLevelSelect / launchLevelGather / launchLevelZero; TEST INFRASTRUCTURE, see
// hip_stub.cpp).  They do the real arithmetic in stream order on the stand-in's "device" memory, written from the definition in
// include/fx8010_amd.h ("Level meters") with a formulation of their own: the level walks a column in FLOATS - fabsf, a volatile
// fp32 product, a float compare for the maximum and for the floor - where the kernel compares bit patterns; the existing
// accumulators are taken by the stand-ins that already exist, queued on the same stream right behind (launchMeter /
// launchMeterTarget: one more stream operation, the same words).  The select is one loop that appends, in long double.  Compiled
// with -ffp-contract=off like everything else; x86-64 keeps fp32 denormals.
#include <atomic>
#include <cmath>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_meter.hpp"
#include "../../fx8010-emulator-core_amd/csrc/fx_meter_list.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_levels{0}, g_targetLevels{0}, g_selects{0}, g_gathers{0}, g_zeros{0}, g_strays{0};

float* levelRow(const void* rows, long long nPad, int c) {
    return reinterpret_cast<float*>(static_cast<char*>(const_cast<void*>(rows)) + (size_t)c * fx::levelChannelBytes(nPad) + fx::levelLevelOff(nPad));
}
uint32_t* quietRow(const void* rows, long long nPad, int c) {
    return reinterpret_cast<uint32_t*>(static_cast<char*>(const_cast<void*>(rows)) + (size_t)c * fx::levelChannelBytes(nPad) + fx::levelQuietOff(nPad));
}
bool badParams(const fx::LevelParams& l) {
    return !l.rows || !(l.release >= 0.0f && l.release <= 1.0f) || !(l.floor >= 0.0f) || std::isinf(l.floor) || std::signbit(l.release) || std::signbit(l.floor);
}
void takeBlock(const fx::MeterArgs& m, const fx::LevelParams& l) {
    for (int c = 0; c < m.channels; ++c) {
        float* level = levelRow(l.rows, m.nPad, c);
        uint32_t* quiet = quietRow(l.rows, m.nPad, c);
        for (long long i = 0; i < m.n; ++i) {
            float lv = level[i];
            uint32_t q = quiet[i];
            for (int s = 0; s < m.samples; ++s) {
                const float y = m.y[((size_t)s * (size_t)m.channels + (size_t)c) * (size_t)m.pitch + (size_t)i];
                const bool fin = std::isfinite(y);
                const float w = fin ? std::fabs(y) : 0.0f;
                const volatile float d = lv * l.release;   // (volatile: a value of its own, rounded to fp32 once)
                const float dv = d;
                lv = w > dv ? w : dv;
                if (!fin || w >= l.floor) q = 0;
                else if (q != 0xffffffffu) ++q;
            }
            level[i] = lv;
            quiet[i] = q;
        }
    }
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
            const size_t at = ((size_t)c * (size_t)a.count + (size_t)k) * 4;
            char* word[2] = {reinterpret_cast<char*>(levelRow(a.rows, a.nPad, c) + inst), reinterpret_cast<char*>(quietRow(a.rows, a.nPad, c) + inst)};
            for (int r = 0; r < 2; ++r) {
                if (gather) std::memcpy(packed + rowWords * 4 * (size_t)r + at, word[r], 4);
                if (!gather || a.reset) std::memset(word[r], 0, 4);
            }
        }
    }
}
}  // namespace

extern "C" long fxstub_meter_level_launches(void) { return g_levels.load(); }
extern "C" long fxstub_meter_target_level_launches(void) { return g_targetLevels.load(); }
extern "C" long fxstub_level_selects(void) { return g_selects.load(); }
extern "C" long fxstub_level_gathers(void) { return g_gathers.load(); }
extern "C" long fxstub_level_zeros(void) { return g_zeros.load(); }
extern "C" long fxstub_level_strays(void) { return g_strays.load(); }   // list entries out of range that a launch met (none is followed)

namespace fx {

hipError_t launchMeterLevel(const MeterLevelArgs& args, hipStream_t stream) {
    if (badParams(args.l)) return hipErrorInvalidValue;
    const hipError_t e = launchMeter(args.m, stream);   // (checks the block's arguments; the four)
    if (e != hipSuccess) return e;
    const MeterLevelArgs a = args;
    fxstubEnqueue(stream, [a] {
        takeBlock(a.m, a.l);
        g_levels.fetch_add(1);
    });
    return hipGetLastError();   // as the real helper does after hipLaunchKernelGGL
}

hipError_t launchMeterTargetLevel(const MeterTargetLevelArgs& args, hipStream_t stream) {
    if (badParams(args.l)) return hipErrorInvalidValue;
    const hipError_t e = launchMeterTarget(args.t, stream);   // (the four and the two of the target)
    if (e != hipSuccess) return e;
    const MeterTargetLevelArgs a = args;
    fxstubEnqueue(stream, [a] {
        takeBlock(a.t.m, a.l);
        g_targetLevels.fetch_add(1);
    });
    return hipGetLastError();
}

hipError_t launchLevelSelect(const LevelSelectArgs& args, hipStream_t stream) {
    if (!args.rows || !args.offsets || args.n < 1 || args.nPad < args.n || args.channels < 1 || args.channels > 4 || args.stat < 0 || args.stat > 1) return hipErrorInvalidValue;
    if (args.first < 0 || args.nRange < 1 || args.first > args.n - args.nRange || args.cap < 0 || (args.cap > 0 && !args.list) || args.threshold != args.threshold) return hipErrorInvalidValue;
    const LevelSelectArgs a = args;
    fxstubEnqueue(stream, [a] {
        unsigned long long found = 0;
        const long double t = a.threshold;
        for (long long col = a.first; col < a.first + a.nRange; ++col) {
            long double v = a.stat == 0 ? (long double)levelRow(a.rows, a.nPad, 0)[col] : (long double)quietRow(a.rows, a.nPad, 0)[col];
            for (int c = 1; c < a.channels; ++c) {
                if (a.stat == 0) {
                    const long double x = levelRow(a.rows, a.nPad, c)[col];
                    if (x > v) v = x;
                } else {
                    const long double x = quietRow(a.rows, a.nPad, c)[col];
                    if (x < v) v = x;
                }
            }
            if (a.below ? !(v < t) : !(v >= t)) continue;
            if (found < (unsigned long long)a.cap) a.list[found] = a.firstGlobal + (col - a.first);
            ++found;
        }
        a.offsets[meterSelectChunks(a.nRange)] = found;
        g_selects.fetch_add(1);
    });
    return hipGetLastError();
}

hipError_t launchLevelGather(const MeterListArgs& args, hipStream_t stream) {
    if (badList(args, true)) return hipErrorInvalidValue;
    const MeterListArgs a = args;
    fxstubEnqueue(stream, [a] {
        columns(a, true);
        g_gathers.fetch_add(1);
    });
    return hipGetLastError();
}

hipError_t launchLevelZero(const MeterListArgs& args, hipStream_t stream) {
    if (badList(args, false)) return hipErrorInvalidValue;
    const MeterListArgs a = args;
    fxstubEnqueue(stream, [a] {
        columns(a, false);
        g_zeros.fetch_add(1);
    });
    return hipGetLastError();
}

}  // namespace fx
