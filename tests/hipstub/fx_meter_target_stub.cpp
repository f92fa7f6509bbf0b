// fx_meter_target_stub.cpp — host stand-ins for the launch functions of the target meters (csrc/fx_meter.hip launchMeterTarget,
// csrc/fx_meter_list.hip launchMatchSelect / launchMeterBest / launchMatchZero; TEST INFRASTRUCTURE, see hip_stub.cpp).  They do
// the real arithmetic in stream order on the stand-in's "device" memory, written from the definition in include/fx8010_amd.h
// ("Target meters") with a formulation of their own: the meter walks sample by sample and takes the target position with `%`
// (the kernel carries a row pointer with a conditional wrap), the select is one loop that appends, the best is one loop per
// group that keeps the first of the best.  The four existing accumulators are taken as fx_meter_stub.cpp takes them, including
// its volatile product.  Compiled with -ffp-contract=off like everything else.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_meter.hpp"
#include "../../fx8010-emulator-core_amd/csrc/fx_meter_list.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_targets{0}, g_selects{0}, g_bests{0}, g_zeros{0}, g_strays{0};

double* matchRow(const void* rows, long long nPad, int c, int stat) {
    char* ch = static_cast<char*>(const_cast<void*>(rows)) + (size_t)c * fx::matchChannelBytes(nPad);
    return reinterpret_cast<double*>(ch + (stat == 0 ? fx::matchErrOff(nPad) : fx::matchCrossOff(nPad)));
}
double valueOf(const void* rows, long long nPad, int channels, int stat, long long col) {
    volatile double sum = matchRow(rows, nPad, 0, stat)[col];
    for (int c = 1; c < channels; ++c) sum = sum + matchRow(rows, nPad, c, stat)[col];
    return sum;
}
}  // namespace

extern "C" long fxstub_meter_target_launches(void) { return g_targets.load(); }
extern "C" long fxstub_match_selects(void) { return g_selects.load(); }
extern "C" long fxstub_match_bests(void) { return g_bests.load(); }
extern "C" long fxstub_match_zeros(void) { return g_zeros.load(); }
extern "C" long fxstub_match_strays(void) { return g_strays.load(); }   // target columns or list entries out of range that a launch met (none is followed)

namespace fx {

hipError_t launchMeterTarget(const MeterTargetArgs& args, hipStream_t stream) {
    const MeterArgs& m = args.m;
    if (!m.y || !m.rows || m.n < 1 || m.nPad < m.n || m.pitch < m.n || m.samples < 1 || m.channels < 1 || m.channels > 4) return hipErrorInvalidValue;
    if ((unsigned long long)m.channels * (unsigned long long)m.pitch * 4u >= (1ull << 32)) return hipErrorInvalidValue;
    if (!args.match || !args.target || args.tSamples < 1 || args.tCols < 1 || args.group < 1 || args.firstGlobal < 0 || args.pos < 0 || (args.loop && args.pos >= args.tSamples)) return hipErrorInvalidValue;
    if (args.firstColumn != args.firstGlobal / args.group || (args.firstGlobal + m.n - 1) / args.group - args.firstColumn >= args.tCols) return hipErrorInvalidValue;
    if ((unsigned long long)m.channels * (unsigned long long)args.tCols * 4u >= (1ull << 32)) return hipErrorInvalidValue;
    const MeterTargetArgs a = args;
    fxstubEnqueue(stream, [a] {
        const MeterArgs& m = a.m;
        for (int c = 0; c < m.channels; ++c) {
            char* rows = static_cast<char*>(m.rows) + (size_t)c * meterChannelBytes(m.nPad);
            double* energy = reinterpret_cast<double*>(rows + meterEnergyOff(m.nPad));
            uint32_t* peak = reinterpret_cast<uint32_t*>(rows + meterPeakOff(m.nPad));
            uint32_t* fullScale = reinterpret_cast<uint32_t*>(rows + meterFullScaleOff(m.nPad));
            uint32_t* nonfinite = reinterpret_cast<uint32_t*>(rows + meterNonfiniteOff(m.nPad));
            double* err = matchRow(a.match, m.nPad, c, 0);
            double* cross = matchRow(a.match, m.nPad, c, 1);
            for (int s = 0; s < m.samples; ++s) {
                const float* y = m.y + ((size_t)s * (size_t)m.channels + (size_t)c) * (size_t)m.pitch;
                long long q = a.pos + s;
                if (a.loop) q %= a.tSamples;
                const float* t = q < a.tSamples ? a.target + ((size_t)q * (size_t)m.channels + (size_t)c) * (size_t)a.tCols : nullptr;
                for (long long i = 0; i < m.n; ++i) {
                    uint32_t word;
                    std::memcpy(&word, y + i, 4);
                    const uint32_t mag = word & 0x7fffffffu;
                    const bool fin = mag < 0x7f800000u;
                    const uint32_t w = fin ? mag : 0u;
                    float wf;
                    std::memcpy(&wf, &w, 4);
                    const volatile double sq = (double)wf * (double)wf;   // (volatile: the product is a value of its own, never part of a fused add)
                    energy[i] = energy[i] + sq;
                    if (w > peak[i]) peak[i] = w;
                    if (fin && mag >= 0x3f800000u && fullScale[i] != 0xffffffffu) ++fullScale[i];
                    if (!fin && nonfinite[i] != 0xffffffffu) ++nonfinite[i];
                    if (!t || !fin) continue;
                    const long long col = (a.firstGlobal + i) / a.group - a.firstColumn;
                    if (col < 0 || col >= a.tCols) { g_strays.fetch_add(1); continue; }
                    uint32_t tw;
                    std::memcpy(&tw, t + col, 4);
                    if ((tw & 0x7fffffffu) >= 0x7f800000u) continue;
                    const double yd = (double)y[i], td = (double)t[col];
                    const volatile double d = yd - td;
                    const volatile double e = d * d;
                    const volatile double yt = yd * td;
                    err[i] = err[i] + e;
                    cross[i] = cross[i] + yt;
                }
            }
        }
        g_targets.fetch_add(1);
    });
    return hipGetLastError();   // as the real helper does after hipLaunchKernelGGL
}

hipError_t launchMatchSelect(const MatchSelectArgs& args, hipStream_t stream) {
    if (!args.rows || !args.offsets || args.n < 1 || args.nPad < args.n || args.channels < 1 || args.channels > 4 || args.stat < 0 || args.stat > 1) return hipErrorInvalidValue;
    if (args.first < 0 || args.nRange < 1 || args.first > args.n - args.nRange || args.cap < 0 || (args.cap > 0 && !args.list) || args.threshold != args.threshold) return hipErrorInvalidValue;
    const MatchSelectArgs a = args;
    fxstubEnqueue(stream, [a] {
        unsigned long long found = 0;
        for (long long col = a.first; col < a.first + a.nRange; ++col) {
            const double v = valueOf(a.rows, a.nPad, a.channels, a.stat, col);
            if (a.below ? !(v < a.threshold) : !(v >= a.threshold)) continue;
            if (found < (unsigned long long)a.cap) a.list[found] = a.firstGlobal + (col - a.first);
            ++found;
        }
        a.offsets[meterSelectChunks(a.nRange)] = found;
        g_selects.fetch_add(1);
    });
    return hipGetLastError();
}

hipError_t launchMeterBest(const MeterBestArgs& args, hipStream_t stream) {
    if (!args.rows || !args.winner || !args.value || args.n < 1 || args.nPad < args.n || args.channels < 1 || args.channels > 4 || args.stat < 0 || args.stat > 1) return hipErrorInvalidValue;
    if (args.group < 1 || args.firstGlobal < 0 || args.firstGroup != args.firstGlobal / args.group || args.groups != (args.firstGlobal + args.n - 1) / args.group - args.firstGroup + 1) return hipErrorInvalidValue;
    const MeterBestArgs a = args;
    fxstubEnqueue(stream, [a] {
        for (long long g = 0; g < a.groups; ++g) {
            long long best = -1;
            double bestV = 0.0;
            // ascending: a later member takes over only when it is strictly better, so ties stay with the smallest number
            for (long long n = (a.firstGroup + g) * a.group; n < (a.firstGroup + g + 1) * a.group; ++n) {
                const long long col = n - a.firstGlobal;
                if (col < 0 || col >= a.n) continue;
                const double v = valueOf(a.rows, a.nPad, a.channels, a.stat, col);
                if (best < 0 || (a.largest ? v > bestV : v < bestV)) {
                    best = n;
                    bestV = v;
                }
            }
            a.winner[g] = best;
            a.value[g] = bestV;
        }
        g_bests.fetch_add(1);
    });
    return hipGetLastError();
}

hipError_t launchMatchZero(const MeterListArgs& args, hipStream_t stream) {
    if (!args.rows || !args.list || args.count < 1 || args.count >= ((long long)1 << 31) || args.n < 1 || args.nPad < args.n || args.channels < 1 || args.channels > 4) return hipErrorInvalidValue;
    const MeterListArgs a = args;
    fxstubEnqueue(stream, [a] {
        for (long long k = 0; k < a.count; ++k) {
            const long long inst = a.list[k];
            if (inst < 0 || inst >= a.n) { g_strays.fetch_add(1); continue; }
            for (int c = 0; c < a.channels; ++c)
                for (int stat = 0; stat < 2; ++stat) matchRow(a.rows, a.nPad, c, stat)[inst] = 0.0;
        }
        g_zeros.fetch_add(1);
    });
    return hipGetLastError();
}

}  // namespace fx
