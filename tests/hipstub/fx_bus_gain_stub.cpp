// fx_bus_gain_stub.cpp — host stand-in for launchBusMixGain of csrc/fx_bus.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).
// It does the real arithmetic in stream order on the stand-in's "device" memory, written from the definition in
// include/fx8010_amd.h ("Bus gains"), one (row, group, member) at a time: the row's sample of the CALL and its channel, the
// member's weight - b, or a + (b - a) * ((float)(s + 1) * r) with exactly b on the call's last sample - the muted term, then the
// order of the unweighted sum (64 partial sums taking the members j * 64 + l for j ascending, then the shuffle-down tree).
// Compiled with -ffp-contract=off like everything else; the volatiles round every intermediate to fp32 where the definition does.
#include <atomic>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_bus.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_gainMixes{0}, g_gainRamps{0};
}  // namespace

extern "C" long fxstub_bus_gain_mixes(void) { return g_gainMixes.load(); }   // launches, ramping ones included
extern "C" long fxstub_bus_gain_ramps(void) { return g_gainRamps.load(); }   // ... of those, the ones with a ramp pending

namespace fx {

hipError_t launchBusMixGain(const BusArgs& args, const BusGainArgs& gains, hipStream_t stream) {
    const bool badBus = args.rows < 1 || args.n < 1 || args.group < 1 || args.group > args.n || args.groups != (args.n + args.group - 1) / args.group ||
                        args.narrowPitch < args.groups || !args.wide || !args.narrowOut;
    const bool badGain = !gains.target || (gains.ramp && !gains.current) || gains.channels < 1 || args.rows % (gains.channels > 0 ? gains.channels : 1) != 0 ||
                         gains.gainPitch < args.n || gains.samples < 1 || gains.sample0 < 0;
    if (badBus || badGain || (long long)gains.sample0 + args.rows / gains.channels > (long long)gains.samples) return hipErrorInvalidValue;
    const BusArgs a = args;
    const BusGainArgs g = gains;
    fxstubEnqueue(stream, [a, g] {
        const long long pieceSamples = a.rows / g.channels;
        for (long long ps = 0; ps < pieceSamples; ++ps)
            for (int c = 0; c < g.channels; ++c) {
                const long long row = ps * g.channels + c;     // [sample of the piece][channel]
                const long long s = ps + g.sample0;            // sample of the call
                const float* y = a.wide + row * a.n;
                const float* ga = g.current ? g.current + (long long)c * g.gainPitch : nullptr;
                const float* gb = g.target + (long long)c * g.gainPitch;
                for (long long grp = 0; grp < a.groups; ++grp) {
                    const long long lo = grp * a.group, hi = lo + a.group < a.n ? lo + a.group : a.n;
                    volatile float p[64];
                    for (int l = 0; l < 64; ++l) p[l] = 0.0f;
                    for (long long i = lo; i < hi; ++i) {
                        volatile float w = gb[i];
                        if (g.ramp && s != (long long)g.samples - 1) {
                            volatile float t = (float)(s + 1) * g.r;
                            volatile float d = gb[i] - ga[i];
                            volatile float m = d * t;
                            w = ga[i] + m;
                        }
                        volatile float term = 0.0f;
                        if (w != 0.0f) term = w * y[i];   // (either zero: +0.0f, whatever y holds)
                        const int l = (int)((i - lo) % 64);
                        p[l] = p[l] + term;
                    }
                    for (int step = 32; step > 0; step >>= 1)
                        for (int l = 0; l < step; ++l) p[l] = p[l] + p[l + step];
                    a.narrowOut[row * a.narrowPitch + grp] = p[0];
                }
            }
        g_gainMixes.fetch_add(1);
        if (g.ramp) g_gainRamps.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

}  // namespace fx
