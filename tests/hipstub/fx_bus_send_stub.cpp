// fx_bus_send_stub.cpp — host stand-in for launchBusSend of csrc/fx_bus.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).
// It does the real arithmetic in stream order on the stand-in's "device" memory, written from the definition in
// include/fx8010_amd.h ("Bus sends") with an addressing of its own: bus by bus, entry by entry in the order of the positions, a
// chunk being the positions q * 1024 .. q * 1024 + 1023 - the host's chunk table is only asked where a bus begins and how many
// entries it has, and is checked against that.  The chunk sums stay on the stack: `partial` is not used.
// Compiled with -ffp-contract=off like everything else; the volatiles round every intermediate to fp32 where the definition does.
#include <atomic>
#include <cstring>
#include <functional>
#include <vector>

#include "../../fx8010-emulator-core_amd/csrc/fx_bus.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_sends{0}, g_sendRamps{0}, g_badSends{0};

// T of the definition over seq[0 .. count - 1]
float tree(const float* seq, long long count) {
    volatile float p[64];
    for (int l = 0; l < 64; ++l) p[l] = 0.0f;
    for (long long m = 0; m < count; ++m) p[m % 64] = p[m % 64] + seq[m];
    for (int step = 32; step > 0; step >>= 1)
        for (int l = 0; l < step; ++l) p[l] = p[l] + p[l + step];
    return p[0];
}
}  // namespace

extern "C" long fxstub_bus_sends(void) { return g_sends.load(); }             // launches, ramping ones included
extern "C" long fxstub_bus_send_ramps(void) { return g_sendRamps.load(); }    // ... of those, the ones with a ramp pending
extern "C" long fxstub_bus_send_strays(void) { return g_badSends.load(); }    // members, columns or table rows out of range that a launch met (none is ever used)

namespace fx {

hipError_t launchBusSend(const BusSendArgs& args, hipStream_t stream) {
    if (!args.wide || !args.bus || !args.auxOut || args.rows < 1 || args.n < 1 || args.n >= ((long long)1 << 30) || args.buses < 1 || args.buses > 65536 ||
        args.auxPitch < args.buses || args.auxPitch > 65536 || args.entries < 0 || args.entries > ((long long)1 << 24) || args.chunks < 0 || args.chunks > args.entries ||
        (args.entries > 0) != (args.chunks > 0) || args.channels < 1 || args.rows % args.channels != 0 || args.samples < 1 || args.sample0 < 0 ||
        (long long)args.sample0 + args.rows / args.channels > (long long)args.samples)
        return hipErrorInvalidValue;
    if (args.chunks > 0 && (!args.idx || !args.target || (args.ramp && !args.current) || !args.chunk || !args.partial || args.gainPitch < args.entries)) return hipErrorInvalidValue;
    const BusSendArgs a = args;
    fxstubEnqueue(stream, [a] {
        std::vector<float> terms, sums;
        for (long long j = 0; j < a.buses; ++j) {
            const BusSendBus bus = a.bus[j];
            const long long column = a.columns ? (long long)bus.column : j;
            if (column >= a.auxPitch || (long long)bus.firstChunk + bus.chunks > a.chunks) {
                g_badSends.fetch_add(1);
                continue;
            }
            // the bus's run of entries: from its first chunk's first entry, as many as its chunks hold
            long long first = 0, count = 0;
            bool sound = true;
            for (uint32_t q = 0; q < bus.chunks; ++q) {
                const BusSendChunk ck = a.chunk[bus.firstChunk + q];
                if (q == 0) first = ck.first;
                sound = sound && (long long)ck.first == first + count && ck.count >= 1 && ck.count <= 1024 && (ck.count == 1024 || q + 1 == bus.chunks);
                count += ck.count;
            }
            if (!sound || first + count > a.entries) {
                g_badSends.fetch_add(1);
                continue;
            }
            for (long long m = 0; m < count; ++m)
                if (a.idx[first + m] >= (uint32_t)a.n) {
                    g_badSends.fetch_add(1);
                    sound = false;
                }
            if (!sound) continue;
            terms.resize((size_t)count);
            for (long long row = 0; row < a.rows; ++row) {
                const long long s = row / a.channels + a.sample0;   // sample of the call
                const int c = (int)(row % a.channels);
                const float* y = a.wide + row * a.n;
                for (long long m = 0; m < count; ++m) {
                    const long long e = first + m;
                    const float gb = a.target[(long long)c * a.gainPitch + e];
                    volatile float w = gb;
                    if (a.ramp && s != (long long)a.samples - 1) {
                        const float ga = a.current[(long long)c * a.gainPitch + e];
                        volatile float t = (float)(s + 1) * a.r;
                        volatile float d = gb - ga;
                        volatile float mul = d * t;
                        w = ga + mul;
                    }
                    volatile float term = 0.0f;
                    if (w != 0.0f) term = w * y[a.idx[e]];   // (either zero: +0.0f, whatever y holds)
                    terms[(size_t)m] = term;
                }
                sums.clear();
                for (long long m0 = 0; m0 < count; m0 += 1024) sums.push_back(tree(terms.data() + m0, count - m0 < 1024 ? count - m0 : 1024));
                const float word = sums.empty() ? 0.0f : (sums.size() == 1 ? sums[0] : tree(sums.data(), (long long)sums.size()));
                std::memcpy(a.auxOut + row * a.auxPitch + column, &word, 4);
            }
        }
        g_sends.fetch_add(1);
        if (a.ramp) g_sendRamps.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

}  // namespace fx
