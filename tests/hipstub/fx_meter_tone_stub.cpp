// fx_meter_tone_stub.cpp — host stand-ins for the launch functions of the tone meters (csrc/fx_meter_tone.hip launchMeterTone /
// launchToneGather / launchToneZero, csrc/fx_meter_list.hip launchToneSelect, csrc/fx_meter_rank.hip launchToneRank; TEST
// INFRASTRUCTURE, see hip_stub.cpp).  They do the real arithmetic in stream order on the stand-in's "device" memory, written from
// the definition in include/fx8010_amd.h ("Tone meters") with a formulation of their own: the recurrence walks ONE column of one
// tone at a time through volatile doubles - every product, sum and difference a value of its own, rounded once - where the kernel
// interleaves the K chains of a lane; the select is one loop that appends, the rank one stable sort, both comparing in long
// double.  The power is csrc/fx_meter_tone.hpp tonePower, the one function that defines it.  Compiled with -ffp-contract=off like
// everything else.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "../../fx8010-emulator-core_amd/csrc/fx_meter_tone.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_tones{0}, g_selects{0}, g_gathers{0}, g_zeros{0}, g_ranks{0}, g_strays{0};

int headerTones(const void* block) {
    long long k;
    std::memcpy(&k, static_cast<const char*>(block) + fx::kToneCountOff, 8);
    return (int)k;
}
double headerCoeff(const void* block, int tone) {
    double c;
    std::memcpy(&c, static_cast<const char*>(block) + 8 * (size_t)tone, 8);
    return c;
}
double* s1Row(const void* block, long long nPad, int tones, int channel, int tone) {
    return reinterpret_cast<double*>(static_cast<char*>(const_cast<void*>(block)) + fx::toneRowOff(nPad, tones, channel, tone));
}
double value(const void* block, long long nPad, int channels, int tone, long long col) {
    const int tones = headerTones(block);
    const double c = headerCoeff(block, tone);
    double best = 0.0;
    for (int ch = 0; ch < channels; ++ch) {
        const double* s1 = s1Row(block, nPad, tones, ch, tone);
        const double v = fx::tonePower(c, s1[col], s1[nPad + col]);
        if (ch == 0 || (long double)v > (long double)best) best = v;
    }
    return best;
}
bool badList(const fx::MeterListArgs& a, bool gather) {
    if (!a.rows || !a.list || a.count < 1 || a.count >= ((long long)1 << 31) || a.n < 1 || a.nPad < a.n || a.channels < 1 || a.channels > 4) return true;
    return gather && !a.packed;
}
void columns(const fx::MeterListArgs& a, bool gather) {
    const int tones = headerTones(a.rows);
    const size_t part = (size_t)tones * (size_t)a.channels * (size_t)a.count;
    double* packed = static_cast<double*>(a.packed);
    for (long long k = 0; k < a.count; ++k) {
        const long long inst = a.list[k];
        if (inst < 0 || inst >= a.n) { g_strays.fetch_add(1); continue; }
        for (int t = 0; t < tones; ++t) {
            for (int ch = 0; ch < a.channels; ++ch) {
                double* s1 = s1Row(a.rows, a.nPad, tones, ch, t) + inst;
                double* s2 = s1 + a.nPad;
                if (gather) {
                    const size_t at = ((size_t)t * (size_t)a.channels + (size_t)ch) * (size_t)a.count + (size_t)k;
                    packed[at] = *s1;
                    packed[part + at] = *s2;
                    packed[2 * part + at] = fx::tonePower(headerCoeff(a.rows, t), *s1, *s2);
                }
                if (!gather || a.reset) *s1 = *s2 = 0.0;
            }
        }
    }
}
}  // namespace

extern "C" long fxstub_meter_tone_launches(void) { return g_tones.load(); }
extern "C" long fxstub_tone_selects(void) { return g_selects.load(); }
extern "C" long fxstub_tone_gathers(void) { return g_gathers.load(); }
extern "C" long fxstub_tone_zeros(void) { return g_zeros.load(); }
extern "C" long fxstub_tone_ranks(void) { return g_ranks.load(); }
extern "C" long fxstub_tone_strays(void) { return g_strays.load(); }   // list entries out of range that a launch met (none is followed)

namespace fx {

hipError_t launchMeterTone(const MeterToneArgs& args, hipStream_t stream) {
    if (!args.y || !args.block || args.n < 1 || args.nPad < args.n || args.pitch < args.n || args.samples < 1 || args.channels < 1 || args.channels > 4) return hipErrorInvalidValue;
    if ((unsigned long long)args.channels * (unsigned long long)args.pitch * 4u >= (1ull << 32)) return hipErrorInvalidValue;
    if (args.tones < 1 || args.tones > kMeterMaxTones) return hipErrorInvalidValue;
    for (int k = 0; k < args.tones; ++k)
        if (!(args.coeff[k] >= -2.0 && args.coeff[k] <= 2.0) || (args.coeff[k] == 0.0 && std::signbit(args.coeff[k]))) return hipErrorInvalidValue;
    const MeterToneArgs a = args;
    fxstubEnqueue(stream, [a] {
        for (int ch = 0; ch < a.channels; ++ch) {
            for (int t = 0; t < a.tones; ++t) {
                double* row1 = s1Row(a.block, a.nPad, a.tones, ch, t);
                double* row2 = row1 + a.nPad;
                for (long long i = 0; i < a.n; ++i) {
                    double s1 = row1[i], s2 = row2[i];
                    for (int s = 0; s < a.samples; ++s) {
                        const float y = a.y[((size_t)s * (size_t)a.channels + (size_t)ch) * (size_t)a.pitch + (size_t)i];
                        const double x = std::isfinite(y) ? (double)y : 0.0;
                        const volatile double p = a.coeff[t] * s1;   // (volatile: a value of its own, rounded to fp64 once)
                        const volatile double q = x + p;
                        const volatile double s0 = q - s2;
                        s2 = s1;
                        s1 = s0;
                    }
                    row1[i] = s1;
                    row2[i] = s2;
                }
            }
        }
        g_tones.fetch_add(1);
    });
    return hipGetLastError();   // as the real helper does after hipLaunchKernelGGL
}

hipError_t launchToneSelect(const ToneSelectArgs& args, hipStream_t stream) {
    if (!args.rows || !args.offsets || args.n < 1 || args.nPad < args.n || args.channels < 1 || args.channels > 4 || args.stat < 0 || args.stat >= kMeterMaxTones) return hipErrorInvalidValue;
    if (args.first < 0 || args.nRange < 1 || args.first > args.n - args.nRange || args.cap < 0 || (args.cap > 0 && !args.list) || args.threshold != args.threshold) return hipErrorInvalidValue;
    const ToneSelectArgs a = args;
    fxstubEnqueue(stream, [a] {
        unsigned long long found = 0;
        const long double t = a.threshold;
        for (long long col = a.first; col < a.first + a.nRange; ++col) {
            const long double v = value(a.rows, a.nPad, a.channels, a.stat, col);
            if (a.below ? !(v < t) : !(v >= t)) continue;
            if (found < (unsigned long long)a.cap) a.list[found] = a.firstGlobal + (col - a.first);
            ++found;
        }
        a.offsets[meterSelectChunks(a.nRange)] = found;
        g_selects.fetch_add(1);
    });
    return hipGetLastError();
}

hipError_t launchToneRank(const MeterRankArgs& args, hipStream_t stream) {
    if (!args.rows || !args.stage || args.n < 1 || args.nPad < args.n || args.channels < 1 || args.channels > 4 || args.family != kRankTone) return hipErrorInvalidValue;
    if (args.stat < 0 || args.stat >= kMeterMaxTones) return hipErrorInvalidValue;
    if (args.first < 0 || args.nRange < 1 || args.first > args.n - args.nRange || args.k < 0 || args.room != std::min(args.k, args.nRange) || args.threshold != args.threshold) return hipErrorInvalidValue;
    const MeterRankArgs a = args;
    fxstubEnqueue(stream, [a] {
        struct Item { long double v; double word; long long n; };
        std::vector<Item> items;
        const long double t = a.threshold;
        for (long long col = a.first; col < a.first + a.nRange; ++col) {
            const double v = value(a.rows, a.nPad, a.channels, a.stat, col);
            if (a.below ? !((long double)v < t) : !((long double)v >= t)) continue;
            items.push_back(Item{(long double)v, v, a.firstGlobal + (col - a.first)});
        }
        const bool largest = a.largest != 0;
        std::stable_sort(items.begin(), items.end(), [largest](const Item& x, const Item& y) { return largest ? x.v > y.v : x.v < y.v; });
        const unsigned long long m = items.size(), r = std::min<unsigned long long>(m, (unsigned long long)a.room);
        a.stage[0] = m;
        a.stage[1] = r;
        for (unsigned long long i = 0; i < r; ++i) {
            a.stage[rankPairsOff() + 2 * i] = (unsigned long long)items[i].n;
            std::memcpy(&a.stage[rankPairsOff() + 2 * i + 1], &items[i].word, 8);
        }
        g_ranks.fetch_add(1);
    });
    return hipGetLastError();
}

hipError_t launchToneGather(const MeterListArgs& args, hipStream_t stream) {
    if (badList(args, true)) return hipErrorInvalidValue;
    const MeterListArgs a = args;
    fxstubEnqueue(stream, [a] {
        columns(a, true);
        g_gathers.fetch_add(1);
    });
    return hipGetLastError();
}

hipError_t launchToneZero(const MeterListArgs& args, hipStream_t stream) {
    if (badList(args, false)) return hipErrorInvalidValue;
    const MeterListArgs a = args;
    fxstubEnqueue(stream, [a] {
        columns(a, false);
        g_zeros.fetch_add(1);
    });
    return hipGetLastError();
}

}  // namespace fx
