// meter_rank_checks.cpp — the meter ranks of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan +
// LeakSanitizer (TEST INFRASTRUCTURE: csrc/Makefile `stubasanmeterrank` links this file with the library's host sources and
// tests/hipstub/; a program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The comparison with the numpy model is tests/test_meter_rank_stub.py; this program is about addresses.  `list` and `value` are
// heap blocks of exactly R = min(M, k) words - the call may touch nothing beyond R, so one word more is a report - and every
// "device" block of the stand-in is a heap block too: a read or write outside the rows, a shard's part of them or the staging is
// a report as well.  It walks N = 1, 5, 65, 200 and 777 on one handle and N = 808 on three shards (their starts are 320 and 576)
// with one, two and four channels; the three families and their stats; the four flag combinations; k of 0, 1, R - 1, R, R + 1 and
// beyond N; ranges that start inside a wavefront and cross the shard borders; the refusals (nothing changes); and an allocation
// failure at each staging allocation.  What comes back is checked against a plain selection written from the definition in
// include/fx8010_amd.h "Meter ranks" over the rows the read calls return.  Exit code 0 = every check held (a sanitizer report turns
// it non-zero).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../include/fx8010_amd.h"
#include "hip_stub.h"

extern "C" long fxstub_meter_ranks(void);   // fx_meter_rank_stub.cpp

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            ++g_failures;                                                                \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                                \
    } while (0)

std::string program(int channels) {
    std::string decl = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\n", code = "macs a, a, vol, in\nmacs out, a, in, 0.25\n";
    for (int c = 1; c < channels; ++c) {
        const std::string k = std::to_string(c);
        decl += "input in" + k + " " + k + "\noutput out" + k + " " + k + "\n";
        code += "macs out" + k + ", in" + k + ", a, 0.5\n";
    }
    return decl + code + "end";
}

uint32_t g_seed = 24680u;
uint32_t draw() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}
// few distinct levels, so that ties are the rule; silence, the rail, a NaN and an infinity among them
float word() {
    const uint32_t d = draw(), kind = (d >> 4) % 16;
    return kind < 5 ? 0.0f : kind == 5 ? 1.0f : kind == 6 ? -0.5f : kind == 7 ? std::numeric_limits<float>::quiet_NaN() : kind == 8 ? -std::numeric_limits<float>::infinity()
                                                                                                                         : (float)((int)((d >> 8) % 9) - 4) / 4.0f;
}

typedef int64_t (*RankCall)(fxb_handle*, int, int64_t, double, int64_t, int64_t, int64_t*, double*, unsigned);
const RankCall kCalls[3] = {fxb_meter_rank, fxb_meter_rank_match, fxb_meter_rank_level};
const int kStats[3] = {4, 2, 2};
const int kCounters[3] = {FXB_INFO_METER_RANKS, FXB_INFO_METER_MATCH_RANKS, FXB_INFO_METER_LEVEL_RANKS};

fxb_handle* create(int64_t n, int channels, int devices, bool modes) {
    static const int three[3] = {0, 1, 2};
    fxb_handle* h = devices > 1 ? fxb_create_on_devices(n, channels, three, 3) : fxb_create(n, channels, 0);
    CHECK(h != nullptr);
    if (!h) std::exit(2);
    CHECK(fxb_load_text(h, program(channels).c_str()) == 1);
    CHECK(fxb_meter_enable(h, 1) == 0);
    if (modes) {
        const size_t words = 4 * (size_t)channels * (size_t)n;
        std::unique_ptr<float[]> target(new float[words]);
        for (size_t i = 0; i < words; ++i) target[i] = (float)((int)(draw() % 5) - 2) / 2.0f;
        CHECK(fxb_meter_set_target(h, target.get(), 4, 1, FXB_METER_TARGET_LOOP) == 0);
        CHECK(fxb_meter_set_level(h, 0.5f, 0.25f, 0) == 0);
    }
    return h;
}

void play(fxb_handle* h, int channels, int64_t n, int samples) {
    const size_t words = (size_t)samples * (size_t)channels * (size_t)n;
    std::unique_ptr<float[]> in(new float[words]), out(new float[words]);
    for (size_t i = 0; i < words; ++i) in[i] = word();
    CHECK(fxb_process_block(h, in.get(), out.get(), samples) == 0);
}

// V(n) of every instance for (family, stat), from the rows the read calls return
std::vector<double> values(fxb_handle* h, int family, int stat, int channels, int64_t n) {
    const size_t k = (size_t)channels * (size_t)n;
    std::vector<double> v((size_t)n);
    if (family == 0) {
        std::unique_ptr<double[]> e(new double[k]);
        std::unique_ptr<float[]> p(new float[k]);
        std::unique_ptr<uint32_t[]> f(new uint32_t[k]), q(new uint32_t[k]);
        CHECK(fxb_meter_read(h, e.get(), p.get(), f.get(), q.get(), 0) == 0);
        for (int64_t i = 0; i < n; ++i)
            for (int c = 0; c < channels; ++c) {
                const size_t at = (size_t)c * (size_t)n + (size_t)i;
                const double w = stat == 0 ? e[at] : stat == 1 ? (double)p[at] : stat == 2 ? (double)f[at] : (double)q[at];
                v[(size_t)i] = c == 0 ? w : std::max(v[(size_t)i], w);
            }
    } else if (family == 1) {
        std::unique_ptr<double[]> e(new double[k]), x(new double[k]);
        CHECK(fxb_meter_read_match(h, e.get(), x.get(), 0) == 0);
        for (int64_t i = 0; i < n; ++i)
            for (int c = 0; c < channels; ++c) {
                const double w = (stat == 0 ? e : x)[(size_t)c * (size_t)n + (size_t)i];
                v[(size_t)i] = c == 0 ? w : v[(size_t)i] + w;
            }
    } else {
        std::unique_ptr<float[]> l(new float[k]);
        std::unique_ptr<uint32_t[]> q(new uint32_t[k]);
        CHECK(fxb_meter_read_level(h, l.get(), q.get(), 0) == 0);
        for (int64_t i = 0; i < n; ++i)
            for (int c = 0; c < channels; ++c) {
                const size_t at = (size_t)c * (size_t)n + (size_t)i;
                const double w = stat == 0 ? (double)l[at] : (double)q[at];
                v[(size_t)i] = c == 0 ? w : stat == 0 ? std::max(v[(size_t)i], w) : std::min(v[(size_t)i], w);
            }
    }
    return v;
}

// the definition: the candidates of the range, the smallest (V, n) taken out one after the other
std::vector<int64_t> wanted(const std::vector<double>& v, int64_t k, double t, bool below, bool largest, int64_t first, int64_t nRange, int64_t* m) {
    std::vector<int64_t> cand, out;
    for (int64_t i = first; i < first + nRange; ++i)
        if (below ? v[(size_t)i] < t : v[(size_t)i] >= t) cand.push_back(i);
    *m = (int64_t)cand.size();
    std::vector<char> taken(cand.size(), 0);
    while ((int64_t)out.size() < std::min<int64_t>(k, *m)) {
        size_t best = cand.size();
        for (size_t j = 0; j < cand.size(); ++j) {
            if (taken[j]) continue;
            if (best == cand.size()) { best = j; continue; }
            const double a = v[(size_t)cand[j]], b = v[(size_t)cand[best]];
            if (largest ? a > b : a < b) best = j;   // (strictly: of equal values the earlier - smaller - number stays)
        }
        taken[best] = 1;
        out.push_back(cand[best]);
    }
    return out;
}

void rankOnce(fxb_handle* h, int family, int stat, const std::vector<double>& v, int64_t k, double t, unsigned flags, int64_t first, int64_t nRange, bool withValues) {
    int64_t m = 0;
    const std::vector<int64_t> want = wanted(v, k, t, (flags & FXB_METER_BELOW) != 0, (flags & FXB_METER_LARGEST) != 0, first, nRange, &m);
    const size_t r = want.size();
    std::unique_ptr<int64_t[]> list(k > 0 ? new int64_t[r] : nullptr);   // (k > 0 with M == 0: a block of no words, not a null pointer)
    std::unique_ptr<double[]> value(withValues ? new double[r] : nullptr);
    const int64_t got = kCalls[family](h, stat, k, t, first, nRange, list.get(), value.get(), flags);
    CHECK(got == m);
    for (size_t i = 0; i < r; ++i) {
        CHECK(list[i] == want[i]);
        if (withValues) CHECK(std::memcmp(&value[i], &v[(size_t)want[i]], 8) == 0);
    }
}

void indexing(int devices) {
    const int64_t single[5] = {1, 5, 65, 200, 777}, sharded[1] = {808};
    const int64_t* sizes = devices > 1 ? sharded : single;
    const int nSizes = devices > 1 ? 1 : 5;
    for (int s = 0; s < nSizes; ++s)
        for (int channels = 1; channels <= 4; channels *= 2) {
            const int64_t n = sizes[s];
            fxb_handle* h = create(n, channels, devices, true);
            play(h, channels, n, 9);
            play(h, channels, n, 4);
            int64_t launched[3] = {0, 0, 0};
            for (int family = 0; family < 3; ++family)
                for (int stat = 0; stat < kStats[family]; ++stat) {
                    const std::vector<double> v = values(h, family, stat, channels, n);
                    const double ts[3] = {-INFINITY, v[(size_t)(n / 2)], INFINITY};
                    for (unsigned flags = 0; flags < 4; ++flags)
                        for (const double t : ts) {
                            int64_t m = 0;
                            wanted(v, 0, t, (flags & 1u) != 0, false, 0, n, &m);
                            const int64_t ks[6] = {0, 1, std::max<int64_t>(m - 1, 0), m, m + 1, n + 5};
                            for (const int64_t k : ks) rankOnce(h, family, stat, v, k, t, flags, 0, n, (k & 1) == 0);
                            launched[family] += 6 * devices;
                            const int64_t firsts[4] = {1 % n, std::min<int64_t>(63, n - 1), n / 2, n == 808 ? 319 : n - 1};
                            for (const int64_t first : firsts) {
                                const int64_t count = n == 808 && first == 319 ? 258 : n - first;
                                rankOnce(h, family, stat, v, 3, t, flags, first, count, true);
                                rankOnce(h, family, stat, v, count, t, flags, first, count, false);
                            }
                            rankOnce(h, family, stat, v, 4, t, flags, n / 2, 0, true);   // an empty range: nothing is launched
                        }
                }
            if (devices == 1)
                for (int family = 0; family < 3; ++family) CHECK(fxb_info(h, kCounters[family]) == launched[family] + kStats[family] * 4 * 3 * 8);
            fxb_destroy(h);
        }
}

void refusals(int devices) {
    const int64_t n = devices > 1 ? 808 : 200;
    std::unique_ptr<int64_t[]> list(new int64_t[3]);
    std::unique_ptr<double[]> value(new double[3]);
    for (int i = 0; i < 3; ++i) list[i] = -77, value[i] = -77.0;
    // the modes off: metering, the target, the level meters - also with nothing to do
    fxb_handle* h = create(n, 2, devices, false);
    play(h, 2, n, 8);
    CHECK(fxb_meter_rank_match(h, 0, 3, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG && fxb_meter_rank_level(h, 0, 3, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG);
    CHECK(fxb_meter_rank_match(h, 0, 0, 0.0, 0, 0, nullptr, nullptr, 0) == FX_E_ARG && fxb_meter_rank_level(h, 0, 0, 0.0, 0, 0, nullptr, nullptr, 0) == FX_E_ARG);
    CHECK(fxb_meter_rank(h, 1, 3, 0.0, 0, n, list.get(), value.get(), 0) == n);
    for (int i = 0; i < 3; ++i) list[i] = -77, value[i] = -77.0;
    CHECK(fxb_meter_enable(h, 0) == 0 && fxb_meter_rank(h, 1, 3, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG && fxb_meter_rank(h, 1, 0, 0.0, 0, 0, nullptr, nullptr, 0) == FX_E_ARG);
    fxb_destroy(h);
    h = create(n, 2, devices, true);
    play(h, 2, n, 8);
    const long ranks = fxstub_meter_ranks();
    for (int family = 0; family < 3; ++family) {
        const RankCall call = kCalls[family];
        CHECK(call(h, kStats[family], 3, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG && call(h, -1, 3, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG);
        CHECK(call(h, 0, 3, std::nan(""), 0, n, list.get(), value.get(), 0) == FX_E_ARG && call(h, 0, 3, 0.0, -1, 2, list.get(), value.get(), 0) == FX_E_ARG);
        CHECK(call(h, 0, 3, 0.0, 1, n, list.get(), value.get(), 0) == FX_E_ARG && call(h, 0, 3, 0.0, n, INT64_MAX, list.get(), value.get(), 0) == FX_E_ARG);
        CHECK(call(h, 0, 3, 0.0, 0, -1, list.get(), value.get(), 0) == FX_E_ARG && call(h, 0, -1, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG);
        CHECK(call(h, 0, 3, 0.0, 0, n, nullptr, value.get(), 0) == FX_E_ARG && call(h, 0, 3, 0.0, 0, n, list.get(), value.get(), 4u) == FX_E_ARG);
        CHECK(call(nullptr, 0, 3, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG && fxb_last_error(h)[0] != 0);
        CHECK(call(h, 0, 3, 0.0, n, 0, list.get(), value.get(), 3u) == 0);   // an empty range at the very end
        CHECK(fxb_info(h, kCounters[family]) == 0);
    }
    CHECK(fxstub_meter_ranks() == ranks);
    for (int i = 0; i < 3; ++i) CHECK(list[i] == -77 && value[i] == -77.0);
    fxb_destroy(h);
}

// an allocation that fails, at each staging allocation of the call (the device block and the pinned block, per shard): FX_E_MEMORY,
// nothing launched and nothing written, then the call goes through
void memory(int devices) {
    const int64_t n = devices > 1 ? 808 : 200;
    for (int nth = 0; nth < 2 * devices; ++nth) {
        fxb_handle* h = create(n, 2, devices, true);
        play(h, 2, n, 8);
        CHECK(fxb_prepare(h, 8, 1) == 0);   // (the builder threads are idle: no allocation of their own meets the injected failure)
        std::unique_ptr<int64_t[]> list(new int64_t[5]);
        std::unique_ptr<double[]> value(new double[5]);
        for (int i = 0; i < 5; ++i) list[i] = -77, value[i] = -77.0;
        const long ranks = fxstub_meter_ranks();
        fxstub_fail_mallocs(nth, 1);
        const int64_t rc = fxb_meter_rank_level(h, 0, 5, -INFINITY, 0, n, list.get(), value.get(), FXB_METER_LARGEST);
        fxstub_fail_mallocs(-1, 0);
        CHECK(rc == FX_E_MEMORY && fxb_last_error(h)[0] != 0 && fxstub_meter_ranks() == ranks && fxb_info(h, FXB_INFO_METER_LEVEL_RANKS) == 0);
        for (int i = 0; i < 5; ++i) CHECK(list[i] == -77 && value[i] == -77.0);
        const std::vector<double> v = values(h, 2, 0, 2, n);
        rankOnce(h, 2, 0, v, 5, -INFINITY, FXB_METER_LARGEST, 0, n, true);
        CHECK(fxb_info(h, FXB_INFO_METER_LEVEL_RANKS) == devices);
        fxb_destroy(h);
    }
}

}  // namespace

int main() {
    setenv("FXSTUB_DEVICES", "3", 1);   // (read by the stand-in at its first call)
    for (int devices = 1; devices <= 3; devices += 2) {
        indexing(devices);
        refusals(devices);
        memory(devices);
        std::printf("  meter ranks, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "meter rank checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("meter rank checks ok\n");
    return 0;
}
