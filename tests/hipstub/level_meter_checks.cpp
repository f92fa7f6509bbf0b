// level_meter_checks.cpp — the level meters of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan +
// LeakSanitizer (TEST INFRASTRUCTURE: csrc/Makefile `stubasanmeterlevel` links this file with the library's host sources and
// tests/hipstub/; a program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The comparison with the numpy model is tests/test_meter_level_stub.py; this program is about addresses.  Every array the caller
// hands in is a heap block of exactly the documented size - [channels][N] per level row, [count] list entries and
// [channels][count] per gathered row, [cap] instance numbers of a select - and every "device" block of the stand-in is a heap
// block too, so a read or write one word outside the level rows, a shard's part of them, the staging or an output is a report.
// It walks N = 1, 5, 65, 200 and 777 on one handle and N = 808 on three shards (their starts are 320 and 576) with one, two and
// four channels; the four parameter pairs; caps of M, M - 1, M + 1, 1 and 0; lists of one entry, with repeats, and one entry per
// shard; the refusals (nothing changes); and an allocation failure at each allocation of a set.  What comes back is checked with
// plain loops written from the definition in include/fx8010_amd.h "Level meters".  Exit code 0 = every check held (a sanitizer
// report turns it non-zero).
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

extern "C" long fxstub_level_strays(void);   // fx_meter_level_stub.cpp

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

uint32_t g_seed = 13579u;
uint32_t draw() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}
float word() {
    const uint32_t d = draw(), kind = (d >> 4) % 16;
    return kind < 6 ? 0.0f : kind == 6 ? 1.0f : kind == 7 ? -0.0f : kind == 8 ? std::numeric_limits<float>::quiet_NaN() : kind == 9 ? -std::numeric_limits<float>::infinity()
                                                                                                                          : (float)((int)((d >> 8) % 2000) - 1000) / 1000.0f;
}

fxb_handle* create(int64_t n, int channels, int devices) {
    static const int three[3] = {0, 1, 2};
    fxb_handle* h = devices > 1 ? fxb_create_on_devices(n, channels, three, 3) : fxb_create(n, channels, 0);
    CHECK(h != nullptr);
    if (!h) std::exit(2);
    CHECK(fxb_load_text(h, program(channels).c_str()) == 1);
    CHECK(fxb_meter_enable(h, 1) == 0);
    return h;
}

// the model: the level rows of one handle, by the definition (this file is compiled with -ffp-contract=off)
struct Level {
    int channels = 0;
    int64_t n = 0;
    float release = 0.0f, floor = 0.0f;
    std::vector<float> level;
    std::vector<uint32_t> quiet;
    void set(int ch, int64_t N) {
        channels = ch, n = N;
        level.assign((size_t)ch * (size_t)N, 0.0f);
        quiet.assign((size_t)ch * (size_t)N, 0u);
    }
    void take(const float* y, int samples) {
        for (int s = 0; s < samples; ++s)
            for (int c = 0; c < channels; ++c)
                for (int64_t i = 0; i < n; ++i) {
                    const float yw = y[((size_t)s * (size_t)channels + (size_t)c) * (size_t)n + (size_t)i];
                    const size_t at = (size_t)c * (size_t)n + (size_t)i;
                    const bool fin = std::fabs(yw) < INFINITY;
                    const float w = fin ? std::fabs(yw) : 0.0f;
                    volatile float d = level[at] * release;
                    const float dv = d;
                    level[at] = w > dv ? w : dv;
                    quiet[at] = (!fin || w >= floor) ? 0u : quiet[at] == 0xffffffffu ? quiet[at] : quiet[at] + 1u;
                }
    }
    double value(int stat, int64_t i) const {
        double v = stat == 0 ? (double)level[(size_t)i] : (double)quiet[(size_t)i];
        for (int c = 1; c < channels; ++c) {
            const size_t at = (size_t)c * (size_t)n + (size_t)i;
            v = stat == 0 ? std::max(v, (double)level[at]) : std::min(v, (double)quiet[at]);
        }
        return v;
    }
    void zero(int64_t i) {
        for (int c = 0; c < channels; ++c) {
            level[(size_t)c * (size_t)n + (size_t)i] = 0.0f;
            quiet[(size_t)c * (size_t)n + (size_t)i] = 0u;
        }
    }
};

void setLevel(fxb_handle* h, Level& m, float release, float floor) {
    CHECK(fxb_meter_set_level(h, release, floor, 0) == 0);
    m.release = release, m.floor = floor;
    std::unique_ptr<float[]> r(new float[1]), f(new float[1]);
    CHECK(fxb_meter_get_level(h, r.get(), f.get()) == 0 && r[0] == release && f[0] == floor);
    CHECK(fxb_meter_get_level(h, nullptr, f.get()) == 0 && fxb_meter_get_level(h, r.get(), nullptr) == 0);
}

void play(fxb_handle* h, Level& m, int samples) {
    const size_t words = (size_t)samples * (size_t)m.channels * (size_t)m.n;
    std::unique_ptr<float[]> in(new float[words]), out(new float[words]);
    for (size_t i = 0; i < words; ++i) in[i] = word();
    CHECK(fxb_process_block(h, in.get(), out.get(), samples) == 0);
    m.take(out.get(), samples);   // (the stand-in's emulation launch copies input to output)
}

void compare(fxb_handle* h, const Level& m) {
    const size_t k = (size_t)m.channels * (size_t)m.n;
    std::unique_ptr<float[]> l(new float[k]);
    std::unique_ptr<uint32_t[]> q(new uint32_t[k]);
    CHECK(fxb_meter_read_level(h, l.get(), q.get(), 0) == 0);
    CHECK(std::memcmp(l.get(), m.level.data(), k * 4) == 0);
    CHECK(std::memcmp(q.get(), m.quiet.data(), k * 4) == 0);
    CHECK(fxb_meter_read_level(h, nullptr, q.get(), 0) == 0 && fxb_meter_read_level(h, l.get(), nullptr, 0) == 0 && fxb_meter_read_level(h, nullptr, nullptr, 0) == 0);
}

void selectOnce(fxb_handle* h, const Level& m, int stat, double t, bool below, int64_t first, int64_t nRange, int64_t cap) {
    std::vector<int64_t> want;
    for (int64_t i = first; i < first + nRange; ++i)
        if (below ? m.value(stat, i) < t : m.value(stat, i) >= t) want.push_back(i);
    std::unique_ptr<int64_t[]> list(cap > 0 ? new int64_t[(size_t)cap] : nullptr);
    for (int64_t i = 0; i < cap; ++i) list[(size_t)i] = -77;
    const int64_t got = fxb_meter_select_level(h, stat, t, first, nRange, list.get(), cap, below ? FXB_METER_BELOW : 0u);
    CHECK(got == (int64_t)want.size());
    const int64_t take = std::min<int64_t>(cap, (int64_t)want.size());
    for (int64_t i = 0; i < cap; ++i) CHECK(list[(size_t)i] == (i < take ? want[(size_t)i] : -77));
}

void queries(fxb_handle* h, const Level& m) {
    const int64_t n = m.n;
    for (int stat = 0; stat < 2; ++stat) {
        const double mid = m.value(stat, n / 2), ts[4] = {-INFINITY, mid, std::nextafter(mid, INFINITY), INFINITY};
        for (const double t : ts)
            for (int below = 0; below < 2; ++below) {
                int64_t M = 0;
                for (int64_t i = 0; i < n; ++i) M += (below ? m.value(stat, i) < t : m.value(stat, i) >= t) ? 1 : 0;
                const int64_t caps[5] = {M, std::max<int64_t>(M - 1, 0), M + 1, 1, 0};
                for (const int64_t cap : caps) selectOnce(h, m, stat, t, below != 0, 0, n, cap);
                const int64_t firsts[4] = {1 % n, std::min<int64_t>(63, n), std::min<int64_t>(64, n), n / 2};
                for (const int64_t first : firsts) selectOnce(h, m, stat, t, below != 0, first, n - first, (n - first) / 2);
            }
    }
}

// a list read on exactly-sized blocks: [count] entries, [channels][count] per row
void readList(fxb_handle* h, Level& m, const std::vector<int64_t>& entries, bool reset) {
    const size_t count = entries.size(), k = (size_t)m.channels * count;
    std::unique_ptr<int64_t[]> list(new int64_t[count]);
    std::copy(entries.begin(), entries.end(), list.get());
    std::unique_ptr<float[]> l(new float[k]);
    std::unique_ptr<uint32_t[]> q(new uint32_t[k]);
    CHECK(fxb_meter_read_level_list(h, list.get(), (int64_t)count, l.get(), q.get(), reset ? 1 : 0) == 0);
    for (int c = 0; c < m.channels; ++c)
        for (size_t i = 0; i < count; ++i) {
            const size_t at = (size_t)c * (size_t)m.n + (size_t)entries[i];
            CHECK(std::memcmp(&l[(size_t)c * count + i], &m.level[at], 4) == 0 && q[(size_t)c * count + i] == m.quiet[at]);
        }
    if (reset)
        for (const int64_t i : entries) m.zero(i);
    else
        CHECK(fxb_meter_read_level_list(h, list.get(), (int64_t)count, nullptr, q.get(), 0) == 0 && fxb_meter_read_level_list(h, list.get(), (int64_t)count, l.get(), nullptr, 0) == 0);
}

void indexing(int devices) {
    const int64_t single[5] = {1, 5, 65, 200, 777}, sharded[1] = {808};
    const int64_t* sizes = devices > 1 ? sharded : single;
    const int nSizes = devices > 1 ? 1 : 5;
    const float params[4][2] = {{0.5f, 0.25f}, {1.0f, 0.0f}, {0.0f, 1.0f}, {0.999f, 1e-4f}};
    for (int s = 0; s < nSizes; ++s)
        for (int channels = 1; channels <= 4; channels *= 2) {
            const int64_t n = sizes[s];
            fxb_handle* h = create(n, channels, devices);
            Level m;
            m.set(channels, n);
            for (int p = 0; p < 4; ++p) {
                setLevel(h, m, params[p][0], params[p][1]);   // (after the first: the parameters alone, the accumulators stay)
                play(h, m, 9);
                play(h, m, 4);
                compare(h, m);
                if (p == 0 || p == 3) queries(h, m);
                // lists: one entry, repeats, the ends and the middle (on three shards: one entry per shard and more)
                readList(h, m, {n - 1}, false);
                readList(h, m, {n - 1, 0, n / 2, 0, n - 1}, false);
                if (n == 808) readList(h, m, {319, 320, 575, 576, 807, 0}, true);
                readList(h, m, {n / 2}, true);
                compare(h, m);
                // a list reset on an exactly-sized list; read_level with reset
                const int64_t count = std::min<int64_t>(n, 3);
                {
                    std::unique_ptr<int64_t[]> l(new int64_t[(size_t)count]);
                    for (int64_t i = 0; i < count; ++i) l[(size_t)i] = i == 0 ? n - 1 : i == 1 ? 0 : n / 2;
                    CHECK(fxb_meter_reset_list(h, l.get(), count) == 0);
                    for (int64_t i = 0; i < count; ++i) m.zero(l[(size_t)i]);
                }
                compare(h, m);
                play(h, m, 3);
                CHECK(fxb_meter_read_level(h, nullptr, nullptr, 1) == 0);
                m.set(channels, n);
                play(h, m, 2);
                compare(h, m);
            }
            // (four blocks per parameter pair, each metered by one launch per shard)
            CHECK(fxb_info(h, FXB_INFO_METER_LEVEL_LAUNCHES) == 4 * 4 * devices && fxb_info(h, FXB_INFO_METER_LAUNCHES) == 4 * 4 * devices);
            CHECK(fxb_meter_clear_level(h) == 0 && fxb_meter_get_level(h, nullptr, nullptr) == FX_E_ARG);
            fxb_destroy(h);
        }
}

void refusals(int devices) {
    const int64_t n = devices > 1 ? 808 : 200;
    fxb_handle* h = create(n, 2, devices);
    Level m;
    m.set(2, n);
    std::unique_ptr<int64_t[]> list(new int64_t[3]);
    std::unique_ptr<float[]> l(new float[2 * (size_t)n]);
    std::unique_ptr<uint32_t[]> q(new uint32_t[2 * (size_t)n]);
    list[0] = list[1] = list[2] = -77;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the mode off: every query is refused
    CHECK(fxb_meter_read_level(h, l.get(), nullptr, 0) == FX_E_ARG && fxb_meter_select_level(h, 0, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_get_level(h, l.get(), l.get() + 1) == FX_E_ARG && fxb_meter_clear_level(h) == 0);
    list[0] = 0;
    CHECK(fxb_meter_read_level_list(h, list.get(), 1, l.get(), q.get(), 0) == FX_E_ARG);
    list[0] = -77;
    // the refusals of the set
    CHECK(fxb_meter_set_level(h, nan, 0.25f, 0) == FX_E_ARG && fxb_meter_set_level(h, inf, 0.25f, 0) == FX_E_ARG && fxb_meter_set_level(h, 1.5f, 0.25f, 0) == FX_E_ARG);
    CHECK(fxb_meter_set_level(h, -0.5f, 0.25f, 0) == FX_E_ARG && fxb_meter_set_level(h, 0.5f, nan, 0) == FX_E_ARG && fxb_meter_set_level(h, 0.5f, inf, 0) == FX_E_ARG);
    CHECK(fxb_meter_set_level(h, 0.5f, -0.25f, 0) == FX_E_ARG && fxb_meter_set_level(h, 0.5f, 0.25f, 1u) == FX_E_ARG && fxb_meter_set_level(nullptr, 0.5f, 0.25f, 0) == FX_E_ARG);
    CHECK(fxb_meter_get_level(h, nullptr, nullptr) == FX_E_ARG);
    // with the mode on: the refusals of the queries
    setLevel(h, m, 0.5f, 0.25f);
    play(h, m, 8);
    CHECK(fxb_meter_select_level(h, 2, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select_level(h, -1, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_level(h, 0, std::nan(""), 0, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select_level(h, 0, 0.0, -1, 2, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_level(h, 0, 0.0, 1, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select_level(h, 0, 0.0, n, INT64_MAX, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_level(h, 0, 0.0, 0, n, list.get(), -1, 0) == FX_E_ARG && fxb_meter_select_level(h, 0, 0.0, 0, n, nullptr, 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_level(h, 0, 0.0, 0, n, list.get(), 3, 2u) == FX_E_ARG && fxb_meter_select_level(nullptr, 0, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(list[0] == -77 && list[1] == -77 && list[2] == -77);
    list[0] = 4, list[1] = n, list[2] = 4;
    CHECK(fxb_meter_read_level_list(h, list.get(), 2, l.get(), q.get(), 0) == FX_E_ARG && fxb_meter_read_level_list(h, list.get(), -1, l.get(), q.get(), 0) == FX_E_ARG);
    list[1] = 7;
    CHECK(fxb_meter_read_level_list(h, list.get(), 3, l.get(), q.get(), 1) == FX_E_ARG && fxb_meter_read_level_list(h, nullptr, 3, l.get(), q.get(), 0) == FX_E_ARG);
    CHECK(fxb_meter_read_level_list(h, list.get(), 0, nullptr, nullptr, 1) == 0);
    CHECK(fxb_meter_set_level(h, 2.0f, 0.25f, 0) == FX_E_ARG);
    CHECK(fxb_info(h, FXB_INFO_METER_LEVEL_SELECTS) == 0 && fxb_info(h, FXB_INFO_METER_LEVEL_LIST_READS) == 0);
    compare(h, m);
    // a program load zeroes the rows and keeps the mode; metering off frees them
    CHECK(fxb_load_text(h, "static zz\nmacs zz, zz, 0.5, 0.5\nend") == 1);
    m.set(2, n);
    compare(h, m);
    play(h, m, 5);
    compare(h, m);
    CHECK(fxb_meter_enable(h, 0) == 0 && fxb_meter_get_level(h, nullptr, nullptr) == FX_E_ARG);
    CHECK(fxb_meter_set_level(h, 0.5f, 0.25f, 0) == FX_E_ARG);   // (metering off)
    fxb_destroy(h);
    // a handle destroyed with the mode on frees the rows (LeakSanitizer)
    h = create(n, 1, devices);
    m.set(1, n);
    setLevel(h, m, 0.999f, 1e-4f);
    play(h, m, 5);
    fxb_destroy(h);
}

// an allocation that fails, at each allocation of a set (one per shard): FX_E_MEMORY, the mode off everywhere, then the call goes through
void memory(int devices) {
    const int64_t n = devices > 1 ? 808 : 200;
    for (int nth = 0; nth < devices; ++nth) {
        fxb_handle* h = create(n, 2, devices);
        Level m;
        m.set(2, n);
        {
            const size_t words = 8 * 2 * (size_t)n;
            std::unique_ptr<float[]> in(new float[words]), out(new float[words]);
            for (size_t i = 0; i < words; ++i) in[i] = word();
            CHECK(fxb_process_block(h, in.get(), out.get(), 8) == 0);
        }
        CHECK(fxb_prepare(h, 8, 1) == 0);   // (the builder threads are idle: no allocation of their own meets the injected failure)
        fxstub_fail_mallocs(nth, 1);
        const int rc = fxb_meter_set_level(h, 0.5f, 0.25f, 0);
        fxstub_fail_mallocs(-1, 0);
        CHECK(rc == FX_E_MEMORY && fxb_last_error(h)[0] != 0);
        CHECK(fxb_meter_get_level(h, nullptr, nullptr) == FX_E_ARG && fxb_meter_read_level(h, nullptr, nullptr, 0) == FX_E_ARG);
        setLevel(h, m, 0.5f, 0.25f);
        play(h, m, 8);
        compare(h, m);
        CHECK(fxb_info(h, FXB_INFO_METER_LEVEL_LAUNCHES) == devices);
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
        std::printf("  level meters, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_level_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "level meter checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("level meter checks ok\n");
    return 0;
}
