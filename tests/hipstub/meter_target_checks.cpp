// meter_target_checks.cpp — the target meters of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan +
// LeakSanitizer (TEST INFRASTRUCTURE: csrc/Makefile `stubasanmetertarget` links this file with the library's host sources and
// tests/hipstub/; a program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The comparison with the numpy model is tests/test_meter_target_stub.py; this program is about addresses.  Every array the
// caller hands in is a heap block of exactly the documented size - [n_samples][channels][G] target words, [channels][N] per match
// row, [cap] instance numbers of a select, [G] winners and [G] values - and every "device" block of the stand-in is a heap block
// too, so a read or write one word outside the target, a shard's part of it, the match rows, the staging or an output is a report.
// It walks N = 1, 5, 65, 200 and 777 on one handle and N = 808 on three shards (their starts, 320 and 576, are no multiples of 3
// or 65) with one, two and four channels; group = 1, 3, 64, 65, N and beyond; targets of one sample and of more samples than a
// block, with and without LOOP; blocks that start at the last position; caps of M, M - 1, M + 1, 1 and 0; the refusals (nothing
// changes); and allocation failures at every allocation of a set.  What comes back is checked with plain loops written from the
// definition in include/fx8010_amd.h "Target meters".  Exit code 0 = every check held (a sanitizer report turns it non-zero).
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

extern "C" long fxstub_match_strays(void);   // fx_meter_target_stub.cpp

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
float word() {
    const uint32_t d = draw(), kind = (d >> 4) % 16;
    return kind == 0 ? 0.0f : kind == 1 ? 1.0f : kind == 2 ? -0.0f : kind == 3 ? std::numeric_limits<float>::quiet_NaN() : kind == 4 ? -std::numeric_limits<float>::infinity()
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

// the model: the match rows of one handle, by the definition (this file is compiled with -ffp-contract=off)
struct Match {
    int channels = 0;
    int64_t n = 0, group = 1, tSamples = 0, cols = 0, pos = 0;
    bool loop = false;
    std::vector<float> target;
    std::vector<double> err, cross;
    void set(int ch, int64_t N, int64_t g, int64_t T, bool lp) {
        channels = ch, n = N, group = std::min(g, N), tSamples = T, loop = lp, pos = 0;
        cols = (n + group - 1) / group;
        target.resize((size_t)(T * ch * cols));
        for (float& t : target) t = word();
        err.assign((size_t)ch * (size_t)n, 0.0);
        cross.assign((size_t)ch * (size_t)n, 0.0);
    }
    void take(const float* y, int samples) {
        for (int s = 0; s < samples; ++s) {
            int64_t q = pos + s;
            if (loop) q %= tSamples;
            if (q >= tSamples) continue;
            for (int c = 0; c < channels; ++c)
                for (int64_t i = 0; i < n; ++i) {
                    const float yw = y[((size_t)s * (size_t)channels + (size_t)c) * (size_t)n + (size_t)i];
                    const float tw = target[((size_t)q * (size_t)channels + (size_t)c) * (size_t)cols + (size_t)(i / group)];
                    if (!(std::fabs(yw) < INFINITY) || !(std::fabs(tw) < INFINITY)) continue;
                    const size_t at = (size_t)c * (size_t)n + (size_t)i;
                    volatile double d = (double)yw - (double)tw;
                    volatile double e = d * d;
                    volatile double yt = (double)yw * (double)tw;
                    err[at] = err[at] + e;
                    cross[at] = cross[at] + yt;
                }
        }
        pos += samples;
        if (loop) pos %= tSamples;
    }
    double value(int stat, int64_t i) const {
        const std::vector<double>& v = stat == 0 ? err : cross;
        volatile double sum = v[(size_t)i];
        for (int c = 1; c < channels; ++c) sum = sum + v[(size_t)c * (size_t)n + (size_t)i];
        return sum;
    }
};

void setTarget(fxb_handle* h, Match& m, int channels, int64_t n, int64_t group, int64_t T, bool loop) {
    m.set(channels, n, group, T, loop);
    std::unique_ptr<float[]> t(new float[m.target.size()]);   // exactly [T][channels][G], freed on return
    std::copy(m.target.begin(), m.target.end(), t.get());
    CHECK(fxb_meter_set_target(h, t.get(), T, group, loop ? FXB_METER_TARGET_LOOP : 0u) == 0);
    CHECK(fxb_meter_target_pos(h) == 0);
}

void play(fxb_handle* h, Match& m, int samples) {
    const size_t words = (size_t)samples * (size_t)m.channels * (size_t)m.n;
    std::unique_ptr<float[]> in(new float[words]), out(new float[words]);
    for (size_t i = 0; i < words; ++i) in[i] = word();
    CHECK(fxb_process_block(h, in.get(), out.get(), samples) == 0);
    m.take(out.get(), samples);   // (the stand-in's emulation launch copies input to output)
}

void compare(fxb_handle* h, const Match& m) {
    const size_t k = (size_t)m.channels * (size_t)m.n;
    std::unique_ptr<double[]> e(new double[k]), x(new double[k]);
    CHECK(fxb_meter_read_match(h, e.get(), x.get(), 0) == 0);
    CHECK(std::memcmp(e.get(), m.err.data(), k * 8) == 0);
    CHECK(std::memcmp(x.get(), m.cross.data(), k * 8) == 0);
    CHECK(fxb_meter_read_match(h, nullptr, x.get(), 0) == 0 && fxb_meter_read_match(h, e.get(), nullptr, 0) == 0 && fxb_meter_read_match(h, nullptr, nullptr, 0) == 0);
    CHECK(fxb_meter_target_pos(h) == m.pos);
}

void selectOnce(fxb_handle* h, const Match& m, int stat, double t, bool below, int64_t first, int64_t nRange, int64_t cap) {
    std::vector<int64_t> want;
    for (int64_t i = first; i < first + nRange; ++i)
        if (below ? m.value(stat, i) < t : m.value(stat, i) >= t) want.push_back(i);
    std::unique_ptr<int64_t[]> list(cap > 0 ? new int64_t[(size_t)cap] : nullptr);
    for (int64_t i = 0; i < cap; ++i) list[(size_t)i] = -77;
    const int64_t got = fxb_meter_select_match(h, stat, t, first, nRange, list.get(), cap, below ? FXB_METER_BELOW : 0u);
    CHECK(got == (int64_t)want.size());
    const int64_t take = std::min<int64_t>(cap, (int64_t)want.size());
    for (int64_t i = 0; i < cap; ++i) CHECK(list[(size_t)i] == (i < take ? want[(size_t)i] : -77));
}

void queries(fxb_handle* h, const Match& m) {
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
        const int64_t groups[7] = {1, 3, 64, 65, n, n + 1, INT64_MAX};
        for (const int64_t group : groups)
            for (int largest = 0; largest < 2; ++largest) {
                const int64_t g = std::min(group, n), G = (n + g - 1) / g;
                std::unique_ptr<int64_t[]> winner(new int64_t[(size_t)G]);   // exactly [G]
                std::unique_ptr<double[]> value(new double[(size_t)G]);
                CHECK(fxb_meter_best(h, stat, group, winner.get(), value.get(), largest ? FXB_MATCH_LARGEST : 0u) == 0);
                for (int64_t k = 0; k < G; ++k) {
                    int64_t best = k * g;
                    for (int64_t i = k * g + 1; i < std::min((k + 1) * g, n); ++i)
                        if (largest ? m.value(stat, i) > m.value(stat, best) : m.value(stat, i) < m.value(stat, best)) best = i;
                    const double v = m.value(stat, best);
                    CHECK(winner[(size_t)k] == best && std::memcmp(&value[(size_t)k], &v, 8) == 0);
                }
                CHECK(fxb_meter_best(h, stat, group, nullptr, value.get(), 0) == 0 && fxb_meter_best(h, stat, group, winner.get(), nullptr, 0) == 0);
            }
    }
}

void indexing(int devices) {
    const int64_t single[5] = {1, 5, 65, 200, 777}, sharded[1] = {808};
    const int64_t* sizes = devices > 1 ? sharded : single;
    const int nSizes = devices > 1 ? 1 : 5;
    for (int s = 0; s < nSizes; ++s)
        for (int channels = 1; channels <= 4; channels *= 2) {
            const int64_t n = sizes[s];
            fxb_handle* h = create(n, channels, devices);
            Match m;
            const int64_t groups[6] = {1, 3, 64, 65, n, n + 7};
            int shape = 0;
            for (const int64_t group : groups) {
                const int64_t T = shape % 3 == 0 ? 1 : shape % 3 == 1 ? 5 : 40;
                const bool loop = shape % 2 == 0;
                ++shape;
                setTarget(h, m, channels, n, group, T, loop);
                play(h, m, 9);
                play(h, m, 4);
                compare(h, m);
                // a block that starts at the last position; one that starts at the end (without LOOP: nothing but the four moves)
                CHECK(fxb_meter_target_seek(h, T - 1) == 0);
                m.pos = T - 1;
                play(h, m, 3);
                if (!loop) {
                    CHECK(fxb_meter_target_seek(h, T) == 0);
                    m.pos = T;
                    play(h, m, 2);
                }
                compare(h, m);
                if (group == 3 || group == n) queries(h, m);
                // a list reset on an exactly-sized list; read_match with reset
                const int64_t count = std::min<int64_t>(n, 3);
                {
                    std::unique_ptr<int64_t[]> l(new int64_t[(size_t)count]);
                    for (int64_t i = 0; i < count; ++i) l[(size_t)i] = i == 0 ? n - 1 : i == 1 ? 0 : n / 2;
                    CHECK(fxb_meter_reset_list(h, l.get(), count) == 0);
                    for (int c = 0; c < channels; ++c)
                        for (int64_t i = 0; i < count; ++i) m.err[(size_t)c * (size_t)n + (size_t)l[(size_t)i]] = m.cross[(size_t)c * (size_t)n + (size_t)l[(size_t)i]] = 0.0;
                }
                compare(h, m);
                CHECK(fxb_meter_read_match(h, nullptr, nullptr, 1) == 0);
                std::fill(m.err.begin(), m.err.end(), 0.0);
                std::fill(m.cross.begin(), m.cross.end(), 0.0);
                play(h, m, 2);
                compare(h, m);
            }
            CHECK(fxb_meter_clear_target(h) == 0 && fxb_meter_target_pos(h) == FX_E_ARG);
            fxb_destroy(h);
        }
}

void refusals(int devices) {
    const int64_t n = devices > 1 ? 808 : 200;
    fxb_handle* h = create(n, 2, devices);
    Match m;
    std::unique_ptr<float[]> t(new float[2 * 4 * 67]);
    for (int i = 0; i < 2 * 4 * 67; ++i) t[(size_t)i] = 0.5f;
    std::unique_ptr<int64_t[]> list(new int64_t[3]);
    std::unique_ptr<double[]> e(new double[2 * (size_t)n]);
    list[0] = list[1] = list[2] = -77;
    // no target: every query is refused
    CHECK(fxb_meter_read_match(h, e.get(), nullptr, 0) == FX_E_ARG && fxb_meter_select_match(h, 0, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_best(h, 0, n, list.get(), nullptr, 0) == FX_E_ARG && fxb_meter_target_seek(h, 0) == FX_E_ARG && fxb_meter_target_pos(h) == FX_E_ARG);
    CHECK(fxb_meter_clear_target(h) == 0);
    // the refusals of the set
    CHECK(fxb_meter_set_target(h, nullptr, 4, 3, 0) == FX_E_ARG && fxb_meter_set_target(h, t.get(), 0, 3, 0) == FX_E_ARG && fxb_meter_set_target(h, t.get(), -1, 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_set_target(h, t.get(), 4, 0, 0) == FX_E_ARG && fxb_meter_set_target(h, t.get(), 4, -3, 0) == FX_E_ARG && fxb_meter_set_target(h, t.get(), 4, 3, 2u) == FX_E_ARG);
    CHECK(fxb_meter_set_target(h, t.get(), INT64_MAX, n, 0) == FX_E_ARG && fxb_meter_set_target(h, t.get(), ((int64_t)1 << 30), n, 0) == FX_E_ARG);
    CHECK(fxb_meter_set_target(nullptr, t.get(), 4, 3, 0) == FX_E_ARG && fxb_meter_target_pos(h) == FX_E_ARG);
    // with a target: the refusals of the queries
    setTarget(h, m, 2, n, 12, 4, true);
    play(h, m, 8);
    CHECK(fxb_meter_select_match(h, 2, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select_match(h, -1, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_match(h, 0, std::nan(""), 0, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select_match(h, 0, 0.0, -1, 2, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_match(h, 0, 0.0, 1, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select_match(h, 0, 0.0, n, INT64_MAX, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_match(h, 0, 0.0, 0, n, list.get(), -1, 0) == FX_E_ARG && fxb_meter_select_match(h, 0, 0.0, 0, n, nullptr, 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_match(h, 0, 0.0, 0, n, list.get(), 3, 2u) == FX_E_ARG && fxb_meter_select_match(nullptr, 0, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_best(h, 2, 3, list.get(), nullptr, 0) == FX_E_ARG && fxb_meter_best(h, 0, 0, list.get(), nullptr, 0) == FX_E_ARG && fxb_meter_best(h, 0, 3, list.get(), nullptr, 1u) == FX_E_ARG);
    CHECK(fxb_meter_best(nullptr, 0, 3, list.get(), nullptr, 0) == FX_E_ARG);
    CHECK(fxb_meter_target_seek(h, 4) == FX_E_ARG && fxb_meter_target_seek(h, -1) == FX_E_ARG && fxb_meter_target_seek(nullptr, 0) == FX_E_ARG);
    CHECK(list[0] == -77 && list[1] == -77 && list[2] == -77);
    CHECK(fxb_info(h, FXB_INFO_METER_MATCH_SELECTS) == 0 && fxb_info(h, FXB_INFO_METER_MATCH_BESTS) == 0);
    compare(h, m);
    // a program load drops the target; metering off drops it
    CHECK(fxb_load_text(h, "static zz\nmacs zz, zz, 0.5, 0.5\nend") == 1);
    CHECK(fxb_meter_target_pos(h) == FX_E_ARG && fxb_meter_read_match(h, e.get(), nullptr, 0) == FX_E_ARG);
    setTarget(h, m, 2, n, 12, 4, false);
    CHECK(fxb_meter_enable(h, 0) == 0 && fxb_meter_target_pos(h) == FX_E_ARG);
    CHECK(fxb_meter_set_target(h, t.get(), 4, 3, 0) == FX_E_ARG);   // (metering off)
    fxb_destroy(h);
    // a handle destroyed with a target set frees it (LeakSanitizer)
    h = create(n, 1, devices);
    setTarget(h, m, 1, n, 3, 7, true);
    play(h, m, 5);
    fxb_destroy(h);
}

// an allocation that fails, at each allocation of a set (two per shard): FX_E_MEMORY, no target, then the call goes through
void memory(int devices) {
    const int64_t n = devices > 1 ? 808 : 200;
    for (int nth = 0; nth < 2 * devices; ++nth) {
        fxb_handle* h = create(n, 2, devices);
        Match m;
        m.set(2, n, 3, 6, true);
        std::unique_ptr<float[]> t(new float[m.target.size()]);
        std::copy(m.target.begin(), m.target.end(), t.get());
        {
            const size_t words = 8 * 2 * (size_t)n;
            std::unique_ptr<float[]> in(new float[words]), out(new float[words]);
            for (size_t i = 0; i < words; ++i) in[i] = word();
            CHECK(fxb_process_block(h, in.get(), out.get(), 8) == 0);
        }
        CHECK(fxb_prepare(h, 8, 1) == 0);   // (the builder threads are idle: no allocation of their own meets the injected failure)
        fxstub_fail_mallocs(nth, 1);
        const int rc = fxb_meter_set_target(h, t.get(), 6, 3, FXB_METER_TARGET_LOOP);
        fxstub_fail_mallocs(-1, 0);
        CHECK(rc == FX_E_MEMORY && fxb_last_error(h)[0] != 0);
        CHECK(fxb_meter_target_pos(h) == FX_E_ARG && fxb_meter_read_match(h, nullptr, nullptr, 0) == FX_E_ARG);
        CHECK(fxb_info(h, FXB_INFO_METER_TARGET_LAUNCHES) == 0);
        CHECK(fxb_meter_set_target(h, t.get(), 6, 3, FXB_METER_TARGET_LOOP) == 0);
        play(h, m, 8);
        compare(h, m);
        CHECK(fxb_info(h, FXB_INFO_METER_TARGET_LAUNCHES) == devices);
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
        std::printf("  meter targets, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_match_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "meter target checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("meter target checks ok\n");
    return 0;
}
