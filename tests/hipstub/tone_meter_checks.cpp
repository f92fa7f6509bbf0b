// tone_meter_checks.cpp — the tone meters of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan +
// LeakSanitizer (TEST INFRASTRUCTURE: csrc/Makefile `stubasanmetertone` links this file with the library's host sources and
// tests/hipstub/; a program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The comparison with the numpy model is tests/test_meter_tone_stub.py; this program is about addresses.  Every array the caller
// hands in is a heap block of exactly the documented size - [tones][channels][N] per row, [count] list entries and
// [tones][channels][count] per gathered row, [cap] instance numbers of a select, [k] numbers and [k] values of a rank, [tones]
// coefficients - and every "device" block of the stand-in is a heap block too, so a read or write one word outside the tone block,
// a shard's part of it, the staging or an output is a report.  It walks N = 1, 5, 65, 200 and 777 on one handle and N = 808 on
// three shards (their starts are 320 and 576) with one, two and four channels and 1, 3 and 8 tones; caps and k of M, M - 1, M + 1,
// 1 and 0; lists of one entry, with repeats, and one entry per shard; the refusals (nothing changes); and an allocation failure at
// each allocation of a set.  What comes back is checked with plain loops written from the definition in include/fx8010_amd.h
// "Tone meters".  Exit code 0 = every check held (a sanitizer report turns it non-zero).
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

extern "C" long fxstub_tone_strays(void);   // fx_meter_tone_stub.cpp

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
    return kind < 4 ? 0.0f : kind == 6 ? 1.0f : kind == 7 ? -0.0f : kind == 8 ? std::numeric_limits<float>::quiet_NaN() : kind == 9 ? -std::numeric_limits<float>::infinity()
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

// the model: the tone rows of one handle, by the definition (this file is compiled with -ffp-contract=off)
struct Tones {
    int tones = 0, channels = 0;
    int64_t n = 0;
    std::vector<double> coeff, s1, s2;
    void set(int k, int ch, int64_t N, const double* c) {
        tones = k, channels = ch, n = N;
        coeff.assign(c, c + k);
        zero();
    }
    void zero() {
        s1.assign((size_t)tones * (size_t)channels * (size_t)n, 0.0);
        s2 = s1;
    }
    size_t at(int t, int c, int64_t i) const { return ((size_t)t * (size_t)channels + (size_t)c) * (size_t)n + (size_t)i; }
    void take(const float* y, int samples) {
        for (int s = 0; s < samples; ++s)
            for (int c = 0; c < channels; ++c)
                for (int64_t i = 0; i < n; ++i) {
                    const float yw = y[((size_t)s * (size_t)channels + (size_t)c) * (size_t)n + (size_t)i];
                    const double x = std::fabs(yw) < INFINITY ? (double)yw : 0.0;
                    for (int t = 0; t < tones; ++t) {
                        const size_t k = at(t, c, i);
                        volatile double p = coeff[(size_t)t] * s1[k];
                        volatile double q = x + p;
                        volatile double s0 = q - s2[k];
                        s2[k] = s1[k];
                        s1[k] = s0;
                    }
                }
    }
    double power(int t, int c, int64_t i) const {
        const size_t k = at(t, c, i);
        volatile double a = s1[k] * s1[k];
        volatile double b = s2[k] * s2[k];
        volatile double sum = a + b;
        volatile double p = coeff[(size_t)t] * s1[k];
        volatile double m = p * s2[k];
        return sum - m;
    }
    double value(int t, int64_t i) const {
        double v = power(t, 0, i);
        for (int c = 1; c < channels; ++c) v = std::max(v, power(t, c, i));
        return v;
    }
    void zeroColumn(int64_t i) {
        for (int t = 0; t < tones; ++t)
            for (int c = 0; c < channels; ++c) s1[at(t, c, i)] = s2[at(t, c, i)] = 0.0;
    }
};

void setTones(fxb_handle* h, Tones& m, int tones, int channels, int64_t n) {
    static const double all[8] = {2.0, -2.0, 0.0, 1.9615705608064609, 0.76536686473017945, -1.4142135623730951, 1.25, -0.5};
    std::unique_ptr<double[]> c(new double[(size_t)tones]);
    std::copy(all, all + tones, c.get());
    CHECK(fxb_meter_set_tones(h, tones, c.get(), 0) == 0);
    m.set(tones, channels, n, c.get());
    std::unique_ptr<double[]> back(new double[FXB_METER_MAX_TONES]);
    std::unique_ptr<int[]> count(new int[1]);
    CHECK(fxb_meter_get_tones(h, count.get(), back.get()) == 0 && count[0] == tones && std::memcmp(back.get(), c.get(), (size_t)tones * 8) == 0);
    CHECK(fxb_meter_get_tones(h, nullptr, back.get()) == 0 && fxb_meter_get_tones(h, count.get(), nullptr) == 0);
}

void play(fxb_handle* h, Tones& m, int samples) {
    const size_t words = (size_t)samples * (size_t)m.channels * (size_t)m.n;
    std::unique_ptr<float[]> in(new float[words]), out(new float[words]);
    for (size_t i = 0; i < words; ++i) in[i] = word();
    CHECK(fxb_process_block(h, in.get(), out.get(), samples) == 0);
    m.take(out.get(), samples);   // (the stand-in's emulation launch copies input to output)
}

void compare(fxb_handle* h, const Tones& m) {
    const size_t k = m.s1.size();
    std::unique_ptr<double[]> a(new double[k]), b(new double[k]), p(new double[k]);
    CHECK(fxb_meter_read_tones(h, a.get(), b.get(), p.get(), 0) == 0);
    CHECK(std::memcmp(a.get(), m.s1.data(), k * 8) == 0);
    CHECK(std::memcmp(b.get(), m.s2.data(), k * 8) == 0);
    bool same = true;
    for (int t = 0; t < m.tones; ++t)
        for (int c = 0; c < m.channels; ++c)
            for (int64_t i = 0; i < m.n; ++i) {
                const double want = m.power(t, c, i);
                same = same && std::memcmp(&p[m.at(t, c, i)], &want, 8) == 0;
            }
    CHECK(same);
    CHECK(fxb_meter_read_tones(h, nullptr, b.get(), nullptr, 0) == 0 && fxb_meter_read_tones(h, a.get(), nullptr, nullptr, 0) == 0 && fxb_meter_read_tones(h, nullptr, nullptr, p.get(), 0) == 0 &&
          fxb_meter_read_tones(h, nullptr, nullptr, nullptr, 0) == 0);
}

void selectOnce(fxb_handle* h, const Tones& m, int tone, double t, bool below, int64_t first, int64_t nRange, int64_t cap) {
    std::vector<int64_t> want;
    for (int64_t i = first; i < first + nRange; ++i)
        if (below ? m.value(tone, i) < t : m.value(tone, i) >= t) want.push_back(i);
    std::unique_ptr<int64_t[]> list(cap > 0 ? new int64_t[(size_t)cap] : nullptr);
    for (int64_t i = 0; i < cap; ++i) list[(size_t)i] = -77;
    const int64_t got = fxb_meter_select_tone(h, tone, t, first, nRange, list.get(), cap, below ? FXB_METER_BELOW : 0u);
    CHECK(got == (int64_t)want.size());
    const int64_t take = std::min<int64_t>(cap, (int64_t)want.size());
    for (int64_t i = 0; i < cap; ++i) CHECK(list[(size_t)i] == (i < take ? want[(size_t)i] : -77));
}

void rankOnce(fxb_handle* h, const Tones& m, int tone, int64_t k, double t, bool below, bool largest, int64_t first, int64_t nRange, bool values) {
    struct Item { double v; int64_t n; };
    std::vector<Item> want;
    for (int64_t i = first; i < first + nRange; ++i)
        if (below ? m.value(tone, i) < t : m.value(tone, i) >= t) want.push_back(Item{m.value(tone, i), i});
    std::stable_sort(want.begin(), want.end(), [largest](const Item& x, const Item& y) { return largest ? x.v > y.v : x.v < y.v; });
    std::unique_ptr<int64_t[]> list(k > 0 ? new int64_t[(size_t)k] : nullptr);
    std::unique_ptr<double[]> value(k > 0 && values ? new double[(size_t)k] : nullptr);
    for (int64_t i = 0; i < k; ++i) {
        list[(size_t)i] = -77;
        if (value) value[(size_t)i] = -77.0;
    }
    const int64_t got = fxb_meter_rank_tone(h, tone, k, t, first, nRange, list.get(), value.get(), (below ? FXB_METER_BELOW : 0u) | (largest ? FXB_METER_LARGEST : 0u));
    CHECK(got == (int64_t)want.size());
    const int64_t take = std::min<int64_t>(k, (int64_t)want.size());
    for (int64_t i = 0; i < k; ++i) {
        CHECK(list[(size_t)i] == (i < take ? want[(size_t)i].n : -77));
        if (value) CHECK(i < take ? std::memcmp(&value[(size_t)i], &want[(size_t)i].v, 8) == 0 : value[(size_t)i] == -77.0);
    }
}

void queries(fxb_handle* h, const Tones& m) {
    const int64_t n = m.n;
    const int tonesToAsk[2] = {0, m.tones - 1};
    for (const int tone : tonesToAsk) {
        const double mid = m.value(tone, n / 2), ts[4] = {-INFINITY, mid, std::nextafter(mid, INFINITY), INFINITY};
        for (const double t : ts)
            for (int below = 0; below < 2; ++below) {
                int64_t M = 0;
                for (int64_t i = 0; i < n; ++i) M += (below ? m.value(tone, i) < t : m.value(tone, i) >= t) ? 1 : 0;
                const int64_t caps[5] = {M, std::max<int64_t>(M - 1, 0), M + 1, 1, 0};
                for (const int64_t cap : caps) {
                    selectOnce(h, m, tone, t, below != 0, 0, n, cap);
                    rankOnce(h, m, tone, cap, t, below != 0, (cap & 1) != 0, 0, n, cap != 1);
                }
                const int64_t firsts[4] = {1 % n, std::min<int64_t>(63, n), std::min<int64_t>(64, n), n / 2};
                for (const int64_t first : firsts) {
                    selectOnce(h, m, tone, t, below != 0, first, n - first, (n - first) / 2);
                    rankOnce(h, m, tone, (n - first) / 2, t, below != 0, below == 0, first, n - first, true);
                }
            }
    }
}

// a list read on exactly-sized blocks: [count] entries, [tones][channels][count] per row
void readList(fxb_handle* h, Tones& m, const std::vector<int64_t>& entries, bool reset) {
    const size_t count = entries.size(), k = (size_t)m.tones * (size_t)m.channels * count;
    std::unique_ptr<int64_t[]> list(new int64_t[count]);
    std::copy(entries.begin(), entries.end(), list.get());
    std::unique_ptr<double[]> a(new double[k]), b(new double[k]), p(new double[k]);
    CHECK(fxb_meter_read_tones_list(h, list.get(), (int64_t)count, a.get(), b.get(), p.get(), reset ? 1 : 0) == 0);
    for (int t = 0; t < m.tones; ++t)
        for (int c = 0; c < m.channels; ++c)
            for (size_t i = 0; i < count; ++i) {
                const size_t from = m.at(t, c, entries[i]), to = ((size_t)t * (size_t)m.channels + (size_t)c) * count + i;
                const double want = m.power(t, c, entries[i]);
                CHECK(std::memcmp(&a[to], &m.s1[from], 8) == 0 && std::memcmp(&b[to], &m.s2[from], 8) == 0 && std::memcmp(&p[to], &want, 8) == 0);
            }
    if (reset)
        for (const int64_t i : entries) m.zeroColumn(i);
    else
        CHECK(fxb_meter_read_tones_list(h, list.get(), (int64_t)count, nullptr, b.get(), nullptr, 0) == 0 && fxb_meter_read_tones_list(h, list.get(), (int64_t)count, a.get(), nullptr, nullptr, 0) == 0 &&
              fxb_meter_read_tones_list(h, list.get(), (int64_t)count, nullptr, nullptr, p.get(), 0) == 0);
}

void indexing(int devices) {
    const int64_t single[5] = {1, 5, 65, 200, 777}, sharded[1] = {808};
    const int64_t* sizes = devices > 1 ? sharded : single;
    const int nSizes = devices > 1 ? 1 : 5;
    const int counts[3] = {1, 3, 8};
    for (int s = 0; s < nSizes; ++s)
        for (int channels = 1; channels <= 4; channels *= 2) {
            const int64_t n = sizes[s];
            fxb_handle* h = create(n, channels, devices);
            Tones m;
            for (int p = 0; p < 3; ++p) {
                setTones(h, m, counts[p], channels, n);   // (every set zeroes; the block is replaced by one of another size)
                compare(h, m);
                play(h, m, 9);
                play(h, m, 4);
                compare(h, m);
                if (p != 1 || n <= 200) queries(h, m);
                // lists: one entry, repeats, the ends and the middle (on three shards: one entry per shard and more)
                readList(h, m, {n - 1}, false);
                readList(h, m, {n - 1, 0, n / 2, 0, n - 1}, false);
                if (n == 808) readList(h, m, {319, 320, 575, 576, 807, 0}, true);
                readList(h, m, {n / 2}, true);
                compare(h, m);
                // a list reset on an exactly-sized list; read_tones with reset
                const int64_t count = std::min<int64_t>(n, 3);
                {
                    std::unique_ptr<int64_t[]> l(new int64_t[(size_t)count]);
                    for (int64_t i = 0; i < count; ++i) l[(size_t)i] = i == 0 ? n - 1 : i == 1 ? 0 : n / 2;
                    CHECK(fxb_meter_reset_list(h, l.get(), count) == 0);
                    for (int64_t i = 0; i < count; ++i) m.zeroColumn(l[(size_t)i]);
                }
                compare(h, m);
                play(h, m, 3);
                CHECK(fxb_meter_read_tones(h, nullptr, nullptr, nullptr, 1) == 0);
                m.zero();
                play(h, m, 2);
                compare(h, m);
            }
            // (four blocks per set, each followed by one tone launch per shard)
            CHECK(fxb_info(h, FXB_INFO_METER_TONE_LAUNCHES) == 3 * 4 * devices && fxb_info(h, FXB_INFO_METER_LAUNCHES) == 3 * 4 * devices);
            CHECK(fxb_meter_clear_tones(h) == 0 && fxb_meter_get_tones(h, nullptr, nullptr) == FX_E_ARG);
            fxb_destroy(h);
        }
}

void refusals(int devices) {
    const int64_t n = devices > 1 ? 808 : 200;
    fxb_handle* h = create(n, 2, devices);
    Tones m;
    std::unique_ptr<int64_t[]> list(new int64_t[3]);
    std::unique_ptr<double[]> value(new double[3]);
    std::unique_ptr<double[]> a(new double[8 * 2 * (size_t)n]);
    std::unique_ptr<double[]> two(new double[2]), nine(new double[9]);
    list[0] = list[1] = list[2] = -77;
    two[0] = 1.0, two[1] = -1.0;
    std::fill(nine.get(), nine.get() + 9, 0.5);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // the mode off: every query is refused
    CHECK(fxb_meter_read_tones(h, a.get(), nullptr, nullptr, 0) == FX_E_ARG && fxb_meter_select_tone(h, 0, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_rank_tone(h, 0, 3, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG && fxb_meter_get_tones(h, nullptr, a.get()) == FX_E_ARG && fxb_meter_clear_tones(h) == 0);
    list[0] = 0;
    CHECK(fxb_meter_read_tones_list(h, list.get(), 1, a.get(), nullptr, nullptr, 0) == FX_E_ARG);
    list[0] = -77;
    // the refusals of the set
    const auto refusedSets = [&] {
        CHECK(fxb_meter_set_tones(h, 0, two.get(), 0) == FX_E_ARG && fxb_meter_set_tones(h, 9, nine.get(), 0) == FX_E_ARG && fxb_meter_set_tones(h, -1, two.get(), 0) == FX_E_ARG);
        CHECK(fxb_meter_set_tones(h, 2, nullptr, 0) == FX_E_ARG && fxb_meter_set_tones(h, 2, two.get(), 1u) == FX_E_ARG && fxb_meter_set_tones(nullptr, 2, two.get(), 0) == FX_E_ARG);
        for (const double bad : {nan, inf, -inf, std::nextafter(2.0, 3.0), std::nextafter(-2.0, -3.0)}) {
            two[1] = bad;
            CHECK(fxb_meter_set_tones(h, 2, two.get(), 0) == FX_E_ARG);
        }
        two[1] = -1.0;
    };
    refusedSets();
    CHECK(fxb_meter_get_tones(h, nullptr, nullptr) == FX_E_ARG);
    // with the mode on: the refusals of the set change nothing; the refusals of the queries
    setTones(h, m, 3, 2, n);
    play(h, m, 8);
    refusedSets();
    compare(h, m);
    CHECK(fxb_meter_select_tone(h, 3, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select_tone(h, -1, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select_tone(h, 8, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_tone(h, 0, std::nan(""), 0, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select_tone(h, 0, 0.0, -1, 2, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_tone(h, 0, 0.0, 1, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select_tone(h, 0, 0.0, n, INT64_MAX, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_tone(h, 0, 0.0, 0, n, list.get(), -1, 0) == FX_E_ARG && fxb_meter_select_tone(h, 0, 0.0, 0, n, nullptr, 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select_tone(h, 0, 0.0, 0, n, list.get(), 3, 2u) == FX_E_ARG && fxb_meter_select_tone(nullptr, 0, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_rank_tone(h, 3, 3, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG && fxb_meter_rank_tone(h, -1, 3, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG);
    CHECK(fxb_meter_rank_tone(h, 0, -1, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG && fxb_meter_rank_tone(h, 0, 3, std::nan(""), 0, n, list.get(), value.get(), 0) == FX_E_ARG);
    CHECK(fxb_meter_rank_tone(h, 0, 3, 0.0, 1, n, list.get(), value.get(), 0) == FX_E_ARG && fxb_meter_rank_tone(h, 0, 3, 0.0, 0, n, nullptr, value.get(), 0) == FX_E_ARG);
    CHECK(fxb_meter_rank_tone(h, 0, 3, 0.0, 0, n, list.get(), value.get(), 4u) == FX_E_ARG && fxb_meter_rank_tone(nullptr, 0, 3, 0.0, 0, n, list.get(), value.get(), 0) == FX_E_ARG);
    CHECK(list[0] == -77 && list[1] == -77 && list[2] == -77);
    list[0] = 4, list[1] = n, list[2] = 4;
    CHECK(fxb_meter_read_tones_list(h, list.get(), 2, a.get(), nullptr, nullptr, 0) == FX_E_ARG && fxb_meter_read_tones_list(h, list.get(), -1, a.get(), nullptr, nullptr, 0) == FX_E_ARG);
    list[1] = 7;
    CHECK(fxb_meter_read_tones_list(h, list.get(), 3, a.get(), nullptr, nullptr, 1) == FX_E_ARG && fxb_meter_read_tones_list(h, nullptr, 3, a.get(), nullptr, nullptr, 0) == FX_E_ARG);
    CHECK(fxb_meter_read_tones_list(h, list.get(), 0, nullptr, nullptr, nullptr, 1) == 0);
    CHECK(fxb_info(h, FXB_INFO_METER_TONE_SELECTS) == 0 && fxb_info(h, FXB_INFO_METER_TONE_LIST_READS) == 0 && fxb_info(h, FXB_INFO_METER_TONE_RANKS) == 0);
    compare(h, m);
    // a set reads exactly n_tones coefficients: a block of one
    {
        std::unique_ptr<double[]> one(new double[1]);
        one[0] = -0.0;
        CHECK(fxb_meter_set_tones(h, 1, one.get(), 0) == 0);
        const double zero = 0.0;
        m.set(1, 2, n, &zero);
        std::unique_ptr<double[]> back(new double[FXB_METER_MAX_TONES]);
        CHECK(fxb_meter_get_tones(h, nullptr, back.get()) == 0 && std::memcmp(back.get(), &zero, 8) == 0);
        play(h, m, 5);
        compare(h, m);
    }
    // a program load zeroes the rows and keeps the mode; metering off frees them
    CHECK(fxb_load_text(h, "static zz\nmacs zz, zz, 0.5, 0.5\nend") == 1);
    m.zero();
    compare(h, m);
    play(h, m, 5);
    compare(h, m);
    CHECK(fxb_meter_enable(h, 0) == 0 && fxb_meter_get_tones(h, nullptr, nullptr) == FX_E_ARG);
    CHECK(fxb_meter_set_tones(h, 2, two.get(), 0) == FX_E_ARG);   // (metering off)
    fxb_destroy(h);
    // a handle destroyed with the mode on frees the rows (LeakSanitizer)
    h = create(n, 1, devices);
    setTones(h, m, 8, 1, n);
    play(h, m, 5);
    fxb_destroy(h);
}

// an allocation that fails, at each allocation of a set (one per shard), with the mode off and with it on: FX_E_MEMORY, the mode
// as it was everywhere, then the call goes through
void memory(int devices) {
    const int64_t n = devices > 1 ? 808 : 200;
    for (int on = 0; on < 2; ++on)
        for (int nth = 0; nth < devices; ++nth) {
            fxb_handle* h = create(n, 2, devices);
            Tones m;
            if (on) setTones(h, m, 2, 2, n);
            {
                const size_t words = 8 * 2 * (size_t)n;
                std::unique_ptr<float[]> in(new float[words]), out(new float[words]);
                for (size_t i = 0; i < words; ++i) in[i] = word();
                CHECK(fxb_process_block(h, in.get(), out.get(), 8) == 0);
                if (on) m.take(out.get(), 8);
            }
            CHECK(fxb_prepare(h, 8, 1) == 0);   // (the builder threads are idle: no allocation of their own meets the injected failure)
            std::unique_ptr<double[]> c(new double[3]);
            c[0] = 0.5, c[1] = 1.5, c[2] = -1.5;
            fxstub_fail_mallocs(nth, 1);
            const int rc = fxb_meter_set_tones(h, 3, c.get(), 0);
            fxstub_fail_mallocs(-1, 0);
            CHECK(rc == FX_E_MEMORY && fxb_last_error(h)[0] != 0);
            if (on) {
                compare(h, m);
                play(h, m, 4);
                compare(h, m);
            } else {
                CHECK(fxb_meter_get_tones(h, nullptr, nullptr) == FX_E_ARG && fxb_meter_read_tones(h, nullptr, nullptr, nullptr, 0) == FX_E_ARG);
            }
            setTones(h, m, 3, 2, n);
            play(h, m, 8);
            compare(h, m);
            CHECK(fxb_info(h, FXB_INFO_METER_TONE_LAUNCHES) == (on ? 3 : 1) * devices);
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
        std::printf("  tone meters, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_tone_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "tone meter checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("tone meter checks ok\n");
    return 0;
}
