// meter_list_checks.cpp — the meter queries by list of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan +
// LeakSanitizer (TEST INFRASTRUCTURE: csrc/Makefile `stubasanmeterlist` links this file with the library's host sources and
// tests/hipstub/; a program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The comparison with the numpy model is tests/test_meter_list_stub.py; this program is about addresses.  Every array the caller
// hands in is a heap block of exactly the documented size - [cap] instance numbers for a select, [count] for a list,
// [channels][count] per output - and every "device" block of the stand-in is a heap block too, so a read or write one word outside
// the list, an output, the staging or an accumulator row is a report.  It walks cap = M, M - 1, M + 1, 1 and 0 (a null list),
// ranges that start and end at any instance, lists of one, two, 63, 64, 65 and all entries with the first and the last instance
// among them, count = 0, null outputs, for N = 1, 5, 65, 200 and 777 on one handle and N = 808 on three shards, with one, two and
// four channels; the refusals (nothing changes); and allocation failures at every allocation of a call.  What comes back is checked
// against fxb_meter_read with plain loops written from the definition in include/fx8010_amd.h "Meter queries by list".
// Exit code 0 = every check held (a sanitizer report turns it non-zero by itself).
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

extern "C" long fxstub_meter_selects(void);   // fx_meter_list_stub.cpp
extern "C" long fxstub_meter_gathers(void);
extern "C" long fxstub_meter_zeros(void);
extern "C" long fxstub_meter_list_strays(void);

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

struct Meters {
    int channels = 0;
    int64_t n = 0;
    std::vector<double> energy;
    std::vector<float> peak;
    std::vector<uint32_t> fullScale, nonfinite;
    double value(int stat, int64_t i) const {
        double best = 0;
        for (int c = 0; c < channels; ++c) {
            const size_t at = (size_t)c * (size_t)n + (size_t)i;
            const double v = stat == 0 ? energy[at] : stat == 1 ? (double)peak[at] : stat == 2 ? (double)fullScale[at] : (double)nonfinite[at];
            best = (c == 0 || v > best) ? v : best;
        }
        return best;
    }
    bool operator==(const Meters& o) const {
        return energy.size() == o.energy.size() && std::memcmp(energy.data(), o.energy.data(), energy.size() * 8) == 0 && std::memcmp(peak.data(), o.peak.data(), peak.size() * 4) == 0 &&
               fullScale == o.fullScale && nonfinite == o.nonfinite;
    }
};

Meters readAll(fxb_handle* h, int channels, int64_t n) {
    Meters m;
    m.channels = channels;
    m.n = n;
    const size_t k = (size_t)channels * (size_t)n;
    m.energy.resize(k);
    m.peak.resize(k);
    m.fullScale.resize(k);
    m.nonfinite.resize(k);
    CHECK(fxb_meter_read(h, m.energy.data(), m.peak.data(), m.fullScale.data(), m.nonfinite.data(), 0) == 0);
    return m;
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

// a block whose words decide the meters (the stand-in's emulation launch copies input to output): levels, the rail, NaN, +-Inf, silence
void play(fxb_handle* h, int64_t n, int channels, int samples) {
    const size_t words = (size_t)samples * (size_t)channels * (size_t)n;
    std::unique_ptr<float[]> in(new float[words]), out(new float[words]);
    for (size_t i = 0; i < words; ++i) {
        const uint32_t d = draw();
        const uint32_t kind = (d >> 4) % 16;
        in[i] = kind == 0 ? 0.0f : kind == 1 ? 1.0f : kind == 2 ? -1.0f : kind == 3 ? std::numeric_limits<float>::quiet_NaN() : kind == 4 ? -std::numeric_limits<float>::infinity()
                                                                                                                                 : (float)((d >> 8) % 1000) / 1000.0f;
        if ((i % (size_t)n) % 5 == 3) in[i] = 0.0f;   // silent voices
    }
    CHECK(fxb_process_block(h, in.get(), out.get(), samples) == 0);
}

// a select into a block of exactly `cap` words; what it must hold and return from the definition
void selectOnce(fxb_handle* h, const Meters& m, int stat, double t, bool below, int64_t first, int64_t nRange, int64_t cap) {
    std::vector<int64_t> want;
    for (int64_t i = first; i < first + nRange; ++i)
        if (below ? m.value(stat, i) < t : m.value(stat, i) >= t) want.push_back(i);
    std::unique_ptr<int64_t[]> list(cap > 0 ? new int64_t[(size_t)cap] : nullptr);
    for (int64_t i = 0; i < cap; ++i) list[(size_t)i] = -77;
    const int64_t got = fxb_meter_select(h, stat, t, first, nRange, list.get(), cap, below ? FXB_METER_BELOW : 0u);
    CHECK(got == (int64_t)want.size());
    const int64_t take = std::min<int64_t>(cap, (int64_t)want.size());
    for (int64_t i = 0; i < cap; ++i) CHECK(list[(size_t)i] == (i < take ? want[(size_t)i] : -77));
}

void selects(fxb_handle* h, const Meters& m) {
    const int64_t n = m.n;
    for (int stat = 0; stat < 4; ++stat) {
        const double mid = m.value(stat, n / 2), ts[6] = {-INFINITY, 0.0, mid, std::nextafter(mid, INFINITY), 0.5, INFINITY};
        for (const double t : ts)
            for (int below = 0; below < 2; ++below) {
                int64_t M = 0;
                for (int64_t i = 0; i < n; ++i) M += (below ? m.value(stat, i) < t : m.value(stat, i) >= t) ? 1 : 0;
                const int64_t caps[6] = {M, std::max<int64_t>(M - 1, 0), M + 1, 1, 0, n + 5};
                for (const int64_t cap : caps) selectOnce(h, m, stat, t, below != 0, 0, n, cap);
                const int64_t firsts[5] = {0, 1, std::min<int64_t>(63, n), std::min<int64_t>(64, n), n / 2};
                for (const int64_t first : firsts) {
                    const int64_t ranges[4] = {0, std::min<int64_t>(1, n - first), std::min<int64_t>(64, n - first), n - first};
                    for (const int64_t r : ranges) {
                        selectOnce(h, m, stat, t, below != 0, first, r, r);
                        selectOnce(h, m, stat, t, below != 0, first, r, r / 2);
                    }
                }
            }
    }
}

std::vector<int64_t> listOf(int64_t n, int64_t count) {
    std::vector<int64_t> list((size_t)count);
    for (int64_t i = 0; i < count; ++i) list[(size_t)i] = (int64_t)(draw() % (uint32_t)n);
    if (count >= 1) list[0] = n - 1;
    if (count >= 2) list[(size_t)count - 1] = 0;
    return list;
}

// no two alike
std::vector<int64_t> distinctOf(int64_t n, int64_t count) {
    std::vector<int64_t> all((size_t)n);
    for (int64_t i = 0; i < n; ++i) all[(size_t)i] = n - 1 - i;
    for (int64_t i = n - 1; i > 1; --i) std::swap(all[(size_t)i], all[1 + draw() % (uint32_t)i]);
    all.resize((size_t)std::min(count, n));
    return all;
}

void readOnce(fxb_handle* h, const Meters& m, const std::vector<int64_t>& list, int which, bool reset) {
    const size_t count = list.size(), k = (size_t)m.channels * count;
    std::unique_ptr<int64_t[]> l(count ? new int64_t[count] : nullptr);
    std::copy(list.begin(), list.end(), l.get());
    std::unique_ptr<double[]> e((which & 1) && k ? new double[k] : nullptr);
    std::unique_ptr<float[]> p((which & 2) && k ? new float[k] : nullptr);
    std::unique_ptr<uint32_t[]> f((which & 4) && k ? new uint32_t[k] : nullptr), q((which & 8) && k ? new uint32_t[k] : nullptr);
    CHECK(fxb_meter_read_list(h, l.get(), (int64_t)count, e.get(), p.get(), f.get(), q.get(), reset ? 1 : 0) == 0);
    for (int c = 0; c < m.channels; ++c)
        for (size_t i = 0; i < count; ++i) {
            const size_t at = (size_t)c * count + i, from = (size_t)c * (size_t)m.n + (size_t)list[i];
            if (e) CHECK(std::memcmp(&e[at], &m.energy[from], 8) == 0);
            if (p) CHECK(std::memcmp(&p[at], &m.peak[from], 4) == 0);
            if (f) CHECK(f[at] == m.fullScale[from]);
            if (q) CHECK(q[at] == m.nonfinite[from]);
        }
}

Meters zeroed(Meters m, const std::vector<int64_t>& list) {
    for (int c = 0; c < m.channels; ++c)
        for (const int64_t i : list) {
            const size_t at = (size_t)c * (size_t)m.n + (size_t)i;
            m.energy[at] = 0.0;
            m.peak[at] = 0.0f;
            m.fullScale[at] = m.nonfinite[at] = 0;
        }
    return m;
}

void indexing(int devices) {
    const int64_t single[5] = {1, 5, 65, 200, 777}, sharded[1] = {808};
    const int64_t* sizes = devices > 1 ? sharded : single;
    const int nSizes = devices > 1 ? 1 : 5;
    for (int s = 0; s < nSizes; ++s)
        for (int channels = 1; channels <= 4; channels *= 2) {
            const int64_t n = sizes[s];
            fxb_handle* h = create(n, channels, devices);
            play(h, n, channels, 9);
            play(h, n, channels, 4);
            Meters m = readAll(h, channels, n);
            selects(h, m);
            CHECK(readAll(h, channels, n) == m);
            const int64_t counts[7] = {0, 1, 2, 63, 64, 65, n};
            for (const int64_t count : counts) {
                readOnce(h, m, listOf(n, count), 15, false);
                readOnce(h, m, listOf(n, count), 1 << (int)(count % 4), false);
                readOnce(h, m, listOf(n, count), 0, false);
                const std::vector<int64_t> distinct = distinctOf(n, count);
                readOnce(h, m, distinct, 15, true);
                m = zeroed(m, distinct);
                CHECK(readAll(h, channels, n) == m);
                play(h, n, channels, 3);
                m = readAll(h, channels, n);
                // a list reset between two blocks, repeats allowed, the list on an exactly-sized block that is freed at once
                const std::vector<int64_t> again = listOf(n, count);
                {
                    std::unique_ptr<int64_t[]> l(count ? new int64_t[(size_t)count] : nullptr);
                    std::copy(again.begin(), again.end(), l.get());
                    CHECK(fxb_meter_reset_list(h, l.get(), count) == 0);
                }
                CHECK(readAll(h, channels, n) == zeroed(m, again));
                play(h, n, channels, 2);
                m = readAll(h, channels, n);
            }
            CHECK(fxb_meter_samples(h) == 9 + 4 + 7 * 5);
            fxb_destroy(h);
        }
}

void refusals(int devices) {
    const int64_t n = devices > 1 ? 808 : 200;
    fxb_handle* h = create(n, 2, devices);
    play(h, n, 2, 8);
    const Meters m = readAll(h, 2, n);
    const int64_t seen[3] = {fxb_info(h, FXB_INFO_METER_SELECTS), fxb_info(h, FXB_INFO_METER_LIST_READS), fxb_info(h, FXB_INFO_METER_LIST_RESETS)};
    const long ran[3] = {fxstub_meter_selects(), fxstub_meter_gathers(), fxstub_meter_zeros()};
    std::unique_ptr<int64_t[]> list(new int64_t[3]);
    std::unique_ptr<double[]> e(new double[6]);
    list[0] = list[1] = list[2] = -77;
    CHECK(fxb_meter_select(h, 4, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select(h, -1, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select(h, 1, std::nan(""), 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select(h, 1, 0.0, -1, 2, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select(h, 1, 0.0, 0, -1, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select(h, 1, 0.0, 1, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select(h, 1, 0.0, n, INT64_MAX, list.get(), 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select(h, 1, 0.0, 0, n, list.get(), -1, 0) == FX_E_ARG);
    CHECK(fxb_meter_select(h, 1, 0.0, 0, n, nullptr, 3, 0) == FX_E_ARG);
    CHECK(fxb_meter_select(h, 1, 0.0, 0, n, list.get(), 3, 2u) == FX_E_ARG);
    CHECK(fxb_meter_select(nullptr, 1, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG);
    CHECK(list[0] == -77 && list[1] == -77 && list[2] == -77);
    const int64_t bad[4][3] = {{0, n, 1}, {0, 1, -1}, {5, 9, 5}, {INT64_MIN, 0, 1}};
    for (int k = 0; k < 4; ++k) {
        std::copy(bad[k], bad[k] + 3, list.get());
        CHECK(fxb_meter_read_list(h, list.get(), 3, e.get(), nullptr, nullptr, nullptr, 1) == FX_E_ARG);
        if (k != 2) CHECK(fxb_meter_read_list(h, list.get(), 3, e.get(), nullptr, nullptr, nullptr, 0) == FX_E_ARG);
        if (k != 2) CHECK(fxb_meter_reset_list(h, list.get(), 3) == FX_E_ARG);
    }
    CHECK(fxb_meter_read_list(h, list.get(), -1, e.get(), nullptr, nullptr, nullptr, 0) == FX_E_ARG && fxb_meter_reset_list(h, list.get(), -1) == FX_E_ARG);
    CHECK(fxb_meter_read_list(h, nullptr, 3, e.get(), nullptr, nullptr, nullptr, 0) == FX_E_ARG && fxb_meter_reset_list(h, nullptr, 3) == FX_E_ARG);
    CHECK(fxb_meter_read_list(h, list.get(), (int64_t)1 << 31, e.get(), nullptr, nullptr, nullptr, 0) == FX_E_ARG);
    CHECK(fxb_meter_read_list(nullptr, list.get(), 3, e.get(), nullptr, nullptr, nullptr, 0) == FX_E_ARG && fxb_meter_reset_list(nullptr, list.get(), 3) == FX_E_ARG);
    CHECK(fxb_info(h, FXB_INFO_METER_SELECTS) == seen[0] && fxb_info(h, FXB_INFO_METER_LIST_READS) == seen[1] && fxb_info(h, FXB_INFO_METER_LIST_RESETS) == seen[2]);
    CHECK(fxstub_meter_selects() == ran[0] && fxstub_meter_gathers() == ran[1] && fxstub_meter_zeros() == ran[2]);
    CHECK(readAll(h, 2, n) == m);
    // metering off
    CHECK(fxb_meter_enable(h, 0) == 0);
    list[0] = 0;
    CHECK(fxb_meter_select(h, 1, 0.0, 0, n, list.get(), 3, 0) == FX_E_ARG && fxb_meter_select(h, 1, 0.0, 0, 0, nullptr, 0, 0) == FX_E_ARG);
    CHECK(fxb_meter_read_list(h, list.get(), 1, e.get(), nullptr, nullptr, nullptr, 0) == FX_E_ARG && fxb_meter_reset_list(h, list.get(), 1) == FX_E_ARG);
    fxb_destroy(h);
}

// an allocation that fails, at each allocation of a call (two per shard): FX_E_MEMORY, nothing changed, then the call goes through
void memory(int devices) {
    const int64_t n = devices > 1 ? 808 : 200;
    const std::vector<int64_t> all = distinctOf(n, n);
    for (int call = 0; call < 3; ++call)
        for (int nth = 0; nth < 2 * devices; ++nth) {
            fxb_handle* h = create(n, 2, devices);
            play(h, n, 2, 8);
            const Meters m = readAll(h, 2, n);
            CHECK(fxb_prepare(h, 8, 1) == 0);   // (the builder threads are idle: no allocation of their own meets the injected failure)
            std::unique_ptr<int64_t[]> list(new int64_t[(size_t)n]);
            std::copy(all.begin(), all.end(), list.get());
            std::unique_ptr<float[]> p(new float[2 * (size_t)n]);
            int64_t rc[2];
            for (int round = 0; round < 2; ++round) {
                if (round == 0) fxstub_fail_mallocs(nth, 1);
                rc[round] = call == 0 ? fxb_meter_select(h, 1, 0.0, 0, n, list.get(), n, 0)
                                      : call == 1 ? fxb_meter_read_list(h, list.get(), n, nullptr, p.get(), nullptr, nullptr, 1) : fxb_meter_reset_list(h, list.get(), n);
                fxstub_fail_mallocs(-1, 0);
                if (round == 0) {
                    CHECK(rc[0] == FX_E_MEMORY && fxb_last_error(h)[0] != 0);
                    CHECK(readAll(h, 2, n) == m);
                    CHECK(fxb_info(h, FXB_INFO_METER_SELECTS) + fxb_info(h, FXB_INFO_METER_LIST_READS) + fxb_info(h, FXB_INFO_METER_LIST_RESETS) == 0);
                }
            }
            CHECK(rc[1] == (call == 0 ? n : 0));
            CHECK(readAll(h, 2, n) == (call == 0 ? m : zeroed(m, all)));
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
        std::printf("  meter lists, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_meter_list_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "meter list checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("meter list checks ok\n");
    return 0;
}
