// gain_list_checks.cpp — the gain sets by list of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan +
// LeakSanitizer (TEST INFRASTRUCTURE: csrc/Makefile `stubasangainlist` links this file with the library's host sources and
// tests/hipstub/; a program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The values are pinned by tests/test_bus_gain_list_stub.py; this program is about addresses.  Every array the caller hands in is
// a heap block of exactly the documented size - [count] indices, [C][count] values - and every "device" block of the stand-in is a
// heap block too, so a read or write one word outside the list, the values, the staging or a gain block of any of the three
// layouts is a report.  It walks the indexing shapes for C = 1 and 2 with the three pitches - N for the bus gains, E for the
// sends, the quad-padded pitch for the feeds (CSR and map form, E no multiple of 4) - with lists of 1, 2, 63, 64, 65 and all
// entries, the first and the last index always among them, on one handle and on three shards; the refusals (nothing changes);
// and allocation failures at every allocation of a call.  Where a result follows without redoing the arithmetic it is checked:
// what get returns after each set, by the definition of include/fx8010_amd.h "Gain sets by list".
// Exit code 0 = every check held (a sanitizer report turns it non-zero by itself).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/fx8010_amd.h"
#include "hip_stub.h"

extern "C" long fxstub_gain_scatter_strays(void);   // fx_gain_scatter_stub.cpp

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            ++g_failures;                                                                \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                                \
    } while (0)

const char* kMono = "input in 0\noutput out 0\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nend";
const char* kStereo = "input in 0\ninput in1 1\noutput out 0\noutput out1 1\ncontrol vol = 0.5\nstatic a\nmacs a, a, vol, in\nmacs out, a, in, 0.25\nmacs out1, in1, a, 0.5\nend";

uint32_t g_seed = 2468u;
uint32_t draw() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}
float noise() { return (float)((int)(draw() & 0xffff) - 32768) / 20000.0f; }

std::vector<float> filled(size_t n) {
    std::vector<float> v(n);
    for (float& x : v) x = noise();
    return v;
}

bool sameWords(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0; }

// `count` distinct indices of 0..range-1 in a shuffled order, the first and the last index among them (from two entries on)
std::vector<int64_t> someOf(int64_t range, int64_t count) {
    std::vector<int64_t> all((size_t)range);
    for (int64_t i = 0; i < range; ++i) all[(size_t)i] = i;
    for (int64_t i = range - 1; i > 0; --i) std::swap(all[(size_t)i], all[(size_t)(draw() % (uint32_t)(i + 1))]);
    count = std::min(count, range);
    if (count >= 2 && count < range) {
        std::swap(*std::find(all.begin(), all.end(), 0), all[0]);
        std::swap(*std::find(all.begin() + 1, all.end(), range - 1), all[(size_t)count - 1]);
    }
    all.resize((size_t)count);
    return all;
}

enum Kind { kGains, kSends, kFeeds, kFeedMap };

// one of the three structures on a handle, with the a / b / pending the definition gives it
struct Mixer {
    fxb_handle* h = nullptr;
    Kind kind = kGains;
    int ch = 1;
    int64_t n = 0, width = 0;   // instances; N, or E
    std::vector<float> a, b;
    bool pending = false;

    bool install(bool weighted) {
        std::vector<float> g;
        if (kind == kGains) {
            width = n;
            g = filled((size_t)ch * (size_t)width);
            if (fxb_bus_set_gains(h, g.data(), 0) != 0) return false;
        } else if (kind == kSends) {
            // buses on the last, the first and the middle third of the instances (808 instances: the three shards, which begin at 0, 320 and 576), and an empty one
            const int64_t sizes[5] = {65, 1030, 3, 0, 64}, part[5] = {2, 0, 1, 0, 1};
            std::vector<int64_t> offsets{0}, members;
            for (int j = 0; j < 5; ++j) {
                const int64_t starts[4] = {0, n == 808 ? 320 : n / 3, n == 808 ? 576 : 2 * n / 3, n};
                const int64_t lo = starts[part[j]], hi = std::max(lo + 1, starts[part[j] + 1]);
                for (int64_t e = 0; e < sizes[j]; ++e) members.push_back(std::min(n - 1, lo + (int64_t)(draw() % (uint32_t)(hi - lo))));
                offsets.push_back((int64_t)members.size());
            }
            width = (int64_t)members.size();
            g = filled((size_t)ch * (size_t)width);
            if (fxb_bus_set_sends(h, 5, offsets.data(), members.data(), g.data()) != 0) return false;
        } else {
            std::vector<int64_t> offsets{0}, sources;
            const int64_t M = 7;
            for (int64_t i = 0; i < n; ++i) {
                const int64_t entries = kind == kFeedMap ? 1 : (i == 0 ? 3 : (i == n - 1 ? 1 : (int64_t)(draw() % 3u) * 3 / 2));   // 0, 1 or 3
                for (int64_t e = 0; e < entries; ++e) sources.push_back((int64_t)(draw() % (uint32_t)M));
                offsets.push_back((int64_t)sources.size());
            }
            width = (int64_t)sources.size();
            g = weighted ? filled((size_t)ch * (size_t)width) : std::vector<float>((size_t)ch * (size_t)width, 1.0f);
            if (fxb_bus_set_feeds(h, M, offsets.data(), sources.data(), weighted ? g.data() : nullptr) != 0) return false;
        }
        a = b = g;
        pending = false;
        return true;
    }
    int raw(const int64_t* list, int64_t count, const float* gains, int ramp) const {
        return kind == kGains ? fxb_bus_set_gains_list(h, list, count, gains, ramp)
             : kind == kSends ? fxb_bus_set_send_gains_list(h, list, count, gains, ramp)
                              : fxb_bus_set_feed_gains_list(h, list, count, gains, ramp);
    }
    // the set through exactly-sized heap blocks, and the definition beside it
    bool listed(const std::vector<int64_t>& list, int ramp) {
        std::vector<float> g = filled((size_t)ch * list.size());
        std::vector<int64_t> given = list;
        if (raw(given.data(), (int64_t)given.size(), g.data(), ramp) != 0) return false;
        if (ramp && !pending) a = b;
        for (int c = 0; c < ch; ++c)
            for (size_t k = 0; k < list.size(); ++k) {
                const size_t at = (size_t)c * (size_t)width + (size_t)list[k];
                b[at] = g[(size_t)c * list.size() + k];
                if (!ramp) a[at] = b[at];
            }
        if (ramp) pending = true;
        std::fill(given.begin(), given.end(), -1);   // the arrays are the caller's again on return
        std::fill(g.begin(), g.end(), std::numeric_limits<float>::quiet_NaN());
        return true;
    }
    std::vector<float> get() const {
        std::vector<float> g((size_t)ch * (size_t)width);
        if (kind == kGains) CHECK(fxb_bus_get_gains(h, g.data()) == 0);
        else if (kind == kSends) CHECK(fxb_bus_get_sends(h, nullptr, nullptr, 0, nullptr, g.data(), width) == width);
        else CHECK(fxb_bus_get_feeds(h, nullptr, nullptr, 0, nullptr, g.data(), width) == width);
        return g;
    }
    const std::vector<float>& inForce() const { return pending ? a : b; }
    // a block that consumes a pending ramp
    bool block(int S) {
        const int64_t K = 64, G = fxb_bus_groups(h, K);
        int rc;
        if (kind == kFeeds || kind == kFeedMap) {
            const std::vector<float> src = filled((size_t)S * ch * 7);
            std::vector<float> out((size_t)S * ch * (size_t)n);
            rc = fxb_process_block_bus_feed(h, src.data(), out.data(), nullptr, nullptr, S, K, 0);
        } else {
            const std::vector<float> in = filled((size_t)S * ch * (size_t)G);
            std::vector<float> out((size_t)S * ch * (size_t)G), aux((size_t)S * ch * 5);
            rc = kind == kSends ? fxb_process_block_bus_aux(h, in.data(), out.data(), nullptr, aux.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT)
                                : fxb_process_block_bus(h, in.data(), out.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT);
        }
        a = b;
        pending = false;
        return rc == 0;
    }
};

fxb_handle* create(int64_t N, int ch, int devices) {
    const int three[3] = {0, 1, 2};
    return devices > 1 ? fxb_create_on_devices(N, ch, three, 3) : fxb_create(N, ch, 0);
}

// one handle (devices == 1) or three shards through every indexing shape
void indexing(int devices) {
    const int64_t single[4] = {5, 65, 200, 777}, sharded[1] = {808};
    const Kind kinds[4] = {kGains, kSends, kFeeds, kFeedMap};
    for (int which = 0; which < (devices > 1 ? 1 : 4); ++which)
        for (int ch = 1; ch <= 2; ++ch)
            for (Kind kind : kinds) {
                Mixer m;
                m.kind = kind;
                m.ch = ch;
                m.n = devices > 1 ? sharded[which] : single[which];
                m.h = create(m.n, ch, devices);
                CHECK(m.h != nullptr);
                if (!m.h) return;
                CHECK(m.install(false));   // (feeds: unweighted - the first list set makes them weighted, a = b = 1.0f)
                CHECK(fxb_load_text(m.h, ch == 1 ? kMono : kStereo) == 1);
                const int64_t counts[6] = {1, 2, 63, 64, 65, m.width};
                int64_t sets = 0;
                for (int round = 0; round < 6; ++round) {
                    const int S = round % 2 ? 1 : 33;
                    // ramp 1 with none pending, ramp 1 with one pending, a block; ramp 0 with none pending; ramp 1, ramp 0 while pending, a block
                    CHECK(m.listed(someOf(m.width, counts[round]), 1) && sameWords(m.get(), m.inForce()));
                    CHECK(m.listed(someOf(m.width, counts[(round + 3) % 6]), 1) && sameWords(m.get(), m.inForce()));
                    CHECK(m.block(S) && sameWords(m.get(), m.inForce()));
                    CHECK(m.listed(someOf(m.width, counts[(round + 1) % 6]), 0) && sameWords(m.get(), m.inForce()));
                    CHECK(m.block(S));
                    CHECK(m.listed(someOf(m.width, counts[(round + 2) % 6]), 1) && sameWords(m.get(), m.inForce()));
                    CHECK(m.listed(someOf(m.width, counts[round]), 0) && m.pending && sameWords(m.get(), m.inForce()));
                    CHECK(m.block(S) && sameWords(m.get(), m.inForce()));
                    sets += 5;
                }
                CHECK(fxb_info(m.h, FXB_INFO_GAIN_LIST_SETS) >= sets && fxb_info(m.h, FXB_INFO_GAIN_LIST_SETS) <= sets * devices);
                CHECK(m.raw(nullptr, 0, nullptr, 1) == 0 && sameWords(m.get(), m.inForce()));   // count 0: nothing
                fxb_destroy(m.h);
            }
}

void refusals(int devices) {
    const Kind kinds[3] = {kGains, kSends, kFeeds};
    for (Kind kind : kinds) {
        Mixer m;
        m.kind = kind;
        m.ch = 2;
        m.n = 808;
        m.h = create(m.n, 2, devices);
        CHECK(m.h != nullptr);
        if (!m.h) return;
        const std::vector<int64_t> good{3, 0, 80};
        const std::vector<float> values = filled(6);
        for (int ramp = 0; ramp <= 1; ++ramp) CHECK(m.raw(good.data(), 3, values.data(), ramp) == FX_E_ARG);   // the mode is off
        CHECK(m.install(true));
        for (int state = 0; state < 2; ++state) {   // static, a ramp pending
            if (state == 1) CHECK(m.listed(someOf(m.width, 65), 1));
            const int64_t sets = fxb_info(m.h, FXB_INFO_GAIN_LIST_SETS);
            const long live = fxstub_live_allocations();
            const float bads[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
            for (int ramp = 0; ramp <= 1; ++ramp) {
                const std::vector<int64_t> twice{5, 9, 5}, above{0, m.width, 1}, below{0, 1, -1};
                CHECK(m.raw(twice.data(), 3, values.data(), ramp) == FX_E_ARG);
                CHECK(m.raw(above.data(), 3, values.data(), ramp) == FX_E_ARG);
                CHECK(m.raw(below.data(), 3, values.data(), ramp) == FX_E_ARG);
                for (int k = 0; k < 3; ++k) {
                    std::vector<float> bad = values;
                    bad[(size_t)k * 2 + 1] = bads[k];
                    CHECK(m.raw(good.data(), 3, bad.data(), ramp) == FX_E_ARG);
                }
                CHECK(m.raw(good.data(), -1, values.data(), ramp) == FX_E_ARG);
                CHECK(m.raw(nullptr, 3, values.data(), ramp) == FX_E_ARG);
                CHECK(m.raw(good.data(), 3, nullptr, ramp) == FX_E_ARG);
            }
            const int ramps[3] = {2, -1, 256};
            for (int ramp : ramps) {
                CHECK(m.raw(good.data(), 3, values.data(), ramp) == FX_E_ARG);
                CHECK(m.raw(nullptr, 0, nullptr, ramp) == FX_E_ARG);
            }
            CHECK(fxstub_live_allocations() == live && fxb_info(m.h, FXB_INFO_GAIN_LIST_SETS) == sets);
            CHECK(sameWords(m.get(), m.inForce()));
        }
        Mixer none = m;
        none.h = nullptr;
        CHECK(none.raw(good.data(), 3, values.data(), 0) == FX_E_ARG);
        // the handle goes on: the pending ramp is consumed by the next block
        CHECK(fxb_load_text(m.h, kStereo) == 1);
        CHECK(m.block(8) && sameWords(m.get(), m.inForce()));
        fxb_destroy(m.h);
    }
}

// an allocation that fails inside a call, at every allocation it makes (the device staging and the pinned staging of every
// shard): FX_E_MEMORY, nothing has changed on any shard, and the same call goes through afterwards
void memory(int devices) {
    const Kind kinds[3] = {kGains, kSends, kFeeds};
    for (Kind kind : kinds)
        for (long nth = 0; nth < 2L * devices; ++nth) {
            Mixer m;
            m.kind = kind;
            m.ch = 2;
            m.n = 808;
            m.h = create(m.n, 2, devices);   // (no program: no builder thread allocates meanwhile)
            CHECK(m.h != nullptr);
            if (!m.h) return;
            CHECK(m.install(true));
            const std::vector<int64_t> list = someOf(m.width, m.width / 2);   // (entries on every shard)
            const std::vector<float> values = filled(2 * list.size());
            fxstub_fail_mallocs(nth, 1);
            const int rc = m.raw(list.data(), (int64_t)list.size(), values.data(), (int)(nth & 1) ^ 1);
            fxstub_fail_mallocs(-1, 0);
            CHECK(rc == FX_E_MEMORY);
            CHECK(fxb_info(m.h, FXB_INFO_GAIN_LIST_SETS) == 0 && sameWords(m.get(), m.inForce()));
            CHECK(m.listed(list, 0) && sameWords(m.get(), m.inForce()));   // (had a ramp begun on some shard, get would show its a there)
            CHECK(m.listed(list, 1) && sameWords(m.get(), m.inForce()));   // destroyed with a ramp pending and a scatter queued
            fxb_destroy(m.h);
        }
}

}  // namespace

int main() {
    setenv("FXSTUB_DEVICES", "3", 1);   // (read by the stand-in at its first call)
    for (int devices = 1; devices <= 3; devices += 2) {
        indexing(devices);
        refusals(devices);
        memory(devices);
        std::printf("  gain lists, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_gain_scatter_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "gain list checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("gain list checks ok\n");
    return 0;
}
