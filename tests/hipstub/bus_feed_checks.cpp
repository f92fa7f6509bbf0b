// bus_feed_checks.cpp — the bus feeds of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan + LeakSanitizer
// (TEST INFRASTRUCTURE: csrc/Makefile `stubasanfeeds` links this file with the library's host sources and tests/hipstub/; a
// program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The routes and the state machine are pinned by tests/test_bus_feed_stub.py; this program is about addresses.  Every array the
// caller hands in is a heap block of exactly the documented size, every "device" block of the stand-in is a heap block too, so a
// read or write one word outside the offsets, the sources, the [C][E] gains, the [S][C][M] source rows, the PCM, the padded
// tables of the device block, a shard's run of the entries or the device copy of the source rows is a report.  It walks CSR
// structures with lists of 0 .. 65 entries and the map form (one and two channels; blocks of 33 and 1 samples; unweighted, static
// and ramping; pageable and pinned source rows; one handle and three shards), the round trip under caps of every size, the
// refusals (nothing changes, the output stays untouched) and an allocation failure at every allocation of a set and of the
// source staging.  The stand-in's emulation launch copies in to out, so `out` is the definition of include/fx8010_amd.h itself.
// Exit code 0 = every check held (a sanitizer report turns it non-zero by itself).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/fx8010_amd.h"
#include "hip_stub.h"

extern "C" long fxstub_bus_feeds(void);
extern "C" long fxstub_bus_feed_strays(void);

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

uint32_t g_seed = 5171u;
uint32_t draw() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

// finite words of many magnitudes
std::vector<float> filled(size_t n) {
    std::vector<float> v(n);
    for (float& x : v) x = ((float)(draw() % 20001u) - 10000.0f) * (1.0f / (float)(1u << (draw() % 24u)));
    return v;
}

const int64_t kN = 809, kM = 70;   // three shards: instances from 0, 320 and 576; an odd count: the padding of every table is in use

struct Structure {
    std::vector<int64_t> offsets{0}, sources;
    int64_t entries() const { return offsets.back(); }
};

// lists of 0, 1, 2, 5 and 65 entries (map: one each), the first and the last instance always fed; `quiet`: no entry in lo .. hi - 1
Structure lists(bool map, int64_t quietLo = 0, int64_t quietHi = 0) {
    const int64_t sizes[5] = {0, 1, 2, 5, 65};
    Structure s;
    for (int64_t i = 0; i < kN; ++i) {
        int64_t count = map ? 1 : sizes[draw() % 5u];
        if (!map && (i == 0 || i == kN - 1)) count = 5;
        if (i >= quietLo && i < quietHi) count = 0;
        for (int64_t k = 0; k < count; ++k) s.sources.push_back((int64_t)(draw() % (uint32_t)kM));
        s.offsets.push_back((int64_t)s.sources.size());
    }
    return s;
}

// the [S * C][N] block a feed block of S samples must have built from the source rows x [S * C][M]; gains null: unweighted
bool blockRight(const float* got, const std::vector<float>& x, int S, int ch, const Structure& s, const std::vector<float>* a, const std::vector<float>* b, bool ramp) {
    const int64_t E = s.entries();
    const float r = 1.0f / (float)S;
    for (int smp = 0; smp < S; ++smp)
        for (int c = 0; c < ch; ++c)
            for (int64_t i = 0; i < kN; ++i) {
                float word = 0.0f;
                for (int64_t e = s.offsets[(size_t)i]; e < s.offsets[(size_t)i + 1]; ++e) {
                    float term = x[(size_t)(((int64_t)smp * ch + c) * kM + s.sources[(size_t)e])];
                    if (b) {
                        volatile float w = (*b)[(size_t)(c * E + e)];
                        if (ramp && smp != S - 1) {
                            volatile float t = (float)(smp + 1) * r;
                            volatile float d = (*b)[(size_t)(c * E + e)] - (*a)[(size_t)(c * E + e)];
                            volatile float m = d * t;
                            w = (*a)[(size_t)(c * E + e)] + m;
                        }
                        volatile float prod = 0.0f;
                        if (w != 0.0f) prod = w * term;
                        term = prod;
                    }
                    if (e == s.offsets[(size_t)i]) {
                        word = term;
                    } else {
                        volatile float sum = word + term;
                        word = sum;
                    }
                }
                if (std::memcmp(&got[((int64_t)smp * ch + c) * kN + i], &word, 4) != 0) return false;
            }
    return true;
}

struct PinnedRows {
    float* p = nullptr;
    explicit PinnedRows(size_t floats) { p = static_cast<float*>(fxb_host_alloc(std::max<size_t>(floats, 1) * 4)); }
    ~PinnedRows() { fxb_host_free(p); }
};

bool feedsAre(fxb_handle* h, const Structure& s, const std::vector<float>& gains, int ch) {
    int64_t M = -1;
    const int64_t E = s.entries();
    if (fxb_bus_get_feeds(h, &M, nullptr, 0, nullptr, nullptr, 0) != E || M != kM) return false;
    std::vector<int64_t> off((size_t)kN + 1, -1), src((size_t)E, -1);
    std::vector<float> g((size_t)(ch * E), -7.0f);
    if (fxb_bus_get_feeds(h, nullptr, off.data(), kN + 1, src.data(), g.data(), E) != E) return false;
    return off == s.offsets && src == s.sources && std::memcmp(g.data(), gains.data(), g.size() * 4) == 0;
}

fxb_handle* handle(int devices, int ch) {
    const int three[3] = {0, 1, 2};
    return devices > 1 ? fxb_create_on_devices(kN, ch, three, 3) : fxb_create(kN, ch, 0);
}

// one handle (devices == 1) or three shards through structures, routes and the round trip
void indexing(int devices) {
    for (int ch = 1; ch <= 2; ++ch)
        for (int form = 0; form < 3; ++form) {   // CSR, CSR with a shard that owns no entry, the map
            fxb_handle* h = handle(devices, ch);
            CHECK(h != nullptr);
            if (!h) return;
            const Structure s = form == 2 ? lists(true) : (form == 1 ? lists(false, 320, 576) : lists(false));
            const int64_t E = s.entries();
            std::vector<float> g0 = filled((size_t)(ch * E)), g1 = filled((size_t)(ch * E));
            const std::vector<float> ones((size_t)(ch * E), 1.0f);
            g0[3] = 0.0f;
            g1[5] = -0.0f;
            {
                Structure given = s;
                CHECK(fxb_bus_set_feeds(h, kM, given.offsets.data(), given.sources.data(), nullptr) == 0);   // (before a program is loaded; unweighted)
                std::fill(given.offsets.begin(), given.offsets.end(), -1);                                     // the caller's arrays are free on return
                std::fill(given.sources.begin(), given.sources.end(), -1);
            }
            CHECK(fxb_load_text(h, ch == 1 ? kMono : kStereo) == 1);
            CHECK(feedsAre(h, s, ones, ch));
            // the round trip under caps of every kind: nothing beyond a cap is written (the blocks are exactly that long)
            for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)7, E - 1}) {
                std::vector<int64_t> off((size_t)std::min<int64_t>(cap, kN + 1)), src((size_t)cap);
                std::vector<float> g((size_t)(ch * E), -7.0f);   // (channel rows keep their pitch of E)
                CHECK(fxb_bus_get_feeds(h, nullptr, off.data(), (int64_t)off.size(), src.data(), g.data(), cap) == E);
                CHECK(std::equal(off.begin(), off.end(), s.offsets.begin()) && std::equal(src.begin(), src.end(), s.sources.begin()));
                for (int c = 0; c < ch; ++c)
                    for (int64_t e = 0; e < E; ++e) CHECK(e < cap ? g[(size_t)(c * E + e)] == 1.0f : g[(size_t)(c * E + e)] == -7.0f);
            }
            int64_t blocks = 0;
            const int lengths[4] = {33, 1, 33, 33};
            for (int step = 0; step < 4; ++step) {   // unweighted, static, ramping, the block after the ramp
                const int S = lengths[step];
                const bool ramp = step == 2;
                if (step == 1) CHECK(fxb_bus_set_feed_gains(h, g0.data(), 0) == 0 && feedsAre(h, s, g0, ch));
                if (ramp) CHECK(fxb_bus_set_feed_gains(h, g1.data(), 1) == 0 && feedsAre(h, s, g0, ch));
                const int64_t rows = (int64_t)S * ch;
                const std::vector<float> x = filled((size_t)(rows * kM));
                std::vector<float> out((size_t)(rows * kN), -7.0f);
                CHECK(fxb_process_block_bus_feed(h, x.data(), out.data(), nullptr, nullptr, S, 1, 0) == 0);
                CHECK(blockRight(out.data(), x, S, ch, s, step == 0 ? nullptr : &g0, step == 0 ? nullptr : (step == 1 ? &g0 : &g1), ramp));
                if (ramp) CHECK(feedsAre(h, s, g1, ch));
                // pinned source rows of exactly rows * M words, and a pinned output
                PinnedRows pin((size_t)(rows * kM)), pout((size_t)(rows * kN));
                CHECK(pin.p != nullptr && pout.p != nullptr);
                if (!pin.p || !pout.p) continue;
                std::memcpy(pin.p, x.data(), x.size() * 4);
                const std::vector<float>* now = step == 0 ? nullptr : (step == 1 ? &g0 : &g1);
                CHECK(fxb_process_block_bus_feed(h, pin.p, pout.p, nullptr, nullptr, S, 1, 0) == 0);
                CHECK(blockRight(pout.p, x, S, ch, s, now, now, false));
                blocks += 2;
            }
            CHECK(fxb_info(h, FXB_INFO_BUS_FEED_BLOCKS) == (int64_t)devices * blocks);
            // back to unweighted, then nobody is fed: no sources, no gains, rows of +0.0f
            CHECK(fxb_bus_set_feed_gains(h, nullptr, 0) == 0 && feedsAre(h, s, ones, ch));
            const std::vector<int64_t> none((size_t)kN + 1, 0);
            CHECK(fxb_bus_set_feeds(h, 1, none.data(), nullptr, nullptr) == 0);
            const std::vector<float> x = filled((size_t)ch);
            std::vector<float> out((size_t)(ch * kN), -7.0f);
            CHECK(fxb_process_block_bus_feed(h, x.data(), out.data(), nullptr, nullptr, 1, 1, 0) == 0);
            CHECK(out == std::vector<float>((size_t)(ch * kN), 0.0f));
            CHECK(fxb_bus_set_feeds(h, 0, nullptr, nullptr, nullptr) == 0 && fxb_bus_get_feeds(h, nullptr, nullptr, 0, nullptr, nullptr, 0) == 0);
            fxb_destroy(h);
        }
}

void refusals(int devices) {
    const int ch = 2, S = 8;
    fxb_handle* h = handle(devices, ch);
    CHECK(h != nullptr);
    if (!h) return;
    CHECK(fxb_load_text(h, kStereo) == 1);
    const Structure good = lists(false);
    const int64_t E = good.entries(), rows = (int64_t)S * ch;
    const std::vector<float> gains = filled((size_t)(ch * E)), x = filled((size_t)(rows * kM)), sentinel((size_t)(rows * kN), -7.0f);
    std::vector<float> out = sentinel, narrow((size_t)(rows * fxb_bus_groups(h, 64)), -7.0f);
    for (int state = 0; state < 2; ++state) {   // off, on
        if (state == 1) CHECK(fxb_bus_set_feeds(h, kM, good.offsets.data(), good.sources.data(), gains.data()) == 0);
        const long live = fxstub_live_allocations(), launches = fxstub_bus_feeds();
        std::vector<int64_t> bad = good.sources;
        bad[(size_t)E - 1] = kM;
        CHECK(fxb_bus_set_feeds(h, kM, good.offsets.data(), bad.data(), gains.data()) == FX_E_ARG);
        bad[(size_t)E - 1] = -1;
        CHECK(fxb_bus_set_feeds(h, kM, good.offsets.data(), bad.data(), nullptr) == FX_E_ARG);
        std::vector<int64_t> offs = good.offsets;
        offs[0] = 1;
        CHECK(fxb_bus_set_feeds(h, kM, offs.data(), good.sources.data(), nullptr) == FX_E_ARG);
        offs = good.offsets;
        offs[(size_t)kN - 1] = offs[(size_t)kN] + 1;
        CHECK(fxb_bus_set_feeds(h, kM, offs.data(), good.sources.data(), nullptr) == FX_E_ARG);
        std::vector<float> inf = gains;
        inf[(size_t)(ch * E) - 1] = HUGE_VALF;
        CHECK(fxb_bus_set_feeds(h, kM, good.offsets.data(), good.sources.data(), inf.data()) == FX_E_ARG);
        CHECK(fxb_bus_set_feeds(h, -1, good.offsets.data(), good.sources.data(), nullptr) == FX_E_ARG);
        CHECK(fxb_bus_set_feeds(h, (int64_t)1 << 29, good.offsets.data(), good.sources.data(), nullptr) == FX_E_ARG);
        CHECK(fxb_bus_set_feeds(h, kM, nullptr, good.sources.data(), nullptr) == FX_E_ARG);
        CHECK(fxb_bus_set_feeds(h, kM, good.offsets.data(), nullptr, nullptr) == FX_E_ARG);
        std::vector<int64_t> tooLong((size_t)kN + 1, 0);
        tooLong[(size_t)kN] = ((int64_t)1 << 24) + 1;
        CHECK(fxb_bus_set_feeds(h, kM, tooLong.data(), good.sources.data(), nullptr) == FX_E_ARG);
        CHECK(fxb_bus_get_feeds(h, nullptr, nullptr, -1, nullptr, nullptr, 0) == FX_E_ARG && fxb_bus_get_feeds(h, nullptr, nullptr, 0, nullptr, nullptr, -1) == FX_E_ARG);
        if (state == 0) {
            CHECK(fxb_process_block_bus_feed(h, x.data(), out.data(), nullptr, nullptr, S, 1, 0) == FX_E_ARG);
            CHECK(fxb_bus_set_feed_gains(h, gains.data(), 0) == FX_E_ARG);
            CHECK(fxb_bus_get_feeds(h, nullptr, nullptr, 0, nullptr, nullptr, 0) == 0);
        } else {
            CHECK(fxb_bus_set_feed_gains(h, inf.data(), 1) == FX_E_ARG && fxb_bus_set_feed_gains(h, gains.data(), 2) == FX_E_ARG);
            CHECK(fxb_process_block_bus_feed(h, x.data(), out.data(), nullptr, nullptr, S, 64, FXB_BUS_SHARED_IN) == FX_E_ARG);
            CHECK(fxb_process_block_bus_feed(h, x.data(), narrow.data(), nullptr, nullptr, S, 64, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == FX_E_ARG);
            CHECK(fxb_process_block_bus_feed(h, x.data(), narrow.data(), nullptr, nullptr, S, 0, FXB_BUS_MIX_OUT) == FX_E_ARG);
            CHECK(fxb_process_block_bus_feed(h, x.data(), out.data(), nullptr, nullptr, -1, 1, 0) == FX_E_ARG);
            CHECK(fxb_process_block_bus_feed(h, nullptr, out.data(), nullptr, nullptr, S, 1, 0) == FX_E_ARG);
            CHECK(fxb_process_block_bus_feed(h, x.data(), nullptr, nullptr, nullptr, S, 1, 0) == FX_E_ARG);
            CHECK(fxb_process_block_bus_feed(h, x.data(), out.data(), nullptr, nullptr, S, 1, 4u) == FX_E_ARG);
            CHECK(fxb_process_block_bus_feed(h, out.data(), out.data(), nullptr, nullptr, S, 1, 0) == FX_E_ARG);                      // no in-place form
            CHECK(fxb_process_block_bus_feed(h, out.data() + ch * kN - 1, out.data(), nullptr, nullptr, 1, 1, 0) == FX_E_ARG);         // one shared word
            CHECK(fxb_process_block_bus_feed(h, x.data(), narrow.data(), out.data(), nullptr, S, 64, FXB_BUS_MIX_OUT) == FX_E_ARG);   // (taps are off)
            CHECK(fxb_process_block_bus_feed(h, x.data(), narrow.data(), nullptr, out.data(), S, 64, FXB_BUS_MIX_OUT) == FX_E_ARG);   // (sends are off)
            CHECK(fxb_process_block_bus_feed_dev(h, x.data(), out.data(), nullptr, nullptr, S, 1, 0, nullptr) == FX_E_ARG);            // pageable
            CHECK(feedsAre(h, good, gains, ch));
        }
        CHECK(fxb_process_block_bus_feed(nullptr, x.data(), out.data(), nullptr, nullptr, S, 1, 0) == FX_E_ARG);
        CHECK(fxb_bus_set_feeds(nullptr, kM, good.offsets.data(), good.sources.data(), nullptr) == FX_E_ARG && fxb_bus_set_feed_gains(nullptr, gains.data(), 0) == FX_E_ARG);
        CHECK(fxb_bus_get_feeds(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) == FX_E_ARG);
        CHECK(fxstub_live_allocations() == live && fxstub_bus_feeds() == launches);
        CHECK(out == sentinel);
        CHECK(fxb_info(h, FXB_INFO_BUS_FEED_BLOCKS) == 0 && fxb_info(h, FXB_INFO_BUS_BLOCKS) == 0);
    }
    // the handle goes on
    CHECK(fxb_process_block_bus_feed(h, x.data(), out.data(), nullptr, nullptr, S, 1, 0) == 0);
    CHECK(blockRight(out.data(), x, S, ch, good, &gains, &gains, false));
    fxb_destroy(h);
}

// an allocation that fails at every allocation of a set, then of the device copy of the source rows: FX_E_MEMORY, the feeds in
// force stay on every shard, nothing is launched, nothing leaks
void memory(int devices) {
    const int ch = 2, S = 4;
    fxb_handle* h = handle(devices, ch);   // (no program yet: no builder thread allocates meanwhile)
    CHECK(h != nullptr);
    if (!h) return;
    const Structure old = lists(true), next = lists(false);
    const std::vector<float> oldGains = filled((size_t)(ch * old.entries())), gains = filled((size_t)(ch * next.entries()));
    for (int state = 0; state < 2; ++state) {   // from off, from a structure in force
        if (state == 1) CHECK(fxb_bus_set_feeds(h, kM, old.offsets.data(), old.sources.data(), oldGains.data()) == 0);
        const long live = fxstub_live_allocations();
        for (long nth = 0; nth < devices; ++nth) {   // one allocation per shard
            fxstub_fail_mallocs(nth, 1);
            const int rc = fxb_bus_set_feeds(h, kM, next.offsets.data(), next.sources.data(), gains.data());
            fxstub_fail_mallocs(-1, 0);
            CHECK(rc == FX_E_MEMORY);
            CHECK(fxstub_live_allocations() == live);
            CHECK(state == 1 ? feedsAre(h, old, oldGains, ch) : fxb_bus_get_feeds(h, nullptr, nullptr, 0, nullptr, nullptr, 0) == 0);
        }
    }
    CHECK(fxb_bus_set_feeds(h, kM, next.offsets.data(), next.sources.data(), gains.data()) == 0);
    CHECK(fxb_load_text(h, kStereo) == 1);
    const int64_t rows = (int64_t)S * ch;
    const std::vector<float> in = filled((size_t)(rows * kN)), x = filled((size_t)(rows * kM)), sentinel((size_t)(rows * kN), -7.0f);
    std::vector<float> out = sentinel;
    CHECK(fxb_process_block_bus(h, in.data(), out.data(), S, 1, FXB_BUS_MIX_OUT) == 0);   // (code, scratch and bus staging are there)
    CHECK(fxb_prepare(h, S, 1) == 0);                                                      // (... and the builder thread is idle)
    out = sentinel;
    // a feed block allocates, per shard, the device copy of its source rows.  Feeds off and on again in front of every attempt
    // frees it, so that every attempt meets all of them: the nth one fails.
    const long live = fxstub_live_allocations(), launches = fxstub_bus_feeds(), kernels = fxstub_kernels_run();
    for (long nth = 0; nth < devices; ++nth) {
        CHECK(fxb_bus_set_feeds(h, 0, nullptr, nullptr, nullptr) == 0);
        CHECK(fxb_bus_set_feeds(h, kM, next.offsets.data(), next.sources.data(), gains.data()) == 0);
        CHECK(fxstub_live_allocations() == live);
        fxstub_fail_mallocs(nth, 1);
        const int rc = fxb_process_block_bus_feed(h, x.data(), out.data(), nullptr, nullptr, S, 1, 0);
        fxstub_fail_mallocs(-1, 0);
        CHECK(rc == FX_E_MEMORY);
        // (on a handle of several shards the other shards have run their block and delivered their columns: the refusal is the
        // failing shard's, as with every allocation of a bus block)
        if (devices == 1) CHECK(out == sentinel && fxstub_bus_feeds() == launches && fxstub_kernels_run() == kernels);
        out = sentinel;
    }
    CHECK(fxstub_live_allocations() <= live + devices);
    CHECK(fxb_process_block_bus_feed(h, x.data(), out.data(), nullptr, nullptr, S, 1, 0) == 0);
    CHECK(blockRight(out.data(), x, S, ch, next, &gains, &gains, false));
    fxb_destroy(h);   // destroyed with feeds on
}

}  // namespace

int main() {
    setenv("FXSTUB_DEVICES", "3", 1);   // (read by the stand-in at its first call)
    for (int devices = 1; devices <= 3; devices += 2) {
        indexing(devices);
        refusals(devices);
        memory(devices);
        std::printf("  bus feeds, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_bus_feed_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "bus feed checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("bus feed checks ok\n");
    return 0;
}
