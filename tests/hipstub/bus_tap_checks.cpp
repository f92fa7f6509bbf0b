// bus_tap_checks.cpp — the bus taps of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan + LeakSanitizer
// (TEST INFRASTRUCTURE: csrc/Makefile `stubasantaps` links this file with the library's host sources and tests/hipstub/; a
// program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The routes and the state machine are pinned by tests/test_bus_tap_stub.py; this program is about addresses.  Every array the
// caller hands in is a heap block of exactly the documented size, every "device" block of the stand-in is a heap block too, so a
// read or write one word outside the list, the [S][C][T] tap rows, the [S][C][G] / [S][C][N] PCM, a shard's columns or a staging
// block is a report.  It walks the indexing shapes (one instance, short groups, a ragged last group, groups above 64, a group of
// the whole batch; one and two channels; blocks of 33 and 1 samples; lists of 1, 3, 64, 65 and 130 entries with the first and the
// last instance, a repeat and an unsorted stretch; pageable and pinned tap rows; three shards on their columns), the refusals
// (nothing changes, the tap rows stay untouched) and an allocation failure at every allocation of a set and of a staged block,
// on one handle and on three shards.  The stand-in's emulation launch copies in to out, so the tap words can be checked here
// without redoing any arithmetic: they are the expanded input's.
// Exit code 0 = every check held (a sanitizer report turns it non-zero by itself).
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/fx8010_amd.h"
#include "hip_stub.h"

extern "C" long fxstub_bus_taps(void);
extern "C" long fxstub_bus_tap_strays(void);

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

uint32_t g_seed = 2463u;
uint32_t draw() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

// words of every kind: a tap moves patterns, NaN payloads included
std::vector<float> filled(size_t n) {
    std::vector<float> v(n);
    for (float& x : v) {
        const uint32_t w = draw() << 8 | (draw() & 0xffu);
        std::memcpy(&x, &w, 4);
    }
    return v;
}

std::vector<int64_t> tapList(int64_t N, int T) {
    std::vector<int64_t> lst = {N - 1, 0, N - 1};
    while ((int)lst.size() < T) lst.push_back((int64_t)(draw() % (uint32_t)N));
    lst.resize((size_t)T);
    return lst;
}

// the tap rows a block must have delivered: column t of row r is word list[t] of the per-instance row r
bool tapsRight(const std::vector<float>& taps, const std::vector<float>& in, bool shared, int64_t rows, int64_t N, int64_t K, int64_t G, const std::vector<int64_t>& lst) {
    const int64_t T = (int64_t)lst.size();
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t t = 0; t < T; ++t) {
            const float* want = shared ? &in[(size_t)(r * G + lst[(size_t)t] / K)] : &in[(size_t)(r * N + lst[(size_t)t])];
            if (std::memcmp(&taps[(size_t)(r * T + t)], want, 4) != 0) return false;
        }
    return true;
}

struct PinnedRows {
    float* p = nullptr;
    explicit PinnedRows(size_t floats) { p = static_cast<float*>(fxb_host_alloc(floats * 4)); }
    ~PinnedRows() { fxb_host_free(p); }
};

// one handle (devices == 1) or three shards through every indexing shape
void indexing(int devices) {
    // (three shards: 808 instances start at 0, 320 and 576, and a group must not straddle a shard)
    const int64_t single[7][2] = {{1, 1}, {5, 2}, {65, 64}, {200, 63}, {200, 65}, {777, 130}, {300, 1000}};
    const int64_t sharded[3][2] = {{808, 64}, {808, 32}, {808, 1}};
    const int three[3] = {0, 1, 2};
    const int64_t(*shapes)[2] = devices > 1 ? sharded : single;
    const int sizes[5] = {1, 3, 64, 65, 130};
    for (int which = 0; which < (devices > 1 ? 3 : 7); ++which)
        for (int ch = 1; ch <= 2; ++ch) {
            const int64_t* shape = shapes[which];
            const int64_t N = shape[0], K = shape[1] < N ? shape[1] : N;
            fxb_handle* h = devices > 1 ? fxb_create_on_devices(N, ch, three, 3) : fxb_create(N, ch, 0);
            CHECK(h != nullptr);
            if (!h) return;
            int64_t blocks = 0;
            for (int T : sizes) {
                std::vector<int64_t> lst = tapList(N, T), given = lst, back((size_t)T, -1);
                CHECK(fxb_bus_set_taps(h, given.data(), T) == 0);   // (the first one: before a program is loaded)
                for (int64_t& v : given) v = -1;                       // the caller's list is free on return
                if (T == sizes[0]) CHECK(fxb_load_text(h, ch == 1 ? kMono : kStereo) == 1);
                CHECK(fxb_bus_get_taps(h, nullptr, 0) == T);
                CHECK(fxb_bus_get_taps(h, back.data(), T) == T && back == lst);
                const int64_t G = fxb_bus_groups(h, K);
                const int lengths[2] = {33, 1};
                for (int S : lengths) {
                    const int64_t rows = (int64_t)S * ch;
                    const std::vector<float> narrow = filled((size_t)(rows * G)), wide = filled((size_t)(rows * N));
                    std::vector<float> out((size_t)(rows * G)), taps((size_t)(rows * T));
                    CHECK(fxb_process_block_bus_tap(h, narrow.data(), out.data(), taps.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == 0);
                    CHECK(tapsRight(taps, narrow, true, rows, N, K, G, lst));
                    CHECK(fxb_process_block_bus_tap(h, wide.data(), out.data(), taps.data(), S, K, FXB_BUS_MIX_OUT) == 0);
                    CHECK(tapsRight(taps, wide, false, rows, N, K, G, lst));
                    // pinned tap rows of exactly rows * T words: stored to in place (every shard its columns)
                    PinnedRows pin((size_t)(rows * T));
                    CHECK(pin.p != nullptr);
                    if (!pin.p) continue;
                    CHECK(fxb_process_block_bus_tap(h, wide.data(), out.data(), pin.p, S, K, FXB_BUS_MIX_OUT) == 0);
                    CHECK(tapsRight(std::vector<float>(pin.p, pin.p + rows * T), wide, false, rows, N, K, G, lst));
                    blocks += 3;
                }
            }
            CHECK(fxb_info(h, FXB_INFO_BUS_TAP_BLOCKS) == (int64_t)devices * blocks);
            CHECK(fxb_bus_set_taps(h, nullptr, 0) == 0 && fxb_bus_get_taps(h, nullptr, 0) == 0);
            fxb_destroy(h);
        }
}

void refusals(int devices) {
    const int64_t N = 300, K = 64;
    const int ch = 2, S = 8, T = 65;
    const int three[3] = {0, 1, 2};
    fxb_handle* h = devices > 1 ? fxb_create_on_devices(N, ch, three, 3) : fxb_create(N, ch, 0);
    CHECK(h != nullptr);
    if (!h) return;
    CHECK(fxb_load_text(h, kStereo) == 1);
    const int64_t G = fxb_bus_groups(h, K), rows = (int64_t)S * ch;
    const std::vector<float> in = filled((size_t)(rows * G)), sentinel((size_t)(rows * T), -7.0f);
    std::vector<float> out((size_t)(rows * G)), wideOut((size_t)(rows * N)), taps = sentinel;
    const std::vector<int64_t> good = tapList(N, T);
    std::vector<int64_t> back((size_t)T, -1);
    for (int state = 0; state < 2; ++state) {   // off, on
        if (state == 1) CHECK(fxb_bus_set_taps(h, good.data(), T) == 0);
        const long live = fxstub_live_allocations(), launches = fxstub_bus_taps();
        std::vector<int64_t> bad = good;
        bad[(size_t)T - 1] = N;
        CHECK(fxb_bus_set_taps(h, bad.data(), T) == FX_E_ARG);
        bad[(size_t)T - 1] = -1;
        CHECK(fxb_bus_set_taps(h, bad.data(), T) == FX_E_ARG);
        CHECK(fxb_bus_set_taps(h, good.data(), -1) == FX_E_ARG);
        CHECK(fxb_bus_set_taps(h, nullptr, 1) == FX_E_ARG);
        const std::vector<int64_t> many(65537, 0);
        CHECK(fxb_bus_set_taps(h, many.data(), 65537) == FX_E_ARG);
        CHECK(fxb_bus_get_taps(h, nullptr, 1) == FX_E_ARG && fxb_bus_get_taps(h, back.data(), -1) == FX_E_ARG);
        // blocks: while taps are off every tapped one is refused; while they are on, the ones the definition names
        if (state == 0) {
            CHECK(fxb_process_block_bus_tap(h, in.data(), out.data(), taps.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == FX_E_ARG);
            CHECK(fxb_bus_get_taps(h, back.data(), T) == 0);
        } else {
            CHECK(fxb_process_block_bus_tap(h, in.data(), wideOut.data(), taps.data(), S, K, FXB_BUS_SHARED_IN) == FX_E_ARG);
            CHECK(fxb_process_block_bus_tap(h, in.data(), out.data(), taps.data(), S, 0, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == FX_E_ARG);
            CHECK(fxb_process_block_bus_tap(h, in.data(), out.data(), taps.data(), -1, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == FX_E_ARG);
            CHECK(fxb_process_block_bus_tap(h, nullptr, out.data(), taps.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == FX_E_ARG);
            CHECK(fxb_process_block_bus_tap(h, in.data(), out.data(), taps.data(), S, K, 4u | FXB_BUS_MIX_OUT) == FX_E_ARG);
            CHECK(fxb_process_block_bus_tap(h, in.data(), out.data(), out.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == FX_E_ARG);
            CHECK(fxb_process_block_bus_tap_dev(h, in.data(), out.data(), taps.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT, nullptr) == FX_E_ARG);   // pageable
            CHECK(fxb_bus_get_taps(h, back.data(), T) == T && back == good);
        }
        CHECK(fxb_process_block_bus_tap(nullptr, in.data(), out.data(), taps.data(), S, K, FXB_BUS_MIX_OUT) == FX_E_ARG);
        CHECK(fxb_bus_set_taps(nullptr, good.data(), T) == FX_E_ARG && fxb_bus_get_taps(nullptr, nullptr, 0) == FX_E_ARG);
        CHECK(fxstub_live_allocations() == live && fxstub_bus_taps() == launches);
        CHECK(taps == sentinel);
        CHECK(fxb_info(h, FXB_INFO_BUS_TAP_BLOCKS) == 0 && fxb_info(h, FXB_INFO_BUS_BLOCKS) == 0);
    }
    // the handle goes on
    CHECK(fxb_process_block_bus_tap(h, in.data(), out.data(), taps.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == 0);
    CHECK(tapsRight(taps, in, true, rows, N, K, G, good));
    fxb_destroy(h);
}

// an allocation that fails at every allocation of a set, then of a staged block: FX_E_MEMORY, the taps in force stay on every shard,
// nothing is launched, nothing leaks
void memory(int devices) {
    const int64_t N = 3 * 256 + 40, K = 64;
    const int ch = 2, S = 4, T = 130;
    const int three[3] = {0, 1, 2};
    fxb_handle* h = devices > 1 ? fxb_create_on_devices(N, ch, three, 3) : fxb_create(N, ch, 0);   // (no program yet: no builder thread allocates meanwhile)
    CHECK(h != nullptr);
    if (!h) return;
    std::vector<int64_t> old = {807, 0, 400, 0}, next = tapList(N, T), back((size_t)T, -1);
    next[7] = 400;   // (an entry of the middle shard, whatever was drawn)
    for (int state = 0; state < 2; ++state) {   // from off, from a list in force
        if (state == 1) CHECK(fxb_bus_set_taps(h, old.data(), (int64_t)old.size()) == 0);
        const long live = fxstub_live_allocations();
        for (long nth = 0; nth < devices; ++nth) {   // one allocation per shard
            fxstub_fail_mallocs(nth, 1);
            const int rc = fxb_bus_set_taps(h, next.data(), T);
            fxstub_fail_mallocs(-1, 0);
            CHECK(rc == FX_E_MEMORY);
            CHECK(fxstub_live_allocations() == live);
            const int64_t want = state == 1 ? (int64_t)old.size() : 0;
            CHECK(fxb_bus_get_taps(h, back.data(), T) == want && std::equal(old.begin(), old.begin() + want, back.begin()));
        }
    }
    CHECK(fxb_bus_set_taps(h, next.data(), T) == 0);
    CHECK(fxb_load_text(h, kStereo) == 1);
    const int64_t G = fxb_bus_groups(h, K), rows = (int64_t)S * ch;
    const std::vector<float> in = filled((size_t)(rows * G)), sentinel((size_t)(rows * T), -7.0f);
    std::vector<float> out((size_t)(rows * G)), taps = sentinel;
    CHECK(fxb_process_block_bus(h, in.data(), out.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == 0);   // (code, scratch and bus staging are there)
    CHECK(fxb_prepare(h, S, 1) == 0);                                                                          // (... and the builder thread is idle)
    // a staged tapped block allocates, per shard, the device staging of its tap rows and - on a handle of several shards - the
    // pinned block from which it places its columns.  Taps off and on again in front of every attempt frees both, so that every
    // attempt meets all of them: the nth one fails.
    const long perShard = devices > 1 ? 2 : 1, live = fxstub_live_allocations(), launches = fxstub_bus_taps(), kernels = fxstub_kernels_run();
    for (long nth = 0; nth < perShard * devices; ++nth) {
        CHECK(fxb_bus_set_taps(h, nullptr, 0) == 0 && fxb_bus_set_taps(h, next.data(), T) == 0);
        CHECK(fxstub_live_allocations() == live);
        fxstub_fail_mallocs(nth, 1);
        const int rc = fxb_process_block_bus_tap(h, in.data(), out.data(), taps.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT);
        fxstub_fail_mallocs(-1, 0);
        CHECK(rc == FX_E_MEMORY);
        // (on a handle of several shards the other shards have run their block and delivered their columns: the refusal is the
        // failing shard's, as with every allocation of a bus block)
        if (devices == 1) CHECK(taps == sentinel && fxstub_bus_taps() == launches && fxstub_kernels_run() == kernels);
        taps = sentinel;
    }
    CHECK(fxstub_live_allocations() <= live + perShard * devices);
    CHECK(fxb_process_block_bus_tap(h, in.data(), out.data(), taps.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == 0);
    CHECK(tapsRight(taps, in, true, rows, N, K, G, next));
    fxb_destroy(h);   // destroyed with taps on
}

}  // namespace

int main() {
    setenv("FXSTUB_DEVICES", "3", 1);   // (read by the stand-in at its first call)
    for (int devices = 1; devices <= 3; devices += 2) {
        indexing(devices);
        refusals(devices);
        memory(devices);
        std::printf("  bus taps, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_bus_tap_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "bus tap checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("bus tap checks ok\n");
    return 0;
}
