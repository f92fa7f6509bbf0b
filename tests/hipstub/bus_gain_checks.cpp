// bus_gain_checks.cpp — the bus gains of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan + LeakSanitizer
// (TEST INFRASTRUCTURE: csrc/Makefile `stubasangains` links this file with the library's host sources and tests/hipstub/; a
// program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The values are pinned by tests/test_bus_gain_stub.py; this program is about addresses.  Every array the caller hands in is a heap
// block of exactly the documented size, every "device" block of the stand-in is a heap block too, so a read or write one word
// outside [C][N] gains, [S][C][G] / [S][C][N] PCM, a shard's columns or the pinned staging is a report.  It walks the indexing
// shapes (one instance, short groups, a ragged last group, groups above 64, a group of the whole batch; one and two channels;
// blocks of 1 and 33 samples; static gains and ramps; shared input or per-instance input; three shards on their columns), the
// refusals (a NaN, an Inf, a bad ramp, get while off, null handles and buffers: nothing changes) and allocation failures at every
// allocation of a set, on one handle and on three shards.  Where a result follows without redoing the arithmetic it is checked:
// gains of 1.0f give the words of gains off, gains of zero give +0.0f everywhere.
// Exit code 0 = every check held (a sanitizer report turns it non-zero by itself).
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../fx8010-emulator-core_amd/csrc/fx_batch_bus_side.hpp"
#include "../../include/fx8010_amd.h"
#include "hip_stub.h"

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

uint32_t g_seed = 12345u;
float noise() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int)(g_seed >> 8 & 0xffff) - 32768) / 20000.0f;
}

std::vector<float> filled(size_t n) {
    std::vector<float> v(n);
    for (float& x : v) x = noise();
    return v;
}

bool sameWords(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0; }

// one handle (devices == 1) or three shards through every indexing shape
void indexing(int devices) {
    // (three shards: 808 instances start at 0, 320 and 576, and a group must not straddle a shard)
    const int64_t single[7][2] = {{1, 1}, {5, 2}, {65, 64}, {200, 63}, {200, 65}, {777, 130}, {300, 1000}};
    const int64_t sharded[3][2] = {{808, 64}, {808, 32}, {808, 1}};
    const int three[3] = {0, 1, 2};
    const int64_t(*shapes)[2] = devices > 1 ? sharded : single;
    for (int which = 0; which < (devices > 1 ? 3 : 7); ++which)
        for (int ch = 1; ch <= 2; ++ch) {
            const int64_t* shape = shapes[which];
            const int64_t N = shape[0], K = shape[1] < N ? shape[1] : N;
            fxb_handle* h = devices > 1 ? fxb_create_on_devices(N, ch, three, 3) : fxb_create(N, ch, 0);
            CHECK(h != nullptr);
            if (!h) return;
            std::vector<float> gains = filled((size_t)ch * N), back((size_t)ch * N);
            gains[0] = 0.0f;
            gains[gains.size() - 1] = -0.0f;
            CHECK(fxb_bus_set_gains(h, gains.data(), 0) == 0);   // before a program is loaded
            CHECK(fxb_load_text(h, ch == 1 ? kMono : kStereo) == 1);
            CHECK(fxb_bus_get_gains(h, back.data()) == 0 && sameWords(back, gains));
            const int64_t G = fxb_bus_groups(h, K);
            CHECK(G == (N + K - 1) / K);
            const int lengths[2] = {33, 1};
            for (int S : lengths) {
                const std::vector<float> narrow = filled((size_t)S * ch * G), wide = filled((size_t)S * ch * N);
                std::vector<float> out((size_t)S * ch * G), off;
                for (int ramp = 0; ramp <= 1; ++ramp) {
                    std::vector<float> next = filled((size_t)ch * N);
                    CHECK(fxb_bus_set_gains(h, next.data(), ramp) == 0);
                    for (float& x : next) x = std::numeric_limits<float>::quiet_NaN();   // the caller's array is free on return
                    CHECK(fxb_process_block_bus(h, narrow.data(), out.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == 0);
                    CHECK(fxb_bus_set_gains(h, gains.data(), ramp) == 0);
                    CHECK(fxb_process_block_bus(h, wide.data(), out.data(), S, K, FXB_BUS_MIX_OUT) == 0);
                    CHECK(fxb_bus_get_gains(h, back.data()) == 0 && sameWords(back, gains));
                }
                // gains of 1.0f, static and as the target of a ramp from 1.0f: the words of gains off; gains of zero: +0.0f
                CHECK(fxb_bus_set_gains(h, nullptr, 0) == 0);
                CHECK(fxb_process_block_bus(h, wide.data(), out.data(), S, K, FXB_BUS_MIX_OUT) == 0);
                off = out;
                const std::vector<float> ones((size_t)ch * N, 1.0f), zeros((size_t)ch * N, -0.0f);
                CHECK(fxb_bus_set_gains(h, ones.data(), 1) == 0);   // (out of "off": a counts as 1.0f)
                CHECK(fxb_process_block_bus(h, wide.data(), out.data(), S, K, FXB_BUS_MIX_OUT) == 0 && sameWords(out, off));
                CHECK(fxb_process_block_bus(h, wide.data(), out.data(), S, K, FXB_BUS_MIX_OUT) == 0 && sameWords(out, off));
                CHECK(fxb_bus_set_gains(h, zeros.data(), 0) == 0);
                CHECK(fxb_process_block_bus(h, wide.data(), out.data(), S, K, FXB_BUS_MIX_OUT) == 0);
                CHECK(sameWords(out, std::vector<float>(out.size(), 0.0f)));
                CHECK(fxb_bus_set_gains(h, gains.data(), 0) == 0);
            }
            CHECK(fxb_info(h, FXB_INFO_BUS_GAIN_BLOCKS) == (int64_t)devices * 2 * (4 + 3));
            fxb_destroy(h);
        }
}

void refusals(int devices) {
    const int64_t N = 300, K = 64;
    const int ch = 2, S = 8;
    const int three[3] = {0, 1, 2};
    fxb_handle* h = devices > 1 ? fxb_create_on_devices(N, ch, three, 3) : fxb_create(N, ch, 0);
    CHECK(h != nullptr);
    if (!h) return;
    const std::vector<float> good = filled((size_t)ch * N), ones((size_t)ch * N, 1.0f);
    std::vector<float> back((size_t)ch * N);
    const float bads[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    const size_t places[3] = {0, good.size() - 1, good.size() / 2};
    for (int state = 0; state < 3; ++state) {   // off, on, a ramp pending
        if (state == 1) CHECK(fxb_bus_set_gains(h, good.data(), 0) == 0);
        if (state == 2) CHECK(fxb_bus_set_gains(h, ones.data(), 1) == 0);
        const long live = fxstub_live_allocations();
        for (int k = 0; k < 3; ++k)
            for (int ramp = 0; ramp <= 1; ++ramp) {
                std::vector<float> bad = good;
                bad[places[k]] = bads[k];
                CHECK(fxb_bus_set_gains(h, bad.data(), ramp) == FX_E_ARG);
            }
        const int ramps[3] = {2, -1, 256};
        for (int ramp : ramps) {
            CHECK(fxb_bus_set_gains(h, good.data(), ramp) == FX_E_ARG);
            CHECK(fxb_bus_set_gains(h, nullptr, ramp) == FX_E_ARG);
        }
        CHECK(fxstub_live_allocations() == live);
        if (state == 0) {
            CHECK(fxb_bus_get_gains(h, back.data()) == FX_E_ARG);
        } else {
            CHECK(fxb_bus_get_gains(h, nullptr) == FX_E_ARG);
            CHECK(fxb_bus_get_gains(h, back.data()) == 0 && sameWords(back, good));
        }
        CHECK(fxb_info(h, FXB_INFO_BUS_GAIN_BLOCKS) == 0);
    }
    CHECK(fxb_bus_set_gains(nullptr, good.data(), 0) == FX_E_ARG);
    CHECK(fxb_bus_get_gains(nullptr, back.data()) == FX_E_ARG);
    // the handle goes on: the pending ramp is consumed by the next block
    CHECK(fxb_load_text(h, kStereo) == 1);
    const int64_t G = fxb_bus_groups(h, K);
    const std::vector<float> in = filled((size_t)S * ch * G);
    std::vector<float> out((size_t)S * ch * G);
    CHECK(fxb_process_block_bus(h, in.data(), out.data(), S, K, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == 0);
    CHECK(fxb_bus_get_gains(h, back.data()) == 0 && sameWords(back, ones));
    fxb_destroy(h);
}

// an allocation that fails inside a set, at every allocation it makes: FX_E_MEMORY, the gains stay off on every shard, nothing leaks
void memory(int devices) {
    const int64_t N = 3 * 256 + 40;
    const int ch = 2;
    const int three[3] = {0, 1, 2};
    fxb_handle* h = devices > 1 ? fxb_create_on_devices(N, ch, three, 3) : fxb_create(N, ch, 0);   // (no program: no builder thread allocates meanwhile)
    CHECK(h != nullptr);
    if (!h) return;
    const std::vector<float> good = filled((size_t)ch * N);
    std::vector<float> back((size_t)ch * N);
    const long live = fxstub_live_allocations();
    for (long nth = 0; nth < 3L * devices; ++nth) {
        fxstub_fail_mallocs(nth, 1);
        const int rc = fxb_bus_set_gains(h, good.data(), (int)(nth & 1));
        fxstub_fail_mallocs(-1, 0);
        CHECK(rc == FX_E_MEMORY);
        CHECK(fxstub_live_allocations() == live);
        CHECK(fxb_bus_get_gains(h, back.data()) == FX_E_ARG);
    }
    CHECK(fxb_bus_set_gains(h, good.data(), 0) == 0);
    CHECK(fxstub_live_allocations() == live + 3L * devices);
    CHECK(fxb_bus_get_gains(h, back.data()) == 0 && sameWords(back, good));
    CHECK(fxb_bus_set_gains(h, nullptr, 0) == 0);
    CHECK(fxstub_live_allocations() == live);
    CHECK(fxb_bus_set_gains(h, good.data(), 1) == 0);   // destroyed with gains on and a ramp pending
    fxb_destroy(h);
}

// the roles of two gain blocks (fx::RampPair, what the bus gains and the send gains both go by): set; ramp; ramp while pending;
// ramp = 0 while pending; and a block that consumes a ramp
void rampPair() {
    fx::RampPair r;
    CHECK(r.writeTarget(0) == 0 && r.inForce() == 0);   // a set replaces b where it is
    r = fx::RampPair{r.writeTarget(0), false};
    CHECK(r.target == 0 && !r.pending && r.inForce() == 0);
    CHECK(r.writeTarget(1) == 1);                        // a ramp with none pending: the blocks swap roles, the old b is in force as a
    r = fx::RampPair{r.writeTarget(1), true};
    CHECK(r.target == 1 && r.pending && r.inForce() == 0);
    CHECK(r.writeTarget(1) == 1);                        // a ramp while one is pending replaces b in place: a stays
    r = fx::RampPair{r.writeTarget(1), true};
    CHECK(r.target == 1 && r.pending && r.inForce() == 0);
    CHECK(r.writeTarget(0) == 1);                        // ramp = 0 while pending: b in place again, and the ramp is dropped
    r = fx::RampPair{r.writeTarget(0), false};
    CHECK(r.target == 1 && !r.pending && r.inForce() == 1);
    r = fx::RampPair{r.writeTarget(1), true};            // ... and the next ramp swaps back
    CHECK(r.target == 0 && r.pending && r.inForce() == 1);
    r.consume();                                         // a block that was fully queued: the target is in force
    CHECK(r.target == 0 && !r.pending && r.inForce() == 0);
}

}  // namespace

int main() {
    rampPair();
    setenv("FXSTUB_DEVICES", "3", 1);   // (read by the stand-in at its first call)
    for (int devices = 1; devices <= 3; devices += 2) {
        indexing(devices);
        refusals(devices);
        memory(devices);
        std::printf("  bus gains, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "bus gain checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("bus gain checks ok\n");
    return 0;
}
