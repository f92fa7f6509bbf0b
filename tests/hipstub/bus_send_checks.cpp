// bus_send_checks.cpp — the bus sends of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan + LeakSanitizer
// (TEST INFRASTRUCTURE: csrc/Makefile `stubasansends` links this file with the library's host sources and tests/hipstub/; a
// program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The routes and the state machine are pinned by tests/test_bus_send_stub.py; this program is about addresses.  Every array the
// caller hands in is a heap block of exactly the documented size, every "device" block of the stand-in is a heap block too, so a
// read or write one word outside the offsets, the members, the [C][E] gains, the [S][C][A] aux rows, the PCM, the tables of the
// device block, a shard's columns, the chunk sums or a staging block is a report.  It walks structures of buses of 0 .. 2 049
// entries (one and two channels; blocks of 33 and 1 samples; static and ramping; pageable and pinned aux rows; one handle and
// three shards on their columns), the round trip under caps of every size, the refusals (nothing changes, the aux rows stay
// untouched) and an allocation failure at every allocation of a set, of the chunk sums and of a staged aux_out.  The stand-in's
// emulation launch copies in to out, so the aux words are the definition of include/fx8010_amd.h over the input itself.
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

extern "C" long fxstub_bus_sends(void);
extern "C" long fxstub_bus_send_strays(void);

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

uint32_t g_seed = 9241u;
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

struct Structure {
    std::vector<int64_t> offsets{0}, members;
    int64_t buses() const { return (int64_t)offsets.size() - 1; }
    int64_t entries() const { return offsets.back(); }
};

// buses of the given sizes with members in lo .. hi - 1: the last one, the first one, random ones
void addBus(Structure& s, int64_t lo, int64_t hi, int64_t size) {
    for (int64_t m = 0; m < size; ++m) s.members.push_back(m == 0 ? hi - 1 : (m == 1 ? lo : lo + (int64_t)(draw() % (uint32_t)(hi - lo))));
    s.offsets.push_back((int64_t)s.members.size());
}

float tree(const float* seq, int64_t count) {
    volatile float p[64];
    for (int l = 0; l < 64; ++l) p[l] = 0.0f;
    for (int64_t m = 0; m < count; ++m) p[m % 64] = p[m % 64] + seq[m];
    for (int step = 32; step > 0; step >>= 1)
        for (int l = 0; l < step; ++l) p[l] = p[l] + p[l + step];
    return p[0];
}

// the aux rows a block of S samples must have delivered, from the per-instance rows y [S * C][N]
bool auxRight(const float* aux, const std::vector<float>& y, int S, int ch, int64_t N, const Structure& s, const std::vector<float>& a, const std::vector<float>& b, bool ramp) {
    const int64_t A = s.buses(), E = s.entries();
    const float r = 1.0f / (float)S;
    std::vector<float> terms, sums;
    for (int smp = 0; smp < S; ++smp)
        for (int c = 0; c < ch; ++c)
            for (int64_t bus = 0; bus < A; ++bus) {
                const int64_t lo = s.offsets[(size_t)bus], hi = s.offsets[(size_t)bus + 1];
                terms.clear();
                for (int64_t e = lo; e < hi; ++e) {
                    volatile float w = b[(size_t)(c * E + e)];
                    if (ramp && smp != S - 1) {
                        volatile float t = (float)(smp + 1) * r;
                        volatile float d = b[(size_t)(c * E + e)] - a[(size_t)(c * E + e)];
                        volatile float m = d * t;
                        w = a[(size_t)(c * E + e)] + m;
                    }
                    volatile float term = 0.0f;
                    if (w != 0.0f) term = w * y[(size_t)(((int64_t)smp * ch + c) * N + s.members[(size_t)e])];
                    terms.push_back((float)term);
                }
                sums.clear();
                for (size_t q = 0; q < terms.size(); q += 1024) sums.push_back(tree(terms.data() + q, (int64_t)std::min<size_t>(1024, terms.size() - q)));
                const float want = sums.empty() ? 0.0f : (sums.size() == 1 ? sums[0] : tree(sums.data(), (int64_t)sums.size()));
                if (std::memcmp(&aux[((int64_t)smp * ch + c) * A + bus], &want, 4) != 0) return false;
            }
    return true;
}

std::vector<float> expanded(const std::vector<float>& narrow, int64_t rows, int64_t N, int64_t K, int64_t G) {
    std::vector<float> y((size_t)(rows * N));
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t i = 0; i < N; ++i) y[(size_t)(r * N + i)] = narrow[(size_t)(r * G + i / K)];
    return y;
}

struct PinnedRows {
    float* p = nullptr;
    explicit PinnedRows(size_t floats) { p = static_cast<float*>(fxb_host_alloc(std::max<size_t>(floats, 1) * 4)); }
    ~PinnedRows() { fxb_host_free(p); }
};

const int64_t kN = 808, kK = 64;                       // three shards: instances from 0, 320 and 576
const int64_t kBounds[4] = {0, 320, 576, 808};

Structure mixed(bool sharded) {
    Structure s;
    const int64_t sizes[9] = {65, 0, 1025, 1, 2049, 64, 3, 1024, 63};
    for (int k = 0; k < 9; ++k) {
        const int shard = sharded ? (k * 2) % 3 : 0;
        addBus(s, sharded ? kBounds[shard] : 0, sharded ? kBounds[shard + 1] : kN, sizes[k]);
    }
    return s;
}

bool sendsAre(fxb_handle* h, const Structure& s, const std::vector<float>& gains, int ch) {
    int64_t A = -1;
    const int64_t E = s.entries();
    if (fxb_bus_get_sends(h, &A, nullptr, 0, nullptr, nullptr, 0) != E || A != s.buses()) return false;
    std::vector<int64_t> off((size_t)A + 1, -1), mem((size_t)E, -1);
    std::vector<float> g((size_t)(ch * E), -7.0f);
    if (fxb_bus_get_sends(h, nullptr, off.data(), A + 1, mem.data(), g.data(), E) != E) return false;
    return off == s.offsets && mem == s.members && std::memcmp(g.data(), gains.data(), g.size() * 4) == 0;
}

// one handle (devices == 1) or three shards through structures, routes and the round trip
void indexing(int devices) {
    const int three[3] = {0, 1, 2};
    for (int ch = 1; ch <= 2; ++ch) {
        fxb_handle* h = devices > 1 ? fxb_create_on_devices(kN, ch, three, 3) : fxb_create(kN, ch, 0);
        CHECK(h != nullptr);
        if (!h) return;
        const Structure s = mixed(devices > 1);
        const int64_t A = s.buses(), E = s.entries();
        std::vector<float> g0 = filled((size_t)(ch * E)), g1 = filled((size_t)(ch * E));
        g0[3] = 0.0f;
        g1[5] = -0.0f;
        {
            Structure given = s;
            std::vector<float> gains = g0;
            CHECK(fxb_bus_set_sends(h, A, given.offsets.data(), given.members.data(), gains.data()) == 0);   // (before a program is loaded)
            std::fill(given.offsets.begin(), given.offsets.end(), -1);                                         // the caller's arrays are free on return
            std::fill(given.members.begin(), given.members.end(), -1);
            std::fill(gains.begin(), gains.end(), -1.0f);
        }
        CHECK(fxb_load_text(h, ch == 1 ? kMono : kStereo) == 1);
        CHECK(sendsAre(h, s, g0, ch));
        // the round trip under caps of every kind: nothing beyond a cap is written (the blocks are exactly that long)
        for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)7, E - 1}) {
            std::vector<int64_t> off((size_t)std::min<int64_t>(cap, A + 1)), mem((size_t)cap);
            std::vector<float> g((size_t)(ch * E), -7.0f);   // (channel rows keep their pitch of E)
            CHECK(fxb_bus_get_sends(h, nullptr, off.data(), (int64_t)off.size(), mem.data(), g.data(), cap) == E);
            CHECK(std::equal(off.begin(), off.end(), s.offsets.begin()) && std::equal(mem.begin(), mem.end(), s.members.begin()));
            for (int c = 0; c < ch; ++c)
                for (int64_t e = 0; e < E; ++e) CHECK(e < cap ? std::memcmp(&g[(size_t)(c * E + e)], &g0[(size_t)(c * E + e)], 4) == 0 : g[(size_t)(c * E + e)] == -7.0f);
        }
        const int64_t G = fxb_bus_groups(h, kK);
        int64_t blocks = 0;
        const int lengths[3] = {33, 1, 33};
        for (int step = 0; step < 3; ++step) {
            const int S = lengths[step];
            const bool ramp = step == 2;
            if (ramp) CHECK(fxb_bus_set_send_gains(h, g1.data(), 1) == 0 && sendsAre(h, s, g0, ch));
            const int64_t rows = (int64_t)S * ch;
            const std::vector<float> narrow = filled((size_t)(rows * G)), wide = filled((size_t)(rows * kN));
            std::vector<float> out((size_t)(rows * G)), aux((size_t)(rows * A));
            CHECK(fxb_process_block_bus_aux(h, narrow.data(), out.data(), nullptr, aux.data(), S, kK, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == 0);
            CHECK(auxRight(aux.data(), expanded(narrow, rows, kN, kK, G), S, ch, kN, s, g0, ramp ? g1 : g0, ramp));
            if (ramp) CHECK(sendsAre(h, s, g1, ch));
            const std::vector<float>& now = ramp ? g1 : g0;
            CHECK(fxb_process_block_bus_aux(h, wide.data(), out.data(), nullptr, aux.data(), S, kK, FXB_BUS_MIX_OUT) == 0);
            CHECK(auxRight(aux.data(), wide, S, ch, kN, s, now, now, false));
            // pinned aux rows of exactly rows * A words: stored to in place (every shard its columns)
            PinnedRows pin((size_t)(rows * A));
            CHECK(pin.p != nullptr);
            if (!pin.p) continue;
            CHECK(fxb_process_block_bus_aux(h, wide.data(), out.data(), nullptr, pin.p, S, kK, FXB_BUS_MIX_OUT) == 0);
            CHECK(auxRight(pin.p, wide, S, ch, kN, s, now, now, false));
            blocks += 3;
        }
        CHECK(fxb_info(h, FXB_INFO_BUS_SEND_BLOCKS) == (int64_t)devices * blocks);
        // only empty buses: no members, no gains, rows of +0.0f
        const int64_t none[4] = {0, 0, 0, 0};
        CHECK(fxb_bus_set_sends(h, 3, none, nullptr, nullptr) == 0);
        std::vector<float> narrow = filled((size_t)(ch * G)), out((size_t)(ch * G)), aux((size_t)(ch * 3), -7.0f);
        CHECK(fxb_process_block_bus_aux(h, narrow.data(), out.data(), nullptr, aux.data(), 1, kK, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == 0);
        CHECK(aux == std::vector<float>((size_t)(ch * 3), 0.0f));
        CHECK(fxb_bus_set_sends(h, 0, nullptr, nullptr, nullptr) == 0 && fxb_bus_get_sends(h, nullptr, nullptr, 0, nullptr, nullptr, 0) == 0);
        fxb_destroy(h);
    }
}

void refusals(int devices) {
    const int ch = 2, S = 8;
    const int three[3] = {0, 1, 2};
    fxb_handle* h = devices > 1 ? fxb_create_on_devices(kN, ch, three, 3) : fxb_create(kN, ch, 0);
    CHECK(h != nullptr);
    if (!h) return;
    CHECK(fxb_load_text(h, kStereo) == 1);
    const Structure good = mixed(devices > 1);
    const int64_t A = good.buses(), E = good.entries(), G = fxb_bus_groups(h, kK), rows = (int64_t)S * ch;
    const std::vector<float> gains = filled((size_t)(ch * E)), in = filled((size_t)(rows * G)), sentinel((size_t)(rows * A), -7.0f);
    std::vector<float> out((size_t)(rows * G)), wideOut((size_t)(rows * kN)), aux = sentinel;
    const unsigned both = FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT;
    for (int state = 0; state < 2; ++state) {   // off, on
        if (state == 1) CHECK(fxb_bus_set_sends(h, A, good.offsets.data(), good.members.data(), gains.data()) == 0);
        const long live = fxstub_live_allocations(), launches = fxstub_bus_sends();
        std::vector<int64_t> bad = good.members;
        bad[(size_t)E - 1] = kN;
        CHECK(fxb_bus_set_sends(h, A, good.offsets.data(), bad.data(), gains.data()) == FX_E_ARG);
        bad[(size_t)E - 1] = -1;
        CHECK(fxb_bus_set_sends(h, A, good.offsets.data(), bad.data(), nullptr) == FX_E_ARG);
        std::vector<int64_t> offs = good.offsets;
        offs[0] = 1;
        CHECK(fxb_bus_set_sends(h, A, offs.data(), good.members.data(), nullptr) == FX_E_ARG);
        offs = good.offsets;
        std::swap(offs[1], offs[3]);
        CHECK(fxb_bus_set_sends(h, A, offs.data(), good.members.data(), nullptr) == FX_E_ARG);
        std::vector<float> inf = gains;
        inf[(size_t)(ch * E) - 1] = HUGE_VALF;
        CHECK(fxb_bus_set_sends(h, A, good.offsets.data(), good.members.data(), inf.data()) == FX_E_ARG);
        CHECK(fxb_bus_set_sends(h, -1, good.offsets.data(), good.members.data(), nullptr) == FX_E_ARG);
        CHECK(fxb_bus_set_sends(h, A, nullptr, good.members.data(), nullptr) == FX_E_ARG);
        CHECK(fxb_bus_set_sends(h, A, good.offsets.data(), nullptr, nullptr) == FX_E_ARG);
        const std::vector<int64_t> many(65538, 0);
        CHECK(fxb_bus_set_sends(h, 65537, many.data(), nullptr, nullptr) == FX_E_ARG);
        const int64_t tooLong[2] = {0, ((int64_t)1 << 24) + 1};
        CHECK(fxb_bus_set_sends(h, 1, tooLong, good.members.data(), nullptr) == FX_E_ARG);
        if (devices > 1) {   // a bus across two shards
            bad = good.members;
            bad[(size_t)good.offsets[1] - 1] = kBounds[1];   // (bus 0 is of the first shard)
            CHECK(fxb_bus_set_sends(h, A, good.offsets.data(), bad.data(), nullptr) == FX_E_ARG);
        }
        CHECK(fxb_bus_get_sends(h, nullptr, nullptr, -1, nullptr, nullptr, 0) == FX_E_ARG && fxb_bus_get_sends(h, nullptr, nullptr, 0, nullptr, nullptr, -1) == FX_E_ARG);
        if (state == 0) {
            CHECK(fxb_process_block_bus_aux(h, in.data(), out.data(), nullptr, aux.data(), S, kK, both) == FX_E_ARG);
            CHECK(fxb_bus_set_send_gains(h, gains.data(), 0) == FX_E_ARG);
            CHECK(fxb_bus_get_sends(h, nullptr, nullptr, 0, nullptr, nullptr, 0) == 0);
        } else {
            CHECK(fxb_bus_set_send_gains(h, inf.data(), 1) == FX_E_ARG && fxb_bus_set_send_gains(h, nullptr, 0) == FX_E_ARG && fxb_bus_set_send_gains(h, gains.data(), 2) == FX_E_ARG);
            CHECK(fxb_process_block_bus_aux(h, in.data(), wideOut.data(), nullptr, aux.data(), S, kK, FXB_BUS_SHARED_IN) == FX_E_ARG);
            CHECK(fxb_process_block_bus_aux(h, in.data(), out.data(), nullptr, aux.data(), S, 0, both) == FX_E_ARG);
            CHECK(fxb_process_block_bus_aux(h, in.data(), out.data(), nullptr, aux.data(), -1, kK, both) == FX_E_ARG);
            CHECK(fxb_process_block_bus_aux(h, nullptr, out.data(), nullptr, aux.data(), S, kK, both) == FX_E_ARG);
            CHECK(fxb_process_block_bus_aux(h, in.data(), out.data(), nullptr, aux.data(), S, kK, 4u | FXB_BUS_MIX_OUT) == FX_E_ARG);
            CHECK(fxb_process_block_bus_aux(h, in.data(), out.data(), nullptr, out.data(), S, kK, both) == FX_E_ARG);
            CHECK(fxb_process_block_bus_aux(h, in.data(), out.data(), aux.data(), aux.data(), S, kK, both) == FX_E_ARG);   // (taps are off, too)
            CHECK(fxb_process_block_bus_aux_dev(h, in.data(), out.data(), nullptr, aux.data(), S, kK, both, nullptr) == FX_E_ARG);   // pageable
            CHECK(sendsAre(h, good, gains, ch));
        }
        CHECK(fxb_process_block_bus_aux(nullptr, in.data(), out.data(), nullptr, aux.data(), S, kK, FXB_BUS_MIX_OUT) == FX_E_ARG);
        CHECK(fxb_bus_set_sends(nullptr, A, good.offsets.data(), good.members.data(), nullptr) == FX_E_ARG && fxb_bus_set_send_gains(nullptr, gains.data(), 0) == FX_E_ARG);
        CHECK(fxb_bus_get_sends(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) == FX_E_ARG);
        CHECK(fxstub_live_allocations() == live && fxstub_bus_sends() == launches);
        CHECK(aux == sentinel);
        CHECK(fxb_info(h, FXB_INFO_BUS_SEND_BLOCKS) == 0 && fxb_info(h, FXB_INFO_BUS_BLOCKS) == 0);
    }
    // the handle goes on
    CHECK(fxb_process_block_bus_aux(h, in.data(), out.data(), nullptr, aux.data(), S, kK, both) == 0);
    CHECK(auxRight(aux.data(), expanded(in, rows, kN, kK, G), S, ch, kN, good, gains, gains, false));
    fxb_destroy(h);
}

// an allocation that fails at every allocation of a set, then of the chunk sums and of a staged block: FX_E_MEMORY, the sends in
// force stay on every shard, nothing is launched, nothing leaks
void memory(int devices) {
    const int ch = 2, S = 4;
    const int three[3] = {0, 1, 2};
    fxb_handle* h = devices > 1 ? fxb_create_on_devices(kN, ch, three, 3) : fxb_create(kN, ch, 0);   // (no program yet: no builder thread allocates meanwhile)
    CHECK(h != nullptr);
    if (!h) return;
    Structure old;
    for (int k = 0; k < 3; ++k) addBus(old, devices > 1 ? kBounds[k] : 0, devices > 1 ? kBounds[k + 1] : kN, 2 + k);
    const Structure next = mixed(devices > 1);
    const std::vector<float> oldGains = filled((size_t)(ch * old.entries())), gains = filled((size_t)(ch * next.entries()));
    for (int state = 0; state < 2; ++state) {   // from off, from a structure in force
        if (state == 1) CHECK(fxb_bus_set_sends(h, old.buses(), old.offsets.data(), old.members.data(), oldGains.data()) == 0);
        const long live = fxstub_live_allocations();
        for (long nth = 0; nth < devices; ++nth) {   // one allocation per shard
            fxstub_fail_mallocs(nth, 1);
            const int rc = fxb_bus_set_sends(h, next.buses(), next.offsets.data(), next.members.data(), gains.data());
            fxstub_fail_mallocs(-1, 0);
            CHECK(rc == FX_E_MEMORY);
            CHECK(fxstub_live_allocations() == live);
            CHECK(state == 1 ? sendsAre(h, old, oldGains, ch) : fxb_bus_get_sends(h, nullptr, nullptr, 0, nullptr, nullptr, 0) == 0);
        }
    }
    CHECK(fxb_bus_set_sends(h, next.buses(), next.offsets.data(), next.members.data(), gains.data()) == 0);
    CHECK(fxb_load_text(h, kStereo) == 1);
    const int64_t A = next.buses(), G = fxb_bus_groups(h, kK), rows = (int64_t)S * ch;
    const std::vector<float> in = filled((size_t)(rows * G)), sentinel((size_t)(rows * A), -7.0f);
    std::vector<float> out((size_t)(rows * G)), aux = sentinel;
    CHECK(fxb_process_block_bus(h, in.data(), out.data(), S, kK, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == 0);   // (code, scratch and bus staging are there)
    CHECK(fxb_prepare(h, S, 1) == 0);                                                                          // (... and the builder thread is idle)
    // a staged block with aux rows allocates, per shard, the chunk sums, the device staging of its aux rows and - on a handle of
    // several shards - the pinned block from which it places its columns.  Sends off and on again in front of every attempt frees
    // them all, so that every attempt meets all of them: the nth one fails.
    const long perShard = devices > 1 ? 3 : 2, live = fxstub_live_allocations(), launches = fxstub_bus_sends(), kernels = fxstub_kernels_run();
    for (long nth = 0; nth < perShard * devices; ++nth) {
        CHECK(fxb_bus_set_sends(h, 0, nullptr, nullptr, nullptr) == 0);
        CHECK(fxb_bus_set_sends(h, next.buses(), next.offsets.data(), next.members.data(), gains.data()) == 0);
        CHECK(fxstub_live_allocations() == live);
        fxstub_fail_mallocs(nth, 1);
        const int rc = fxb_process_block_bus_aux(h, in.data(), out.data(), nullptr, aux.data(), S, kK, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT);
        fxstub_fail_mallocs(-1, 0);
        CHECK(rc == FX_E_MEMORY);
        // (on a handle of several shards the other shards have run their block and delivered their columns: the refusal is the
        // failing shard's, as with every allocation of a bus block)
        if (devices == 1) CHECK(aux == sentinel && fxstub_bus_sends() == launches && fxstub_kernels_run() == kernels);
        aux = sentinel;
    }
    CHECK(fxstub_live_allocations() <= live + perShard * devices);
    CHECK(fxb_process_block_bus_aux(h, in.data(), out.data(), nullptr, aux.data(), S, kK, FXB_BUS_SHARED_IN | FXB_BUS_MIX_OUT) == 0);
    CHECK(auxRight(aux.data(), expanded(in, rows, kN, kK, G), S, ch, kN, next, gains, gains, false));
    fxb_destroy(h);   // destroyed with sends on
}

}  // namespace

int main() {
    setenv("FXSTUB_DEVICES", "3", 1);   // (read by the stand-in at its first call)
    for (int devices = 1; devices <= 3; devices += 2) {
        indexing(devices);
        refusals(devices);
        memory(devices);
        std::printf("  bus sends, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_bus_send_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "bus send checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("bus send checks ok\n");
    return 0;
}
