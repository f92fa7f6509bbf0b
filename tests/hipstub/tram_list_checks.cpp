// tram_list_checks.cpp — the delay-line windows by list of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan +
// LeakSanitizer (TEST INFRASTRUCTURE: csrc/Makefile `stubasantramlist` links this file with the library's host sources and
// tests/hipstub/; a program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The twin comparison is tests/test_tram_list_stub.py; this program is about addresses.  Every array the caller hands in is a heap
// block of exactly the documented size - [count] instances, [count][n_words] values, [n_words] with FXB_TRAM_BROADCAST - and every
// "device" block of the stand-in is a heap block too, so a read or write one word outside the list, the values, the staging or a
// delay line is a report.  It walks lists of 1, 2, 63, 64, 65 and all entries, the first and the last instance always among them,
// windows of 1, 63, 64, 65 and Z words that begin at the start, in the middle and at the last word of a ring, physical and logical,
// under both addressings, for N = 5, 65, 200 and 777 on one handle and N = 808 on three shards, with positions that differ per
// instance (loaded with a state image), a block in front of and behind every set; the refusals (nothing changes); and allocation
// failures at every allocation of a call.  The words are checked against a host model of the lines written from the definition in
// include/fx8010_amd.h "Delay-line windows by list" with `%`: by fxb_get_tram_list in both modes and by fxb_get_tram_i.
// Exit code 0 = every check held (a sanitizer report turns it non-zero by itself).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fx8010_amd.h"
#include "hip_stub.h"

extern "C" long fxstub_tram_scatters(void);   // fx_tram_stub.cpp
extern "C" long fxstub_tram_gathers(void);
extern "C" long fxstub_tram_strays(void);

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            ++g_failures;                                                                \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                                \
    } while (0)

// iTRAM a ring of 64, xTRAM a ring of 500
const char* kRings = "itramsize 64 \nxtramsize 500 \ninput in 0\noutput out 0\ncontrol vol = 0.5\nstatic r1\nstatic xr\nidelay write, in, at, 0\nidelay read, r1, at, 3\n"
                     "xdelay write, in, at, 0\nxdelay read, xr, at, 2\nmacs out, r1, xr, vol\nend";
// iTRAM a ring of 64, xTRAM written at offset 3: 503 slots for a line of 500, no ring
const char* kOffset = "itramsize 64 \nxtramsize 500 \ninput in 0\noutput out 0\ncontrol vol = 0.5\nstatic r1\nstatic xr\nidelay write, in, at, 0\nidelay read, r1, at, 7\n"
                      "xdelay write, in, at, 3\nxdelay read, xr, at, 403\nmacs out, r1, xr, vol\nend";

uint32_t g_seed = 24680u;
uint32_t draw() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

// words of every kind: mostly plain patterns, and +-0, denormals, +-1e30, a quiet NaN with a payload and a signalling one
uint32_t word() {
    static const uint32_t kSpecial[8] = {0x00000000u, 0x80000000u, 0x00000001u, 0x807fffffu, 0x7149f2cau, 0xf149f2cau, 0x7fc12345u, 0x7f812345u};
    const uint32_t d = draw();
    return (d >> 16) % 5 == 0 ? kSpecial[(d >> 19) & 7] : d * 2654435761u;
}

// `count` distinct instances of 0..range-1 in a shuffled order, the first and the last among them (from two entries on)
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

fxb_handle* create(int64_t N, int devices) {
    const int three[3] = {0, 1, 2};
    return devices > 1 ? fxb_create_on_devices(N, 1, three, 3) : fxb_create(N, 1, 0);
}

// a handle and what its two delay lines must hold: line[which][instance * slots + slot], and the write positions
struct Model {
    fxb_handle* h = nullptr;
    int64_t n = 0;
    bool dane = false;
    int slots[2] = {0, 0};
    std::vector<uint32_t> line[2];
    std::vector<int64_t> pos[2];

    // positions that differ per instance, through the whole-batch image: header (64 bytes: ... int32 channels, registers, rows,
    // iSlots, xSlots at byte 16), then the state rows [rows][n] - the four position rows begin at registers + channels
    bool open(const char* text, int64_t N, int devices, bool daneModel) {
        n = N;
        dane = daneModel;
        h = create(N, devices);
        if (!h) return false;
        if (dane && fxb_set_option(h, FX_OPT_TRAM_DANE, 1) != 0) return false;
        if (fxb_load_text(h, text) != 1) return false;
        slots[0] = (int)fxb_info(h, FXB_INFO_ITRAM_SLOTS);
        slots[1] = (int)fxb_info(h, FXB_INFO_XTRAM_SLOTS);
        const int64_t bytes = fxb_state_size(h);
        if (bytes < 64) return false;
        std::vector<unsigned char> image((size_t)bytes);
        if (fxb_save_state(h, image.data(), bytes) < 0) return false;
        int32_t shape[5];
        std::memcpy(shape, image.data() + 16, sizeof shape);
        const int64_t cursors = (int64_t)shape[1] + shape[0];
        const int size[2] = {64, 500};
        for (int which = 0; which < 2; ++which) {
            pos[which].assign((size_t)n, 0);
            for (int64_t i = 0; i < n; ++i) {
                const uint32_t w = (uint32_t)((i * 7 + which * 3) % size[which]), r = (uint32_t)((i * 5 + 1) % size[which]);
                pos[which][(size_t)i] = w;
                std::memcpy(image.data() + 64 + ((cursors + 2 * which) * n + i) * 4, &w, 4);
                std::memcpy(image.data() + 64 + ((cursors + 2 * which + 1) * n + i) * 4, &r, 4);
            }
        }
        if (fxb_load_state(h, image.data(), bytes) != 0) return false;
        for (int which = 0; which < 2; ++which) {
            line[which].assign((size_t)n * (size_t)slots[which], 0u);
            int32_t cur[4];
            for (int64_t i = 0; i < n; ++i) CHECK(fxb_get_cursors_i(h, i, cur) == 0 && cur[2 * which] == pos[which][(size_t)i]);
        }
        return true;
    }
    int64_t slotOf(int which, int64_t inst, int64_t k, bool logical) const {
        if (!logical) return k;
        const int64_t Z = slots[which], p = pos[which][(size_t)inst];
        return dane ? (p + 1 + k) % Z : (((p - 1 - k) % Z) + Z) % Z;
    }
    bool set(int which, const std::vector<int64_t>& list, int first, int nWords, unsigned flags) {
        const bool broadcast = (flags & FXB_TRAM_BROADCAST) != 0, logical = (flags & FXB_TRAM_LOGICAL) != 0;
        std::vector<uint32_t> values((broadcast ? 1 : list.size()) * (size_t)nWords);
        for (uint32_t& v : values) v = word();
        std::vector<int64_t> given = list;
        std::vector<uint32_t> handed = values;
        if (fxb_set_tram_list(h, which, given.data(), (int64_t)given.size(), first, nWords, reinterpret_cast<const float*>(handed.data()), flags) != 0) return false;
        std::fill(given.begin(), given.end(), -5);   // the arrays are the caller's again on return
        std::fill(handed.begin(), handed.end(), 0xdeadbeefu);
        for (size_t i = 0; i < list.size(); ++i)
            for (int j = 0; j < nWords; ++j)
                line[which][(size_t)list[i] * (size_t)slots[which] + (size_t)slotOf(which, list[i], first + j, logical)] = values[(broadcast ? 0 : i * (size_t)nWords) + (size_t)j];
        return true;
    }
    // the get in both modes (logical where the line is a ring, physical where the window fits the slots) and, on short lists, fxb_get_tram_i
    bool same(int which, const std::vector<int64_t>& list, int first, int nWords, bool ring) {
        bool ok = true;
        for (int logical = 0; logical <= (ring ? 1 : 0); ++logical) {
            if (!logical && first + nWords > slots[which]) continue;   // (a window that wraps the ring has no physical twin)
            std::vector<uint32_t> got(list.size() * (size_t)nWords, 0x99999999u);
            if (fxb_get_tram_list(h, which, list.data(), (int64_t)list.size(), first, nWords, reinterpret_cast<float*>(got.data()), logical ? FXB_TRAM_LOGICAL : 0u) != 0) return false;
            for (size_t i = 0; i < list.size(); ++i)
                for (int j = 0; j < nWords; ++j)
                    ok = ok && got[i * (size_t)nWords + (size_t)j] == line[which][(size_t)list[i] * (size_t)slots[which] + (size_t)slotOf(which, list[i], first + j, logical != 0)];
        }
        if (list.size() <= 3) {
            std::vector<uint32_t> whole((size_t)slots[which]);
            for (const int64_t inst : list) {
                if (fxb_get_tram_i(h, which, inst, reinterpret_cast<float*>(whole.data()), slots[which]) != 0) return false;
                ok = ok && std::memcmp(whole.data(), line[which].data() + (size_t)inst * (size_t)slots[which], (size_t)slots[which] * 4) == 0;
            }
        }
        return ok;
    }
    bool block(int S) {
        std::vector<float> in((size_t)S * (size_t)n, 0.25f), out(in.size(), 0.0f);
        return fxb_process_block(h, in.data(), out.data(), S) == 0;
    }
};

// one handle (devices == 1) or three shards through every indexing shape
void indexing(int devices) {
    const int64_t single[4] = {5, 65, 200, 777}, sharded[1] = {808};
    for (int which = 0; which < (devices > 1 ? 1 : 4); ++which)
        for (int dane = 0; dane <= 1; ++dane) {
            Model m;
            CHECK(m.open(kRings, devices > 1 ? sharded[which] : single[which], devices, dane != 0));
            if (!m.h) return;
            CHECK(fxb_info(m.h, FXB_INFO_INSTANCE_RINGS) == 3 && m.slots[0] == 64 && m.slots[1] == 500);
            const int64_t counts[6] = {1, 2, 63, 64, 65, m.n};
            const long strays = fxstub_tram_strays();
            int64_t sets = 0;
            int round = 0;
            for (int line = 0; line < 2; ++line) {
                const int Z = m.slots[line];
                for (const int nWords : {1, 63, 64, 65, Z}) {
                    if (nWords > Z) continue;
                    for (int logical = 0; logical <= 1; ++logical, ++round) {
                        const int firsts[3] = {0, logical ? Z / 2 : (Z - nWords) / 2, logical ? Z - 1 : Z - nWords};
                        const int first = firsts[round % 3];
                        const std::vector<int64_t> list = someOf(m.n, counts[round % 6]);
                        const unsigned flags = (logical ? FXB_TRAM_LOGICAL : 0u) | (round % 4 == 3 ? FXB_TRAM_BROADCAST : 0u);
                        CHECK(m.set(line, list, first, nWords, flags));
                        CHECK(m.same(line, list, first, nWords, true));
                        CHECK(m.same(line, someOf(m.n, counts[(round + 1) % 6]), first, nWords, true));
                        CHECK(m.block(round % 3 == 0 ? 33 : round % 3));
                        CHECK(m.same(line, list, first, nWords, true));
                        ++sets;
                    }
                }
            }
            CHECK(fxb_info(m.h, FXB_INFO_TRAM_LIST_SETS) >= sets && fxb_info(m.h, FXB_INFO_TRAM_LIST_SETS) <= sets * devices);
            CHECK(fxb_info(m.h, FXB_INFO_TRAM_LIST_GETS) >= 1);
            // repeats in a get; nothing listed; no words
            const std::vector<int64_t> again{m.n - 1, 0, m.n - 1, m.n - 1};
            CHECK(m.same(1, again, 499, 500, true));
            CHECK(fxb_set_tram_list(m.h, 0, nullptr, 0, 0, 4, nullptr, 0) == 0 && fxb_get_tram_list(m.h, 1, nullptr, 0, 0, 4, nullptr, FXB_TRAM_LOGICAL) == 0);
            CHECK(fxb_set_tram_list(m.h, 0, again.data(), 1, 64, 0, nullptr, 0) == 0);
            CHECK(fxb_sync(m.h) == 0 && fxstub_tram_strays() == strays);
            fxb_destroy(m.h);
        }
}

void refusals(int devices) {
    Model e;
    e.h = create(808, devices);
    CHECK(e.h != nullptr);
    if (!e.h) return;
    const std::vector<int64_t> good{3, 0, 807};
    std::vector<float> values(3 * 65, 0.5f);
    CHECK(fxb_set_tram_list(e.h, 0, good.data(), 3, 0, 4, values.data(), 0) == FX_E_NOTREADY);   // no program
    CHECK(fxb_get_tram_list(e.h, 0, good.data(), 3, 0, 4, values.data(), 0) == FX_E_NOTREADY);
    fxb_destroy(e.h);
    Model m;
    CHECK(m.open(kOffset, 808, devices, false));
    if (!m.h) return;
    CHECK(fxb_info(m.h, FXB_INFO_INSTANCE_RINGS) == 1 && m.slots[1] == 503);
    CHECK(m.set(0, someOf(m.n, 65), 60, 64, FXB_TRAM_LOGICAL) && m.set(1, someOf(m.n, 65), 438, 65, 0) && m.block(8));
    const int64_t sets = fxb_info(m.h, FXB_INFO_TRAM_LIST_SETS), gets = fxb_info(m.h, FXB_INFO_TRAM_LIST_GETS);
    const long live = fxstub_live_allocations(), scatters = fxstub_tram_scatters(), gathers = fxstub_tram_gathers();
    const std::vector<int64_t> twice{5, 9, 5}, above{0, 808, 1}, below{0, 1, -1}, lone{0};
    CHECK(fxb_set_tram_list(m.h, 0, twice.data(), 3, 0, 4, values.data(), 0) == FX_E_ARG && std::strstr(fxb_last_error(m.h), "entry 2"));
    CHECK(fxb_get_tram_list(m.h, 0, good.data(), 3, 0, 4, values.data(), FXB_TRAM_BROADCAST) == FX_E_ARG && std::strstr(fxb_last_error(m.h), "flags"));
    for (int get = 0; get <= 1; ++get) {
        auto call = [&](int which, const int64_t* list, int64_t count, int first, int nWords, float* v, unsigned flags) {
            return get ? fxb_get_tram_list(m.h, which, list, count, first, nWords, v, flags) : fxb_set_tram_list(m.h, which, list, count, first, nWords, v, flags);
        };
        CHECK(call(0, above.data(), 3, 0, 4, values.data(), 0) == FX_E_ARG && std::strstr(fxb_last_error(m.h), "entry 1"));
        CHECK(call(0, below.data(), 3, 0, 4, values.data(), FXB_TRAM_LOGICAL) == FX_E_ARG && std::strstr(fxb_last_error(m.h), "entry 2"));
        CHECK(call(0, good.data(), -1, 0, 4, values.data(), 0) == FX_E_ARG);
        CHECK(call(0, lone.data(), (int64_t)1 << 31, 0, 4, values.data(), 0) == FX_E_ARG);   // refused before the list is read
        CHECK(call(0, nullptr, 3, 0, 4, values.data(), 0) == FX_E_ARG);
        CHECK(call(0, good.data(), 3, 0, 4, nullptr, 0) == FX_E_ARG);
        CHECK(call(2, good.data(), 3, 0, 4, values.data(), 0) == FX_E_ARG && std::strstr(fxb_last_error(m.h), "which"));
        CHECK(call(-1, good.data(), 3, 0, 4, values.data(), 0) == FX_E_ARG);
        CHECK(call(0, good.data(), 3, 0, 4, values.data(), 4u) == FX_E_ARG && std::strstr(fxb_last_error(m.h), "flags"));
        CHECK(call(0, good.data(), 3, -1, 4, values.data(), 0) == FX_E_ARG);
        CHECK(call(0, good.data(), 3, 0, -1, values.data(), 0) == FX_E_ARG);
        CHECK(call(0, good.data(), 3, 0, 0, values.data(), FXB_TRAM_LOGICAL) == FX_E_ARG);
        CHECK(call(0, good.data(), 3, 61, 4, values.data(), 0) == FX_E_ARG);                  // physical: one word past the slots
        CHECK(call(1, good.data(), 3, 500, 4, values.data(), 0) == FX_E_ARG);                 // ... of the line that is no ring
        CHECK(call(0, good.data(), 3, 64, 1, values.data(), FXB_TRAM_LOGICAL) == FX_E_ARG);   // logical: first = Z
        CHECK(call(0, good.data(), 3, 0, 65, values.data(), FXB_TRAM_LOGICAL) == FX_E_ARG);   // logical: n_words = Z + 1
        CHECK(call(1, good.data(), 3, 0, 4, values.data(), FXB_TRAM_LOGICAL) == FX_E_ARG && std::strstr(fxb_last_error(m.h), "ring"));
        CHECK((get ? fxb_get_tram_list(nullptr, 0, good.data(), 3, 0, 4, values.data(), 0) : fxb_set_tram_list(nullptr, 0, good.data(), 3, 0, 4, values.data(), 0)) == FX_E_ARG);
    }
    CHECK(fxstub_live_allocations() == live && fxstub_tram_scatters() == scatters && fxstub_tram_gathers() == gathers);
    CHECK(fxb_info(m.h, FXB_INFO_TRAM_LIST_SETS) == sets && fxb_info(m.h, FXB_INFO_TRAM_LIST_GETS) == gets);
    CHECK(std::all_of(values.begin(), values.end(), [](float v) { return v == 0.5f; }));
    CHECK(m.same(0, good, 0, 64, true) && m.same(1, good, 0, 503, false));
    CHECK(fxb_get_tram_list(m.h, 0, twice.data(), 3, 0, 4, values.data(), FXB_TRAM_LOGICAL) == 0);   // repeats are a refusal of the set only
    CHECK(m.block(8) && m.same(1, good, 0, 503, false));
    fxb_destroy(m.h);
}

// an allocation that fails inside a call, at every allocation it makes (the device staging and the pinned staging of every
// shard): FX_E_MEMORY, nothing has changed on any shard, and the same call goes through afterwards
void memory(int devices) {
    for (int get = 0; get <= 1; ++get)
        for (long nth = 0; nth < 2L * devices; ++nth) {
            Model m;
            CHECK(m.open(kRings, 808, devices, false));
            if (!m.h) return;
            const std::vector<int64_t> list = someOf(m.n, m.n / 2);   // (entries on every shard)
            CHECK(fxb_prepare(m.h, 8, 1) == 0 && m.block(8) && fxb_prepare(m.h, 8, 1) == 0);   // (the builder threads are idle while allocations fail)
            std::vector<float> values(list.size() * 65, 0.5f);
            fxstub_fail_mallocs(nth, 1);
            const int rc = get ? fxb_get_tram_list(m.h, 1, list.data(), (int64_t)list.size(), 470, 65, values.data(), FXB_TRAM_LOGICAL)
                               : fxb_set_tram_list(m.h, 1, list.data(), (int64_t)list.size(), 470, 65, values.data(), FXB_TRAM_LOGICAL);
            fxstub_fail_mallocs(-1, 0);
            CHECK(rc == FX_E_MEMORY);
            CHECK(fxb_info(m.h, FXB_INFO_TRAM_LIST_SETS) == 0 && fxb_info(m.h, FXB_INFO_TRAM_LIST_GETS) == 0);
            CHECK(std::all_of(values.begin(), values.end(), [](float v) { return v == 0.5f; }));
            CHECK(m.same(1, {0, m.n - 1, 400}, 0, 500, true));
            CHECK(m.set(1, list, 470, 65, FXB_TRAM_LOGICAL) && m.same(1, list, 470, 65, true));
            CHECK(m.block(8));
            CHECK(m.set(0, someOf(m.n, 65), 0, 64, 0));   // destroyed with a scatter queued
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
        std::printf("  tram lists, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_tram_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "tram list checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("tram list checks ok\n");
    return 0;
}
