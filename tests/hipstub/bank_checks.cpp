// bank_checks.cpp — the record bank (fxb_bank_*) driven without a GPU under AddressSanitizer + UBSan + LeakSanitizer (TEST
// INFRASTRUCTURE: csrc/Makefile `stubasanbank` links this file with the library's host sources and tests/hipstub/; a program of its
// own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The rule and the state machine are pinned by tests/test_bank_stub.py; this program is about addresses.  Every array the caller
// hands in is a heap block of exactly the documented size, every "device" block of the stand-in is a heap block too - the bank with
// exactly n_slots records, the pairs, the cells - so a read or write one word outside a list, an image, a slot, a shard's run of
// the entries or a delay line's column is a report.  It walks ring sizes on both sides of the 64-word tile, lists of 1, 64 and 65
// entries with the LAST slot of the bank among them, one handle and three shards, compares the whole state block with a rotation
// done here, and goes through the three gates (nothing changes, the entry and the reason are reported), the host refusals and an
// allocation failure at every allocation of a create.  Exit code 0 = every check held (a sanitizer report turns it non-zero by
// itself).
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fx8010_amd.h"
#include "hip_stub.h"

extern "C" long fxstub_bank_gathers(void);
extern "C" long fxstub_bank_scatters(void);
extern "C" long fxstub_bank_gated(void);
extern "C" long fxstub_bank_strays(void);

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            ++g_failures;                                                                \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                                \
    } while (0)

uint32_t g_seed = 4711u;
uint32_t draw() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 4;
}

std::string rings(int zi, int zx) {
    return "itramsize " + std::to_string(zi) + " \nxtramsize " + std::to_string(zx) +
           " \ninput in 0\noutput out 0\nstatic r1\nstatic xr\nidelay write, in, at, 0\nidelay read, r1, at, 0\nxdelay write, in, at, 0\nxdelay read, xr, at, 0\nmacs out, r1, xr, 0.5\nend";
}
const char* kOffset = "itramsize 8 \ninput in 0\noutput out 0\nstatic r1\nidelay write, in, at, 3\nidelay read, r1, at, 0\nmacs out, r1, 0.5, 0.5\nend";

const int64_t kN = 809;   // three shards: instances from 0, 320 and 576

fxb_handle* handle(int devices, const char* text) {
    const int three[3] = {0, 1, 2};
    fxb_handle* h = devices > 1 ? fxb_create_on_devices(kN, 1, three, 3) : fxb_create(kN, 1, 0);
    CHECK(h != nullptr);
    if (h) CHECK(fxb_load_text(h, text) == 1);
    return h;
}

// a whole-batch image taken apart (the layout of include/fx8010_amd.h fxb_save_state): records[n][W]
struct Block {
    std::vector<uint8_t> raw;
    int64_t n = 0;
    int channels = 0, regs = 0, rows = 0, islots = 0, xslots = 0;
    int64_t words() const { return (int64_t)rows + islots + xslots; }
    int cursors() const { return regs + channels; }
    uint32_t* body() { return reinterpret_cast<uint32_t*>(raw.data() + 64); }
    uint32_t& at(int64_t inst, int64_t w) {
        if (w < rows) return body()[w * n + inst];
        w -= rows;
        if (w < islots) return body()[(int64_t)rows * n + inst * islots + w];
        return body()[(int64_t)rows * n + n * islots + inst * xslots + (w - islots)];
    }
};

bool saved(fxb_handle* h, Block* b) {
    const int64_t bytes = fxb_state_size(h);
    if (bytes < 64) return false;
    b->raw.assign((size_t)bytes, 0);
    if (fxb_save_state(h, b->raw.data(), bytes) != 0) return false;
    std::memcpy(&b->n, b->raw.data() + 8, 8);
    int32_t f[5];
    std::memcpy(f, b->raw.data() + 16, 20);
    b->channels = f[0]; b->regs = f[1]; b->rows = f[2]; b->islots = f[3]; b->xslots = f[4];
    return b->n == kN && bytes == 64 + kN * b->words() * 4;
}

// positions: every instance at (wi, wi, wx, wx) with values of its own; random words behind the position rows
void fill(fxb_handle* h, Block* b, int zi, int zx) {
    CHECK(saved(h, b));
    for (int64_t i = 0; i < kN; ++i) {
        const uint32_t wi = draw() % (uint32_t)zi, wx = zx > 0 ? draw() % (uint32_t)zx : 0u;
        b->at(i, b->cursors() + 0) = wi; b->at(i, b->cursors() + 1) = wi;
        b->at(i, b->cursors() + 2) = wx; b->at(i, b->cursors() + 3) = wx;
        for (int64_t w = b->cursors() + 4; w < b->words(); ++w) b->at(i, w) = draw() * 2654435761u;
    }
    CHECK(fxb_load_state(h, b->raw.data(), (int64_t)b->raw.size()) == 0);
}

int mod(int64_t v, int z) { return (int)(((v % z) + z) % z); }

bool status(fxb_handle* h, int64_t refused, int64_t entry, int reason, int reset = 0) {
    int64_t r = -7, e = -7;
    int why = -7;
    return fxb_bank_status(h, &r, &e, &why, reset) == 0 && r == refused && e == entry && why == reason;
}

void indexing(int devices) {
    const int sizes[7][2] = {{1, 5}, {5, 7}, {7, 63}, {63, 64}, {64, 65}, {65, 1000}, {1000, 1}};
    for (const auto& z : sizes) {
        fxb_handle* h = handle(devices, rings(z[0], z[1]).c_str());
        if (!h) return;
        for (int64_t count : {(int64_t)1, (int64_t)64, (int64_t)65}) {
            Block b;
            fill(h, &b, z[0], z[1]);
            CHECK(fxb_bank_create(h, count) == 0 && fxb_bank_slots(h) == count);   // exactly the slots the call uses: the last one is in the list
            // sources from the front, destinations across the shard boundaries from the back; exactly-sized heap blocks
            std::vector<int64_t> src((size_t)count), dst((size_t)count), slots((size_t)count);
            for (int64_t k = 0; k < count; ++k) { src[(size_t)k] = k * 5 % 300 + (k % 3) * 250; dst[(size_t)k] = kN - 1 - k * 7; slots[(size_t)k] = count - 1 - k; }
            CHECK(fxb_bank_store(h, slots.data(), src.data(), count) == 0);
            const int64_t bytes = fxb_instance_image_size(h, count);
            std::vector<uint8_t> image((size_t)bytes), stored((size_t)bytes);
            CHECK(fxb_save_instances(h, src.data(), count, image.data(), bytes) == 0);
            CHECK(fxb_bank_get(h, slots.data(), count, stored.data(), bytes) == 0 && stored == image);
            CHECK(fxb_bank_recall(h, slots.data(), dst.data(), count) == 0);
            CHECK(status(h, 0, -1, 0));
            Block want = b, got;
            for (int64_t k = 0; k < count; ++k) {
                const int64_t s = src[(size_t)k], d = dst[(size_t)k];
                const int di = mod((int64_t)b.at(d, b.cursors()) - (int64_t)b.at(s, b.cursors()), z[0]);
                const int dx = mod((int64_t)b.at(d, b.cursors() + 2) - (int64_t)b.at(s, b.cursors() + 2), z[1]);
                for (int64_t w = 0; w < b.rows; ++w)
                    if (w < b.cursors() || w >= b.cursors() + 4) want.at(d, w) = b.at(s, w);
                for (int j = 0; j < z[0]; ++j) want.at(d, b.rows + (j + di) % z[0]) = b.at(s, b.rows + j);
                for (int j = 0; j < z[1]; ++j) want.at(d, b.rows + b.islots + (j + dx) % z[1]) = b.at(s, b.rows + b.islots + j);
            }
            CHECK(saved(h, &got));
            CHECK(got.raw == want.raw);
            // the same records through put, into a fresh bank: the same block again
            CHECK(fxb_load_state(h, b.raw.data(), (int64_t)b.raw.size()) == 0);
            CHECK(fxb_bank_create(h, count) == 0 && fxb_bank_put(h, slots.data(), count, image.data(), bytes) == 0);
            CHECK(fxb_bank_recall(h, slots.data(), dst.data(), count) == 0);
            CHECK(saved(h, &got) && got.raw == want.raw);
        }
        CHECK(fxb_info(h, FXB_INFO_INSTANCE_ROTATIONS) == 0 && fxb_info(h, FXB_INFO_INSTANCE_SCATTERS) == 0);
        fxb_destroy(h);
    }
}

void gates(int devices) {
    for (int program = 0; program < 2; ++program) {   // two rings; one line written at offset 3: no ring
        const int zi = program == 0 ? 64 : 8, zx = program == 0 ? 65 : 0;
        fxb_handle* h = handle(devices, program == 0 ? rings(zi, zx).c_str() : kOffset);
        if (!h) return;
        Block b, now;
        fill(h, &b, zi, zx);
        // (destinations of one shard: the gate holds per shard, and here nothing at all may change)
        const std::vector<int64_t> src = {0, 400, 700}, dst = {808, 590, 650}, slots = {2, 0, 1};
        // (the good entries of the line that is no ring: sources at their destinations' position)
        if (program == 1) {
            for (int k = 0; k < 3; ++k)
                for (int w = 0; w < 2; ++w) b.at(src[(size_t)k], b.cursors() + w) = b.at(dst[(size_t)k], b.cursors());
            CHECK(fxb_load_state(h, b.raw.data(), (int64_t)b.raw.size()) == 0);
        }
        const int64_t bytes = fxb_instance_image_size(h, 3);
        std::vector<uint8_t> good((size_t)bytes);
        CHECK(fxb_save_instances(h, src.data(), 3, good.data(), bytes) == 0);
        CHECK(fxb_bank_create(h, 3) == 0);
        auto word = [&](std::vector<uint8_t>& image, int64_t k, int64_t w) { return reinterpret_cast<uint32_t*>(image.data() + 64) + k * b.words() + w; };
        int64_t refusedCalls = 0;
        auto gated = [&](const std::vector<uint8_t>& image, int64_t entry, int reason) {
            const long before = fxstub_bank_gated();
            CHECK(fxb_bank_put(h, slots.data(), 3, image.data(), bytes) == 0);
            CHECK(fxb_bank_recall(h, slots.data(), dst.data(), 3) == 0);
            ++refusedCalls;
            CHECK(status(h, refusedCalls, entry, reason));
            CHECK(fxstub_bank_gated() > before);
            CHECK(saved(h, &now) && now.raw == b.raw);
        };
        for (int k = 0; k < 3; ++k)
            for (int w = 0; w < (program == 0 ? 4 : 2); ++w) {
                std::vector<uint8_t> bad = good;
                *word(bad, k, b.cursors() + w) = (uint32_t)(w < 2 ? zi : zx);   // outside 0 .. Z - 1
                gated(bad, k, FXB_BANK_BAD_POSITION);
                bad = good;
                *word(bad, k, b.cursors() + w) = (*word(bad, k, b.cursors() + w) + 1u) % (uint32_t)(w < 2 ? zi : zx);   // one kind moved alone
                gated(bad, k, FXB_BANK_PHASE);
            }
        if (program == 1) {
            std::vector<uint8_t> bad = good;   // both kinds one step on: a rotation the line cannot take
            for (int w = 0; w < 2; ++w) *word(bad, 1, b.cursors() + w) = (*word(bad, 1, b.cursors() + w) + 1u) % (uint32_t)zi;
            gated(bad, 1, FXB_BANK_NO_RING);
        }
        CHECK(status(h, refusedCalls, program == 1 ? 1 : 2, program == 1 ? FXB_BANK_NO_RING : FXB_BANK_PHASE, 1) && status(h, 0, -1, 0));
        // the host refusals: nothing launched, nothing changed
        const long gathers = fxstub_bank_gathers(), scatters = fxstub_bank_scatters(), live = fxstub_live_allocations();
        const std::vector<int64_t> twice = {590, 650, 590}, beyond = {590, 650, kN}, slotTwice = {0, 1, 0}, slotBeyond = {0, 1, 3}, slotBelow = {0, -1, 2};
        CHECK(fxb_bank_recall(h, slots.data(), twice.data(), 3) == FX_E_ARG && fxb_bank_recall(h, slots.data(), beyond.data(), 3) == FX_E_ARG);
        CHECK(fxb_bank_recall(h, slotBeyond.data(), dst.data(), 3) == FX_E_ARG && fxb_bank_recall(h, slotBelow.data(), dst.data(), 3) == FX_E_ARG);
        CHECK(fxb_bank_store(h, slotTwice.data(), src.data(), 3) == FX_E_ARG && fxb_bank_store(h, slotBeyond.data(), src.data(), 3) == FX_E_ARG);
        CHECK(fxb_bank_store(h, slots.data(), beyond.data(), 3) == FX_E_ARG && fxb_bank_store(h, nullptr, src.data(), 3) == FX_E_ARG);
        CHECK(fxb_bank_store(h, slots.data(), nullptr, 3) == FX_E_ARG && fxb_bank_store(h, slots.data(), src.data(), -1) == FX_E_ARG);
        CHECK(fxb_bank_put(h, slotTwice.data(), 3, good.data(), bytes) == FX_E_ARG && fxb_bank_put(h, slots.data(), 3, good.data(), bytes - 4) == FX_E_ARG);
        CHECK(fxb_bank_put(h, slots.data(), 2, good.data(), bytes) == FX_E_ARG && fxb_bank_put(h, slots.data(), 3, nullptr, bytes) == FX_E_ARG);
        std::vector<uint8_t> out((size_t)bytes - 4);
        CHECK(fxb_bank_get(h, slots.data(), 3, out.data(), bytes - 4) == FX_E_ARG && fxb_bank_get(h, slotBeyond.data(), 3, out.data(), bytes - 4) == FX_E_ARG);
        CHECK(fxb_bank_store(h, nullptr, nullptr, 0) == 0 && fxb_bank_recall(h, nullptr, nullptr, 0) == 0);
        CHECK(fxstub_bank_gathers() == gathers && fxstub_bank_scatters() == scatters && fxstub_live_allocations() == live);
        CHECK(saved(h, &now) && now.raw == b.raw);
        // ... and the good image still recalls
        CHECK(fxb_bank_put(h, slots.data(), 3, good.data(), bytes) == 0 && fxb_bank_recall(h, slots.data(), dst.data(), 3) == 0 && status(h, 0, -1, 0));
        CHECK(saved(h, &now));
        for (int k = 0; k < 3; ++k) CHECK(now.at(dst[(size_t)k], b.cursors() + 4) == b.at(src[(size_t)k], b.cursors() + 4));
        // an allocation that fails at every allocation of a create: FX_E_MEMORY, the bank in force stays and still holds its records
        const unsigned long long bytesInUse = fxstub_bytes_in_use();
        for (long nth = 0; nth < 8; ++nth) {
            fxstub_fail_mallocs(nth, 1);
            const int rc = fxb_bank_create(h, 7);
            fxstub_fail_mallocs(-1, 0);
            if (rc == 0) break;   // (every allocation of the call has been met)
            CHECK(rc == FX_E_MEMORY && fxb_bank_slots(h) == 3 && fxstub_bytes_in_use() == bytesInUse);
            std::vector<uint8_t> kept((size_t)bytes);
            CHECK(fxb_bank_get(h, slots.data(), 3, kept.data(), bytes) == 0 && kept == good);
        }
        CHECK(fxb_bank_slots(h) == 7);
        CHECK(fxb_bank_create(h, 0) == 0 && fxb_bank_slots(h) == 0 && fxb_bank_recall(h, slots.data(), dst.data(), 3) == FX_E_ARG);
        fxb_destroy(h);
    }
}

}  // namespace

int main() {
    setenv("FXSTUB_DEVICES", "3", 1);   // (read by the stand-in at its first call)
    CHECK(fxb_bank_create(nullptr, 1) == FX_E_ARG && fxb_bank_slots(nullptr) == 0);
    for (int devices = 1; devices <= 3; devices += 2) {
        indexing(devices);
        gates(devices);
        std::printf("  record bank, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_bank_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    if (g_failures) {
        std::fprintf(stderr, "record bank checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("record bank checks ok\n");
    return 0;
}
