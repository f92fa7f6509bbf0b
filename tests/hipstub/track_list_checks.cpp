// track_list_checks.cpp — the register tracks by list of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan +
// LeakSanitizer (TEST INFRASTRUCTURE: csrc/Makefile `stubasantracklist` links this file with the library's host sources and
// tests/hipstub/; a program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The bookkeeping is pinned by tests/test_track_list_stub.py; this program is about addresses.  Every array the caller hands in is
// a heap block of exactly the documented size - [n_keys] names, [count] instances, [n_steps][n_keys][count] values - and every
// "device" block of the stand-in is a heap block too, so a read or write one word outside the list, the values, the staging, the
// ranges or the event rows is a report.  It walks lists of 1, 2, 63, 64, 65 and all entries, one and two keys, the schedule shapes
// (first, period, steps) = (0, 8, 4), (0, 1, 32), (13, 1, 1), (3, 5, 9), (32, 1, 1), (31, 7, 2) for blocks of 32 and 45 samples, two
// schedules on one register, on the translated tier (the expanded rows are read back and compared with a host model) and, with
// FX_KERNEL=asm in the environment of a second pass, on a tier that cuts the block (the rows of the registers afterwards), for
// N = 200 on one handle and N = 808 on three shards; the refusals (nothing changes); allocation failures at every allocation.
// Exit code 0 = every check held (a sanitizer report turns it non-zero by itself).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/fx8010_amd.h"
#include "hip_stub.h"

extern "C" long fxstub_track_holds(void);   // fx_tracks_stub.cpp
extern "C" long fxstub_track_scatters(void);
extern "C" long fxstub_track_strays(void);
extern "C" long long fxstub_track_table(int* out, int cap);
extern "C" long long fxstub_track_rows(uint32_t* out, long long cap);
extern "C" long fxstub_reg_strays(void);    // fx_registers_stub.cpp

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            ++g_failures;                                                                \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                                \
    } while (0)

const char* kText = "input in 0\noutput out 0\ncontrol coef = 0.5\ncontrol gain = 0.25\nstatic a\nmacs a, a, coef, in\nmacs out, a, in, gain\nend";
const int kShapes[6][3] = {{0, 8, 4}, {0, 1, 32}, {13, 1, 1}, {3, 5, 9}, {32, 1, 1}, {31, 7, 2}};

uint32_t g_seed = 24680u;
uint32_t draw() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}
float word() {
    static const uint32_t kSpecial[8] = {0x00000000u, 0x80000000u, 0x00000001u, 0x807fffffu, 0x7149f2cau, 0xf149f2cau, 0x7fc12345u, 0xffa00001u};
    const uint32_t d = draw();
    float f = (float)((int)(d & 0xffff) - 32768) / 20000.0f;
    if ((d >> 16) % 5 == 0) std::memcpy(&f, &kSpecial[(d >> 19) & 7], 4);
    return f;
}
uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

std::vector<int64_t> someOf(int64_t lo, int64_t hi, int64_t count) {   // `count` distinct instances of lo..hi-1, shuffled, lo and hi-1 among them
    std::vector<int64_t> all;
    for (int64_t i = lo; i < hi; ++i) all.push_back(i);
    for (size_t i = all.size() - 1; i > 0; --i) std::swap(all[i], all[draw() % (uint32_t)(i + 1)]);
    count = std::min<int64_t>(count, (int64_t)all.size());
    if (count >= 2 && count < (int64_t)all.size()) {
        std::swap(*std::find(all.begin(), all.end(), lo), all[0]);
        std::swap(*std::find(all.begin() + 1, all.end(), hi - 1), all[(size_t)count - 1]);
    }
    all.resize((size_t)count);
    return all;
}

fxb_handle* create(int64_t N, int devices) {
    const int three[3] = {0, 1, 2};
    return devices > 1 ? fxb_create_on_devices(N, 1, three, 3) : fxb_create(N, 1, 0);
}

struct Schedule {
    std::vector<std::string> keys;
    std::vector<int64_t> list;
    std::vector<float> values;   // [steps][keys][count]
    int steps, first, period;
    std::vector<int> due(int S) const {
        std::vector<int> d;
        for (int q = 0; q < steps && first + q * period < S; ++q) d.push_back(first + q * period);
        return d;
    }
};

Schedule make(const std::vector<std::string>& keys, const std::vector<int64_t>& list, int first, int period, int steps) {
    Schedule s{keys, list, std::vector<float>((size_t)steps * keys.size() * list.size()), steps, first, period};
    for (float& v : s.values) v = word();
    return s;
}

// arms through exactly-sized heap blocks, which are scribbled on and freed before the block runs
int arm(fxb_handle* h, const Schedule& s) {
    const char** table = static_cast<const char**>(std::malloc(sizeof(char*) * s.keys.size()));
    for (size_t k = 0; k < s.keys.size(); ++k) table[k] = s.keys[k].c_str();
    int64_t* list = static_cast<int64_t*>(std::malloc(8 * s.list.size()));
    float* values = static_cast<float*>(std::malloc(4 * s.values.size()));
    std::memcpy(list, s.list.data(), 8 * s.list.size());
    std::memcpy(values, s.values.data(), 4 * s.values.size());
    const int rc = fxb_set_register_tracks_list(h, table, (int)s.keys.size(), list, (int64_t)s.list.size(), values, s.steps, s.first, s.period);
    std::memset(list, 0xee, 8 * s.list.size());
    std::memset(values, 0xee, 4 * s.values.size());
    std::free(list);
    std::free(values);
    std::free(table);
    return rc;
}

std::vector<float> row(fxb_handle* h, const char* key, int64_t N) {
    std::vector<float> r((size_t)N);
    CHECK(fxb_get_register_array(h, key, r.data()) == 0);
    return r;
}

void block(fxb_handle* h, int64_t N, int S) {
    std::vector<float> x((size_t)S * (size_t)N), y((size_t)S * (size_t)N, -3.0f);
    for (float& v : x) v = word();
    CHECK(fxb_process_block(h, x.data(), y.data(), S) == 0);
    CHECK(std::memcmp(x.data(), y.data(), x.size() * 4) == 0);   // (the stand-in's emulation launch copies its input)
}

// one block with `schedules` armed.  Translated tier, one shard: the expanded rows against the model.  A tier that cuts the block:
// the registers' rows afterwards - a listed voice holds its last applied step, every other voice what it held.
void run(fxb_handle* h, int64_t N, int S, const std::vector<Schedule>& schedules, bool cuts, bool oneShard, const std::map<std::string, int>& regOf) {
    std::map<std::string, std::vector<float>> held;
    for (const Schedule& s : schedules)
        for (const std::string& k : s.keys)
            if (!held.count(k)) held[k] = row(h, k.c_str(), N);
    for (const Schedule& s : schedules) CHECK(arm(h, s) == 0);
    const long holds = fxstub_track_holds();
    block(h, N, S);
    CHECK(fxb_sync(h) == 0);
    bool any = false;
    for (const Schedule& s : schedules) any = any || !s.due(S).empty();
    if (cuts) {
        CHECK(fxstub_track_holds() == holds);
        for (auto& kv : held) {
            std::vector<float> want = kv.second;
            for (const Schedule& s : schedules) {
                const auto at = std::find(s.keys.begin(), s.keys.end(), kv.first);
                const std::vector<int> due = s.due(S);
                if (at == s.keys.end() || due.empty()) continue;
                const size_t k = (size_t)(at - s.keys.begin()), q = due.size() - 1;
                for (size_t i = 0; i < s.list.size(); ++i) want[(size_t)s.list[i]] = s.values[(q * s.keys.size() + k) * s.list.size() + i];
            }
            const std::vector<float> got = row(h, kv.first.c_str(), N);
            CHECK(std::memcmp(got.data(), want.data(), (size_t)N * 4) == 0);
        }
        return;
    }
    if (!oneShard) { CHECK(any ? fxstub_track_holds() > holds : fxstub_track_holds() == holds); return; }
    CHECK(fxstub_track_holds() == holds + (any ? 1 : 0));
    if (!any) return;
    int table[1 + 3 * 16] = {0};
    const long long nPad = fxstub_track_table(table, 1 + 3 * 16);
    const long long total = fxstub_track_rows(nullptr, 0);
    std::vector<uint32_t> rows((size_t)(total * nPad));
    CHECK(fxstub_track_rows(rows.data(), (long long)rows.size()) == total);
    for (auto& kv : held) {
        std::set<int> samples;
        for (const Schedule& s : schedules)
            if (std::find(s.keys.begin(), s.keys.end(), kv.first) != s.keys.end())
                for (int t : s.due(S)) samples.insert(t);
        const std::vector<int> events(samples.begin(), samples.end());
        if (events.empty()) continue;
        std::vector<std::vector<float>> want(events.size(), kv.second);
        for (const Schedule& s : schedules) {
            const auto at = std::find(s.keys.begin(), s.keys.end(), kv.first);
            if (at == s.keys.end()) continue;
            const size_t k = (size_t)(at - s.keys.begin());
            const std::vector<int> due = s.due(S);
            for (size_t q = 0; q < due.size(); ++q) {
                const size_t lo = (size_t)(std::find(events.begin(), events.end(), due[q]) - events.begin());
                const size_t hi = q + 1 < due.size() ? (size_t)(std::find(events.begin(), events.end(), due[q + 1]) - events.begin()) : events.size();
                for (size_t e = lo; e < hi; ++e)
                    for (size_t i = 0; i < s.list.size(); ++i) want[e][(size_t)s.list[i]] = s.values[(q * s.keys.size() + k) * s.list.size() + i];
            }
        }
        int first = -1, count = 0;
        for (int t = 0; t < table[0]; ++t)
            if (table[1 + 3 * t] == regOf.at(kv.first)) { first = table[2 + 3 * t]; count = table[3 + 3 * t]; }
        CHECK(first >= 0 && count == (int)events.size());
        if (first < 0 || count != (int)events.size()) continue;
        for (size_t e = 0; e < events.size(); ++e)
            for (int64_t i = 0; i < N; ++i) CHECK(rows[(size_t)((first + (long long)e) * nPad + i)] == bits(want[e][(size_t)i]));
    }
}

void shapes(int64_t N, int devices, bool cuts) {
    fxb_handle* h = create(N, devices);
    CHECK(h && fxb_load_text(h, kText) == 1);
    if (!h) return;
    std::map<std::string, int> regOf;   // (a register's state row is its number)
    fxp_handle* p = fxp_create(1);
    CHECK(p && fxp_load_text(p, kText) == 1);
    for (int r = 0; p && r < fxp_num_registers(p); ++r) regOf[fxp_register_name(p, r)] = r;
    fxp_destroy(p);
    CHECK(regOf.count("coef") && regOf.count("gain"));
    std::vector<float> per((size_t)N);
    for (float& v : per) v = word();
    CHECK(fxb_set_register_array(h, "coef", per.data()) == 0);
    block(h, N, 8);
    const int64_t counts[6] = {1, 2, 63, 64, 65, N};
    int step = 0;
    for (int S : {32, 45})
        for (int64_t count : counts)
            for (const int* shape : {kShapes[0], kShapes[1], kShapes[2], kShapes[3], kShapes[4], kShapes[5]}) {
                const std::vector<std::string> keys = (step++ % 2) ? std::vector<std::string>{"gain", "coef"} : std::vector<std::string>{"coef"};
                run(h, N, S, {make(keys, someOf(0, N, count), shape[0], shape[1], shape[2])}, cuts, devices == 1, regOf);
            }
    // two schedules on one register, disjoint lists, interleaved events; a third on the other register
    const std::vector<int64_t> all = someOf(0, N, N);
    const std::vector<int64_t> a(all.begin(), all.begin() + 65), b(all.begin() + 65, all.begin() + 130), c(all.begin() + 130, all.end());
    for (int S : {32, 45}) run(h, N, S, {make({"coef"}, a, 0, 8, 4), make({"gain", "coef"}, b, 3, 5, 9), make({"gain"}, c, 13, 1, 1)}, cuts, devices == 1, regOf);
    fxb_destroy(h);
}

void refusals(int64_t N, int devices) {
    fxb_handle* h = create(N, devices);
    CHECK(h != nullptr);
    if (!h) return;
    const Schedule good = make({"coef", "gain"}, someOf(0, N, 3), 0, 8, 2);
    CHECK(arm(h, good) == FX_E_NOTREADY);
    CHECK(fxb_load_text(h, kText) == 1);
    block(h, N, 8);
    const long holds = fxstub_track_holds();
    auto refused = [&](Schedule s, int rc) {
        CHECK(arm(h, s) == rc);
        CHECK(fxb_last_error(h)[0] != 0);
    };
    Schedule s = good;
    s.list[1] = N; refused(s, FX_E_ARG);
    s = good; s.list[2] = -1; refused(s, FX_E_ARG);
    s = good; s.list[2] = s.list[0]; refused(s, FX_E_ARG);
    s = good; s.keys[1] = "coef"; refused(s, FX_E_ARG);
    s = good; s.keys[1] = "nosuch"; refused(s, 1);
    s = good; s.keys[0] = "a"; refused(s, FX_E_ARG);
    s = good; s.keys[0] = "out"; refused(s, FX_E_ARG);
    s = good; s.period = 0; refused(s, FX_E_ARG);
    s = good; s.first = -1; refused(s, FX_E_ARG);
    const char* names[2] = {"coef", "gain"};
    CHECK(fxb_set_register_tracks_list(h, names, 2, good.list.data(), 3, good.values.data(), 0, 0, 8) == FX_E_ARG);
    CHECK(fxb_set_register_tracks_list(h, names, 2, good.list.data(), -1, good.values.data(), 2, 0, 8) == FX_E_ARG);
    CHECK(fxb_set_register_tracks_list(h, names, -1, good.list.data(), 3, good.values.data(), 2, 0, 8) == FX_E_ARG);
    CHECK(fxb_set_register_tracks_list(h, nullptr, 2, good.list.data(), 3, good.values.data(), 2, 0, 8) == FX_E_ARG);
    CHECK(fxb_set_register_tracks_list(h, names, 2, nullptr, 3, good.values.data(), 2, 0, 8) == FX_E_ARG);
    CHECK(fxb_set_register_tracks_list(h, names, 2, good.list.data(), 3, nullptr, 2, 0, 8) == FX_E_ARG);
    CHECK(fxb_set_register_tracks_list(h, names, 2, good.list.data(), (int64_t)1 << 29, good.values.data(), 2, 0, 8) == FX_E_ARG);
    CHECK(fxb_set_register_tracks_list(h, names, 2, nullptr, 0, nullptr, 2, 0, 8) == 0);
    CHECK(fxb_set_register_tracks_list(h, names, 0, good.list.data(), 3, nullptr, 2, 0, 8) == 0);
    CHECK(fxb_set_register_tracks_list(nullptr, names, 2, good.list.data(), 3, good.values.data(), 2, 0, 8) == FX_E_ARG);
    block(h, N, 32);
    CHECK(fxstub_track_holds() == holds);
    // a voice named twice for one register; a dense track on the register, and the converse; the 65th schedule; a clear
    CHECK(arm(h, good) == 0);
    s = make({"gain"}, {good.list[2]}, 1, 1, 1); refused(s, FX_E_ARG);
    const float dense[2] = {0.5f, 0.25f};
    CHECK(fxb_set_register_track(h, "gain", dense, 2, 8, 0) == FX_E_ARG);
    CHECK(fxb_clear_register_tracks_list(h) == 0);
    CHECK(fxb_set_register_track(h, "gain", dense, 2, 8, 0) == 0);
    refused(good, FX_E_ARG);
    block(h, N, 32);
    CHECK(fxstub_track_holds() == holds);
    for (int i = 0; i < 64; ++i) CHECK(arm(h, make({"coef"}, {(int64_t)i}, i % 32, 1, 2)) == 0);
    refused(make({"coef"}, {(int64_t)100}, 0, 1, 1), FX_E_ARG);
    block(h, N, 32);
    CHECK(fxstub_track_holds() > holds);
    fxb_destroy(h);
}

void allocationFailures(int64_t N, int devices) {
    // every allocation of an arming call fails in turn (per shard: the pinned staging, the device staging, the track buffer), then
    // the call goes through
    for (int nth = 0; nth < 3 * devices + 1; ++nth) {
        fxb_handle* h = create(N, devices);
        CHECK(h && fxb_load_text(h, kText) == 1);
        if (!h) return;
        CHECK(fxb_prepare(h, 32, 1) == 0);
        block(h, N, 32);
        CHECK(fxb_prepare(h, 32, 1) == 0);
        const Schedule s = make({"coef", "gain"}, someOf(0, N, 130), 0, 8, 4);
        const long holds = fxstub_track_holds();
        fxstub_fail_mallocs(nth, 1);
        const int rc = arm(h, s);
        fxstub_fail_mallocs(-1, 0);
        if (nth < 3 * devices) {
            CHECK(rc == FX_E_MEMORY && fxb_last_error(h)[0] != 0);
            block(h, N, 32);
            CHECK(fxstub_track_holds() == holds);
            CHECK(arm(h, s) == 0);
        } else {
            CHECK(rc == 0);
        }
        block(h, N, 32);
        CHECK(fxstub_track_holds() == holds + devices);
        fxb_destroy(h);
    }
}

}  // namespace

int main() {
    setenv("FXSTUB_DEVICES", "3", 1);   // (read by the stand-in at its first call)
    shapes(200, 1, false);
    shapes(808, 3, false);
    refusals(200, 1);
    refusals(808, 3);
    allocationFailures(200, 1);
    allocationFailures(808, 3);
    // the tiers that cut the block (the knob is read when a handle is created)
    setenv("FX_KERNEL", "asm", 1);
    shapes(200, 1, true);
    shapes(808, 3, true);
    CHECK(fxstub_track_strays() == 0 && fxstub_reg_strays() == 0);
    CHECK(fxstub_live_allocations() == 0);
    if (g_failures) {
        std::fprintf(stderr, "%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("track list checks ok\n");
    return 0;
}
