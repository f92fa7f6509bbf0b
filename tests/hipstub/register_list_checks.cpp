// register_list_checks.cpp — the register calls by list of libfx8010_amd.so driven without a GPU under AddressSanitizer + UBSan +
// LeakSanitizer (TEST INFRASTRUCTURE: csrc/Makefile `stubasanreglist` links this file with the library's host sources and
// tests/hipstub/; a program of its own, so the sanitizer runtime is linked in and nothing has to be preloaded).
//
// The bookkeeping is pinned by tests/test_register_list_stub.py; this program is about addresses.  Every array the caller hands
// in is a heap block of exactly the documented size - [n_keys] names, [count] instances, [n_keys][count] values - and every
// "device" block of the stand-in is a heap block too, so a read or write one word outside the list, the values, the staging or the
// state rows is a report.  It walks lists of 1, 2, 63, 64, 65 and all entries, the first and the last instance always among them,
// with one key, two keys and every register, for N = 5, 65, 200 and 777 on one handle and N = 808 on three shards, a block in
// front of and behind every set; the refusals (nothing changes); and allocation failures at every allocation of a call.  The
// values are checked against a host model of the rows by the two definitions of include/fx8010_amd.h "Register sets by list":
// get_registers_list, and fxb_get_register_i word by word on the short lists.
// Exit code 0 = every check held (a sanitizer report turns it non-zero by itself).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/fx8010_amd.h"
#include "hip_stub.h"

extern "C" long fxstub_reg_scatters(void);   // fx_registers_stub.cpp
extern "C" long fxstub_reg_gathers(void);
extern "C" long fxstub_reg_strays(void);

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

uint32_t g_seed = 97531u;
uint32_t draw() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

// words of every kind: mostly plain values, and +-0, denormals, +-1e30 and a NaN with a payload
float word() {
    static const uint32_t kSpecial[8] = {0x00000000u, 0x80000000u, 0x00000001u, 0x807fffffu, 0x7149f2cau, 0xf149f2cau, 0x7fc12345u, 0xffa00001u};
    const uint32_t d = draw();
    float f = (float)((int)(d & 0xffff) - 32768) / 20000.0f;
    if ((d >> 16) % 5 == 0) std::memcpy(&f, &kSpecial[(d >> 19) & 7], 4);
    return f;
}

bool sameWord(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

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

fxb_handle* create(int64_t N, int ch, int devices) {
    const int three[3] = {0, 1, 2};
    return devices > 1 ? fxb_create_on_devices(N, ch, three, 3) : fxb_create(N, ch, 0);
}

// exactly-sized heap copies of the names: n pointers
struct Keys {
    std::vector<std::string> held;
    const char** table = nullptr;
    explicit Keys(const std::vector<std::string>& names) : held(names) {
        table = static_cast<const char**>(std::malloc(sizeof(char*) * std::max<size_t>(names.size(), 1)));
        for (size_t k = 0; k < held.size(); ++k) table[k] = held[k].c_str();
    }
    ~Keys() { std::free(table); }
    Keys(const Keys&) = delete;
    Keys& operator=(const Keys&) = delete;
    int n() const { return (int)held.size(); }
};

// a handle and what the rows of the registers the test writes must hold: rows[name][instance]
struct Model {
    fxb_handle* h = nullptr;
    int64_t n = 0;
    int ch = 1;
    std::map<std::string, std::vector<float>> rows;

    void follow(const std::string& name) {
        if (rows.count(name)) return;
        std::vector<float> row((size_t)n);
        CHECK(fxb_get_register_array(h, name.c_str(), row.data()) == 0);
        rows[name] = row;
    }
    bool set(const std::vector<std::string>& names, const std::vector<int64_t>& list) {
        Keys keys(names);
        for (const std::string& name : names) follow(name);
        std::vector<int64_t> given = list;
        std::vector<float> values(names.size() * list.size());
        for (float& v : values) v = word();
        std::vector<float> handed = values;
        if (fxb_set_registers_list(h, keys.table, keys.n(), given.data(), (int64_t)given.size(), handed.data()) != 0) return false;
        std::fill(given.begin(), given.end(), -5);   // the arrays are the caller's again on return
        std::fill(handed.begin(), handed.end(), 7.0f);
        for (size_t k = 0; k < names.size(); ++k)
            for (size_t i = 0; i < list.size(); ++i) rows[names[k]][(size_t)list[i]] = values[k * list.size() + i];
        return true;
    }
    // the two definitions of the get, for these keys at these instances
    bool same(const std::vector<std::string>& names, const std::vector<int64_t>& list) {
        Keys keys(names);
        std::vector<float> got(names.size() * list.size(), 9.0f);
        if (fxb_get_registers_list(h, keys.table, keys.n(), list.data(), (int64_t)list.size(), got.data()) != 0) return false;
        bool ok = true;
        for (size_t k = 0; k < names.size(); ++k)
            for (size_t i = 0; i < list.size(); ++i) {
                ok = ok && sameWord(got[k * list.size() + i], rows[names[k]][(size_t)list[i]]);
                if (list.size() <= 3) ok = ok && sameWord(got[k * list.size() + i], fxb_get_register_i(h, names[k].c_str(), list[i]));
            }
        return ok;
    }
    // the rows the program does not write, whole
    bool sameRows() {
        std::vector<float> row((size_t)n);
        for (const auto& kv : rows) {
            if (kv.first != "vol") continue;   // (the program writes the others in every block; the stand-in's kernel writes none)
            if (fxb_get_register_array(h, kv.first.c_str(), row.data()) != 0 || std::memcmp(row.data(), kv.second.data(), (size_t)n * 4) != 0) return false;
        }
        return true;
    }
    bool block(int S) {
        std::vector<float> in((size_t)S * (size_t)ch * (size_t)n, 0.25f), out(in.size(), 0.0f);
        return fxb_process_block(h, in.data(), out.data(), S) == 0;
    }
};

const std::vector<std::string>& everyRegister(int ch) {
    static const std::vector<std::string> mono{"in", "out", "vol", "a"}, stereo{"in", "in1", "out", "out1", "vol", "a"};
    return ch == 1 ? mono : stereo;
}

// one handle (devices == 1) or three shards through every indexing shape
void indexing(int devices) {
    const int64_t single[4] = {5, 65, 200, 777}, sharded[1] = {808};
    for (int which = 0; which < (devices > 1 ? 1 : 4); ++which)
        for (int ch = 1; ch <= 2; ++ch) {
            Model m;
            m.ch = ch;
            m.n = devices > 1 ? sharded[which] : single[which];
            m.h = create(m.n, ch, devices);
            CHECK(m.h != nullptr);
            if (!m.h) return;
            CHECK(fxb_load_text(m.h, ch == 1 ? kMono : kStereo) == 1);
            const std::vector<std::vector<std::string>> keySets{{"vol"}, {"a", "vol"}, everyRegister(ch)};
            const int64_t counts[6] = {1, 2, 63, 64, 65, m.n};
            int64_t sets = 0;
            const long strays = fxstub_reg_strays();
            for (const auto& names : keySets)
                for (int round = 0; round < 6; ++round) {
                    const int S = round % 3 == 0 ? 33 : round % 3;
                    const std::vector<int64_t> list = someOf(m.n, counts[round]);
                    CHECK(m.set(names, list));
                    CHECK(m.same(names, list));
                    CHECK(m.same(names, someOf(m.n, counts[(round + 1) % 6])));
                    CHECK(m.sameRows());
                    CHECK(m.block(S));
                    CHECK(m.same({"vol"}, list) && m.sameRows());
                    ++sets;
                }
            CHECK(fxb_info(m.h, FXB_INFO_REGISTER_LIST_SETS) >= sets && fxb_info(m.h, FXB_INFO_REGISTER_LIST_SETS) <= sets * devices);
            CHECK(fxb_info(m.h, FXB_INFO_REGISTER_LIST_GETS) >= 1);
            // repeats in a get; nothing listed
            const std::vector<int64_t> again{m.n - 1, 0, m.n - 1, m.n - 1};
            CHECK(m.same({"vol", "a", "vol"}, again));
            Keys one({"vol"});
            CHECK(fxb_set_registers_list(m.h, one.table, 1, nullptr, 0, nullptr) == 0 && fxb_get_registers_list(m.h, one.table, 1, nullptr, 0, nullptr) == 0);
            CHECK(fxb_set_registers_list(m.h, nullptr, 0, again.data(), 4, nullptr) == 0);
            CHECK(fxb_sync(m.h) == 0 && fxstub_reg_strays() == strays);
            fxb_destroy(m.h);
        }
}

void refusals(int devices) {
    Model m;
    m.ch = 2;
    m.n = 808;
    m.h = create(m.n, 2, devices);
    CHECK(m.h != nullptr);
    if (!m.h) return;
    const std::vector<int64_t> good{3, 0, 807};
    std::vector<float> values(6, 0.5f);
    Keys two({"vol", "a"}), same({"vol", "vol"}), unknown({"vol", "nosuch"});
    CHECK(fxb_set_registers_list(m.h, two.table, 2, good.data(), 3, values.data()) == FX_E_NOTREADY);   // no program
    CHECK(fxb_get_registers_list(m.h, two.table, 2, good.data(), 3, values.data()) == FX_E_NOTREADY);
    CHECK(fxb_load_text(m.h, kStereo) == 1);
    CHECK(m.set({"vol", "a"}, someOf(m.n, 65)) && m.block(8));
    const int64_t sets = fxb_info(m.h, FXB_INFO_REGISTER_LIST_SETS), gets = fxb_info(m.h, FXB_INFO_REGISTER_LIST_GETS);
    const long live = fxstub_live_allocations(), scatters = fxstub_reg_scatters(), gathers = fxstub_reg_gathers();
    const std::vector<int64_t> twice{5, 9, 5}, above{0, 808, 1}, below{0, 1, -1}, lone{0};
    CHECK(fxb_set_registers_list(m.h, two.table, 2, twice.data(), 3, values.data()) == FX_E_ARG);
    CHECK(fxb_set_registers_list(m.h, same.table, 2, good.data(), 3, values.data()) == FX_E_ARG);
    CHECK(fxb_set_registers_list(m.h, unknown.table, 2, good.data(), 3, values.data()) == 1 && std::strstr(fxb_last_error(m.h), "nosuch"));
    CHECK(fxb_get_registers_list(m.h, unknown.table, 2, good.data(), 3, values.data()) == 1 && std::strstr(fxb_last_error(m.h), "nosuch"));
    for (int get = 0; get <= 1; ++get) {
        auto call = [&](const char* const* keys, int nKeys, const int64_t* list, int64_t count, float* v) {
            return get ? fxb_get_registers_list(m.h, keys, nKeys, list, count, v) : fxb_set_registers_list(m.h, keys, nKeys, list, count, v);
        };
        CHECK(call(two.table, 2, above.data(), 3, values.data()) == FX_E_ARG);
        CHECK(call(two.table, 2, below.data(), 3, values.data()) == FX_E_ARG);
        CHECK(call(two.table, 2, good.data(), -1, values.data()) == FX_E_ARG);
        CHECK(call(two.table, -1, good.data(), 3, values.data()) == FX_E_ARG);
        CHECK(call(nullptr, 2, good.data(), 3, values.data()) == FX_E_ARG);
        CHECK(call(two.table, 2, nullptr, 3, values.data()) == FX_E_ARG);
        CHECK(call(two.table, 2, good.data(), 3, nullptr) == FX_E_ARG);
        CHECK(call(two.table, 2, lone.data(), (int64_t)1 << 30, values.data()) == FX_E_ARG);   // n_keys * count = 2^31: refused before the list is read
        CHECK(call(two.table, 1, lone.data(), (int64_t)1 << 31, values.data()) == FX_E_ARG);
        CHECK((get ? fxb_get_registers_list(nullptr, two.table, 2, good.data(), 3, values.data()) : fxb_set_registers_list(nullptr, two.table, 2, good.data(), 3, values.data())) == FX_E_ARG);
    }
    CHECK(fxstub_live_allocations() == live && fxstub_reg_scatters() == scatters && fxstub_reg_gathers() == gathers);
    CHECK(fxb_info(m.h, FXB_INFO_REGISTER_LIST_SETS) == sets && fxb_info(m.h, FXB_INFO_REGISTER_LIST_GETS) == gets);
    CHECK(std::all_of(values.begin(), values.end(), [](float v) { return v == 0.5f; }));
    CHECK(m.sameRows() && m.same({"vol"}, good));
    CHECK(fxb_get_registers_list(m.h, same.table, 2, twice.data(), 3, values.data()) == 0);   // repeats are a refusal of the set only
    CHECK(m.block(8) && m.sameRows());
    fxb_destroy(m.h);
}

// an allocation that fails inside a call, at every allocation it makes (the device staging and the pinned staging of every
// shard): FX_E_MEMORY, nothing has changed on any shard, and the same call goes through afterwards
void memory(int devices) {
    for (int get = 0; get <= 1; ++get)
        for (long nth = 0; nth < 2L * devices; ++nth) {
            Model m;
            m.ch = 2;
            m.n = 808;
            m.h = create(m.n, 2, devices);
            CHECK(m.h != nullptr);
            if (!m.h) return;
            CHECK(fxb_load_text(m.h, kStereo) == 1);
            const std::vector<int64_t> list = someOf(m.n, m.n / 2);   // (entries on every shard)
            // (per-instance rows, so that a get launches on every shard; the builder threads are idle while allocations fail)
            std::vector<float> ramp((size_t)m.n);
            for (size_t i = 0; i < ramp.size(); ++i) ramp[i] = (float)i / 1024.0f;
            CHECK(fxb_set_register_array(m.h, "vol", ramp.data()) == 0 && fxb_set_register_array(m.h, "a", ramp.data()) == 0);
            CHECK(fxb_prepare(m.h, 8, 1) == 0 && m.block(8) && fxb_prepare(m.h, 8, 1) == 0);
            m.follow("vol");
            Keys two({"vol", "a"});
            std::vector<float> values(2 * list.size(), 0.5f);
            fxstub_fail_mallocs(nth, 1);
            const int rc = get ? fxb_get_registers_list(m.h, two.table, 2, list.data(), (int64_t)list.size(), values.data())
                               : fxb_set_registers_list(m.h, two.table, 2, list.data(), (int64_t)list.size(), values.data());
            fxstub_fail_mallocs(-1, 0);
            CHECK(rc == FX_E_MEMORY);
            CHECK(fxb_info(m.h, FXB_INFO_REGISTER_LIST_SETS) == 0 && (devices > 1 || fxb_info(m.h, FXB_INFO_REGISTER_LIST_GETS) == 0));
            CHECK(m.sameRows());
            CHECK(m.set({"vol", "a"}, list) && m.same({"vol"}, list) && m.sameRows());
            CHECK(m.block(8));
            CHECK(m.set({"a", "vol"}, someOf(m.n, 65)));   // destroyed with a scatter queued
            fxb_destroy(m.h);
        }
}

// the one list check (Batch::checkList) at the edges of its two repeat paths: a list of two entries is looked up in a bitmap while
// the batch has at most 2048 instances (32 words <= 16 * 2) and in a sorted copy from 2049 on; the pair sits on the bit and word
// edges of the bitmap and, with three shards, in the last one.  Both paths name entry 1, and of several repeats the first in list
// order; the entries outside the batch are the first and the last of the list.
void repeatPaths(int devices) {
    for (const int64_t n : {(int64_t)2048, (int64_t)2049}) {
        Model m;
        m.n = n;
        m.h = create(n, 1, devices);
        CHECK(m.h != nullptr);
        if (!m.h) return;
        CHECK(fxb_load_text(m.h, kMono) == 1);
        CHECK(m.set({"vol"}, someOf(n, 65)) && fxb_sync(m.h) == 0);
        const int64_t sets = fxb_info(m.h, FXB_INFO_REGISTER_LIST_SETS);
        const long scatters = fxstub_reg_scatters();
        Keys one({"vol"});
        std::vector<float> values(4, 0.5f);
        for (const int64_t a : {(int64_t)0, (int64_t)63, (int64_t)64, n - 64, n - 1}) {
            const std::vector<int64_t> pair{a, a};
            CHECK(fxb_set_registers_list(m.h, one.table, 1, pair.data(), 2, values.data()) == FX_E_ARG);
            CHECK(std::strstr(fxb_last_error(m.h), ("instance " + std::to_string(a) + " is listed more than once").c_str()));
            CHECK(fxb_get_registers_list(m.h, one.table, 1, pair.data(), 2, values.data()) == 0 && sameWord(values[0], values[1]));
            CHECK(sameWord(values[0], m.rows["vol"][(size_t)a]));
        }
        // (four entries: a bitmap on both handles; the sorted copy of two entries is covered above)
        const std::vector<int64_t> several{5, 9, 9, 5};
        CHECK(fxb_set_registers_list(m.h, one.table, 1, several.data(), 4, values.data()) == FX_E_ARG);
        CHECK(std::strstr(fxb_last_error(m.h), "instance 9 is listed more than once"));
        for (const int64_t bad : {(int64_t)-1, n})
            for (int at = 0; at <= 1; ++at) {
                const std::vector<int64_t> list{at == 0 ? bad : 0, at == 1 ? bad : 1};
                for (int get = 0; get <= 1; ++get) {
                    const int rc = get ? fxb_get_registers_list(m.h, one.table, 1, list.data(), 2, values.data()) : fxb_set_registers_list(m.h, one.table, 1, list.data(), 2, values.data());
                    CHECK(rc == FX_E_ARG && std::strstr(fxb_last_error(m.h), ("entry " + std::to_string(at) + " of the list is outside 0.." + std::to_string(n - 1)).c_str()));
                }
            }
        CHECK(fxb_info(m.h, FXB_INFO_REGISTER_LIST_SETS) == sets && fxstub_reg_scatters() == scatters && m.sameRows());
        fxb_destroy(m.h);
    }
}

}  // namespace

int main() {
    setenv("FXSTUB_DEVICES", "3", 1);   // (read by the stand-in at its first call)
    for (int devices = 1; devices <= 3; devices += 2) {
        indexing(devices);
        refusals(devices);
        repeatPaths(devices);
        memory(devices);
        std::printf("  register lists, %d device(s): %d failed check(s) so far\n", devices, g_failures);
    }
    CHECK(fxstub_reg_strays() == 0);
    CHECK(fxstub_cross_device_errors() == 0);
    CHECK(fxstub_bad_pcm_launches() == 0);
    if (g_failures) {
        std::fprintf(stderr, "register list checks: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("register list checks ok\n");
    return 0;
}
