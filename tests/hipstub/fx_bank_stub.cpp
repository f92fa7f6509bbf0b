// fx_bank_stub.cpp — host stand-ins for the launch functions of csrc/fx_bank.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).  They do
// the real moves, in stream order, on the stand-in's "device" memory, word by word as 32-bit patterns.  The addressing is written
// out on its own here, from the RECORD's side as in fx_instances_rot_stub.cpp (the kernels walk the destination's words): state
// row w of instance i is state[w][i]; slot s of a delay line is at [i / cols][s][i % cols]; record word w of bank slot b is
// bank[b * W + w]; the record's slot j of a ring of Z slots lands in slot (j + d) mod Z.  The rule of the rotations is written out
// again as well, with the distances taken the other way round (the position the record would have to stand at).  An instance
// outside the batch, a slot outside the bank or a pair outside the ring counts as a stray: the runtime never sends one.
#include <atomic>
#include <cstring>
#include <functional>

#include "../../fx8010-emulator-core_amd/csrc/fx_bank.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp

namespace {
std::atomic<long> g_gathers{0}, g_rotations{0}, g_scatters{0}, g_gated{0}, g_strays{0};

bool bad(const fx::BankArgs& b) {
    const fx::InstArgs& a = b.base;
    if (!a.state || !a.list || !b.bank || !b.slots || b.nSlots < 1 || b.nSlots >= ((long long)1 << 31)) return true;
    if (a.count < 1 || a.count >= ((long long)1 << 31) || a.n < 1 || a.nPad < a.n) return true;
    if (a.stateRows < 1 || a.iSlots < 0 || a.xSlots < 0 || (a.iSlots > 0 && !a.itram) || (a.xSlots > 0 && !a.xtram)) return true;
    if (a.cols != 64 && a.cols != 128 && a.cols != 256) return true;
    return a.skipLo < 0 || a.skipHi < a.skipLo || a.skipHi > a.stateRows;
}
bool badRot(const fx::BankRotArgs& r) {
    if (bad(r.bank)) return true;
    if (!r.pairs) return false;
    return !r.cells || r.cursorBase < 0 || r.cursorBase + 4 > r.bank.base.stateRows;
}
uint32_t* column(uint32_t* tram, long long inst, int cols, int slots) { return tram + (inst / cols) * (long long)slots * cols + inst % cols; }
// the record of entry k, or null
uint32_t* recordOf(const fx::BankArgs& b, long long k) {
    const long long slot = b.slots[k] & 0xffffffffll, inst = b.base.list[k];
    if (slot >= b.nSlots || inst < 0 || inst >= b.base.n) { g_strays.fetch_add(1); return nullptr; }
    return b.bank + slot * fx::instanceWords(b.base);
}
void putLine(uint32_t* tram, const uint32_t* rec, long long inst, int cols, int slots, int ring, int d) {
    if (d < 0 || (d != 0 && d >= ring)) { g_strays.fetch_add(1); d = 0; }
    for (int j = 0; j < slots; ++j) std::memcpy(column(tram, inst, cols, slots) + (long long)(j < ring ? (j + d) % ring : j) * cols, rec + j, 4);
}
}  // namespace

extern "C" long fxstub_bank_gathers(void) { return g_gathers.load(); }
extern "C" long fxstub_bank_rotations(void) { return g_rotations.load(); }
extern "C" long fxstub_bank_scatters(void) { return g_scatters.load(); }
extern "C" long fxstub_bank_gated(void) { return g_gated.load(); }
extern "C" long fxstub_bank_strays(void) { return g_strays.load(); }

namespace fx {

hipError_t launchBankGather(const BankArgs& args, hipStream_t stream) {
    if (bad(args)) return hipErrorInvalidValue;
    const BankArgs b = args;
    fxstubEnqueue(stream, [b] {
        const InstArgs& a = b.base;
        for (long long k = 0; k < a.count; ++k) {
            uint32_t* rec = recordOf(b, k);
            if (!rec) continue;
            const long long inst = a.list[k];
            for (int w = 0; w < a.stateRows; ++w) std::memcpy(rec + w, a.state + (long long)w * a.nPad + inst, 4);
            for (int j = 0; j < a.iSlots; ++j) std::memcpy(rec + a.stateRows + j, column(a.itram, inst, a.cols, a.iSlots) + (long long)j * a.cols, 4);
            for (int j = 0; j < a.xSlots; ++j) std::memcpy(rec + a.stateRows + a.iSlots + j, column(a.xtram, inst, a.cols, a.xSlots) + (long long)j * a.cols, 4);
        }
        g_gathers.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

hipError_t launchBankRotations(const BankRotArgs& args, hipStream_t stream) {
    if (badRot(args) || !args.pairs) return hipErrorInvalidValue;
    const BankRotArgs r = args;
    fxstubEnqueue(stream, [r] {
        const InstArgs& a = r.bank.base;
        for (long long k = 0; k < a.count; ++k) {
            const uint32_t* rec = recordOf(r.bank, k);
            for (int which = 0; which < 2; ++which) {
                const BankLine& l = r.line[which];
                int d = 0, fault = 0;
                if (rec && l.slots > 0 && l.size > 0) {
                    const uint32_t Z = (uint32_t)l.size;
                    const uint32_t* pos = rec + r.cursorBase + 2 * which;
                    bool have = false;
                    for (int kind = 0; kind < (r.dane ? 1 : 2); ++kind) {
                        if (pos[kind] >= Z) { fault = kBankBadPosition; break; }
                        if (!r.dane && !(kind ? l.reads : l.writes)) continue;
                        const uint32_t t = a.state[(long long)(r.cursorBase + 2 * which + kind) * a.nPad + a.list[k]];
                        // the smallest step that takes the record's position to the destination's
                        uint32_t step = 0;
                        while ((pos[kind] + step) % Z != t % Z) ++step;
                        if (have && (int)step != d) { fault = kBankPhase; break; }
                        d = (int)step;
                        have = true;
                    }
                    if (!fault && d != 0 && !l.ring) fault = kBankNoRing;
                    if (fault) d = 0;
                }
                r.pairs[2 * k + which] = d;
                if (fault) {
                    const unsigned long long key = ((unsigned long long)r.bank.slots[k] >> 32) << 3 | (unsigned long long)which << 2 | (unsigned long long)fault;
                    r.cells[kBankCellFaults] += 1;
                    if (~key > r.cells[kBankCellLowest]) r.cells[kBankCellLowest] = ~key;
                }
            }
        }
        g_rotations.fetch_add(1);
    });
    return hipGetLastError();
}

hipError_t launchBankScatterRot(const BankRotArgs& args, hipStream_t stream) {
    if (badRot(args)) return hipErrorInvalidValue;
    const BankRotArgs r = args;
    fxstubEnqueue(stream, [r] {
        const InstArgs& a = r.bank.base;
        g_scatters.fetch_add(1);
        if (r.pairs && r.cells[kBankCellFaults] != 0) {
            r.cells[kBankCellRefused] += 1;
            r.cells[kBankCellLastKey] = ~r.cells[kBankCellLowest];
            r.cells[kBankCellLastCall] = (unsigned long long)r.serial;
            g_gated.fetch_add(1);
            return;
        }
        for (long long k = 0; k < a.count; ++k) {
            const uint32_t* rec = recordOf(r.bank, k);
            if (!rec) continue;
            const long long inst = a.list[k];
            for (int w = 0; w < a.stateRows; ++w)
                if (w < a.skipLo || w >= a.skipHi) std::memcpy(a.state + (long long)w * a.nPad + inst, rec + w, 4);
            if (a.iSlots > 0) putLine(a.itram, rec + a.stateRows, inst, a.cols, a.iSlots, r.line[0].ring ? a.iSlots : 0, r.pairs ? r.pairs[2 * k] : 0);
            if (a.xSlots > 0) putLine(a.xtram, rec + a.stateRows + a.iSlots, inst, a.cols, a.xSlots, r.line[1].ring ? a.xSlots : 0, r.pairs ? r.pairs[2 * k + 1] : 0);
        }
    });
    return hipGetLastError();
}

}  // namespace fx
