// fx_batch_bank.cpp — the record bank of one batch (fx_batch.hpp "Record bank", kernels: fx_bank.hip): instance records kept in
// device memory, stored from and recalled into listed instances without a copy to the host.
//
// store and recall run inside the by-list frame (fx_batch.hpp "THE BY-LIST FRAME", fx_batch_list.cpp) on the staging of the
// instance calls: the host waits for the previous list call only, copies the two 64-bit lists into the pinned block and queues the
// rest on the handle's stream behind every queued block - a gather into the slots, or the three steps of a recall: the gate's two
// cells zeroed, fx_bank_rotations, fx_bank_scatter_rot.  The bank is the source: no record scratch, no piece loop.  What
// fxb_load_instances_rotated refuses from the record (recordRotations), the device refuses here, all or nothing per call
// (fx_bank.hip "THE GATE"); bankStatus reads the kept cells behind the stream.  put and get are plain synchronous copies.
//
// THE REGISTER SHADOW.  promoteLoaded compares the words of an image with hostValue_; a record that never visits the host cannot
// be compared, so the host keeps per slot what it knows of every register that is neither tracked nor intrinsically per lane: a
// put knows every word, a store knows hostValue_'s bits for a register the host holds as one value at that moment (laneWritten_
// clear) and nothing otherwise, and a recall notes a register as written per instance unless every recalled slot is known to
// hold the bits the host holds now.
#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"
#include "fx_bank.hpp"
#include "fx_batch.hpp"

namespace fx {

namespace {
// how many of the `most` slots from p on are consecutive: one copy moves their records
int64_t slotRun(const int64_t* p, int64_t most) {
    int64_t run = 1;
    while (run < most && p[run] == p[run - 1] + 1) ++run;
    return run;
}
}  // namespace

int Batch::checkBankLists(const char* who, const int64_t* slots, const int64_t* list, int64_t count, int64_t nSlots, int64_t n, bool uniqueSlots, std::string* why) {
    const std::string name(who);
    if (count < 0) *why = name + ": a negative count";
    else if (nSlots < 1) *why = name + ": the handle has no bank (fxb_bank_create)";
    else if (count > 0 && (!slots || (n > 0 && !list))) *why = name + ": a null list";
    else if (count >= ((int64_t)1 << 31)) *why = name + ": more than 2^31 - 1 list entries";
    else {
        why->clear();
        // (n == 0: put and get have no instance list)
        ListFault f = checkList(slots, count, nSlots, uniqueSlots);
        if (f.kind == ListFault::kOutside) *why = listOutside(name + ", slots", f, nSlots);
        else if (f) *why = name + ": entry " + std::to_string(f.entry) + " repeats a slot";
        else if (n > 0 && (f = checkList(list, count, n, !uniqueSlots))) {
            if (f.kind == ListFault::kOutside) *why = listOutside(name + ", instances", f, n);
            else *why = name + ": entry " + std::to_string(f.entry) + " repeats a destination";
        }
    }
    return why->empty() ? 0 : FX_E_ARG;
}

int Batch::bankReserve(int64_t nSlots) {
    (void)hipSetDevice(device_);
    const int rc = ensureLowered();
    if (rc != 0) return rc;
    if (nSlots < 0 || nSlots >= ((int64_t)1 << 31)) return fail(FX_E_ARG, "bank_create: n_slots must be 0 .. 2^31 - 1");
    bankRelease();
    if (nSlots == 0) return 0;
    const size_t W = (size_t)stateRows_ + (size_t)iSlotsAlloc_ + (size_t)xSlotsAlloc_, bytes = (size_t)nSlots * W * 4;
    bankNewShadow_.assign((size_t)nSlots * (size_t)stateLayout_.nRegs, 0);   // (a zero-filled slot: every register is known to hold 0)
    hipError_t e = bankCells_ ? hipSuccess : hipMalloc(reinterpret_cast<void**>(&bankCells_), kBankCells * sizeof(unsigned long long));
    if (e != hipSuccess) { bankCells_ = nullptr; bankRelease(); return hipFail(e, "hipMalloc bank cells"); }
    if ((e = hipMalloc(reinterpret_cast<void**>(&bankNew_), bytes)) != hipSuccess) { bankNew_ = nullptr; bankRelease(); return hipFail(e, "hipMalloc bank"); }
    bankNewSlots_ = nSlots;
    // (on the handle's stream, and waited for: the cells are read by bankStatus, the slots by a get, with plain copies)
    e = hipMemsetAsync(bankNew_, 0, bytes, stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    if (e != hipSuccess) { bankRelease(); return hipFail(e, "bank_create: zero-filling the slots"); }
    return 0;
}

void Batch::bankRelease() {
    (void)hipSetDevice(device_);
    if (bankNew_) (void)hipFree(bankNew_);
    bankNew_ = nullptr;
    bankNewSlots_ = 0;
    std::vector<uint64_t>().swap(bankNewShadow_);
}

void Batch::bankTake() {
    freeBank();   // (waits for what is queued: a recall may still be reading the old slots)
    if (!bankNew_) return;
    bank_ = bankNew_;
    bankSlots_ = bankNewSlots_;
    bankWords_ = (int64_t)stateRows_ + iSlotsAlloc_ + xSlotsAlloc_;
    bankRegs_ = stateLayout_.nRegs;
    bankShadow_.swap(bankNewShadow_);
    bankNew_ = nullptr;
    bankRelease();
    // (the kept cells start at zero with every bank; nothing is queued: a synchronous set will do)
    (void)hipMemsetAsync(bankCells_, 0, kBankCells * sizeof(unsigned long long), stream_);
    (void)hipStreamSynchronize(stream_);
}

void Batch::freeBank() {
    if (!bank_) return;
    (void)hipSetDevice(device_);
    waitLastLaunch();
    if (stream_) (void)hipStreamSynchronize(stream_);
    (void)hipFree(bank_);
    bank_ = nullptr;
    bankSlots_ = bankWords_ = 0;
    bankRegs_ = 0;
    std::vector<uint64_t>().swap(bankShadow_);
}

int Batch::bankReady(const char* who) {
    (void)hipSetDevice(device_);
    const int rc = ensureLowered();
    if (rc != 0) return rc;
    if (!bank_) return fail(FX_E_ARG, std::string(who) + ": the handle has no bank (fxb_bank_create)");
    if (bankWords_ != (int64_t)stateRows_ + iSlotsAlloc_ + xSlotsAlloc_ || bankRegs_ != stateLayout_.nRegs)
        return fail(FX_E_ARG, std::string(who) + ": the record of an instance has changed its size since the bank was created");
    return 0;
}

int Batch::reserveBankCall(int64_t count) {
    (void)hipSetDevice(device_);
    if (count < 1) return 0;
    hipError_t e = hipSuccess;
    if (!evInst_ && (e = hipEventCreateWithFlags(&evInst_, hipEventDisableTiming)) != hipSuccess) { evInst_ = nullptr; return hipFail(e, "instance event"); }
    const size_t entries = (size_t)count;
    if (entries <= instList_.cap && entries <= hInstList_.cap && entries <= bankPairs_.cap) return 0;
    // (the previous list call may still be reading the blocks that go)
    int rc = waitPreviousInstCall("bank: waiting for the previous list call");
    if (rc == 0) rc = growBlock(hInstList_, entries, true, "pinned instance lists", 2 * sizeof(long long));
    if (rc == 0) rc = growBlock(instList_, entries, false, "hipMalloc instance lists", 2 * sizeof(long long));
    if (rc == 0) rc = growBlock(bankPairs_, entries, false, "hipMalloc bank rotation pairs", 2 * sizeof(int));
    return rc;
}

// check (this batch's part), stage, order: the lists are on their way on return, and the stream stands behind the queued blocks
int Batch::beginBankCall(const char* who, const int64_t* slots, const int64_t* list, const int64_t* pos, int64_t count) {
    int rc = bankReady(who);
    if (rc != 0) return rc;
    if (!slots || !list || count < 1 || count >= ((int64_t)1 << 31)) return fail(FX_E_ARG, std::string(who) + ": a null list");
    for (int64_t i = 0; i < count; ++i) {
        const int64_t at = pos ? pos[i] : i;
        if (list[i] < 0 || list[i] >= n_ || at < 0 || at >= ((int64_t)1 << 31) || slots[at] < 0 || slots[at] >= bankSlots_)
            return fail(FX_E_ARG, std::string(who) + ": an instance outside the batch or a slot outside the bank");
    }
    if ((rc = reserveBankCall(count)) != 0) return rc;
    if ((rc = waitPreviousInstCall("bank: waiting for the previous list call")) != 0) return rc;
    const size_t entries = (size_t)count;
    std::memcpy(hInstList_.p, list, entries * 8);
    long long* words = hInstList_.p + hInstList_.cap;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t at = pos ? pos[i] : i;
        words[i] = (long long)((uint64_t)slots[at] | (uint64_t)at << 32);
    }
    hipError_t e = hipMemcpyAsync(instList_.p, hInstList_.p, entries * 8, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = hipMemcpyAsync(instList_.p + instList_.cap, words, entries * 8, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = orderBehindQueuedBlocks();
    return e == hipSuccess ? 0 : closeInstCall(e, "bank: lists to the device");
}

int Batch::bankStore(const int64_t* slots, const int64_t* list, const int64_t* pos, int64_t count) {
    if (count == 0) return 0;
    int rc = beginBankCall("bank_store", slots, list, pos, count);
    if (rc != 0) return rc;
    BankArgs b{};
    b.base = instArgs();
    b.base.list = instList_.p;
    b.base.count = count;
    b.bank = bank_;
    b.slots = instList_.p + instList_.cap;
    b.nSlots = bankSlots_;
    const hipError_t e = launchBankGather(b, stream_);
    if ((rc = closeInstCall(e, "launch fx_bank_gather")) != 0) return rc;
    ++bankStores_;
    for (int64_t i = 0; i < count; ++i) {
        uint64_t* row = bankShadow_.data() + (size_t)slots[pos ? pos[i] : i] * (size_t)bankRegs_;
        for (int r = 0; r < bankRegs_; ++r) row[r] = (shadowed(r) && !laneWritten_[(size_t)r]) ? (uint64_t)bitsOf(hostValue_[(size_t)r]) : kBankUnknown;
    }
    return 0;
}

int Batch::bankRecall(const int64_t* slots, const int64_t* list, const int64_t* pos, int64_t count, int64_t serial) {
    if (count == 0) return 0;
    int rc = beginBankCall("bank_recall", slots, list, pos, count);
    if (rc != 0) return rc;
    BankRotArgs r{};
    r.bank.base = instArgs();
    r.bank.base.list = instList_.p;
    r.bank.base.count = count;
    r.bank.bank = bank_;
    r.bank.slots = instList_.p + instList_.cap;
    r.bank.nSlots = bankSlots_;
    r.serial = serial;
    hipError_t e = hipSuccess;
    // (no delay-line instruction runs: the positions never move and nothing reads them - the plain scatter, position words included)
    if (c_.low.tramOpsPerSample > 0) {
        for (int which = 0; which < 2; ++which) {
            const RingLine l = ringLine(which);
            r.line[which] = BankLine{l.size, l.slots, l.ring() ? 1 : 0, l.writes ? 1 : 0, l.reads ? 1 : 0};
        }
        r.cursorBase = stateLayout_.cursorBase;
        r.dane = c_.low.tramDane ? 1 : 0;
        r.pairs = bankPairs_.p;
        r.cells = bankCells_;
        r.bank.base.skipLo = stateLayout_.cursorBase;
        r.bank.base.skipHi = stateLayout_.cursorBase + 4;
        e = hipMemsetAsync(bankCells_, 0, 2 * sizeof(unsigned long long), stream_);   // kBankCellFaults, kBankCellLowest
        if (e == hipSuccess) e = launchBankRotations(r, stream_);
    }
    if (e == hipSuccess) e = launchBankScatterRot(r, stream_);
    if ((rc = closeInstCall(e, "launch fx_bank_rotations / fx_bank_scatter_rot")) != 0) return rc;
    ++bankRecalls_;
    return 0;
}

void Batch::bankNoteRecalled(const int64_t* slots, int64_t count) {
    if (!bank_ || !slots) return;
    for (int r = 0; r < bankRegs_; ++r) {
        if (!shadowed(r)) continue;
        const uint64_t held = bitsOf(hostValue_[(size_t)r]);
        bool differs = false;
        for (int64_t k = 0; k < count && !differs; ++k) differs = slots[k] < 0 || slots[k] >= bankSlots_ || bankShadowRow(slots[k])[r] != held;
        if (differs) noteRegisterWritten(r);   // as if setRegisterAt had written it
    }
}

int Batch::bankPutRecords(const int64_t* slots, int64_t count, const uint32_t* records, const uint64_t* shadow) {
    if (count == 0) return 0;
    const int rc = bankReady("bank_put");
    if (rc != 0) return rc;
    std::string why;
    if (!records || checkBankLists("bank_put", slots, nullptr, count, bankSlots_, 0, true, &why) != 0) return fail(FX_E_ARG, why.empty() ? "bank_put: a null buffer" : why);
    waitLastLaunch();   // (a queued recall may still be reading the slots)
    const size_t W = (size_t)bankWords_;
    hipError_t e = hipSuccess;
    for (int64_t k = 0, run = 0; k < count && e == hipSuccess; k += run) {
        run = slotRun(slots + k, count - k);
        e = hipMemcpy(bank_ + (size_t)slots[k] * W, records + (size_t)k * W, (size_t)run * W * 4, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return hipFail(e, "bank_put: records to the device");
    for (int64_t k = 0; k < count; ++k) {
        uint64_t* row = bankShadow_.data() + (size_t)slots[k] * (size_t)bankRegs_;
        for (int r = 0; r < bankRegs_; ++r) row[r] = shadow ? shadow[(size_t)k * (size_t)bankRegs_ + (size_t)r] : (uint64_t)records[(size_t)k * W + (size_t)r];
    }
    return 0;
}

int Batch::bankGetRecords(const int64_t* slots, int64_t count, uint32_t* records) {
    if (count == 0) return 0;
    const int rc = bankReady("bank_get");
    if (rc != 0) return rc;
    std::string why;
    if (!records || checkBankLists("bank_get", slots, nullptr, count, bankSlots_, 0, false, &why) != 0) return fail(FX_E_ARG, why.empty() ? "bank_get: a null buffer" : why);
    waitLastLaunch();   // (a queued store may still be writing the slots)
    const size_t W = (size_t)bankWords_;
    hipError_t e = hipSuccess;
    for (int64_t k = 0, run = 0; k < count && e == hipSuccess; k += run) {
        run = slotRun(slots + k, count - k);
        e = hipMemcpy(records + (size_t)k * W, bank_ + (size_t)slots[k] * W, (size_t)run * W * 4, hipMemcpyDeviceToHost);
    }
    return e == hipSuccess ? 0 : hipFail(e, "bank_get: records to the host");
}

int Batch::bankStatus(uint64_t out[3], bool reset) {
    out[0] = out[1] = out[2] = 0;
    (void)hipSetDevice(device_);
    if (!bank_) return fail(FX_E_ARG, "bank_status: the handle has no bank (fxb_bank_create)");
    waitLastLaunch();
    unsigned long long cells[kBankCells];
    hipError_t e = hipMemcpy(cells, bankCells_, sizeof(cells), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hipFail(e, "bank_status: reading the cells");
    out[0] = cells[kBankCellRefused];
    out[1] = cells[kBankCellLastKey];
    out[2] = cells[kBankCellLastCall];
    if (reset && out[0] != 0) {
        std::memset(cells, 0, sizeof(cells));
        if ((e = hipMemcpy(bankCells_, cells, sizeof(cells), hipMemcpyHostToDevice)) != hipSuccess) return hipFail(e, "bank_status: zeroing the cells");
    }
    return 0;
}

}  // namespace fx
