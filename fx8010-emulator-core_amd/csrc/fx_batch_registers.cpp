// fx_batch_registers.cpp — the register calls by list of one batch: the (register, instance) words a host moves, scattered on the
// device, and the gather back (include/fx8010_amd.h "Register sets by list", fx_batch.hpp "Register calls by list", kernels:
// fx_registers.hip).
//
// A set runs inside the by-list frame (fx_batch.hpp "THE BY-LIST FRAME", fx_batch_list.cpp) without the lowering of the instance
// calls: the list, the caller's columns and the rows are staged, fx_reg_scatter is the kernel in front of evInst_.  The bookkeeping
// of setRegisterAt follows, per register, once the scatter is queued: a refusal or a failed launch has changed nothing the host knows.
//
// The program is NOT lowered here: the state rows exist from the load on and hold every register's value for every instance
// (setRegister's invariant), also for a register the code in force has folded in.  The first per-instance write to such a register
// asks for other code (forcedLane_, lowDirty_: the next block lowers again, as after setRegisterAt); later sets are plain scatters.
#include "fx_batch.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

int Batch::resolveRegisters(const char* const* keys, int nKeys, std::vector<int>* regs) {
    regs->assign((size_t)std::max(nKeys, 0), -1);
    for (int k = 0; k < nKeys; ++k) {
        const int r = keys[k] ? prog_.findRegister(keys[k]) : -1;
        if (r < 0) return fail(1, std::string("registers by list: no register named '") + (keys[k] ? keys[k] : "(null)") + "'");
        (*regs)[(size_t)k] = r;
    }
    return 0;
}

int Batch::checkRegisterList(const char* what, const std::vector<int>& regs, const int64_t* list, int64_t count, int64_t n, const void* values, bool unique, std::string* why) {
    const std::string name(what);
    if (count < 0) { *why = name + ": count < 0"; return FX_E_ARG; }
    if (count == 0 || regs.empty()) return 0;
    if (!list || !values) { *why = name + ": a null list or null values"; return FX_E_ARG; }
    if ((int64_t)regs.size() * count >= ((int64_t)1 << 31) || count >= ((int64_t)1 << 31)) { *why = name + ": n_keys * count must stay below 2^31"; return FX_E_ARG; }
    // (the order of the refusals: an entry outside the batch, a register twice, an instance twice)
    const ListFault f = checkList(list, count, n, unique);
    if (f.kind == ListFault::kOutside) { *why = listOutside(name, f, n); return FX_E_ARG; }
    if (!unique) return 0;
    std::vector<int> sortedRegs(regs);
    std::sort(sortedRegs.begin(), sortedRegs.end());
    if (std::adjacent_find(sortedRegs.begin(), sortedRegs.end()) != sortedRegs.end()) { *why = name + ": two keys name the same register"; return FX_E_ARG; }
    if (f) { *why = name + ": instance " + std::to_string(list[f.entry]) + " is listed more than once"; return FX_E_ARG; }
    return 0;
}

int Batch::reserveRegisterList(int nKeys, int64_t count) {
    (void)hipSetDevice(device_);
    if (nKeys < 1 || count < 1) return 0;
    static const char* const kTexts[3] = {"register list event", "hipMalloc register list staging", "pinned staging of the register list"};
    return reserveListStage(regList_, hRegList_, regListWords(nKeys, count), evInst_, instLaunched_, true, kTexts);
}

// the list and the rows into the pinned staging, the device pointers of all three parts into *a (the values are the caller's to fill)
int Batch::stageRegisterList(const std::vector<int>& regs, const int64_t* list, int64_t count, RegListArgs* a) {
    const size_t k = (size_t)count, nk = regs.size(), words = regListWords((int)nk, count);
    if (words > regList_.cap || words > hRegList_.cap || !evInst_) return fail(FX_E_ARG, "registers by list: no staging reserved (reserveRegisterList)");
    if (const int rc = waitPreviousInstCall("registers by list: waiting for the previous call")) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == 4, "register list staging");
    std::memcpy(hRegList_.p, list, k * 8);
    std::memcpy(hRegList_.p + k * 2 + nk * k, regs.data(), nk * 4);   // (a register's row is its number: StateLayout)
    *a = RegListArgs{};
    a->state = dState_;
    a->list = reinterpret_cast<const long long*>(regList_.p);   // (hipMalloc aligns the block: the 64-bit part comes first)
    a->values = regList_.p + k * 2;
    a->rows = reinterpret_cast<const int*>(regList_.p + k * 2 + nk * k);
    a->count = count;
    a->n = n_;
    a->nPad = nPad_;
    a->nKeys = (int)nk;
    a->stateRows = stateRows_;
    return 0;
}

int Batch::setRegistersList(const std::vector<int>& regs, const int64_t* list, const int64_t* pos, int64_t count, int64_t total, const float* values) {
    (void)hipSetDevice(device_);
    if (!dState_) return fail(FX_E_NOTREADY, "no program loaded");
    if (count == 0 || regs.empty()) return 0;
    RegListArgs a;
    const int rc = stageRegisterList(regs, list, count, &a);
    if (rc != 0) return rc;
    const size_t k = (size_t)count, nk = regs.size(), words = regListWords((int)nk, count);
    uint32_t* stage = hRegList_.p + k * 2;
    for (size_t j = 0; j < nk; ++j) copyColumn(&stage[j * k], values + j * (size_t)total, pos, k, 4, false);
    hipError_t e = hipMemcpyAsync(regList_.p, hRegList_.p, words * 4, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = orderBehindQueuedBlocks();
    if (e == hipSuccess) e = launchRegScatter(a, stream_);
    if (const int failed = closeInstCall(e, "registers by list: queueing the scatter")) return failed;
    ++regListSets_;
    noteRegistersWritten(regs);   // once the scatter is queued: a refusal or a failed launch has changed nothing the host knows
    return 0;
}

int Batch::getRegistersList(const std::vector<int>& regs, const int64_t* list, const int64_t* pos, int64_t count, int64_t total, float* values) {
    (void)hipSetDevice(device_);
    if (count == 0 || regs.empty()) return 0;
    // as getRegisterAt: a register without a row that counts is what the host holds
    std::vector<int> resident;
    std::vector<size_t> keyOf;
    for (size_t j = 0; j < regs.size(); ++j)
        if (dState_ && laneResident(regs[j])) {
            resident.push_back(regs[j]);
            keyOf.push_back(j);
        }
    int rc = resident.empty() ? 0 : reserveRegisterList((int)resident.size(), count);
    if (rc != 0) return rc;   // (nothing written)
    for (size_t j = 0; j < regs.size(); ++j)
        if (!(dState_ && laneResident(regs[j])))
            for (int64_t i = 0; i < count; ++i) values[j * (size_t)total + (size_t)(pos ? pos[i] : i)] = hostValue_[(size_t)regs[j]];
    if (resident.empty()) return 0;
    waitLastLaunch();
    RegListArgs a;
    if ((rc = stageRegisterList(resident, list, count, &a)) != 0) return rc;
    const size_t k = (size_t)count, nk = resident.size();
    // (the list and the rows: the two ends of the staging, around the values the gather writes)
    hipError_t e = hipMemcpyAsync(regList_.p, hRegList_.p, k * 8, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = hipMemcpyAsync(regList_.p + k * 2 + nk * k, hRegList_.p + k * 2 + nk * k, nk * 4, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = launchRegGather(a, stream_);
    if (e == hipSuccess) {
        ++regListGets_;
        e = hipMemcpyAsync(hRegList_.p + k * 2, regList_.p + k * 2, nk * k * 4, hipMemcpyDeviceToHost, stream_);
    }
    const hipError_t se = hipStreamSynchronize(stream_);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hipFail(e, "registers by list: the gather");
    const uint32_t* stage = hRegList_.p + k * 2;
    for (size_t j = 0; j < nk; ++j) copyColumn(values + keyOf[j] * (size_t)total, &stage[j * k], pos, k, 4, true);
    return 0;
}

}  // namespace fx
