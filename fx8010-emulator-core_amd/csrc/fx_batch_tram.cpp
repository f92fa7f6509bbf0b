// fx_batch_tram.cpp — the delay-line windows by list of one batch: windows of one delay line of the instances a host names,
// scattered on the device, and the gather back (include/fx8010_amd.h "Delay-line windows by list", fx_batch.hpp "Delay-line
// windows by list", kernels: fx_tram.hip).
//
// A set runs inside the by-list frame (fx_batch.hpp "THE BY-LIST FRAME", fx_batch_list.cpp), once per piece: the list and the
// caller's windows are staged, fx_tram_scatter is the kernel in front of evInst_.
//
// Unlike a register set it lowers the program first (reserveTramList): the delay memory and its size come from the lowering.
// Where a ring stands is NOT looked up here: in logical mode the kernel reads each instance's position word itself, behind the
// queued blocks.  The position rows are current behind a block on every tier and launch path - the translated tier keeps the
// positions in SGPRs during a block and spills them at its end (the rotated load of records already relies on it).  There is no
// host mirror of delay memory, so a set has no bookkeeping: no code is generated again and nothing else changes.
//
// The staging is a block of this file's own under the record scratch's discipline: at most kInstScratchBytes of windows, grown
// on demand and kept; a call whose windows exceed it runs in pieces along the list, each of which first waits for the one before.
#include "fx_batch.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

int Batch::checkTramList(bool set, int which, const int64_t* list, int64_t count, int64_t n, int first, int nWords, const void* values, unsigned flags, std::string* why) {
    const std::string name(set ? "set_tram_list" : "get_tram_list");
    if (which < 0 || which > 1) { *why = name + ": which must be 0 (iTRAM) or 1 (xTRAM)"; return FX_E_ARG; }
    if (flags & ~(unsigned)(FXB_TRAM_LOGICAL | FXB_TRAM_BROADCAST)) { *why = name + ": flags has an unknown bit"; return FX_E_ARG; }
    if (!set && (flags & FXB_TRAM_BROADCAST)) { *why = name + ": flags: FXB_TRAM_BROADCAST is for the set only"; return FX_E_ARG; }
    if (count < 0) { *why = name + ": count < 0"; return FX_E_ARG; }
    if (count >= ((int64_t)1 << 31)) { *why = name + ": count must stay below 2^31"; return FX_E_ARG; }
    if (first < 0) { *why = name + ": first < 0"; return FX_E_ARG; }
    if (nWords < 0 || ((flags & FXB_TRAM_LOGICAL) && nWords < 1)) { *why = name + ": n_words must be at least " + ((flags & FXB_TRAM_LOGICAL) ? "1" : "0"); return FX_E_ARG; }
    if (count == 0) return 0;
    // n_words == 0 moves nothing, and null pointers are fine then - but a list that is there is checked like any other: the
    // header returns 0 "once the other arguments have been checked" (a sequence of tools/fuzz_voices.py found such a call accepted
    // with an instance of N, and with an instance listed twice)
    if (nWords == 0 && !list) return 0;
    if (!list) { *why = name + ": a null list"; return FX_E_ARG; }
    if (nWords > 0 && !values) { *why = name + ": null values"; return FX_E_ARG; }
    const ListFault f = checkList(list, count, n, set);
    if (f.kind == ListFault::kOutside) { *why = listOutside(name, f, n); return FX_E_ARG; }
    if (f) { *why = name + ": entry " + std::to_string(f.entry) + " of the list names instance " + std::to_string(list[f.entry]) + " a second time"; return FX_E_ARG; }
    return 0;
}

int Batch::reserveTramList(bool set, int which, int64_t count, int first, int nWords, unsigned flags) {
    (void)hipSetDevice(device_);
    const std::string name(set ? "set_tram_list" : "get_tram_list");
    if (!dState_) return fail(FX_E_NOTREADY, "no program loaded");
    int rc = ensureLowered();
    if (rc != 0) return rc;
    const RingLine l = ringLine(which);
    const char* line = which ? "xTRAM" : "iTRAM";
    if (flags & FXB_TRAM_LOGICAL) {
        if (l.slots < 1 || l.size < 1) return fail(FX_E_ARG, name + ": flags: FXB_TRAM_LOGICAL on " + line + ", which the program does not have");
        if (!l.ring()) return fail(FX_E_ARG, name + ": flags: FXB_TRAM_LOGICAL on " + line + ", which is no ring (FXB_INFO_INSTANCE_RINGS)");
        if (first >= l.size) return fail(FX_E_ARG, name + ": first must lie in 0.." + std::to_string(l.size - 1) + " (the size of " + line + ")");
        if (nWords > l.size) return fail(FX_E_ARG, name + ": n_words must lie in 1.." + std::to_string(l.size) + " (the size of " + line + ")");
    } else if ((int64_t)first + nWords > l.slots) {
        return fail(FX_E_ARG, name + ": first + n_words passes the " + std::to_string(l.slots) + " allocated slots of " + line);
    }
    if (count < 1 || nWords < 1) return 0;
    const int64_t entries = std::min(count, tramEntriesPerPiece(nWords));
    const size_t words = (size_t)entries * 2 + ((flags & FXB_TRAM_BROADCAST) ? (size_t)nWords : (size_t)entries * (size_t)nWords);
    static const char* const kTexts[3] = {"tram list event", "hipMalloc tram list staging", "pinned staging of the tram list"};
    return reserveListStage(tramStage_, hTramStage_, words, evInst_, instLaunched_, true, kTexts);
}

int Batch::tramList(int which, const int64_t* list, const int64_t* pos, int64_t count, int first, int nWords, const float* in, float* out, unsigned flags) {
    (void)hipSetDevice(device_);
    if (!dState_) return fail(FX_E_NOTREADY, "no program loaded");
    if (count == 0 || nWords == 0) return 0;
    const bool set = in != nullptr, broadcast = (flags & FXB_TRAM_BROADCAST) != 0, logical = (flags & FXB_TRAM_LOGICAL) != 0;
    const RingLine l = ringLine(which);
    const int64_t per = tramEntriesPerPiece(nWords);
    const size_t nw = (size_t)nWords;
    {
        const size_t entries = (size_t)std::min(count, per), words = entries * 2 + (broadcast ? nw : entries * nw);
        if (words > tramStage_.cap || words > hTramStage_.cap || !evInst_ || l.slots < 1) return fail(FX_E_ARG, "tram list: no staging reserved (reserveTramList)");
    }
    TramListArgs a{};
    a.line = reinterpret_cast<uint32_t*>(which ? dXTram_ : dITram_);
    a.state = dState_;
    a.n = n_;
    a.nPad = nPad_;
    a.slots = l.slots;
    a.cols = 64 * instPerLane_;
    a.posRow = stateLayout_.cursorBase + 2 * which;
    a.ringSize = logical ? l.size : 0;
    a.dane = c_.low.tramDane ? 1 : 0;
    a.first = first;
    a.nWords = nWords;
    a.valueStride = broadcast ? 0 : (long long)nWords;
    static_assert(sizeof(long long) == sizeof(int64_t), "tram list staging");
    if (!set) waitLastLaunch();
    for (int64_t off = 0; off < count; off += per) {
        const size_t k = (size_t)std::min(per, count - off), valueWords = broadcast ? nw : k * nw;
        if (const int rc = waitPreviousInstCall("tram list: waiting for the previous call")) return rc;
        std::memcpy(hTramStage_.p, list + off, k * 8);
        uint32_t* stage = hTramStage_.p + k * 2;
        a.list = reinterpret_cast<const long long*>(tramStage_.p);   // (hipMalloc aligns the block: the 64-bit part comes first)
        a.values = tramStage_.p + k * 2;
        a.count = (long long)k;
        hipError_t e = hipSuccess;
        if (set) {
            // (a window is one element of the column: the windows of this piece begin at entry `off`)
            if (broadcast) std::memcpy(stage, in, nw * 4);
            else copyColumn(stage, pos ? in : in + (size_t)off * nw, pos ? pos + off : nullptr, k, nw * 4, false);
            e = hipMemcpyAsync(tramStage_.p, hTramStage_.p, (k * 2 + valueWords) * 4, hipMemcpyHostToDevice, stream_);
            if (e == hipSuccess) e = orderBehindQueuedBlocks();
            if (e == hipSuccess) e = launchTramScatter(a, stream_);
            if (const int failed = closeInstCall(e, "tram list: queueing the scatter")) return failed;
            ++tramListSets_;
        } else {
            e = hipMemcpyAsync(tramStage_.p, hTramStage_.p, k * 8, hipMemcpyHostToDevice, stream_);
            if (e == hipSuccess) e = launchTramGather(a, stream_);
            if (e == hipSuccess) {
                ++tramListGets_;
                e = hipMemcpyAsync(stage, tramStage_.p + k * 2, valueWords * 4, hipMemcpyDeviceToHost, stream_);
            }
            const hipError_t se = hipStreamSynchronize(stream_);
            if (e == hipSuccess) e = se;
            if (e != hipSuccess) return hipFail(e, "tram list: the gather");
            copyColumn(pos ? out : out + (size_t)off * nw, stage, pos ? pos + off : nullptr, k, nw * 4, true);
        }
    }
    return 0;
}

}  // namespace fx
