// fx_batch_instances.cpp — the per-instance state calls of one batch: copy, reset, records to and from the host (fx_batch.hpp
// "Per-instance state calls", kernels: fx_instances.hip).
//
// Every call runs inside the by-list frame (fx_batch.hpp "THE BY-LIST FRAME", fx_batch_list.cpp).  beginInstanceCall lowers the
// program (the delay memory exists from then on), refuses instance numbers outside the batch, waits for the previous call, grows
// and fills the lists and orders the handle's stream behind the queued blocks.  The kernels then run on the handle's stream, in
// pieces of at most recordsPerPiece() records on the one record scratch - stream order alone keeps a piece's scatter in front of
// the next piece's gather.  endInstanceCall records evInst_ behind the last of them.  The rotated load (recordRotations,
// scatterRecordsRotated) has the frame of the load; its rotation pairs travel with the list, in the place of the second one.
#include "fx_batch.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

namespace {
// how many of the `most` positions from p on are consecutive: one copy moves their records
int64_t recordRun(const int64_t* p, int64_t most) {
    int64_t run = 1;
    while (run < most && p[run] == p[run - 1] + 1) ++run;
    return run;
}
}  // namespace

int Batch::checkInstanceLists(const int64_t* src, const int64_t* dst, int64_t count, int64_t n, const char** why) {
    *why = nullptr;
    if (count < 0) *why = "instances: a negative count";
    else if (count > 0 && !src && !dst) *why = "instances: a null list";
    else if (count >= ((int64_t)1 << 31)) *why = "instances: more than 2^31 - 1 list entries";
    if (*why) return FX_E_ARG;
    // (src may repeat; the order of the refusals: either list outside the batch, a destination twice, a destination as a source)
    const ListFault fs = src ? checkList(src, count, n, false) : ListFault{}, fd = dst ? checkList(dst, count, n, true) : ListFault{};
    if (fs || fd.kind == ListFault::kOutside) { *why = "instances: an instance number outside the batch"; return FX_E_ARG; }
    if (fd) { *why = "instances: a destination is listed twice"; return FX_E_ARG; }
    if (!dst || !src) return 0;
    std::vector<int64_t> sorted(dst, dst + count);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t k = 0; k < count; ++k)
        if (std::binary_search(sorted.begin(), sorted.end(), src[k])) { *why = "instances: a destination is also a source"; return FX_E_ARG; }
    return 0;
}

int Batch::instanceShape(SnapshotHeader* hdr, int64_t count) {
    const int rc = snapshotShape(hdr);
    if (rc != 0) return rc;
    hdr->magic = kInstanceMagic;
    hdr->n = count;
    return 0;
}

int Batch::checkInstanceImage(const SnapshotHeader& hdr, int64_t count, int64_t bytes) {
    SnapshotHeader mine;
    const int rc = instanceShape(&mine, count);
    if (rc != 0) return rc;
    // (every field is compared before any of them enters an address: the image may be a damaged file.  Equal to ours, the
    // counts are sane and count * W * 4 cannot overflow: count < 2^31, W < 2^22)
    if (hdr.magic != mine.magic || hdr.version != mine.version) return fail(FX_E_ARG, "instance image: not an instance image of this library version");
    if (hdr.n != count || count < 0 || count >= ((int64_t)1 << 31)) return fail(FX_E_ARG, "instance image: it holds another number of records than the list has entries");
    if (hdr.channels != mine.channels || hdr.nRegs != mine.nRegs || hdr.stateRows != mine.stateRows || hdr.iSlots != mine.iSlots || hdr.xSlots != mine.xSlots)
        return fail(FX_E_ARG, "instance image: the image is of another program (registers, channels or delay lines differ)");
    if (bytes < (int64_t)sizeof(SnapshotHeader) + count * instanceWords(mine) * 4) return fail(FX_E_ARG, "instance image: truncated");
    return 0;
}

InstArgs Batch::instArgs() const {
    InstArgs a{};
    a.state = dState_;
    a.itram = reinterpret_cast<uint32_t*>(dITram_);
    a.xtram = reinterpret_cast<uint32_t*>(dXTram_);
    a.n = n_;
    a.nPad = nPad_;
    a.stateRows = stateRows_;
    a.iSlots = iSlotsAlloc_;
    a.xSlots = xSlotsAlloc_;
    a.cols = 64 * instPerLane_;
    a.recStride = fx::instanceWords(a);
    return a;
}

int64_t Batch::recordsPerPiece() const {
    const size_t w = (size_t)stateRows_ + (size_t)iSlotsAlloc_ + (size_t)xSlotsAlloc_;
    return (int64_t)std::max<size_t>(kInstScratchBytes / (w * 4), 1);
}

int Batch::beginInstanceCall(const int64_t* a, const int64_t* b, int64_t count, size_t recordWords, const int32_t* pairs) {
    (void)hipSetDevice(device_);
    int rc = ensureLowered();
    if (rc != 0) return rc;
    const char* why = nullptr;
    if (checkInstanceLists(a, nullptr, count, n_, &why) != 0 || (b && checkInstanceLists(b, nullptr, count, n_, &why) != 0)) return fail(FX_E_ARG, why);
    if (!a || count < 1) return fail(FX_E_ARG, "instances: a null list");
    hipError_t e = hipSuccess;
    if (!evInst_ && (e = hipEventCreateWithFlags(&evInst_, hipEventDisableTiming)) != hipSuccess) { evInst_ = nullptr; return hipFail(e, "instance event"); }
    if ((rc = waitPreviousInstCall("waiting for the previous instance call")) != 0) return rc;
    const size_t entries = (size_t)count;
    // (two lists of `entries` each; the previous call, the only user of these blocks, has been waited for)
    if ((rc = growBlock(hInstList_, entries, true, "pinned instance lists", 2 * sizeof(long long))) != 0) return rc;
    if ((rc = growBlock(instList_, entries, false, "hipMalloc instance lists", 2 * sizeof(long long))) != 0) return rc;
    if ((rc = growBlock(instRec_, recordWords, false, "hipMalloc instance records")) != 0) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "instance lists");
    std::memcpy(hInstList_.p, a, entries * 8);
    static_assert(2 * sizeof(int32_t) == sizeof(long long), "a pair of rotations travels in the place of a list entry");
    const void* second = b ? static_cast<const void*>(b) : static_cast<const void*>(pairs);
    if (second) std::memcpy(hInstList_.p + hInstList_.cap, second, entries * 8);
    e = hipMemcpyAsync(instList_.p, hInstList_.p, entries * 8, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess && second) e = hipMemcpyAsync(instList_.p + instList_.cap, hInstList_.p + hInstList_.cap, entries * 8, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = orderBehindQueuedBlocks();
    if (e != hipSuccess) {
        (void)endInstanceCall(true);   // (the list copies may be on their way)
        return hipFail(e, "instances: lists to the device");
    }
    return 0;
}

// (closeInstCall with two differences that stay: the event is recorded behind a failed launch too - the pieces in front of it are
// queued - and a synchronous call waits for the stream and leaves nothing outstanding)
int Batch::endInstanceCall(bool wait) {
    hipError_t e = hipEventRecord(evInst_, stream_);
    if (e == hipSuccess) instLaunched_ = true;
    if (wait || e != hipSuccess) {
        const hipError_t se = hipStreamSynchronize(stream_);
        if (se == hipSuccess) instLaunched_ = false;
        if (e == hipSuccess) e = se;
    }
    return e == hipSuccess ? 0 : hipFail(e, "instances: end of the call");
}

int Batch::copyInstances(const int64_t* src, const int64_t* dst, int64_t count) {
    if (count == 0) return ensureLowered();
    if (!src || !dst) return fail(FX_E_ARG, "instances: a null list");
    int rc = ensureLowered();
    if (rc != 0) return rc;
    const int64_t per = recordsPerPiece();
    InstArgs a = instArgs();
    if ((rc = beginInstanceCall(src, dst, count, (size_t)std::min(count, per) * (size_t)a.recStride)) != 0) return rc;
    a.records = instRec_.p;
    hipError_t e = hipSuccess;
    for (int64_t off = 0; off < count && e == hipSuccess; off += per) {
        a.count = std::min(per, count - off);
        a.list = instList_.p + off;
        if ((e = launchInstGather(a, stream_)) != hipSuccess) break;
        ++instGathers_;
        a.list = instList_.p + instList_.cap + off;
        if ((e = launchInstScatter(a, stream_)) == hipSuccess) ++instScatters_;
    }
    rc = endInstanceCall(e != hipSuccess);
    return e != hipSuccess ? hipFail(e, "launch fx_inst_gather / fx_inst_scatter") : rc;
}

int Batch::resetInstances(const int64_t* list, int64_t count) {
    if (count == 0) return ensureLowered();
    int rc = ensureLowered();
    if (rc != 0) return rc;
    InstArgs a = instArgs();
    const size_t W = (size_t)a.recStride;
    if ((rc = beginInstanceCall(list, nullptr, count, W)) != 0) return rc;
    hipError_t e = hipSuccess;
    if ((rc = growBlock(hInstRec_, W, true, "pinned reset record")) != 0) {
        const std::string why = lastError_;
        (void)endInstanceCall(true);
        return fail(rc, why);
    }
    // the record of a freshly created instance (ensureState): registers as the last broadcast write left them, latches 0, the
    // reference's LFSR seeds, flags 0, counter 0, delay memory 0 - the four position words are skipped by the scatter
    std::memset(hInstRec_.p, 0, W * 4);
    for (int r = 0; r < stateLayout_.nRegs; ++r) hInstRec_.p[r] = bitsOf(hostValue_[(size_t)r]);
    hInstRec_.p[stateLayout_.noiseBase + 0] = 0x70f4f854u;   // g_x1, include/FX8010.h:290
    hInstRec_.p[stateLayout_.noiseBase + 1] = 0xe1e9f0a7u;   // g_x2, include/FX8010.h:291
    e = hipMemcpyAsync(instRec_.p, hInstRec_.p, W * 4, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) {
        a.records = instRec_.p;
        a.recStride = 0;
        a.list = instList_.p;
        a.count = count;
        a.skipLo = stateLayout_.cursorBase;
        a.skipHi = stateLayout_.cursorBase + 4;
        if ((e = launchInstScatter(a, stream_)) == hipSuccess) ++instScatters_;
    }
    rc = endInstanceCall(e != hipSuccess);
    return e != hipSuccess ? hipFail(e, "launch fx_inst_scatter") : rc;
}

int Batch::gatherRecords(const int64_t* list, const int64_t* pos, int64_t count, uint32_t* buf) {
    if (count == 0) return ensureLowered();
    if (!buf) return fail(FX_E_ARG, "instances: a null buffer");
    int rc = ensureLowered();
    if (rc != 0) return rc;
    const int64_t per = recordsPerPiece();
    InstArgs a = instArgs();
    const size_t W = (size_t)a.recStride;
    if ((rc = beginInstanceCall(list, nullptr, count, (size_t)std::min(count, per) * W)) != 0) return rc;
    a.records = instRec_.p;
    hipError_t e = hipSuccess;
    for (int64_t off = 0; off < count && e == hipSuccess; off += per) {
        a.count = std::min(per, count - off);
        a.list = instList_.p + off;
        if ((e = launchInstGather(a, stream_)) != hipSuccess) break;
        ++instGathers_;
        // one copy per piece, straight to where the records belong - with positions, one per run of consecutive positions
        for (int64_t k = 0, run = 0; k < a.count && e == hipSuccess; k += run) {
            run = pos ? recordRun(pos + off + k, a.count - k) : a.count;
            e = hipMemcpyAsync(buf + (size_t)(pos ? pos[off + k] : off + k) * W, instRec_.p + (size_t)k * W, (size_t)run * W * 4, hipMemcpyDeviceToHost, stream_);
        }
    }
    rc = endInstanceCall(true);
    return e != hipSuccess ? hipFail(e, "instances: records to the host") : rc;
}

int Batch::scatterRecords(const int64_t* list, const int64_t* pos, int64_t count, const uint32_t* buf) {
    if (count == 0) return ensureLowered();
    if (!buf) return fail(FX_E_ARG, "instances: a null buffer");
    int rc = ensureLowered();
    if (rc != 0) return rc;
    const int64_t per = recordsPerPiece();
    InstArgs a = instArgs();
    const size_t W = (size_t)a.recStride;
    if ((rc = beginInstanceCall(list, nullptr, count, (size_t)std::min(count, per) * W)) != 0) return rc;
    a.records = instRec_.p;
    hipError_t e = hipSuccess;
    for (int64_t off = 0; off < count && e == hipSuccess; off += per) {
        a.count = std::min(per, count - off);
        a.list = instList_.p + off;
        for (int64_t k = 0, run = 0; k < a.count && e == hipSuccess; k += run) {
            run = pos ? recordRun(pos + off + k, a.count - k) : a.count;
            e = hipMemcpyAsync(instRec_.p + (size_t)k * W, buf + (size_t)(pos ? pos[off + k] : off + k) * W, (size_t)run * W * 4, hipMemcpyHostToDevice, stream_);
        }
        if (e == hipSuccess && (e = launchInstScatter(a, stream_)) == hipSuccess) ++instScatters_;
    }
    rc = endInstanceCall(true);
    return e != hipSuccess ? hipFail(e, "instances: records to the device") : rc;
}

int Batch::checkRecordCursors(const int64_t* list, const int64_t* pos, int64_t count, const uint32_t* buf) {
    (void)hipSetDevice(device_);
    int rc = ensureLowered();
    if (rc != 0 || count == 0) return rc;
    const char* why = nullptr;
    if (!list || !buf || checkInstanceLists(list, nullptr, count, n_, &why) != 0) return fail(FX_E_ARG, why ? why : "instances: a null list or buffer");
    if (c_.low.tramOpsPerSample == 0) return 0;   // (no delay-line instruction runs: the positions never move and nothing reads them)
    waitLastLaunch();
    std::vector<uint32_t> cur((size_t)4 * (size_t)n_);
    const hipError_t e = hipMemcpy2D(cur.data(), (size_t)n_ * 4, dState_ + (size_t)stateLayout_.cursorBase * nPad_, (size_t)nPad_ * 4, (size_t)n_ * 4, 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hipFail(e, "instances: reading the delay-line positions");
    const size_t W = (size_t)stateRows_ + (size_t)iSlotsAlloc_ + (size_t)xSlotsAlloc_;
    for (int64_t k = 0; k < count; ++k) {
        const uint32_t* rec = buf + (size_t)(pos ? pos[k] : k) * W + (size_t)stateLayout_.cursorBase;
        for (int j = 0; j < 4; ++j)
            if (rec[j] != cur[(size_t)j * (size_t)n_ + (size_t)list[k]])
                return fail(FX_E_ARG, "load_instances: a record's delay-line positions differ from those of its destination (the handles have not run the same number of samples)");
    }
    return 0;
}

Batch::RingLine Batch::ringLine(int which) const {
    RingLine l;
    l.size = which ? std::min(prog_.xTramSize, kMaxXTram) : std::min(prog_.iTramSize, kMaxITram);
    l.slots = which ? xSlotsAlloc_ : iSlotsAlloc_;
    l.writes = tramWrites_[which];   // (found at the lowering, beside the slots: ensureTram)
    l.reads = tramReads_[which];
    return l;
}

int Batch::rotationApplies(bool* applies) {
    const int rc = ensureLowered();
    *applies = rc == 0 && c_.low.tramOpsPerSample > 0 && (iSlotsAlloc_ > 0 || xSlotsAlloc_ > 0);
    return rc;
}

int Batch::recordRotations(const int64_t* list, const int64_t* pos, int64_t count, const uint32_t* buf, std::vector<int32_t>* rot) {
    (void)hipSetDevice(device_);
    rot->clear();
    int rc = ensureLowered();
    if (rc != 0 || count == 0) return rc;
    const char* why = nullptr;
    if (!list || !buf || checkInstanceLists(list, nullptr, count, n_, &why) != 0) return fail(FX_E_ARG, why ? why : "instances: a null list or buffer");
    waitLastLaunch();
    std::vector<uint32_t> cur((size_t)4 * (size_t)n_);
    const hipError_t e = hipMemcpy2D(cur.data(), (size_t)n_ * 4, dState_ + (size_t)stateLayout_.cursorBase * nPad_, (size_t)nPad_ * 4, (size_t)n_ * 4, 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hipFail(e, "instances: reading the delay-line positions");
    const size_t W = (size_t)stateRows_ + (size_t)iSlotsAlloc_ + (size_t)xSlotsAlloc_;
    const bool dane = c_.low.tramDane;
    rot->assign((size_t)count * 2, 0);
    for (int which = 0; which < 2; ++which) {
        const RingLine l = ringLine(which);
        if (l.slots == 0 || l.size < 1) continue;   // (the program has no memory on this line: nothing to rotate, nothing reads the positions)
        const char* name = which ? "xTRAM" : "iTRAM";
        const int64_t Z = l.size;
        auto refuse = [&](int64_t k, const char* what) {
            rot->clear();
            return fail(FX_E_ARG, std::string("load_instances_rotated: ") + name + ", list entry " + std::to_string(pos ? pos[k] : k) + ": " + what);   // (the caller's entry: a shard's pos[k])
        };
        for (int64_t k = 0; k < count; ++k) {
            const uint32_t* rec = buf + (size_t)(pos ? pos[k] : k) * W + (size_t)stateLayout_.cursorBase + (size_t)which * 2;
            const uint32_t* dst = cur.data() + (size_t)which * 2 * (size_t)n_ + (size_t)list[k];
            // kind 0: the write position, kind 1: the read position (the DANE model has one counter, in the write word)
            int64_t d = -1;
            for (int kind = 0; kind < (dane ? 1 : 2); ++kind) {
                const int64_t s = rec[kind], t = dst[(size_t)kind * (size_t)n_];
                if (s >= Z) return refuse(k, "a position word of the record lies outside the line (0 .. size - 1)");
                if (!dane && !(kind ? l.reads : l.writes)) continue;   // (never moves: does not count)
                const int64_t dk = (((t - s) % Z) + Z) % Z;
                if (d >= 0 && dk != d)
                    return refuse(k, "the record's write and read positions are not at one distance from the destination's (another phase of a program whose reads and writes drift apart, or of a delay instruction in a SKIP shadow)");
                d = dk;
            }
            if (d < 0) d = 0;
            if (d != 0 && !l.ring())
                return refuse(k, "the record's delay-line positions differ from the destination's and the line is no ring (a delay write at an offset above 0): it cannot be rotated");
            (*rot)[(size_t)k * 2 + (size_t)which] = (int32_t)d;
        }
    }
    return 0;
}

int Batch::scatterRecordsRotated(const int64_t* list, const int64_t* pos, int64_t count, const uint32_t* buf, const int32_t* rot) {
    if (count == 0) return ensureLowered();
    if (!buf || !rot) return fail(FX_E_ARG, "instances: a null buffer");
    int rc = ensureLowered();
    if (rc != 0) return rc;
    const int64_t per = recordsPerPiece();
    InstRotArgs r{};
    InstArgs& a = r.base;
    a = instArgs();
    const size_t W = (size_t)a.recStride;
    // (lists, rotations and record scratch grow here, in front of the first launch)
    if ((rc = beginInstanceCall(list, nullptr, count, (size_t)std::min(count, per) * W, rot)) != 0) return rc;
    a.records = instRec_.p;
    a.skipLo = stateLayout_.cursorBase;
    a.skipHi = stateLayout_.cursorBase + 4;
    r.iSize = ringLine(0).ring() ? iSlotsAlloc_ : 0;
    r.xSize = ringLine(1).ring() ? xSlotsAlloc_ : 0;
    hipError_t e = hipSuccess;
    for (int64_t off = 0; off < count && e == hipSuccess; off += per) {
        a.count = std::min(per, count - off);
        a.list = instList_.p + off;
        r.rot = reinterpret_cast<const int*>(instList_.p + instList_.cap + off);   // (a pair per entry, in the place of the second list)
        for (int64_t k = 0, run = 0; k < a.count && e == hipSuccess; k += run) {
            run = pos ? recordRun(pos + off + k, a.count - k) : a.count;
            e = hipMemcpyAsync(instRec_.p + (size_t)k * W, buf + (size_t)(pos ? pos[off + k] : off + k) * W, (size_t)run * W * 4, hipMemcpyHostToDevice, stream_);
        }
        if (e == hipSuccess && (e = launchInstScatterRot(r, stream_)) == hipSuccess) ++instRotations_;
    }
    rc = endInstanceCall(true);
    return e != hipSuccess ? hipFail(e, "instances: records to the device, rotated") : rc;
}

void Batch::promoteLoaded(const uint32_t* buf, int64_t total) {
    const size_t W = (size_t)stateRows_ + (size_t)iSlotsAlloc_ + (size_t)xSlotsAlloc_;
    for (int r = 0; r < stateLayout_.nRegs; ++r) {
        if (tracked(r) || intrinsicLane(r)) continue;
        const uint32_t held = bitsOf(hostValue_[(size_t)r]);
        bool differs = false;
        for (int64_t k = 0; k < total && !differs; ++k) differs = buf[(size_t)k * W + (size_t)r] != held;
        if (!differs) continue;
        noteRegisterWritten(r);   // as if setRegisterAt had written it
    }
}

}  // namespace fx
