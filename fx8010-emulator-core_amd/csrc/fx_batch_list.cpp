// fx_batch_list.cpp — the by-list frame of one batch (fx_batch.hpp "THE BY-LIST FRAME"): the one list check behind the check...
// functions of the by-list calls, and the pieces of the staging frame that the instance calls (fx_batch_instances.cpp), the record
// bank (fx_batch_bank.cpp) and the list sets (fx_batch_registers.cpp, fx_batch_tram.cpp, fx_batch_meter_list.cpp, fx_batch_tracks.cpp) are written in.
#include "fx_batch.hpp"

#include <algorithm>

namespace fx {

Batch::ListFault Batch::checkList(const int64_t* list, int64_t count, int64_t range, bool unique) {
    for (int64_t i = 0; i < count; ++i)
        if (list[i] < 0 || list[i] >= range) return {ListFault::kOutside, i};
    if (!unique || count < 2) return {};
    // repeats: a bitmap over the range where that is the cheaper one to clear, else a sorted copy
    if ((range + 63) / 64 <= 16 * count) {
        std::vector<uint64_t> seen((size_t)((range + 63) / 64), 0);
        for (int64_t i = 0; i < count; ++i) {
            uint64_t& word = seen[(size_t)(list[i] >> 6)];
            const uint64_t bit = (uint64_t)1 << (list[i] & 63);
            if (word & bit) return {ListFault::kRepeat, i};
            word |= bit;
        }
        return {};
    }
    std::vector<int64_t> sorted(list, list + count);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end()) return {};
    // a refusal, off the hot path: the entry the bitmap would have named - of every value listed more than once its second entry,
    // and of those the first in list order
    std::vector<std::pair<int64_t, int64_t>> byValue((size_t)count);
    for (int64_t i = 0; i < count; ++i) byValue[(size_t)i] = {list[i], i};
    std::sort(byValue.begin(), byValue.end());
    int64_t entry = count;
    for (size_t i = 1; i < byValue.size(); ++i)
        if (byValue[i].first == byValue[i - 1].first) entry = std::min(entry, byValue[i].second);
    return {ListFault::kRepeat, entry};
}

std::string Batch::listOutside(const std::string& name, const ListFault& f, int64_t range) {
    return name + ": entry " + std::to_string(f.entry) + " of the list is outside 0.." + std::to_string(range - 1);
}

int Batch::waitPreviousInstCall(const char* what) {
    if (!instLaunched_) return 0;
    const hipError_t e = hipEventSynchronize(evInst_);
    if (e != hipSuccess) return hipFail(e, what);
    instLaunched_ = false;
    return 0;
}

hipError_t Batch::orderBehindQueuedBlocks() {
    hipError_t e = launched_ ? hipStreamWaitEvent(stream_, ev1_, 0) : hipSuccess;
    if (e == hipSuccess && busLaunched_) e = hipStreamWaitEvent(stream_, evBus_, 0);
    return e;
}

int Batch::closeInstCall(hipError_t e, const char* what) {
    if (e == hipSuccess) e = hipEventRecord(evInst_, stream_);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream_);   // (nothing may still read the staging)
        return hipFail(e, what);
    }
    instLaunched_ = true;
    return 0;
}

void Batch::noteRegisterWritten(int r) {
    if (coldControl(r)) coldSetChanged();
    if (!forcedLane_[(size_t)r] && !intrinsicLane(r) && readByProgram(r)) {
        forcedLane_[(size_t)r] = 1;
        lowDirty_ = true;
    }
    laneWritten_[(size_t)r] = 1;
}

}  // namespace fx
