// fx_tracks_stub.cpp — host stand-ins for the launch functions of csrc/fx_tracks.hip (TEST INFRASTRUCTURE, see hip_stub.cpp).
// Both do the real moves in stream order on the stand-in's "device" memory, written from the definition in fx_tracks.hpp with an
// addressing of its own - not the kernel's 16 bytes per lane and lane per entry: the hold goes register by register, event row
// by event row, word by word; the scatter range by range, row by row, entry by entry.  Words move with memcpy: bit patterns.
// A table entry, an entry of the list or a range that points outside its block is counted and never followed.
//
// The stand-in remembers where the last hold wrote (the first event row, the number of rows, the table), so that a test can
// read the expanded rows back once the stream has drained (fxstub_track_rows), and at which count of emulation kernels
// (fxstub_kernels_run) the last hold and the last scatter ran: the order of the launches of a block.
#include <atomic>
#include <cstring>
#include <functional>
#include <mutex>

#include "../../fx8010-emulator-core_amd/csrc/fx_tracks.hpp"

void fxstubEnqueue(hipStream_t stream, std::function<void()> op);   // hip_stub.cpp
extern "C" long fxstub_kernels_run(void);

namespace {
std::atomic<long> g_holds{0}, g_scatters{0}, g_strays{0}, g_seq{0};
std::mutex g_mu;
fx::TrackHoldArgs g_last{};          // of the most recent hold that ran
long g_holdAt = -1, g_scatterAt = -1, g_holdSeq = -1, g_scatterSeq = -1;

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

void hold(const fx::TrackHoldArgs& a) {
    for (int t = 0; t < a.nRegs; ++t) {
        const long long srow = a.stateRow[t], first = a.firstRow[t], rows = a.rowCount[t];
        if (srow < 0 || srow >= a.stateRows || first < 0 || rows < 1 || first + rows > a.totalRows) { g_strays.fetch_add(1); continue; }
        for (long long e = 0; e < rows; ++e)
            for (long long i = 0; i < a.nPad; ++i) std::memcpy(a.rows + (first + e) * a.nPad + i, a.state + srow * a.nPad + i, 4);
    }
    std::lock_guard<std::mutex> lock(g_mu);
    g_last = a;
    g_holdAt = fxstub_kernels_run();
    g_holdSeq = g_seq.fetch_add(1);
}

void scatter(const fx::TrackScatterArgs& a) {
    for (int j = 0; j < a.nRanges; ++j) {
        const fx::TrackRange r = a.ranges[j];
        if (r.valueRow < 0 || r.valueRow >= a.valueRows || r.rowLo < 0 || r.rowHi > a.totalRows || r.rowLo >= r.rowHi) { g_strays.fetch_add(1); continue; }
        for (long long row = r.rowLo; row < r.rowHi; ++row)
            for (long long i = 0; i < a.count; ++i) {
                const long long inst = a.list[i];
                if (inst < 0 || inst >= a.n) {
                    if (j == 0 && row == r.rowLo) g_strays.fetch_add(1);
                    continue;
                }
                std::memcpy(a.rows + row * a.nPad + inst, a.values + (long long)r.valueRow * a.count + i, 4);
            }
    }
    std::lock_guard<std::mutex> lock(g_mu);
    g_scatterAt = fxstub_kernels_run();
    g_scatterSeq = g_seq.fetch_add(1);
}
}  // namespace

extern "C" long fxstub_track_holds(void) { return g_holds.load(); }         // launches that ran
extern "C" long fxstub_track_scatters(void) { return g_scatters.load(); }
extern "C" long fxstub_track_strays(void) { return g_strays.load(); }       // table entries, list entries and ranges out of range (none is ever followed)
// the emulation kernels that had run when the last hold / the last scatter ran, and the order of those two among the launches here
extern "C" long fxstub_track_hold_at(void) { std::lock_guard<std::mutex> lock(g_mu); return g_holdAt; }
extern "C" long fxstub_track_scatter_at(void) { std::lock_guard<std::mutex> lock(g_mu); return g_scatterAt; }
extern "C" long fxstub_track_hold_before_scatter(void) { std::lock_guard<std::mutex> lock(g_mu); return g_holdSeq >= 0 && g_holdSeq < g_scatterSeq; }
// the table of the last hold: out[0] = registers, then (state row, first event row, rows) each; returns nPad
extern "C" long long fxstub_track_table(int* out, int cap) {
    std::lock_guard<std::mutex> lock(g_mu);
    if (cap > 0) out[0] = g_last.nRegs;
    for (int t = 0; t < g_last.nRegs && 1 + 3 * t + 2 < cap; ++t) {
        out[1 + 3 * t] = g_last.stateRow[t];
        out[2 + 3 * t] = g_last.firstRow[t];
        out[3 + 3 * t] = g_last.rowCount[t];
    }
    return g_last.nPad;
}
// the event rows the last hold filled, as they are now ([totalRows][nPad], at most `cap` words): call with the streams drained and
// before the next block (the buffer is the handle's); returns totalRows
extern "C" long long fxstub_track_rows(uint32_t* out, long long cap) {
    std::lock_guard<std::mutex> lock(g_mu);
    if (!g_last.rows) return 0;
    const long long words = g_last.totalRows * g_last.nPad;
    if (out && cap > 0) std::memcpy(out, g_last.rows, (size_t)(words < cap ? words : cap) * 4);
    return g_last.totalRows;
}

namespace fx {

hipError_t launchTrackHold(const TrackHoldArgs& args, hipStream_t stream) {
    if (!args.state || !args.rows || !aligned16(args.state) || !aligned16(args.rows)) return hipErrorInvalidValue;
    if (args.nPad < 256 || args.nPad % 256 != 0 || args.totalRows < 1 || args.stateRows < 1 || args.nRegs < 1 || args.nRegs > kMaxTrackHolds) return hipErrorInvalidValue;
    const TrackHoldArgs a = args;
    fxstubEnqueue(stream, [a] {
        hold(a);
        g_holds.fetch_add(1);
    });
    return hipGetLastError();   // as the real helpers do after hipLaunchKernelGGL
}

hipError_t launchTrackScatter(const TrackScatterArgs& args, hipStream_t stream) {
    if (!args.rows || !args.list || !args.values || !args.ranges) return hipErrorInvalidValue;
    if (args.count < 1 || args.count >= ((long long)1 << 31) || args.valueRows < 1 || (long long)args.valueRows * args.count >= ((long long)1 << 31)) return hipErrorInvalidValue;
    if (args.n < 1 || args.nPad < args.n || args.totalRows < 1 || args.nRanges < 1) return hipErrorInvalidValue;
    const TrackScatterArgs a = args;
    fxstubEnqueue(stream, [a] {
        scatter(a);
        g_scatters.fetch_add(1);
    });
    return hipGetLastError();
}

}  // namespace fx
