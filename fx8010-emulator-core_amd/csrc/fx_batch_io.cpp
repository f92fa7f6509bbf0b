// fx_batch_io.cpp — from "a block arrives" to "the kernel is launched": the host and device entry points, the routes a host block
// can take (the library's small pinned pair, in place on the caller's pinned buffers, staged in one piece, staged in pieces on
// three streams), the argument and addressability checks, the kernel arguments and the launch.
#include "fx_batch.hpp"

#include <cstddef>
#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

// pitch: instances per PCM row of the HOST buffers (>= n_); a shard of a larger batch reads / writes its columns of the
// caller's [sample][channel][all instances] arrays in place (fx_shard.cpp)
namespace {
constexpr size_t kPinnedFloats = 512;
// the kernels step through PCM by two 32-bit byte strides: channels * pitch * 4 (a sample period) and pitch * 4 (a channel)
inline bool pcmStrideTooWide(int channels, int64_t pitch) { return (uint64_t)std::max(channels, 1) * (uint64_t)pitch * 4u >= ((uint64_t)1 << 32); }
// A host block of 32 MiB and more is cut into eight pieces (consecutive sample ranges) whose copy-in, kernel and copy-out overlap
// on three streams (round 2: 268 MB each way in 6.5 instead of 12.7 ms from pinned buffers).  Smaller blocks were tried in pieces in
// round 5 (by size, 2-8 of them) for real-time callers and gained little - 32 samples x 131 072 instances: 806 -> 622 us - because
// the runtime's copy-OUT is a shader copy that slows a kernel running beside it threefold (profiles/r05_rt_timeline_131072.txt),
// and pieces are not timed by the stage tuner; what serves those callers is the in-place path above (pinned buffers: 486 us).
constexpr size_t kPipelinedBytes = (size_t)32 << 20;
inline int hostPieces(size_t bytes, int nSamples, int most) { return (bytes >= kPipelinedBytes && nSamples >= 2 * most) ? most : 1; }

inline bool pointerAttributes(const void* p, hipPointerAttribute_t* attr) {
    std::memset(attr, 0, sizeof(*attr));
    if (hipPointerGetAttributes(attr, p) == hipSuccess) return true;
    (void)hipGetLastError();   // (pageable memory: the runtime says "invalid value", which must not stay behind as the thread's last error)
    return false;
}

// Can the device address the whole of [p, p + bytes)?  Yes for pinned host memory (hipHostMalloc / hipHostRegister - e.g. a torch
// pinned tensor) that lies inside ONE mapping, and - only when the caller allows device memory: device >= 0 - for memory of that
// device whose allocation holds the range.  *dev: the address the kernel takes.  The range comes from the runtime's own record of
// the allocation the address belongs to; where it keeps none for registered host memory, both ends pinned with one address offset
// between them will do.  (A caller that registered part of a buffer takes the staged copies.)
inline bool addressable(const void* p, size_t bytes, int device, const void** dev) {
    hipPointerAttribute_t attr;
    if (!pointerAttributes(p, &attr)) return false;
    const bool host = attr.type == hipMemoryTypeHost;
    if (host ? !attr.devicePointer : (device < 0 || attr.type != hipMemoryTypeDevice || attr.device != device)) return false;
    *dev = host ? attr.devicePointer : p;
    if (host && bytes <= 1) return true;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(*dev)) == hipSuccess && base && size) {
        const char *lo = static_cast<const char*>(base), *at = static_cast<const char*>(*dev);
        return at >= lo && bytes <= size && static_cast<size_t>(at - lo) <= size - bytes;
    }
    (void)hipGetLastError();   // (reported by the answer: not again by the next launch helper that asks)
    hipPointerAttribute_t last;
    if (!host || !pointerAttributes(static_cast<const char*>(p) + (bytes - 1), &last) || last.type != hipMemoryTypeHost || !last.devicePointer) return false;
    return static_cast<const char*>(last.devicePointer) - static_cast<const char*>(*dev) == static_cast<std::ptrdiff_t>(bytes - 1);
}

// Bytes from the first to the last element of a [rows][pitch] PCM block whose instances are columns 0..n-1.
inline size_t pcmExtent(size_t rows, int64_t n, int64_t pitch) { return ((rows - 1) * (size_t)pitch + (size_t)n) * 4; }

// in == out is fine in place (an instance reads its sample before it writes it, and no other instance touches that word), and so
// are two footprints that share no element - e.g. two column ranges of one buffer.  Footprints that overlap in any other way need
// the whole input read before the first output is written: the staged copies do that.  Both have the same pitch: element r * P + c
// (c < n) of `out` is element r' * P + c' of `in` only if c - c' = m (mod P), m = (out - in) mod P, which |c - c'| < n rules out
// for n <= m <= P - n.
inline bool pcmDisjointOrSame(const float* in, const float* out, size_t rows, int64_t n, int64_t pitch) {
    if (in == out) return true;
    const size_t bytes = pcmExtent(rows, n, pitch);
    const char *x = reinterpret_cast<const char*>(in), *y = reinterpret_cast<const char*>(out);
    if (x + bytes <= y || y + bytes <= x) return true;
    const std::ptrdiff_t d = y - x;
    if (d % 4 != 0) return false;
    int64_t m = (int64_t)(d / 4) % pitch;
    if (m < 0) m += pitch;
    return m >= n && m <= pitch - n;
}
}  // namespace

// Tiers without in-kernel tracks (interpreter, HIP C++ kernel): the same schedule by cutting the block at its change
// points and writing the registers in between - what the caller would have had to do.
int Batch::processWithTrackFallback(const float* dIn, float* dOut, int nSamples, hipStream_t stream, int64_t pitch) {
    std::vector<PendingTrack> tracks;
    tracks.swap(pendingTracks_);
    pendingTracks_.resize(trackRegs_.size());
    // (list schedules, fx_batch_tracks.cpp: their steps are applied at the cuts by the scatter of the register list sets)
    std::vector<ListSchedule> lists;
    lists.swap(listSchedules_);
    std::vector<int> cuts{0, nSamples};
    for (const PendingTrack& t : tracks)
        for (int k = 0; k < t.steps && (int64_t)k * t.period < nSamples; ++k) cuts.push_back(k * t.period);
    bool listSteps = false;
    for (const ListSchedule& l : lists)
        for (int q = 0; q < (l.list.empty() ? 0 : l.stepsInside(nSamples)); ++q) {
            cuts.push_back(l.first + q * l.period);
            listSteps = true;
        }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    const size_t rowFloats = (size_t)prog_.numChannels * (size_t)pitch;   // floats per sample period
    int rc = 0;
    for (size_t c = 0; c + 1 < cuts.size() && rc == 0; ++c) {
        const int lo = cuts[c], hi = cuts[c + 1];
        for (size_t k = 0; k < tracks.size() && rc == 0; ++k) {
            const PendingTrack& t = tracks[k];
            if (t.steps <= 0 || lo % t.period != 0 || lo / t.period >= t.steps) continue;
            const std::string& name = prog_.regs[(size_t)trackRegs_[k]].name;
            rc = t.perInstance ? setRegisterArray(name, &t.values[(size_t)(lo / t.period) * (size_t)n_]) : setRegister(name, t.values[(size_t)(lo / t.period)]);
            if (rc > 0) rc = fail(FX_E_ARG, "track: register vanished");
        }
        if (rc == 0) rc = applyTrackListsAt(lists, lo);
        controlHeat_ = 0;  // these writes are the schedule, not a moving slider
        if (rc == 0) rc = processDevice(dIn + (size_t)lo * rowFloats, dOut + (size_t)lo * rowFloats, hi - lo, stream, pitch);
    }
    // (the staging is free again behind the last scatter, which ran on the handle's stream)
    const int rc2 = finishTrackLists(stream_, listSteps);
    return rc != 0 ? rc : rc2;
}

// The refusals of every entry point, written once: a call that is refused has changed nothing and launches nothing.
int Batch::checkBlock(const float* in, const float* out, int nSamples, int64_t* pitch) {
    if (*pitch <= 0) *pitch = n_;
    if (nSamples < 0) return fail(FX_E_ARG, "n_samples < 0");
    if (*pitch < n_) return fail(FX_E_ARG, "PCM row pitch below the instance count");
    if (pcmStrideTooWide(prog_.numChannels, *pitch)) return fail(FX_E_ARG, "PCM row pitch too wide: channels * pitch * 4 must stay below 2^32");
    if (nSamples > 0 && (!in || !out)) return fail(FX_E_ARG, "null buffer");
    return 0;
}

// Head of a block as the caller sees it (once for a host block that is launched in pieces: a translation must not fire between
// two of them).  The class of block lengths goes by what the kernel is launched with - the piece -, the sample clock by the block.
void Batch::beginBlock(int nSamples, int pieces) {
    pendingSamples_ = nSamples / pieces;
    if (controlHeat_ > 0 && --controlHeat_ == 0 && c_.deferred) lowDirty_ = true;  // quiet again: translate
    // (as it has been: pieces are not timed, and the stage tuner does not move on at the head of a block in pieces either - whether
    // it should is a question of its own)
    if (pieces == 1) noteLaunchTime();
    noteBlockLength(pendingSamples_);
    leanStep();
    sampleClock_ += nSamples;
}

int Batch::processDevice(const float* dIn, float* dOut, int nSamples, hipStream_t stream, int64_t pitch) {
    (void)hipSetDevice(device_);
    const int rc = checkBlock(dIn, dOut, nSamples, &pitch);
    if (rc != 0) return rc;
    beginBlock(nSamples);
    return launchBlock(dIn, dOut, nSamples, stream, pitch, kWholeBlock);
}

KernelArgs Batch::kernelArgs(const float* dIn, float* dOut, int nSamples, int64_t pitch) const {
    KernelArgs a{};
    const size_t nOps = c_.low.steady.size();
    a.steady = c_.dStream;
    a.last = c_.dStream + nOps * 8;
    a.rowTable = c_.dStream + nOps * 16;
    a.state = dState_;
    a.in = dIn;
    a.out = dOut;
    a.itram = dITram_;
    a.xtram = dXTram_;
    a.lut = dLut_;
    a.n = n_;
    a.nPad = nPad_;
    a.pcmPitch = pitch;
    a.nOps = (int)nOps;
    a.nLoad = (int)c_.low.loadRows.size();
    a.nStore = (int)c_.low.storeRows.size();
    a.nSamples = nSamples;
    a.channels = prog_.numChannels;
    for (int c = 0; c < kMaxChannels; ++c) {
        a.inRow[c] = c < prog_.numChannels ? c_.low.inRow[c] : -1;
        a.latchRow[c] = c < prog_.numChannels ? c_.low.latchRow[c] : 0;
    }
    a.iSlots = iSlotsAlloc_;
    a.xSlots = xSlotsAlloc_;
    a.iSize = prog_.iTramSize;
    a.xSize = prog_.xTramSize;
    a.nZero = (int)c_.low.zeroRows.size();
    const uint32_t rowBytes = 256u * (uint32_t)instPerLane_;
    a.skipOff = c_.low.skipRow >= 0 ? (uint32_t)c_.low.skipRow * rowBytes : 0;
    a.cursorOff = c_.low.cursorRow >= 0 ? (uint32_t)c_.low.cursorRow * rowBytes : 0;
    a.noiseOff = c_.low.noiseRow >= 0 ? (uint32_t)c_.low.noiseRow * rowBytes : 0;
    a.oodOff = c_.low.oodRow >= 0 ? (uint32_t)c_.low.oodRow * rowBytes : 0;
    a.aliveOff = c_.low.aliveRow >= 0 ? (uint32_t)c_.low.aliveRow * rowBytes : 0;
    a.hasShadow = c_.low.skipRow >= 0 ? 1 : 0;
    a.instPerLane = instPerLane_;
    a.tramDane = (c_.low.tramDane && c_.low.cursorRow >= 0) ? 1 : 0;
    a.oodRow = stateLayout_.oodRow;
    a.countLo = stateLayout_.countLo;
    a.countHi = stateLayout_.countHi;
    a.staticCount = c_.low.staticCount;
    a.nRows = c_.low.nRows;
    return a;
}

// the same block for the assembly tiers (interpreter and generated code)
AsmArgs Batch::asmArgs(const KernelArgs& a) const {
    AsmArgs g{};
    g.steady = a.steady; g.last = a.last; g.rowTable = a.rowTable; g.state = a.state;
    g.in = a.in; g.out = a.out; g.itram = a.itram; g.xtram = a.xtram; g.lut = a.lut;
    g.n = a.n; g.nPad = a.nPad; g.pcmPitch = a.pcmPitch; g.nLoad = a.nLoad; g.nStore = a.nStore;
    g.nSamples = a.nSamples; g.channels = a.channels;
    for (int c = 0; c < kMaxChannels; ++c) {
        g.inOff[c] = a.inRow[c] >= 0 ? a.inRow[c] * (int)c_.low.rowPitch : -1;
        g.latchOff[c] = a.latchRow[c] * (int)c_.low.rowPitch;
    }
    g.iSlots = a.iSlots; g.xSlots = a.xSlots; g.iSize = a.iSize; g.xSize = a.xSize;
    g.cursorRow = stateLayout_.cursorBase; g.noiseRow = stateLayout_.noiseBase;
    g.oodRow = a.oodRow; g.countLo = a.countLo; g.countHi = a.countHi; g.staticCount = a.staticCount;
    g.lutX1Off = kLutX1Off * 8;
    g.tramDane = (c_.low.tramDane && (c_.low.usesITram || c_.low.usesXTram)) ? 1 : 0;   // (like the other tiers: counters step where the program has taps)
    if (c_.low.multipass) g.tramDane |= 2;
    if (!c_.useXlate && c_.variant != ASM_LDS && priorityTurns(c_.variant)) {
        // the interpreter's wavefronts take turns like generated code's: a turn = 1/24 of the block at about 20 us per sample and
        // four wavefronts, between 0.66 and 10 ms
        int shift = 6;
        while ((1 << (shift - 6 + 1)) <= a.nSamples) ++shift;   // floor(log2(samples of the launch)) + 6
        g.tramDane |= 4 | (std::min(std::max(shift, 16), 20) << 8);
    }
    if (c_.useXlate) {
        // code streams are named by their byte offset from the kernel entry: {fast, exact} per argument
        g.steady = reinterpret_cast<const uint32_t*>((uintptr_t)c_.steady);
        g.last = reinterpret_cast<const uint32_t*>((uintptr_t)c_.last);
        g.initOff = (int)c_.initOff;
        g.tracks = trackRegs_.empty() ? nullptr : dTracks_;
        if (c_.stages > 1) {
            g.stages = a.rowTable + c_.low.loadRows.size() + c_.low.storeRows.size() + c_.low.zeroRows.size();
            g.nStages = c_.stages;
        }
    }
    return g;
}

#ifdef FX_DIAGNOSTICS
// the end stamps' own buffer rides in the kernarg slot of the stage descriptors, which an unstaged launch leaves unused (nStages
// stays 0: the template never looks at the pointer)
int Batch::ensureEndStamps() {
    const size_t words = ((size_t)n_ + 63) / 64;
    if (words <= stampWords_) return 0;
    waitLastLaunch();
    (void)hipFree(dStamps_);
    dStamps_ = nullptr;
    stampWords_ = 0;
    if (hipMalloc(reinterpret_cast<void**>(&dStamps_), words * 4) != hipSuccess) return fail(FX_E_MEMORY, "end stamps");
    stampWords_ = words;
    return 0;
}
#endif

// the quiet loop's exit words ride in the kernarg slot of the stage descriptors, which an unstaged launch leaves unused (nStages
// stays 0: the template never looks at the pointer)
// (two words per wavefront: a loop with sum groups writes pairs {exit sample, repairs}, one without them the first half only)
int Batch::ensureQuietLeft() {
    const size_t words = 2 * (((size_t)n_ + 63) / 64);
    if (words <= quietLeftWords_) return 0;
    waitLastLaunch();
    (void)hipFree(dQuietLeft_);
    dQuietLeft_ = nullptr;
    quietLeftWords_ = 0;
    if (hipMalloc(reinterpret_cast<void**>(&dQuietLeft_), words * 4) != hipSuccess) return fail(FX_E_MEMORY, "exit words of the quiet loop");
    quietLeftWords_ = words;
    return 0;
}

// Lower if need be and launch: the block has been checked and counted (beginBlock) by the caller.
int Batch::launchBlock(const float* dIn, float* dOut, int nSamples, hipStream_t stream, int64_t pitch, unsigned mode) {
    int rc = ensureLowered();
    if (rc != 0) return rc;
    everLowered_ = true;
    if (nSamples == 0) return 0;
    if (tracksArmed() && !c_.useXlate) return processWithTrackFallback(dIn, dOut, nSamples, stream, pitch);
    hipStream_t s = pick(stream);
    // (instance calls run on stream_: a block on another stream follows the last of them that may still be running)
    if (instLaunched_ && s != stream_) {
        const hipError_t we = hipStreamWaitEvent(s, evInst_, 0);
        if (we != hipSuccess) return hipFail(we, "waiting for the instance call in front of the block");
    }
    if (c_.useXlate && !trackRegs_.empty() && (rc = uploadTracks(nSamples, s)) != 0) return rc;
    const bool timed = !(mode & kUntimed);
    hipError_t e = hipSuccess;
    for (;;) {
        const KernelArgs a = kernelArgs(dIn, dOut, nSamples, pitch);
        e = timed ? hipEventRecord(ev0_, s) : hipSuccess;
        lastLaunchQuiet_ = lastLaunchSums_ = false;
        if (e == hipSuccess && c_.useAsm) {
            AsmArgs g = asmArgs(a);
#ifdef FX_DIAGNOSTICS
            if (c_.useXlate && c_.stages <= 1 && FX_DIAG_KNOB("FX_XLATE_ENDSTAMP")) {
                if ((rc = ensureEndStamps()) != 0) return rc;
                g.stages = dStamps_;
            }
#endif
            const bool quiet = c_.useXlate && c_.quiet && c_.stages <= 1;
            if (quiet) {
                if ((rc = ensureQuietLeft()) != 0) return rc;
                g.stages = dQuietLeft_;
                e = hipMemsetAsync(dQuietLeft_, 0xff, quietLeftWords_ * 4, s);
            }
            lastLaunchQuiet_ = quiet;
            lastLaunchSums_ = quiet && c_.sumGroups;
            if (e == hipSuccess)
                e = c_.useXlate ? launchAsmFunction(c_.fn, g, (unsigned)((n_ + 63) / 64), c_.ldsBytes, s, (unsigned)c_.stages)
                            : launchAsmInterp(g, c_.variant, c_.variant == ASM_LDS ? (size_t)a.nRows * 256 : 0, device_, s);
        } else if (e == hipSuccess) {
            e = launchStepBlock(a, c_.low.multipass, s);
        }
        const hipError_t launchError = e;   // (of the event record in front of the launch or of the launch itself)
        // Metering: the meter kernel reads the block this launch writes, right behind it on the same stream and in front of the
        // ev1_ record - every wait for "the last launch" covers its read of the caller's buffer, and the kernel time includes it.
        if (e == hipSuccess && dMeter_) {
            MeterArgs m{};
            m.y = dOut;
            m.rows = dMeter_;
            m.n = n_;
            m.nPad = nPad_;
            m.pitch = pitch;
            m.samples = nSamples;
            m.channels = prog_.numChannels;
            if (dTarget_) {
                // a target is set: fx_meter_target in place of fx_meter - the block is read once - and the target position moves
                // on by this launch's samples, so that however a stream is cut every sample meets the same target row
                // (with level meters on, fx_meter_target_level: the same block read once, two more accumulators)
                if (dLevel_) {
                    if ((e = launchMeterTargetLevel(MeterTargetLevelArgs{meterTargetArgs(m), levelParams()}, s)) != hipSuccess) return hipFail(e, "launch fx_meter_target_level");
                    ++meterLevelLaunches_;
                } else if ((e = launchMeterTarget(meterTargetArgs(m), s)) != hipSuccess) {
                    return hipFail(e, "launch fx_meter_target");
                }
                ++meterTargetLaunches_;
                targetPos_ += nSamples;
                if (targetLoop_) targetPos_ %= targetSamples_;
            } else {
                if (dLevel_) {
                    if ((e = launchMeterLevel(MeterLevelArgs{m, levelParams()}, s)) != hipSuccess) return hipFail(e, "launch fx_meter_level");
                    ++meterLevelLaunches_;
                } else if ((e = launchMeter(m, s)) != hipSuccess) {
                    return hipFail(e, "launch fx_meter");
                }
                ++meterLaunches_;
            }
            meterSamples_ += nSamples;
            // tone meters: a launch of its own behind whichever of the four ran, reading the same block, in front of ev1_
            if (dTone_) {
                if ((rc = launchToneMeter(m, s)) != 0) return rc;
            }
        }
        if (e == hipSuccess && timed) e = hipEventRecord(ev1_, s);
        // A workgroup of several wavefronts that the device will not start (registers x wavefronts beyond a CU, LDS): the plain
        // program runs everywhere - no stages for this handle from now on, and a second pass for this block.  Only for what a launch
        // CONFIGURATION can cause: any other error (a fault of an earlier kernel that this call merely inherits, a lost device) is
        // reported as it is and leaves the handle's choice of code alone.  Nothing has been consumed at this point that the second
        // pass needs: a staged program has no control tracks (planStages refuses them), so uploadTracks has not run.
        const bool configError = launchError == hipErrorInvalidValue || launchError == hipErrorInvalidConfiguration || launchError == hipErrorLaunchOutOfResources;
        if (!(configError && c_.useXlate && c_.stages > 1 && !stagingOff_ && trackRegs_.empty())) break;
        (void)hipGetLastError();   // (the launch's own error, just read: not a sticky one)
        stagingOff_ = true;
        lowDirty_ = true;
        if ((rc = ensureLowered()) != 0) return rc;
    }
    if (e != hipSuccess) return hipFail(e, "launch fx_step_block");
    launched_ = timed;  // (an untimed launch is synchronised by its caller before anything else happens)
    timed_ = timed;
    lastLaunchTimed_ = timed && !(mode & kPiece);
    lastLaunchPick_ = c_.stagePick;
    lastLaunchSamples_ = nSamples;
    lastLaunchClass_ = c_.useXlate ? c_.blockClass : -1;
    lastGrid_ = (unsigned)((n_ + 64 * instPerLane_ - 1) / (64 * instPerLane_));
    return 0;
}

// The device entries' check of a caller's buffer (fx_batch_bus_side.hpp CheckedAddr): memory of this handle's device, or
// device-visible host memory, over the whole of [p, p + bytes).  A refusal leaves nothing cached.
int Batch::lookup(CheckedAddr& c, const void* p, size_t bytes, const char* what) {
    if (c.holds(p, bytes)) return 0;
    c.forget();
    const void* dev = nullptr;
    if (!addressable(p, bytes, device_, &dev)) return fail(FX_E_ARG, what);
    c.host = p;
    c.bytes = bytes;
    c.dev = const_cast<void*>(dev);
    return 0;
}

// ... of an input / output pair, which is checked together: a pair that misses in either half is looked up afresh, one buffer
// given as both is looked up once, and a refusal of either leaves neither cached
int Batch::lookupPair(CheckedAddr& cIn, const void* in, size_t inBytes, CheckedAddr& cOut, const void* out, size_t outBytes) {
    static const char* const what = "d_in / d_out: not memory of this handle's device or device-visible host memory over the whole block";
    if (cIn.holds(in, inBytes) && cOut.holds(out, outBytes)) return 0;
    cIn.forget();
    cOut.forget();
    int rc = lookup(cIn, in, inBytes, what);
    if (rc != 0) return rc;
    if (out == in && outBytes == inBytes) cOut = cIn;
    else if ((rc = lookup(cOut, out, outBytes, what)) != 0) cIn.forget();
    return rc;
}

// rows of `width` bytes; one plain copy when neither side has a gap between its rows
hipError_t Batch::copyRows(void* dst, size_t dstPitch, const void* src, size_t srcPitch, size_t width, size_t rows, hipMemcpyKind kind, hipStream_t stream) {
    if (dstPitch == width && srcPitch == width) return hipMemcpyAsync(dst, src, rows * width, kind, stream);
    return hipMemcpy2DAsync(dst, dstPitch, src, srcPitch, width, rows, kind, stream);
}

int Batch::processDeviceChecked(const float* dIn, float* dOut, int nSamples, int64_t pitch, hipStream_t stream) {
    (void)hipSetDevice(device_);
    const int rc = checkBlock(dIn, dOut, nSamples, &pitch);
    if (rc != 0) return rc;
    if (nSamples > 0) {
        const size_t rows = (size_t)nSamples * (size_t)prog_.numChannels, bytes = pcmExtent(rows, n_, pitch);
        if (!checkedIn_.holds(dIn, bytes) || !checkedOut_.holds(dOut, bytes)) {
            checkedIn_.forget();
            checkedOut_.forget();
            if (!pcmDisjointOrSame(dIn, dOut, rows, n_, pitch)) return fail(FX_E_ARG, "input and output overlap without being one buffer");
            // memory of this device, or pinned host memory (its device address goes to the kernel)
            if (int lrc = lookupPair(checkedIn_, dIn, bytes, checkedOut_, dOut, bytes)) return lrc;
        }
        dIn = static_cast<const float*>(checkedIn_.dev);
        dOut = static_cast<float*>(checkedOut_.dev);
    }
    beginBlock(nSamples);
    return launchBlock(dIn, dOut, nSamples, stream, pitch, kWholeBlock);
}

int Batch::processHost(const float* in, float* out, int nSamples, int64_t pitch) {
    (void)hipSetDevice(device_);
    int rc = checkBlock(in, out, nSamples, &pitch);
    if (rc != 0) return rc;
    if (nSamples == 0) return ensureLowered();
    const size_t count = (size_t)nSamples * prog_.numChannels * (size_t)n_;
    const size_t rows = (size_t)nSamples * prog_.numChannels;
    // A few KB of PCM (per-sample calls on a handful of instances): two staged copies cost more than the launch.  The kernel
    // reads and writes pinned host memory instead - one launch, one synchronisation.
    if (count <= kPinnedFloats && pitch == n_) {
        if (!pinTried_) {
            pinTried_ = true;
            if (hipHostMalloc(reinterpret_cast<void**>(&hPinIn_), kPinnedFloats * 4, hipHostMallocDefault) != hipSuccess ||
                hipHostMalloc(reinterpret_cast<void**>(&hPinOut_), kPinnedFloats * 4, hipHostMallocDefault) != hipSuccess) {
                if (hPinIn_) (void)hipHostFree(hPinIn_);
                hPinIn_ = hPinOut_ = nullptr;
                (void)hipGetLastError();
            }
        }
        if (hPinIn_ && hPinOut_) {
            ++hostStagedBlocks_;
            std::memcpy(hPinIn_, in, count * 4);
            waitLastLaunch();
            // no event pair around a launch that is waited for right here (last_kernel_ms: -1) - unless schedules are armed:
            // the tiers that cut the block at every step launch several times and wait for each launch through its event
            beginBlock(nSamples);
            rc = launchBlock(hPinIn_, hPinOut_, nSamples, stream_, n_, tracksArmed() ? kWholeBlock : kUntimed);
            if (rc != 0) return rc;
            hipError_t se = hipStreamSynchronize(stream_);
            if (se != hipSuccess) return hipFail(se, "synchronising a small block");
            std::memcpy(out, hPinOut_, count * 4);
            return 0;
        }
    }
    // The caller's buffers are pinned host memory (a real-time host keeps its PCM in such buffers): NO copies at all - the kernel
    // reads its input from and stores its output to the caller's memory over PCIe, in both directions at once, while it
    // computes.  One launch, one wait.  Measured (tools/realtime_capacity.py, 32-sample blocks of config5): the staged path's
    // copy-out is a shader copy (__amd_rocclr_copyBuffer) that slows a kernel running beside it threefold
    // (profiles/r05_rt_timeline_131072.txt); in place, a block of 131 072 instances takes about what its 16.8 MB each way take the
    // link.  FX_HOST_PIPELINE=0 keeps the staged copies.  Any row pitch: the kernels address [sample][channel][pitch] - a shard of a
    // larger batch works on its columns of the caller's buffers, on its own device (this runs on the shard's thread, the device
    // current: the lookup below is that device's view of the memory).
    if (knobs_.hostPipeline) {
        const void *dIn = nullptr, *dOut = nullptr;
        const size_t bytes = pcmExtent(rows, n_, pitch);
        // (pinned HOST memory only: anything else handed to this entry, memory of the device included, is staged)
        if (pcmDisjointOrSame(in, out, rows, n_, pitch) && addressable(in, bytes, -1, &dIn) &&
            (static_cast<const void*>(out) == in ? (dOut = dIn, true) : addressable(out, bytes, -1, &dOut))) {
            ++hostInplaceBlocks_;
            rc = processDevice(static_cast<const float*>(dIn), static_cast<float*>(const_cast<void*>(dOut)), nSamples, stream_, pitch);
            const hipError_t se = hipStreamSynchronize(stream_);   // (also when the call failed: nothing of it may still touch the caller's memory)
            if (rc != 0) return rc;
            return se == hipSuccess ? 0 : hipFail(se, "synchronising a block on pinned host buffers");
        }
    }
    if (count > ioCap_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipFree(dIn_);
        (void)hipFree(dOut_);
        dIn_ = dOut_ = nullptr;
        ioCap_ = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&dIn_), count * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dOut_), count * 4);
        if (e != hipSuccess) return hipFail(e, "hipMalloc io");
        ioCap_ = count;
    }
    // Large blocks: copy-in, kernel and copy-out of consecutive pieces overlap.  268 MB each way (tools/host_block_rate.py):
    // pinned caller buffers 6.5 ms instead of 12.7 (both DMA directions at once), pageable ones 9.7 instead of 12.9 (the driver
    // pins them on the fly; a freshly allocated, untouched output buffer costs 2-3 x that in page faults either way).
    ++hostStagedBlocks_;
    const int pieces = hostPieces(count * 4, nSamples, kHostPieces);
    if (pieces >= 2 && !tracksArmed() && knobs_.hostPipeline)
        return processHostPipelined(in, out, nSamples, pitch, pieces);
    const size_t width = (size_t)n_ * 4;
    hipError_t e = copyRows(dIn_, width, in, (size_t)pitch * 4, width, rows, hipMemcpyHostToDevice, stream_);
    if (e != hipSuccess) return hipFail(e, "H2D");
    rc = processDevice(dIn_, dOut_, nSamples, stream_);
    if (rc != 0) {
        (void)hipStreamSynchronize(stream_);   // (whatever went wrong: no copy may still read the caller's buffer when this returns)
        return rc;
    }
    e = copyRows(out, (size_t)pitch * 4, dOut_, width, width, rows, hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream_);
        return hipFail(e, "D2H");
    }
    return 0;
}

// A large host block in pieces (dIn_ / dOut_ hold the whole block): while the kernel works on piece p, piece p + 1 is on its way
// in and piece p - 1 on its way out - two copy streams beside the compute stream, ordered by events.  The pieces are
// consecutive blocks to the kernel: state carries over exactly as between two calls.
int Batch::processHostPipelined(const float* in, float* out, int nSamples, int64_t pitch, int pieces) {
    if (!copyIn_) {
        hipError_t c = hipStreamCreateWithFlags(&copyIn_, hipStreamNonBlocking);
        if (c == hipSuccess) c = hipStreamCreateWithFlags(&copyOut_, hipStreamNonBlocking);
        for (int k = 0; k < kHostPieces && c == hipSuccess; ++k) {
            c = hipEventCreateWithFlags(&evIn_[k], hipEventDisableTiming);
            if (c == hipSuccess) c = hipEventCreateWithFlags(&evDone_[k], hipEventDisableTiming);
        }
        if (c != hipSuccess) return hipFail(c, "streams for the pipelined host block");
    }
    const size_t ch = (size_t)prog_.numChannels, width = (size_t)n_ * 4;
    auto lo = [&](int p) { return (int)((int64_t)nSamples * p / pieces); };
    auto copyIn = [&](int p) {
        const size_t first = (size_t)lo(p) * ch, rows = (size_t)(lo(p + 1) - lo(p)) * ch;
        hipError_t e = copyRows(dIn_ + first * (size_t)n_, width, in + first * (size_t)pitch, (size_t)pitch * 4, width, rows, hipMemcpyHostToDevice, copyIn_);
        if (e == hipSuccess) e = hipEventRecord(evIn_[p], copyIn_);
        return e;
    };
    auto launch = [&](int p) -> int {
        hipError_t e = hipStreamWaitEvent(stream_, evIn_[p], 0);
        if (e != hipSuccess) return hipFail(e, "pipelined host block");
        const size_t first = (size_t)lo(p) * ch * (size_t)n_;
        const int rc = launchBlock(dIn_ + first, dOut_ + first, lo(p + 1) - lo(p), stream_, n_, kPiece);
        if (rc != 0) return rc;
        e = hipEventRecord(evDone_[p], stream_);
        return e == hipSuccess ? 0 : hipFail(e, "pipelined host block");
    };
    auto copyOut = [&](int p) {
        const size_t first = (size_t)lo(p) * ch, rows = (size_t)(lo(p + 1) - lo(p)) * ch;
        hipError_t e = hipStreamWaitEvent(copyOut_, evDone_[p], 0);
        if (e != hipSuccess) return e;
        return copyRows(out + first * (size_t)pitch, (size_t)pitch * 4, dOut_ + first * (size_t)n_, width, width, rows, hipMemcpyDeviceToHost, copyOut_);
    };
    // (whatever goes wrong: no copy may still touch the caller's buffers when this returns)
    auto drain = [&]() {
        (void)hipStreamSynchronize(copyIn_);
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamSynchronize(copyOut_);
    };
    waitLastLaunch();
    // the block is ONE call to the bookkeeping of control changes and to the lowering, not kHostPieces
    beginBlock(nSamples, pieces);
    int rc = ensureLowered();
    if (rc != 0) return rc;
    hipError_t e = copyIn(0);
    if (e != hipSuccess) { drain(); return hipFail(e, "H2D"); }
    rc = launch(0);
    if (rc != 0) { drain(); return rc; }
    for (int p = 0; p < pieces; ++p) {
        if (p + 1 < pieces) {
            if ((e = copyIn(p + 1)) != hipSuccess) { drain(); return hipFail(e, "H2D"); }
            if ((rc = launch(p + 1)) != 0) { drain(); return rc; }
        }
        if ((e = copyOut(p)) != hipSuccess) { drain(); return hipFail(e, "D2H"); }
    }
    e = hipStreamSynchronize(copyOut_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    return e == hipSuccess ? 0 : hipFail(e, "pipelined host block");
}

// ---- group buses: a shared input and / or a mixed output per group of instances (fx_bus.hpp) ---------------------------------------
//
// None of the three kernel tiers knows about groups: a bus block is expand -> the ordinary launch, in place on a per-instance
// scratch block in device memory -> mix, ordered on one stream.  What crosses PCIe is the [sample][channel][group] side only.
// A feed block (fx_batch_bus_feed.cpp) fills the scratch from per-instance lists of a source block's columns instead.

bool Batch::busBuffersApart(const float* in, const float* out, size_t rows, int64_t inWidth, int64_t inPitch, int64_t outWidth, int64_t outPitch) {
    const bool oneLayout = inWidth == outWidth && inPitch == outPitch;
    if (in == out) return oneLayout;
    const char *x = reinterpret_cast<const char*>(in), *y = reinterpret_cast<const char*>(out);
    if (x + pcmExtent(rows, inWidth, inPitch) <= y || y + pcmExtent(rows, outWidth, outPitch) <= x) return true;
    return oneLayout && pcmDisjointOrSame(in, out, rows, inWidth, inPitch);   // (two column ranges of one buffer)
}

// the source block [rows][sources] of a feed block and the output: no shared byte
bool Batch::feedSourceApart(const float* src, const float* out, size_t rows, int64_t sources, int64_t outWidth, int64_t outPitch) {
    const char *x = reinterpret_cast<const char*>(src), *y = reinterpret_cast<const char*>(out);
    return x + pcmExtent(rows, sources, sources) <= y || y + pcmExtent(rows, outWidth, outPitch) <= x;
}

// The refusals of the bus entries, in front of everything else: a refused call has launched nothing and changed nothing.
int Batch::checkBus(const float* in, const float* out, const float* tapOut, const float* auxOut, int nSamples, int64_t group, unsigned flags, int64_t inPitch, int64_t outPitch, BusShape* shape,
                    bool feed) {
    if (nSamples < 0) return fail(FX_E_ARG, "n_samples < 0");
    if (group < 1) return fail(FX_E_ARG, "bus: group must be at least 1");
    if (flags & ~(unsigned)kBusFlags) return fail(FX_E_ARG, "bus: unknown flag bits");
    if (feed && feed_.sources < 1) return fail(FX_E_ARG, "bus feeds: feeds are off (fxb_bus_set_feeds)");
    if (feed && (flags & kBusSharedIn)) return fail(FX_E_ARG, "bus feeds: FXB_BUS_SHARED_IN does not go with a source block");
    BusShape s;
    s.group = std::min(group, n_);   // (a larger group is the one group of everything)
    s.groups = (n_ + s.group - 1) / s.group;
    s.inWidth = feed ? feed_.sources : (flags & kBusSharedIn) ? s.groups : n_;
    s.outWidth = (flags & kBusMixOut) ? s.groups : n_;
    if (feed) inPitch = s.inWidth;   // (the source block has a row pitch of exactly M)
    s.inPitch = inPitch > 0 ? inPitch : s.inWidth;
    s.outPitch = outPitch > 0 ? outPitch : s.outWidth;
    if (s.inPitch < s.inWidth || s.outPitch < s.outWidth) return fail(FX_E_ARG, "bus: row pitch below the width of the layout");
    if (pcmStrideTooWide(prog_.numChannels, s.inPitch) || pcmStrideTooWide(prog_.numChannels, s.outPitch) || pcmStrideTooWide(prog_.numChannels, n_))
        return fail(FX_E_ARG, "bus: PCM row too wide: channels * row length * 4 must stay below 2^32 in every layout");
    if (nSamples > 0 && (!in || !out)) return fail(FX_E_ARG, "null buffer");
    if (nSamples > 0 && feed && !feedSourceApart(in, out, (size_t)nSamples * (size_t)prog_.numChannels, s.inWidth, s.outWidth, s.outPitch))
        return fail(FX_E_ARG, "bus feeds: src overlaps the output (the layouts differ: there is no in-place form)");
    if (nSamples > 0 && !feed && !busBuffersApart(in, out, (size_t)nSamples * (size_t)prog_.numChannels, s.inWidth, s.inPitch, s.outWidth, s.outPitch))
        return fail(FX_E_ARG, "bus: input and output overlap without being one buffer with one layout");
    if (const char* why = checkTapShape(in, out, tapOut, (size_t)std::max(nSamples, 0) * (size_t)prog_.numChannels, tapTotal_, flags, s.inWidth, s.inPitch, s.outWidth, s.outPitch))
        return fail(FX_E_ARG, why);
    if (const char* why = checkAuxShape(nSamples > 0 ? in : nullptr, nSamples > 0 ? out : nullptr, tapOut, auxOut, (size_t)std::max(nSamples, 0) * (size_t)prog_.numChannels,
                                        send_.totalBuses, tapTotal_, flags, s.inWidth, s.inPitch, s.outWidth, s.outPitch))
        return fail(FX_E_ARG, why);
    *shape = s;
    return 0;
}

int Batch::ensureBusScratch(size_t floats) {
    if (!evBus_) {
        const hipError_t e = hipEventCreateWithFlags(&evBus_, hipEventDisableTiming);
        if (e != hipSuccess) { evBus_ = nullptr; return hipFail(e, "bus event"); }
    }
    if (floats <= bus_.cap) return 0;
    // (a block on the caller's stream may still be working on the old one)
    if (busLaunched_) (void)hipEventSynchronize(evBus_);
    (void)hipStreamSynchronize(stream_);
    return growBlock(bus_, floats, false, "hipMalloc bus scratch");
}

int Batch::ensureBusStage(size_t floats) {
    if (floats <= busStage_.cap) return 0;
    (void)hipStreamSynchronize(stream_);
    return growBlock(busStage_, floats, false, "hipMalloc bus staging");
}

// The block itself, asynchronous on `stream`.  in / out: the per-instance sides as the caller gave them (copied to / from the
// scratch by the runtime), narrowIn / narrowOut: the per-group sides as the device addresses them.  A block whose scratch would
// exceed kBusScratchBytes runs in consecutive sample ranges that fit - consecutive blocks to the kernel, like the pieces of
// processHostPipelined; with control tracks armed the block stays whole (a schedule counts samples from the head of ONE launch).
int Batch::busPieceSamples(int nSamples) const {
    const size_t perSample = (size_t)prog_.numChannels * (size_t)n_;
    const int most = tracksArmed() ? nSamples : (int)std::min<size_t>((size_t)nSamples, std::max<size_t>(kBusScratchBytes / (perSample * 4), 1));
    const int pieces = (nSamples + most - 1) / most;
    return (nSamples + pieces - 1) / pieces;
}

int Batch::runBus(const float* in, float* out, const float* narrowIn, int64_t narrowInPitch, float* narrowOut, int64_t narrowOutPitch, int nSamples, unsigned flags,
                  const BusShape& shape, hipStream_t stream, const Route* tap, const Route* aux, const FeedRoute* feed) {
    const size_t ch = (size_t)prog_.numChannels, perSample = ch * (size_t)n_;
    const int most = tracksArmed() ? nSamples : (int)std::min<size_t>((size_t)nSamples, std::max<size_t>(kBusScratchBytes / (perSample * 4), 1));
    const int pieces = (nSamples + most - 1) / most;
    int rc = ensureBusScratch((size_t)((nSamples + pieces - 1) / pieces) * perSample);
    if (rc != 0) return rc;
    hipStream_t s = pick(stream);
    // The scratch is one buffer: the previous bus block, on whatever stream it ran, must have emptied it before this one fills it
    // (the host entry has waited for it on the host already: waitLastLaunch).
    if (busLaunched_) {
        const hipError_t we = hipStreamWaitEvent(s, evBus_, 0);
        if (we != hipSuccess) return hipFail(we, "bus: waiting for the previous bus block");
    }
    // ... and with gains on, the most recent copy into a gain block (on the handle's stream) must have landed
    const bool weighted = (flags & kBusMixOut) && gainsOn_;
    if (weighted && gainCopied_) {
        const hipError_t we = hipStreamWaitEvent(s, evGain_, 0);
        if (we != hipSuccess) return hipFail(we, "bus: waiting for the gains");
    }
    // ... and a list set of the send or feed gains (fx_batch_bus_gain_list.cpp), where this block reads those
    if ((aux || feed) && sideListCopied_) {
        const hipError_t we = hipStreamWaitEvent(s, evList_, 0);
        if (we != hipSuccess) return hipFail(we, "bus: waiting for the gains set by list");
    }
    BusGainArgs gain{};
    if (weighted) {
        gain.target = dGain_[gainRamp_.target];
        gain.current = gainRamp_.pending ? dGain_[gainRamp_.target ^ 1] : nullptr;
        gain.gainPitch = n_;
        setRamp(gain, gainRamp_, nSamples, 0);
    }
    beginBlock(nSamples, pieces);   // ONE block to the bookkeeping of control changes and to the lowering
    if ((rc = ensureLowered()) != 0) return rc;
    auto lo = [&](int p) { return (int)((int64_t)nSamples * p / pieces); };
    // a failure behind the first launch of a piece: what has been queued still uses the scratch
    auto failQueued = [&](int rc0, hipError_t e, const char* what) {
        if (hipEventRecord(evBus_, s) == hipSuccess) busLaunched_ = true;
        return e != hipSuccess ? hipFail(e, what) : rc0;
    };
    const size_t width = (size_t)n_ * 4;
    for (int p = 0; p < pieces; ++p) {
        const int count = lo(p + 1) - lo(p);
        const size_t first = (size_t)lo(p) * ch;
        BusArgs a{};
        a.wide = bus_.p;
        a.rows = (long long)count * (long long)ch;
        a.n = n_;
        a.group = shape.group;
        a.groups = shape.groups;
        hipError_t e;
        if (feed) {
            // the third way to fill the scratch: from the lists of the feeds, out of this piece's source rows
            e = launchFeed(*feed, first, a.rows, nSamples, lo(p), s);
        } else if (flags & kBusSharedIn) {
            a.narrowIn = narrowIn + first * (size_t)narrowInPitch;
            a.narrowPitch = narrowInPitch;
            e = launchBusExpand(a, s);
        } else {
            e = copyRows(bus_.p, width, in + first * (size_t)shape.inPitch, (size_t)shape.inPitch * 4, width, (size_t)a.rows, hipMemcpyDefault, s);
        }
        if (e != hipSuccess) return hipFail(e, "bus: filling the scratch block");
        if ((rc = launchBlock(bus_.p, bus_.p, count, s, n_, pieces > 1 ? kPiece : kWholeBlock)) != 0) return failQueued(rc, hipSuccess, nullptr);
        // the taps read the scratch block where the emulation has just written it, like the meter (inside launchBlock): pre-fader
        if (tap && tap->dst && (e = launchTaps(*tap, first, a.rows, s)) != hipSuccess) return failQueued(0, e, "bus: the tap kernel");
        // ... and so do the sends, behind the taps and in front of the mix: chunk sums, then the fold to the aux rows
        if (aux && aux->dst && (e = launchSends(*aux, first, a.rows, nSamples, lo(p), s)) != hipSuccess) return failQueued(0, e, "bus: the send kernels");
        if (flags & kBusMixOut) {
            a.narrowIn = nullptr;
            a.narrowOut = narrowOut + first * (size_t)narrowOutPitch;
            a.narrowPitch = narrowOutPitch;
            gain.sample0 = lo(p);
            e = weighted ? launchBusMixGain(a, gain, s) : launchBusMix(a, s);
        } else {
            e = copyRows(out + first * (size_t)shape.outPitch, (size_t)shape.outPitch * 4, bus_.p, width, width, (size_t)a.rows, hipMemcpyDefault, s);
        }
        if (e == hipSuccess) e = hipEventRecord(evBus_, s);
        if (e != hipSuccess) return hipFail(e, "bus: emptying the scratch block");
        busLaunched_ = true;
    }
    ++busBlocks_;   // (blocks whose every piece was queued)
    if (tap) ++busTapBlocks_;   // (counted by every shard that was handed the rows, whether or not an entry falls into it)
    if (aux) {
        ++busSendBlocks_;      // (the same)
        sendRamp_.consume();   // as the ramp of the bus gains below
    }
    if (weighted) {
        ++busGainBlocks_;
        gainRamp_.consume();
    }
    if (feed) {
        ++busFeedBlocks_;
        feedRamp_.consume();   // (the same)
    }
    return 0;
}

int Batch::processBus(const float* in, float* out, int nSamples, int64_t group, unsigned flags, int64_t inPitch, int64_t outPitch, BusEntry entry, hipStream_t stream,
                      float* tapOut, float* auxOut, bool feed) {
    (void)hipSetDevice(device_);
    BusShape shape;
    int rc = checkBus(in, out, tapOut, auxOut, nSamples, group, flags, inPitch, outPitch, &shape, feed);
    if (rc != 0) return rc;
    if (nSamples == 0) return ensureLowered();
    const size_t rows = (size_t)nSamples * (size_t)prog_.numChannels;
    const size_t inBytes = pcmExtent(rows, shape.inWidth, shape.inPitch), outBytes = pcmExtent(rows, shape.outWidth, shape.outPitch);
    const size_t tapBytes = rows * (size_t)tapTotal_ * 4;
    const size_t auxBytes = rows * (size_t)send_.totalBuses * 4;
    const size_t pieceRows = (size_t)busPieceSamples(nSamples) * (size_t)prog_.numChannels;
    const void *devIn = nullptr, *devOut = nullptr, *devTap = nullptr, *devAux = nullptr;
    Route tapRoute, auxRoute;   // (of a side without rows: empty, and nothing below does anything with it)
    const Route* tap = tapOut ? &tapRoute : nullptr;
    const Route* aux = auxOut ? &auxRoute : nullptr;
    FeedRoute feedRoute;
    const FeedRoute* fed = feed ? &feedRoute : nullptr;
    // a source block is gathered where it lies only if the pointer attributes show memory of this device: every word of it is
    // read many times, and none of those reads may cross PCIe (anything else is copied into the device block of planFeedRoute)
    auto deviceSource = [&]() -> const void* {
        hipPointerAttribute_t attr;
        const void* dev = nullptr;
        return (pointerAttributes(in, &attr) && attr.type == hipMemoryTypeDevice && addressable(in, inBytes, device_, &dev)) ? dev : nullptr;
    };
    if (entry == kBusDevice) {
        if ((rc = lookupPair(busIn_, in, inBytes, busOut_, out, outBytes)) != 0) return rc;
        if (tapOut && (rc = lookup(tapRows_.checked, tapOut, tapBytes, kTapTexts.notAddressable)) != 0) return rc;
        if (auxOut && (rc = lookup(auxRows_.checked, auxOut, auxBytes, kAuxTexts.notAddressable)) != 0) return rc;
        if (tapOut && (rc = planSideRoute(tapRows_, kTapTexts, tapOut, tapRows_.checked.dev, rows, tapList_.size(), tapTotal_, tapPlace(), &tapRoute)) != 0) return rc;
        if (auxOut && (rc = planAuxRoute(auxOut, auxRows_.checked.dev, rows, pieceRows, &auxRoute)) != 0) return rc;
        if (feed && (rc = planFeedRoute(in, deviceSource(), rows, &feedRoute)) != 0) return rc;
        const float* dIn = static_cast<const float*>(busIn_.dev);
        float* dOut = static_cast<float*>(busOut_.dev);
        return runBus(dIn, dOut, dIn, shape.inPitch, dOut, shape.outPitch, nSamples, flags, shape, stream, tap, aux, fed);
    }
    // Host entry.  Pinned buffers: the bus kernels read the group words from and store the sums to the caller's memory over PCIe
    // (256 bytes per wavefront access), no copies.  Anything else: the [sample][channel][group] sides are staged.  Whatever
    // happens, nothing of the call may still touch the caller's memory when it returns.
    waitLastLaunch();
    // The tap rows take their own route, whichever the two sides take: stored in place where tap_out is pinned, else gathered into
    // a device block and copied out behind the block.  Everything that route needs is allocated here, in front of the first launch.
    if (tapOut) {
        if (!(knobs_.hostPipeline && addressable(tapOut, tapBytes, -1, &devTap))) devTap = nullptr;
        if ((rc = planSideRoute(tapRows_, kTapTexts, tapOut, devTap, rows, tapList_.size(), tapTotal_, tapPlace(), &tapRoute)) != 0) return rc;
    }
    // ... and the aux rows of the sends theirs, in the same way
    if (auxOut) {
        if (!(knobs_.hostPipeline && addressable(auxOut, auxBytes, -1, &devAux))) devAux = nullptr;
        if ((rc = planAuxRoute(auxOut, devAux, rows, pieceRows, &auxRoute)) != 0) return rc;
    }
    // ... and the source rows of the feeds: in place only where they are memory of this device
    if (feed && (rc = planFeedRoute(in, deviceSource(), rows, &feedRoute)) != 0) return rc;
    // the tail of both host paths behind runBus and the copies of the two sides (e: their result): the staged side rows on their
    // way out, the wait - also when the call failed -, the columns of a shard into their places
    auto finish = [&](int rc0, hipError_t e, const char* what) {
        if (rc0 == 0 && e == hipSuccess) e = queueSideCopyOut(tapRows_, tapRoute, tapOut, rows, stream_);
        if (rc0 == 0 && e == hipSuccess) e = queueSideCopyOut(auxRows_, auxRoute, auxOut, rows, stream_);
        const hipError_t se = hipStreamSynchronize(stream_);
        if (rc0 != 0) return rc0;
        if (e != hipSuccess || se != hipSuccess) return hipFail(e != hipSuccess ? e : se, what);
        placeSideColumns(tapRows_, tapRoute, tapOut, rows);
        placeSideColumns(auxRows_, auxRoute, auxOut, rows);
        return 0;
    };
    if (knobs_.hostPipeline && (feed || addressable(in, inBytes, -1, &devIn)) && addressable(out, outBytes, -1, &devOut)) {
        const float* dIn = static_cast<const float*>(devIn);   // (a feed block: the source rows go by feedRoute, not by this)
        float* dOut = static_cast<float*>(const_cast<void*>(devOut));
        rc = runBus(dIn, dOut, dIn, shape.inPitch, dOut, shape.outPitch, nSamples, flags, shape, stream_, tap, aux, fed);
        if ((rc = finish(rc, hipSuccess, "synchronising a bus block on pinned host buffers")) == 0) ++hostInplaceBlocks_;   // (blocks that were processed: a failed one is not counted)
        return rc;
    }
    const size_t side = rows * (size_t)shape.groups;
    const bool sharedIn = (flags & kBusSharedIn) != 0, mixOut = (flags & kBusMixOut) != 0;
    if ((rc = ensureBusStage(side * ((sharedIn ? 1 : 0) + (mixOut ? 1 : 0)))) != 0) return rc;
    float* stageIn = busStage_.p;
    float* stageOut = busStage_.p + (sharedIn ? side : 0);
    const size_t narrow = (size_t)shape.groups * 4;
    hipError_t e = hipSuccess;
    if (sharedIn) e = copyRows(stageIn, narrow, in, (size_t)shape.inPitch * 4, narrow, rows, hipMemcpyDefault, stream_);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream_);
        return hipFail(e, "bus H2D");
    }
    rc = runBus(in, out, stageIn, shape.groups, stageOut, shape.groups, nSamples, flags, shape, stream_, tap, aux, fed);
    if (rc == 0 && mixOut) e = copyRows(out, (size_t)shape.outPitch * 4, stageOut, narrow, narrow, rows, hipMemcpyDefault, stream_);
    if ((rc = finish(rc, e, "bus D2H")) == 0) ++hostStagedBlocks_;
    return rc;
}

// ---- instance-major blocks: one interleaved [sample][channel] stream per instance (fx_imajor.hpp) ---------------------------------
//
// The same sandwich as a bus block, on the same scratch: gather (a transposition of the n runs into [rows][n]) -> the ordinary
// launch in place -> scatter.  What crosses PCIe is each stream's run, once each way.

namespace {
// Do the runs of `in` and of `out` - n runs of `run` floats at their strides - share an element?  Not when one footprint ends
// before the other begins.  With one stride, run j of `out` lies d + (j - k) * stride floats behind run k of `in`: the distances
// nearest to zero are m = d mod stride and m - stride, so no two runs meet iff run <= m <= stride - run.  With two strides the
// runs of both, each in ascending order, are walked once.
bool imajorFootprintsApart(const float* in, const float* out, int64_t run, int64_t n, int64_t inStride, int64_t outStride) {
    const char *x = reinterpret_cast<const char*>(in), *y = reinterpret_cast<const char*>(out);
    const size_t inBytes = ((size_t)(n - 1) * (size_t)inStride + (size_t)run) * 4, outBytes = ((size_t)(n - 1) * (size_t)outStride + (size_t)run) * 4;
    if (x + inBytes <= y || y + outBytes <= x) return true;
    if (inStride == outStride) {
        const std::ptrdiff_t d = y - x;
        if (d % 4 != 0) return false;
        int64_t m = (int64_t)(d / 4) % inStride;
        if (m < 0) m += inStride;
        return m >= run && m <= inStride - run;
    }
    const size_t bytes = (size_t)run * 4;
    for (int64_t i = 0, j = 0; i < n && j < n;) {
        const char *a = x + (size_t)i * (size_t)inStride * 4, *b = y + (size_t)j * (size_t)outStride * 4;
        if (a + bytes <= b) ++i;
        else if (b + bytes <= a) ++j;
        else return false;
    }
    return true;
}
}  // namespace

int Batch::checkImajorShape(const float* in, const float* out, int nSamples, int channels, int64_t n, int64_t* inStride, int64_t* outStride, const char** why) {
    *why = nullptr;
    if (nSamples < 0) *why = "n_samples < 0";
    const int64_t run = (int64_t)std::max(nSamples, 0) * (int64_t)std::max(channels, 1);
    if (!*why && run >= ((int64_t)1 << 31)) *why = "instance-major block: n_samples * num_channels must stay below 2^31";
    if (!*why && (*inStride < 0 || *outStride < 0)) *why = "instance-major block: negative stride";
    if (*why) return FX_E_ARG;
    if (*inStride == 0) *inStride = run;
    if (*outStride == 0) *outStride = run;
    if (*inStride < run || *outStride < run) *why = "instance-major block: stride below n_samples * num_channels";
    else if (std::max(*inStride, *outStride) > (((int64_t)1 << 60) / std::max<int64_t>(n, 1))) *why = "instance-major block: stride too wide";
    else if (nSamples > 0 && (!in || !out)) *why = "null buffer";
    else if (nSamples > 0 && (in == out ? *inStride != *outStride : !imajorFootprintsApart(in, out, run, n, *inStride, *outStride)))
        *why = "instance-major block: input and output overlap without being one buffer with one stride";
    return *why ? FX_E_ARG : 0;
}

// The block itself, asynchronous on `stream`: in / out as the device addresses them.  Pieces as in runBus - consecutive sample
// ranges that fit the scratch, every piece gathering and scattering its sub-run of every stream; a piece is wholly gathered before
// anything of it is scattered and pieces are disjoint ranges, so in == out is safe.
int Batch::runImajor(const float* in, int64_t inStride, float* out, int64_t outStride, int nSamples, hipStream_t stream) {
    const size_t ch = (size_t)prog_.numChannels, perSample = ch * (size_t)n_;
    const int most = tracksArmed() ? nSamples : (int)std::min<size_t>((size_t)nSamples, std::max<size_t>(kBusScratchBytes / (perSample * 4), 1));
    const int pieces = (nSamples + most - 1) / most;
    int rc = ensureBusScratch((size_t)((nSamples + pieces - 1) / pieces) * perSample);
    if (rc != 0) return rc;
    hipStream_t s = pick(stream);
    // (the scratch is the bus blocks': whatever filled it last, on whatever stream, must have emptied it)
    if (busLaunched_) {
        const hipError_t we = hipStreamWaitEvent(s, evBus_, 0);
        if (we != hipSuccess) return hipFail(we, "instance-major block: waiting for the previous block on the scratch");
    }
    beginBlock(nSamples, pieces);   // ONE block to the bookkeeping of control changes and to the lowering
    if ((rc = ensureLowered()) != 0) return rc;
    auto lo = [&](int p) { return (int)((int64_t)nSamples * p / pieces); };
    for (int p = 0; p < pieces; ++p) {
        const int count = lo(p + 1) - lo(p);
        ImajorArgs a{};
        a.wide = bus_.p;
        a.first = (long long)lo(p) * (long long)ch;
        a.rows = (long long)count * (long long)ch;
        a.n = n_;
        a.in = in;
        a.stride = inStride;
        hipError_t e = launchImajorGather(a, s);
        if (e != hipSuccess) return hipFail(e, "instance-major block: filling the scratch block");
        if ((rc = launchBlock(bus_.p, bus_.p, count, s, n_, pieces > 1 ? kPiece : kWholeBlock)) != 0) {
            if (hipEventRecord(evBus_, s) == hipSuccess) busLaunched_ = true;   // (what has been queued still uses the scratch)
            return rc;
        }
        a.in = nullptr;
        a.out = out;
        a.stride = outStride;
        e = launchImajorScatter(a, s);
        if (e == hipSuccess) e = hipEventRecord(evBus_, s);
        if (e != hipSuccess) return hipFail(e, "instance-major block: emptying the scratch block");
        busLaunched_ = true;
    }
    ++imajorBlocks_;   // (blocks whose every piece was queued)
    return 0;
}

int Batch::processImajor(const float* in, float* out, int nSamples, int64_t inStride, int64_t outStride, BusEntry entry, hipStream_t stream) {
    (void)hipSetDevice(device_);
    const char* why = nullptr;
    int rc = checkImajorShape(in, out, nSamples, prog_.numChannels, n_, &inStride, &outStride, &why);
    if (rc != 0) return fail(rc, why);
    if (pcmStrideTooWide(prog_.numChannels, n_)) return fail(FX_E_ARG, "instance-major block: channels * instances * 4 must stay below 2^32");
    if (nSamples == 0) return ensureLowered();
    const size_t run = (size_t)nSamples * (size_t)prog_.numChannels;
    const size_t inBytes = ((size_t)(n_ - 1) * (size_t)inStride + run) * 4, outBytes = ((size_t)(n_ - 1) * (size_t)outStride + run) * 4;
    const void *devIn = nullptr, *devOut = nullptr;
    if (entry == kBusDevice) {
        if ((rc = lookupPair(imajorIn_, in, inBytes, imajorOut_, out, outBytes)) != 0) return rc;
        return runImajor(static_cast<const float*>(imajorIn_.dev), inStride, static_cast<float*>(imajorOut_.dev), outStride, nSamples, stream);
    }
    // Host entry.  Pinned buffers: the two kernels read the runs from and store them to the caller's memory over PCIe, no copies.
    // Anything else: the n runs are staged as rows of a 2-D copy, [n][run] in device memory, and transposed from there.  Whatever
    // happens, nothing of the call may still touch the caller's memory when it returns.
    waitLastLaunch();
    if (knobs_.hostPipeline && addressable(in, inBytes, -1, &devIn) && (static_cast<const void*>(out) == in ? (devOut = devIn, true) : addressable(out, outBytes, -1, &devOut))) {
        rc = runImajor(static_cast<const float*>(devIn), inStride, static_cast<float*>(const_cast<void*>(devOut)), outStride, nSamples, stream_);
        const hipError_t se = hipStreamSynchronize(stream_);
        if (rc != 0) return rc;
        if (se != hipSuccess) return hipFail(se, "synchronising an instance-major block on pinned host buffers");
        ++hostInplaceBlocks_;   // (blocks that were processed: a failed one is not counted)
        return 0;
    }
    // (one staging block serves both directions: a piece's sub-runs are scattered to where they were gathered from)
    if ((rc = ensureBusStage(run * (size_t)n_)) != 0) return rc;
    hipError_t e = copyRows(busStage_.p, run * 4, in, (size_t)inStride * 4, run * 4, (size_t)n_, hipMemcpyDefault, stream_);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream_);
        return hipFail(e, "instance-major H2D");
    }
    rc = runImajor(busStage_.p, (int64_t)run, busStage_.p, (int64_t)run, nSamples, stream_);
    if (rc == 0) e = copyRows(out, (size_t)outStride * 4, busStage_.p, run * 4, run * 4, (size_t)n_, hipMemcpyDefault, stream_);
    const hipError_t se = hipStreamSynchronize(stream_);
    if (rc != 0) return rc;
    if (e != hipSuccess || se != hipSuccess) return hipFail(e != hipSuccess ? e : se, "instance-major D2H");
    ++hostStagedBlocks_;
    return 0;
}

// Generate the code a stream of `nSamples`-sample blocks will run, now - a real-time caller does this after loading, before the
// stream starts, instead of paying for the translation in its first block.  wait: also until the builder thread has finished
// what it was asked for (the variant with the controls in rows, other stage counts on trial).
int Batch::prepare(int nSamples, bool wait) {
    (void)hipSetDevice(device_);
    if (nSamples < 1) return fail(FX_E_ARG, "prepare: n_samples >= 1");
    pendingSamples_ = nSamples;
    noteBlockLength(nSamples);
    int rc = ensureLowered();
    if (rc != 0) return rc;
    everLowered_ = true;
    leanStep();   // (controls have rows and some of them rest: their variant is asked for now)
    if (wait && builder_) {
        std::unique_lock<std::mutex> lock(builder_->mu);
        builder_->cv.wait(lock, [&] { return builder_->running.empty() && builder_->jobs.empty(); });
        lock.unlock();
        collectBuilt();
        leanStep();   // ... and in force when this returns
        rc = ensureLowered();
        if (rc != 0) return rc;
    }
    return 0;
}

int Batch::sync() {
    (void)hipSetDevice(device_);
    hipError_t e = hipStreamSynchronize(stream_);
    if (e == hipSuccess && launched_) e = hipEventSynchronize(ev1_);
    if (e == hipSuccess && busLaunched_) e = hipEventSynchronize(evBus_);   // (the last kernel of a bus block on the caller's stream)
    if (e == hipSuccess && instLaunched_ && (e = hipEventSynchronize(evInst_)) == hipSuccess) instLaunched_ = false;
    if (e == hipSuccess) listCopied_ = sideListCopied_ = false;   // (list sets run on the handle's stream, which has drained)
    return e == hipSuccess ? 0 : hipFail(e, "sync");
}

}  // namespace fx
