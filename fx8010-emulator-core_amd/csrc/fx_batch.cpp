// fx_batch.cpp — device state of one batch of instances: construction, load, state and delay-line allocation, registers, control
// tracks, snapshot, counters.
//
// Device-resident state (all instance-fastest so a wavefront touches contiguous 256-byte runs):
//   state  [rows][nPad] u32   one row per reference register (index = reference register index),
//                             then output latches, TRAM cursors, LFSR words, ood flags, counter
//   itram  [wave][iSlots][64] f32   reference smallDelayBuffer, include/FX8010.h:210
//   xtram  [wave][xSlots][64] f32   reference largeDelayBuffer, include/FX8010.h:211
//   lut    [64][65] f64             LOG tables 0..31, EXP tables 32..63
//   stream steady | last | row table
// Registers the decoder classifies as uniform live only in hostValue_ (and as immediates in the
// stream); their state rows are refreshed when they turn per-instance.
// The code cache, the builder thread and the lowering are in fx_batch_code.cpp; the path of a PCM block from the C ABI to the
// kernel launch is in fx_batch_io.cpp.
#include "fx_batch.hpp"

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "../../include/fx8010_amd.h"

namespace fx {

namespace {
const Luts& sharedLuts() {
    static const Luts l;
    return l;
}
constexpr size_t kScratchBytes = 1 << 16;
}  // namespace

Batch::Batch(int64_t nInstances, int channels, int device) : prog_(channels), knobs_(ReleaseKnobs::fromEnvironment()) {
    if (nInstances < 1) throw std::runtime_error("n_instances must be >= 1");
    if (channels < 1 || channels > kMaxChannels) throw std::runtime_error("num_channels must be 1..4");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        throw std::runtime_error(std::string("no usable HIP device (hipGetDeviceCount: ") + hipGetErrorString(e) + "); this library has no CPU fallback");
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= count) throw std::runtime_error("HIP device ordinal out of range");
    device_ = device;
    n_ = nInstances;
    nPad_ = (nInstances + 255) / 256 * 256;  // whole wavefronts for every K in {1,2,4}
    auto chk = [&](hipError_t r, const char* what) {
        if (r != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(r));
    };
    chk(hipSetDevice(device_), "hipSetDevice");
    chk(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    chk(hipEventCreate(&ev0_), "hipEventCreate");
    chk(hipEventCreate(&ev1_), "hipEventCreate");
    chk(hipMalloc(reinterpret_cast<void**>(&dLut_), sizeof(double) * kLutBlobDoubles), "hipMalloc lut");
    chk(hipMalloc(reinterpret_cast<void**>(&dScratch_), kScratchBytes), "hipMalloc scratch");
    static const LutDevice lutDev(sharedLuts());
    chk(hipMemcpy(dLut_, lutDev.blob.data(), sizeof(double) * kLutBlobDoubles, hipMemcpyHostToDevice), "lut upload");
}

Batch::~Batch() {
    (void)hipSetDevice(device_);
    drainBuilder(true);
    if (stream_) (void)hipStreamSynchronize(stream_);
    (void)hipFree(dState_);
    (void)hipFree(dITram_);
    (void)hipFree(dXTram_);
    (void)hipFree(dLut_);
    clearCodeCache();
    (void)hipFree(dScratch_);
    (void)hipFree(dTracks_);
    (void)hipFree(dQuietLeft_);
    (void)hipFree(dIn_);
    (void)hipFree(dOut_);
    freeBlock(bus_, false);
    freeBlock(busStage_, false);
    (void)hipFree(dMeter_);
    (void)hipFree(dTarget_);
    (void)hipFree(dMatch_);
    releaseMeterTarget();
    (void)hipFree(dLevel_);
    releaseMeterLevel();
    (void)hipFree(dTone_);
    releaseMeterTones();
    (void)hipFree(dGain_[0]);
    (void)hipFree(dGain_[1]);
    if (hGain_) (void)hipHostFree(hGain_);
    if (evGain_) (void)hipEventDestroy(evGain_);
    freeBlock(gainList_, false);
    freeBlock(hGainList_, true);
    if (evList_) (void)hipEventDestroy(evList_);
    (void)hipFree(tap_.cur);
    (void)hipFree(tap_.reserved);
    freeSideRows(tapRows_);
    (void)hipFree(sendBlock_.cur);
    (void)hipFree(sendBlock_.reserved);
    freeSendBlocks();
    (void)hipFree(feedBlock_.cur);
    (void)hipFree(feedBlock_.reserved);
    freeBlock(feedSrc_, false);
    freeBlock(instList_, false);
    freeBlock(instRec_, false);
    freeBlock(hInstList_, true);
    freeBlock(hInstRec_, true);
    freeBank();
    bankRelease();
    (void)hipFree(bankCells_);
    freeBlock(bankPairs_, false);
    freeBlock(regList_, false);
    freeBlock(hRegList_, true);
    freeBlock(tramStage_, false);
    freeBlock(hTramStage_, true);
    freeBlock(trackList_, false);
    freeBlock(hTrackList_, true);
    if (evTrackCopy_) (void)hipEventDestroy(evTrackCopy_);
    if (evTrackList_) (void)hipEventDestroy(evTrackList_);
    freeBlock(meterStage_, false);
    freeBlock(hMeterStage_, true);
    if (evInst_) (void)hipEventDestroy(evInst_);
    if (evBus_) (void)hipEventDestroy(evBus_);
#ifdef FX_DIAGNOSTICS
    (void)hipFree(dStamps_);
#endif
    if (hPinIn_) (void)hipHostFree(hPinIn_);
    if (hPinOut_) (void)hipHostFree(hPinOut_);
    for (int k = 0; k < kHostPieces; ++k) {
        if (evIn_[k]) (void)hipEventDestroy(evIn_[k]);
        if (evDone_[k]) (void)hipEventDestroy(evDone_[k]);
    }
    if (copyIn_) (void)hipStreamDestroy(copyIn_);
    if (copyOut_) (void)hipStreamDestroy(copyOut_);
    if (ev0_) (void)hipEventDestroy(ev0_);
    if (ev1_) (void)hipEventDestroy(ev1_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

// The caller's stream may be gone by the time we need the previous launch to have finished (a torch stream that was
// garbage-collected): wait on the event recorded behind that launch instead of holding the foreign handle.
void Batch::waitLastLaunch() {
    if (launched_) (void)hipEventSynchronize(ev1_);
    // (a bus block ends behind its emulation launch: the mix kernel, or the copy out of the scratch block)
    if (busLaunched_) (void)hipEventSynchronize(evBus_);
    // (a copy or a reset of instances queued behind it: once it has been waited for no later launch needs to)
    if (instLaunched_ && hipEventSynchronize(evInst_) == hipSuccess) instLaunched_ = false;
}

int Batch::fail(int code, const std::string& what) {
    lastError_ = what;
    return code;
}
int Batch::hipFail(hipError_t e, const char* where) {
    // The runtime also keeps the error as the calling thread's "last error", and the launch helpers of fx_kernel.hip report
    // hipGetLastError() after their kernel: an allocation that failed here would come back as the result of the next launch that
    // works (found by tests/test_gpu_boundary.py::test_delay_memory_that_cannot_be_allocated: fxb_ood_flags said ~0 after a
    // recovered out-of-memory).  It has been reported: clear it.
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? FX_E_MEMORY : FX_E_NODEVICE, std::string(where) + ": " + hipGetErrorString(e));
}

bool Batch::loadFile(const std::string& path) { drainBuilder(false); return afterLoad(prog_.loadFile(path)) == 1; }
bool Batch::loadText(const std::string& text) { drainBuilder(false); return afterLoad(prog_.loadText(text)) == 1; }

int Batch::setOption(unsigned option, bool on) {
    if (option & ~kOptAll) return -3;
    drainBuilder(false);
    prog_.options = on ? (prog_.options | option) : (prog_.options & ~option);
    lowDirty_ = true;
    return 0;
}

int Batch::afterLoad(bool ok) {
    (void)hipSetDevice(device_);
    if (dTarget_) (void)clearMeterTarget();   // a program load drops the target of the program that was
    if (dMeter_) (void)meterReset();          // ... resets the meters and keeps them enabled
    freeBank();                               // ... and frees the record bank: its slots hold records of the program that was
    // registers may have been created even when the load failed; keep host mirrors in step
    const size_t old = hostValue_.size();
    hostValue_.resize(prog_.regs.size());
    forcedLane_.resize(prog_.regs.size(), 0);
    laneWritten_.resize(prog_.regs.size(), 0);
    for (size_t r = old; r < prog_.regs.size(); ++r) hostValue_[r] = prog_.regs[r].value;
    lowDirty_ = true;
    // code generated for the program as it was is of no use any more (registers and instructions accumulate over loads)
    clearCodeCache();
    ++loadGen_;
    wantedClass_ = -1;
    otherClassBlocks_ = 0;
    for (Tuner& t : tune_) t = Tuner();
    // registers the program itself keeps per-instance (it writes them, reads them from a delay line or the PCM input): a
    // property of the program, valid until the next load
    intrinsicLane_.assign(prog_.regs.size(), 0);
    readByProgram_.assign(prog_.regs.size(), 0);
    declared_.assign(prog_.regs.size(), 0);
    for (const std::string& name : prog_.controls) {
        const int r = prog_.findRegister(name);
        if (r >= 0) declared_[(size_t)r] = 1;
    }
    hotControl_.assign(prog_.regs.size(), 0);   // (nothing has moved since THIS load)
    lastControlWrite_.assign(prog_.regs.size(), 0);
    coolAfter_.assign(prog_.regs.size(), kCoolSamples);
    cooledOnce_.assign(prog_.regs.size(), 0);
    leanActive_ = leanPending_ = false;
    leanStale_ = controlMode_;
    leanKey_.clear();
    leanFolded_.clear();
    leanWant_.clear();
    if (!prog_.instrs.empty()) {   // (also after a load that failed: its registers and instructions have been appended, as in the reference)
        const Lowered probe = lowerProgram(prog_, hostValue_, std::vector<uint8_t>(prog_.regs.size(), 0), 1, false, 1);
        for (size_t r = 0; r < probe.rowOfReg.size() && r < intrinsicLane_.size(); ++r) intrinsicLane_[r] = probe.rowOfReg[r] >= 0;
        for (const Instr& in : prog_.instrs)
            for (int o : {in.a, in.x, in.y})
                if (o >= 0 && (size_t)o < readByProgram_.size()) readByProgram_[(size_t)o] = 1;
    }
    // a load that failed after an earlier good one has still appended registers (literals and declarations are created
    // before the error, as in the reference): the state block must follow, or set_register of a new one would land in
    // the rows behind the registers (output latches, cursors, LFSR, counter)
    if (!ok) {
        if (dState_) (void)ensureState();
        return 0;
    }
    loaded_ = true;
    if (controlMode_) markControls();   // (a further load may have declared more controls)
    if (ensureState() != 0) return 0;
    return 1;
}

int Batch::fillRows(const std::vector<uint32_t>& rows, const std::vector<uint32_t>& values) {
    size_t done = 0;
    const size_t chunk = kScratchBytes / 8;
    while (done < rows.size()) {
        const size_t k = std::min(chunk, rows.size() - done);
        hipError_t e = hipMemcpyAsync(dScratch_, rows.data() + done, k * 4, hipMemcpyHostToDevice, stream_);
        if (e == hipSuccess) e = hipMemcpyAsync(dScratch_ + chunk, values.data() + done, k * 4, hipMemcpyHostToDevice, stream_);
        if (e == hipSuccess) e = launchFillRows(dState_, nPad_, dScratch_, dScratch_ + chunk, (int)k, stream_);
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);  // host vectors are pageable and reused
        if (e != hipSuccess) return hipFail(e, "fillRows");
        done += k;
    }
    return 0;
}

// Allocate the state block, or grow it when a further loadFile() added registers
// (the reference accumulates registers across loads, source/FX8010.cpp:777 ff.).
int Batch::ensureState() {
    const StateLayout want = makeLayout((int)prog_.regs.size(), prog_.numChannels);
    if (dState_ && want.totalRows == stateRows_) return 0;
    uint32_t* fresh = nullptr;
    const size_t rowBytes = (size_t)nPad_ * 4;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&fresh), rowBytes * want.totalRows);
    if (e != hipSuccess) return hipFail(e, "hipMalloc state");
    std::vector<uint32_t> rows, values;
    const uint32_t* old = dState_;
    const StateLayout was = stateLayout_;
    dState_ = fresh;
    int firstNew = 0;
    if (old) {
        waitLastLaunch();
        auto copyRow = [&](int dst, int src) {
            return hipMemcpyAsync(fresh + (size_t)dst * nPad_, old + (size_t)src * nPad_, rowBytes, hipMemcpyDeviceToDevice, stream_);
        };
        for (int r = 0; r < was.nRegs && e == hipSuccess; ++r) e = copyRow(r, r);
        const int specials = was.totalRows - was.outBase;
        for (int k = 0; k < specials && e == hipSuccess; ++k) e = copyRow(want.outBase + k, was.outBase + k);
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);
        (void)hipFree(const_cast<uint32_t*>(old));
        if (e != hipSuccess) return hipFail(e, "state grow");
        firstNew = was.nRegs;
    } else {
        // specials of a fresh batch: latches 0, cursors 0, reference LFSR seeds, flags 0, counter 0
        for (int k = want.outBase; k < want.totalRows; ++k) { rows.push_back(k); values.push_back(0); }
        values[want.noiseBase - want.outBase + 0] = 0x70f4f854u;  // g_x1, include/FX8010.h:290
        values[want.noiseBase - want.outBase + 1] = 0xe1e9f0a7u;  // g_x2, include/FX8010.h:291
    }
    for (int r = firstNew; r < want.nRegs; ++r) { rows.push_back(r); values.push_back(bitsOf(hostValue_[r])); }
    stateLayout_ = want;
    stateRows_ = want.totalRows;
    return fillRows(rows, values);
}

int Batch::ensureTram(const Lowered& low) {
    auto grow = [&](float*& buf, int& have, int want) -> int {
        if (want <= have) return 0;
        size_t waves = (size_t)((n_ + 64 * instPerLane_ - 1) / (64 * instPerLane_));
        const size_t pitch = 256 * (size_t)instPerLane_;  // bytes of one slot of one wavefront
        float* fresh = nullptr;
        const size_t bytes = waves * (size_t)want * pitch;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&fresh), bytes);
        if (e != hipSuccess) return hipFail(e, "hipMalloc TRAM");
        e = hipMemsetAsync(fresh, 0, bytes, stream_);  // the parity domain assumes zeroed delay memory
        if (e == hipSuccess && buf && have > 0) {
            waitLastLaunch();
            e = copyRows(fresh, (size_t)want * pitch, buf, (size_t)have * pitch, (size_t)have * pitch, waves, hipMemcpyDeviceToDevice, stream_);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);
        if (e != hipSuccess) { (void)hipFree(fresh); return hipFail(e, "TRAM init"); }
        (void)hipFree(buf);
        buf = fresh;
        have = want;
        return 0;
    };
    int rc = grow(dITram_, iSlotsAlloc_, low.iSlots);
    if (rc == 0) rc = grow(dXTram_, xSlotsAlloc_, low.xSlots);
    // which position kinds the program has an instruction of, per line (ringLine: the rule of fxb_load_instances_rotated)
    for (int which = 0; which < 2; ++which) tramWrites_[which] = tramReads_[which] = false;
    for (const Instr& I : prog_.instrs) {
        if (I.op != IDELAY && I.op != XDELAY) continue;
        const int which = I.op == XDELAY ? 1 : 0;
        if (prog_.regs[(size_t)I.r].type == R_WRITE) tramWrites_[which] = true;
        if (prog_.regs[(size_t)I.r].type == R_READ) tramReads_[which] = true;
    }
    return rc;
}

// K = instances stepped by one lane.  More instances per lane amortise the scalar fetch/dispatch of
// a record over more work and widen every LDS access, but shrink the number of wavefronts; the LDS
// register file (rows * 256 * K bytes per wavefront) bounds how many wavefronts a CU can hold.
// Once TRAM has been allocated its [wave][slot][64][K] tiling pins K for the life of the batch.
int Batch::chooseInstPerLane() const {
    if (iSlotsAlloc_ > 0 || xSlotsAlloc_ > 0) return instPerLane_;
    if (knobs_.instPerLane) return knobs_.instPerLane;
    const Lowered probe = lowerProgram(prog_, hostValue_, laneForced(), 1);
    if (!probe.error.empty()) return 1;
    for (int k : {4, 2}) {
        const long long waves = (n_ + 64LL * k - 1) / (64LL * k);
        const long long perCu = kLdsBytesPerCU / ((long long)probe.nRows * 256 * k);
        if (waves >= 2048 && perCu >= 4) return k;  // >= 2 wavefronts per SIMD in flight and one per SIMD resident
    }
    return 1;
}

bool Batch::intrinsicLane(int reg) const { return reg >= 0 && (size_t)reg < intrinsicLane_.size() && intrinsicLane_[reg] != 0; }

bool Batch::laneResident(int reg) const {
    if ((reg < (int)forcedLane_.size() && (forcedLane_[reg] || laneWritten_[reg])) || tracked(reg)) return true;
    return !lowDirty_ ? c_.low.rowOfReg[reg] >= 0 : (reg < (int)c_.low.rowOfReg.size() && c_.low.rowOfReg[reg] >= 0);
}

// A register whose value is compiled into the instruction stream (a literal of the generated code, an immediate of a record)
// and that the caller changes AFTER the program has run is a moving control - the reference's setRegisterValue is a store
// (source/FX8010.cpp:236-253), called every 8 samples by its harness (source/main.cpp:107-114).  Such a register is given a
// row of the register file, once: the code then reads it as a VGPR operand, and every later change is a fill of that row -
// no re-lowering, no re-translation.  Not for the few operand positions that shape the code itself: a LOG / EXP table
// number, a SKIP's condition or count, a delay-line offset (those keep being compiled in).
bool Batch::movableControl(int r) const {
    for (const Instr& in : prog_.instrs) {
        if ((in.op == LOG || in.op == EXP) && in.x == r) return false;
        if (in.op == SKIP && (in.x == r || in.y == r)) return false;
        if ((in.op == IDELAY || in.op == XDELAY) && in.y == r) return false;
    }
    return true;
}

// Every declared control (`control name = v`, the reference's control list, source/FX8010.cpp:408-411) that an instruction reads
// as a plain operand gets its row - all of them at the first touch of any: a host that moves one slider moves others (a preset
// recall writes the whole panel), and one change of code for the panel is one stall at most - none when the variant was built
// ahead (prebuildControlVariant).  Registers no instruction reads never get a row: their value cannot reach the code.
void Batch::markControls() {
    for (const std::string& name : prog_.controls) {
        const int r = prog_.findRegister(name);
        if (r < 0 || forcedLane_[(size_t)r] || intrinsicLane(r) || !readByProgram(r) || !movableControl(r)) continue;
        // (not noteRegisterWritten: nothing has been written - the row is for company, laneWritten_ stays)
        forcedLane_[(size_t)r] = 1;
        lowDirty_ = true;
    }
}

bool Batch::readByProgram(int reg) const { return reg >= 0 && (size_t)reg < readByProgram_.size() && readByProgram_[(size_t)reg] != 0; }

bool Batch::declaredControl(int reg) const { return reg >= 0 && (size_t)reg < declared_.size() && declared_[(size_t)reg] != 0; }

int Batch::setRegister(const std::string& key, float v) {
    (void)hipSetDevice(device_);
    const int r = prog_.findRegister(key);
    if (r < 0) return 1;
    hostValue_[r] = v;
    if (tracked(r) || intrinsicLane(r)) {
        // the register lives in a row whatever the host does (a schedule, or the program writes it): the fill below is all there is to do
    } else if (forcedLane_[r]) {
        if (controlMode_ && declaredControl(r)) controlWritten(r);   // (a control that had its row for company starts moving itself: lean code with its value folded in goes)
        // a row from an earlier write.  One that only per-instance writes asked for is given back now that every instance holds
        // the same value again (the register file does not grow with every register a host has ever touched) - unless it is a
        // moving control, whose next change should stay a fill
        if (laneWritten_[r] && !(controlMode_ && declaredControl(r)) ) {
            forcedLane_[r] = 0;
            lowDirty_ = true;
        }
    } else if (!readByProgram(r)) {
        // no instruction reads it: the value lives in the state row (get_register) and nowhere in the code
    } else if (loaded_ && everLowered_ && movableControl(r)) {
        // a moving control: a row from now on - and with it the other declared controls (one change of code for the panel)
        if (declaredControl(r)) {
            controlMode_ = true;
            markControls();
            coldSetChanged();
            controlWritten(r);
        }
        forcedLane_[r] = 1;
        lowDirty_ = true;
    } else {
        lowDirty_ = true;    // immediates (and possibly the classification) change
        if (loaded_ && everLowered_) controlHeat_ = kHeatPerChange;
    }
    laneWritten_[r] = 0;
    if (dState_) {
        // Invariant: the state row of EVERY register holds its current value for every instance, also while the
        // register is uniform (folded into the code) - so that a later per-instance write only has to force the
        // register per-lane, whatever the lowering in force says about it.
        waitLastLaunch();
        int rc = fillRows({(uint32_t)r}, {bitsOf(v)});
        if (rc != 0) return rc;
    }
    return 0;
}

int Batch::setRegisterAt(const std::string& key, int64_t inst, float v) {
    (void)hipSetDevice(device_);
    const int r = prog_.findRegister(key);
    if (r < 0) return 1;
    if (inst < 0 || inst >= n_) return fail(FX_E_ARG, "instance out of range");
    if (!dState_) return fail(FX_E_NOTREADY, "no program loaded");
    waitLastLaunch();
    if (coldControl(r)) coldSetChanged();
    if (!forcedLane_[r] && !intrinsicLane(r) && readByProgram(r)) {  // (the row is valid, see setRegister; the next lowering keeps the register per-lane)
        forcedLane_[r] = 1;
        lowDirty_ = true;
    }
    laneWritten_[r] = 1;
    hipError_t e = hipMemcpy(dState_ + (size_t)r * nPad_ + inst, &v, 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hipFail(e, "setRegisterAt");
    return 0;
}

int Batch::setRegisterArray(const std::string& key, const float* values) {
    (void)hipSetDevice(device_);
    const int r = prog_.findRegister(key);
    if (r < 0) return 1;
    if (!values) return fail(FX_E_ARG, "null buffer");
    if (!dState_) return fail(FX_E_NOTREADY, "no program loaded");
    waitLastLaunch();
    if (coldControl(r)) coldSetChanged();
    if (!forcedLane_[r] && !intrinsicLane(r) && readByProgram(r)) {  // from now on a per-instance row (every lane is overwritten below)
        forcedLane_[r] = 1;
        lowDirty_ = true;
    }
    laneWritten_[r] = 1;
    hipError_t e = hipMemcpy(dState_ + (size_t)r * nPad_, values, sizeof(float) * (size_t)n_, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hipFail(e, "setRegisterArray");
    return 0;
}

int Batch::getRegisterArray(const std::string& key, float* values) {
    (void)hipSetDevice(device_);
    const int r = prog_.findRegister(key);
    if (r < 0) return 1;
    if (!values) return fail(FX_E_ARG, "null buffer");
    if (!dState_ || !laneResident(r)) {
        for (int64_t i = 0; i < n_; ++i) values[i] = hostValue_[r];
        return 0;
    }
    waitLastLaunch();
    hipError_t e = hipMemcpy(values, dState_ + (size_t)r * nPad_, sizeof(float) * (size_t)n_, hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : hipFail(e, "getRegisterArray");
}

float Batch::getRegisterAt(const std::string& key, int64_t inst) {
    (void)hipSetDevice(device_);
    const int r = prog_.findRegister(key);
    if (r < 0) return 1.0f;  // reference getRegisterValue default, source/FX8010.cpp:265
    if (inst < 0 || inst >= n_ || !dState_ || !laneResident(r)) return hostValue_[r];
    waitLastLaunch();
    float v = 0.0f;
    if (hipMemcpy(&v, dState_ + (size_t)r * nPad_ + inst, 4, hipMemcpyDeviceToHost) != hipSuccess) return hostValue_[r];
    return v;
}

int Batch::seedNoiseAt(int64_t inst, int32_t x1, int32_t x2) {
    (void)hipSetDevice(device_);
    if (inst < 0 || inst >= n_) return fail(FX_E_ARG, "instance out of range");
    if (!dState_) return fail(FX_E_NOTREADY, "no program loaded");
    waitLastLaunch();
    hipError_t e = hipMemcpy(dState_ + (size_t)(stateLayout_.noiseBase + 0) * nPad_ + inst, &x1, 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dState_ + (size_t)(stateLayout_.noiseBase + 1) * nPad_ + inst, &x2, 4, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : hipFail(e, "seedNoiseAt");
}

bool Batch::tracked(int reg) const { return std::find(trackRegs_.begin(), trackRegs_.end(), reg) != trackRegs_.end(); }

std::vector<uint8_t> Batch::laneForcedFull() const {
    std::vector<uint8_t> f = forcedLane_;
    for (int reg : trackRegs_)
        if ((size_t)reg < f.size()) f[(size_t)reg] = 1;
    return f;
}

int Batch::setRegisterTrack(const std::string& key, const float* values, int nSteps, int period, bool perInstance, int64_t pitch) {
    (void)hipSetDevice(device_);
    const int r = prog_.findRegister(key);
    if (r < 0) return 1;
    if (!values || nSteps < 1 || period < 1) return fail(FX_E_ARG, "track: values, n_steps >= 1 and period >= 1 are required");
    if (!dState_) return fail(FX_E_NOTREADY, "no program loaded");
    if (pitch <= 0) pitch = n_;
    if (perInstance && pitch < n_) return fail(FX_E_ARG, "track: pitch below the instance count");
    if (listScheduled(r)) return fail(FX_E_ARG, "track: register '" + key + "' has list schedules armed (set_register_tracks_list)");
    size_t slot = 0;
    while (slot < trackRegs_.size() && trackRegs_[slot] != r) ++slot;
    if (slot == trackRegs_.size()) {
        if (trackRegs_.size() >= (size_t)kMaxTracks) return fail(FX_E_ARG, "track: at most " + std::to_string(kMaxTracks) + " registers can have schedules");
        coldSetChanged();
        trackRegs_.push_back(r);
        pendingTracks_.resize(trackRegs_.size());
        lowDirty_ = true;  // the register gets a row of its own and the generated loop the code to re-load it
    }
    PendingTrack& t = pendingTracks_[slot];
    t.period = period;
    t.steps = nSteps;
    t.perInstance = perInstance;
    if (perInstance) {
        t.values.resize((size_t)nSteps * (size_t)n_);
        for (int k = 0; k < nSteps; ++k) std::memcpy(&t.values[(size_t)k * (size_t)n_], values + (size_t)k * (size_t)pitch, (size_t)n_ * 4);
    } else {
        t.values.assign(values, values + nSteps);
    }
    return 0;
}

// the events of the armed schedules, sorted by sample, and their values -> dTracks_ (on the launch stream, ahead of the kernel);
// the schedules are one-shot.  A register with list schedules (fx_batch_tracks.cpp) contributes the sorted union of the samples
// at which its schedules have a step inside the block; each of those events owns a row of nPad words BEHIND the part of the
// buffer that the host image covers - the header copy does not touch them, the device fills them (expandTrackLists).  The host
// image ends with the ranges of fx_track_scatter: per schedule, one per step inside the block and key.
int Batch::uploadTracks(int nSamples, hipStream_t s) {
    if (!tracksArmed() && tracksClear_ && dTracks_) return 0;  // nothing armed and the device list already says so
    struct Due { uint32_t sample, slot, step; int64_t row; };   // row >= 0: an event of a list-armed register, its row
    std::vector<Due> due;
    std::vector<int> used(pendingTracks_.size(), 0);
    size_t valueWords = 0;
    // list schedules: the events of every register, its first row, the rows in all
    std::vector<std::vector<int>> listEvents(trackRegs_.size());
    for (const ListSchedule& sch : listSchedules_) {
        if (sch.list.empty()) continue;
        const int inside = sch.stepsInside(nSamples);
        for (const int slot : sch.slots)
            for (int q = 0; q < inside; ++q) listEvents[(size_t)slot].push_back(sch.first + q * sch.period);
    }
    std::vector<size_t> firstRow(trackRegs_.size(), 0);
    ListExpansion x;
    for (size_t k = 0; k < listEvents.size(); ++k) {
        std::vector<int>& ev = listEvents[k];
        std::sort(ev.begin(), ev.end());
        ev.erase(std::unique(ev.begin(), ev.end()), ev.end());
        firstRow[k] = x.totalRows;
        if (ev.empty()) continue;
        x.hold.stateRow[x.hold.nRegs] = trackRegs_[k];   // (a register's row is its number: StateLayout)
        x.hold.firstRow[x.hold.nRegs] = (int)x.totalRows;
        x.hold.rowCount[x.hold.nRegs] = (int)ev.size();
        ++x.hold.nRegs;
        x.totalRows += ev.size();
    }
    for (size_t k = 0; k < pendingTracks_.size(); ++k) {
        const PendingTrack& t = pendingTracks_[k];
        for (size_t e = 0; e < listEvents[k].size(); ++e) due.push_back({(uint32_t)listEvents[k][e], (uint32_t)k, 0u, (int64_t)(firstRow[k] + e)});
        if (t.steps <= 0) continue;
        used[k] = std::min(t.steps, (nSamples + t.period - 1) / t.period);  // changes that fall inside this block
        for (int q = 0; q < used[k]; ++q) due.push_back({(uint32_t)q * (uint32_t)t.period, (uint32_t)k, (uint32_t)q, -1});
        valueWords += t.perInstance ? (size_t)used[k] * (size_t)nPad_ : (size_t)used[k];
    }
    std::stable_sort(due.begin(), due.end(), [](const Due& a, const Due& b) { return a.sample < b.sample; });  // (same sample: by slot, as armed)
    // the ranges: a step runs from its own event up to the same schedule's next one, the last step inside to the register's last event
    std::vector<TrackRange> ranges;
    for (size_t j = 0; j < listSchedules_.size(); ++j) {
        const ListSchedule& sch = listSchedules_[j];
        const int inside = sch.list.empty() ? 0 : sch.stepsInside(nSamples);
        if (inside == 0) continue;
        x.launches.push_back({j, ranges.size(), inside * (int)sch.regs.size()});
        for (int q = 0; q < inside; ++q)
            for (size_t k = 0; k < sch.regs.size(); ++k) {
                const size_t slot = (size_t)sch.slots[k];
                const std::vector<int>& ev = listEvents[slot];
                const size_t lo = (size_t)(std::lower_bound(ev.begin(), ev.end(), sch.first + q * sch.period) - ev.begin());
                const size_t hi = q + 1 < inside ? (size_t)(std::lower_bound(ev.begin(), ev.end(), sch.first + (q + 1) * sch.period) - ev.begin()) : ev.size();
                ranges.push_back({q * (int)sch.regs.size() + (int)k, (int)(firstRow[slot] + lo), (int)(firstRow[slot] + hi), 0});
            }
    }
    static_assert(sizeof(TrackRange) == 16, "TrackRange layout");
    const size_t listWords = (due.size() + 1) * 4;
    const size_t rangesAt = (listWords + valueWords + 3) & ~(size_t)3;
    const size_t words = rangesAt + ranges.size() * 4;   // the host image; a multiple of 4: the rows behind it are 16-byte aligned
    const size_t bytes = (words + x.totalRows * (size_t)nPad_) * 4;
    if (x.totalRows > 0 && bytes >= ((size_t)1 << 32)) return fail(FX_E_MEMORY, "tracks: the event rows of this block would pass 4 GiB");
    if (bytes > tracksCap_) {
        waitLastLaunch();
        (void)hipFree(dTracks_);
        dTracks_ = nullptr;
        tracksCap_ = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&dTracks_), bytes + 256);
        if (e != hipSuccess) return hipFail(e, "hipMalloc tracks");
        tracksCap_ = bytes + 256;
    }
    waitLastLaunch();  // trackStage_ / dTracks_ of the previous block are free again
    trackStage_.assign(words, 0);
    std::vector<size_t> valuesAt(pendingTracks_.size(), 0);
    size_t at = listWords;
    for (size_t k = 0; k < pendingTracks_.size(); ++k) {
        PendingTrack& t = pendingTracks_[k];
        const int reg = trackRegs_[k];
        if (!listEvents[k].empty()) {   // (as a per-instance track)
            forcedLane_[(size_t)reg] = 1;
            laneWritten_[(size_t)reg] = 1;
        }
        if (t.steps <= 0) continue;
        valuesAt[k] = at;
        if (t.perInstance) {
            for (int q = 0; q < used[k]; ++q) std::memcpy(&trackStage_[at + (size_t)q * (size_t)nPad_], &t.values[(size_t)q * (size_t)n_], (size_t)n_ * 4);
            at += (size_t)used[k] * (size_t)nPad_;
            forcedLane_[(size_t)reg] = 1;
            laneWritten_[(size_t)reg] = 1;
        } else {
            std::memcpy(&trackStage_[at], t.values.data(), (size_t)used[k] * 4);
            at += (size_t)used[k];
            hostValue_[(size_t)reg] = t.values[(size_t)used[k] - 1];  // what every instance holds after the block
            forcedLane_[(size_t)reg] = 0;
            laneWritten_[(size_t)reg] = 0;
        }
    }
    for (size_t i = 0; i < due.size(); ++i) {
        const Due& d = due[i];
        const PendingTrack& t = pendingTracks_[d.slot];
        const bool row = d.row >= 0 || t.perInstance;
        const size_t value = d.row >= 0 ? words + (size_t)d.row * (size_t)nPad_ : valuesAt[d.slot] + (t.perInstance ? (size_t)d.step * (size_t)nPad_ : (size_t)d.step);
        const TrackEvent ev{d.sample, d.slot, (uint32_t)(value * 4), row ? (uint32_t)(nPad_ * 4) : 4u};
        std::memcpy(&trackStage_[i * 4], &ev, sizeof(ev));
    }
    const TrackEvent closing{0xffffffffu, 0, 0, 4};
    std::memcpy(&trackStage_[due.size() * 4], &closing, sizeof(closing));
    if (!ranges.empty()) std::memcpy(&trackStage_[rangesAt], ranges.data(), ranges.size() * sizeof(TrackRange));
    for (PendingTrack& t : pendingTracks_) {
        t.steps = 0;
        t.values.clear();
    }
    tracksClear_ = due.empty();
    hipError_t e = hipMemcpyAsync(dTracks_, trackStage_.data(), words * 4, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        (void)finishTrackLists(s, false);
        return hipFail(e, "tracks upload");
    }
    x.rowsAt = words;
    for (ListExpansion::Launch& l : x.launches) l.rangesAt = rangesAt + l.rangesAt * 4;   // (ranges -> words of the buffer)
    const int rc = expandTrackLists(x, s);
    const int rc2 = finishTrackLists(s, rc == 0 && x.totalRows > 0);
    return rc != 0 ? rc : rc2;
}

// ---- state snapshot ------------------------------------------------------------------------------------------------------------
int Batch::snapshotShape(SnapshotHeader* hdr) {
    (void)hipSetDevice(device_);
    int rc = ensureLowered();
    if (rc != 0) return rc;
    *hdr = SnapshotHeader();
    hdr->n = n_;
    hdr->channels = prog_.numChannels;
    hdr->nRegs = (int32_t)prog_.regs.size();
    hdr->stateRows = stateRows_;
    hdr->iSlots = iSlotsAlloc_;
    hdr->xSlots = xSlotsAlloc_;
    return 0;
}

namespace {
// delay memory on the device: [wave][slot][64 * K] (K instances per lane: the HIP C++ tier), an instance i at
// wave i / (64 K), column i % (64 K); in an image: [instance][slot]
constexpr size_t kTramChunkBytes = (size_t)64 << 20;
}

int Batch::saveStateColumns(uint8_t* image, const SnapshotHeader& hdr, int64_t first) {
    (void)hipSetDevice(device_);
    if (!image || first < 0 || first + n_ > hdr.n) return fail(FX_E_ARG, "snapshot: bad image");
    SnapshotHeader mine;
    int rc = snapshotShape(&mine);
    if (rc != 0) return rc;
    if (mine.channels != hdr.channels || mine.nRegs != hdr.nRegs || mine.stateRows != hdr.stateRows || mine.iSlots != hdr.iSlots || mine.xSlots != hdr.xSlots)
        return fail(FX_E_ARG, "snapshot: the image was laid out for another program");
    waitLastLaunch();
    hipError_t e = hipStreamSynchronize(stream_);
    uint8_t* rows = image + sizeof(SnapshotHeader);
    if (e == hipSuccess)
        e = hipMemcpy2D(rows + (size_t)first * 4, (size_t)hdr.n * 4, dState_, (size_t)nPad_ * 4, (size_t)n_ * 4, (size_t)stateRows_, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hipFail(e, "snapshot: state rows");
    uint8_t* sec = rows + (size_t)hdr.stateRows * (size_t)hdr.n * 4;
    for (int which = 0; which < 2; ++which) {
        const float* dev = which ? dXTram_ : dITram_;
        const int slots = which ? xSlotsAlloc_ : iSlotsAlloc_;
        float* out = reinterpret_cast<float*>(sec);
        sec += (size_t)hdr.n * (size_t)slots * 4;
        if (slots == 0) continue;
        const size_t cols = 64 * (size_t)instPerLane_, waveFloats = (size_t)slots * cols;
        const size_t waves = ((size_t)n_ + cols - 1) / cols, chunk = std::max<size_t>(1, kTramChunkBytes / (waveFloats * 4));
        std::vector<float> tmp(std::min(waves, chunk) * waveFloats);
        for (size_t w0 = 0; w0 < waves; w0 += chunk) {
            const size_t nw = std::min(chunk, waves - w0);
            e = hipMemcpy(tmp.data(), dev + w0 * waveFloats, nw * waveFloats * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return hipFail(e, "snapshot: delay memory");
            for (size_t w = 0; w < nw; ++w)
                for (size_t j = 0; j < cols; ++j) {
                    const size_t inst = (w0 + w) * cols + j;
                    if (inst >= (size_t)n_) break;
                    float* line = out + ((size_t)first + inst) * (size_t)slots;
                    const float* src = tmp.data() + w * waveFloats + j;
                    for (int s = 0; s < slots; ++s) line[s] = src[(size_t)s * cols];
                }
        }
    }
    return 0;
}

int Batch::loadStateColumns(const uint8_t* image, const SnapshotHeader& hdr, int64_t first) {
    (void)hipSetDevice(device_);
    if (!image || first < 0 || first + n_ > hdr.n) return fail(FX_E_ARG, "snapshot: bad image");
    SnapshotHeader mine;
    int rc = snapshotShape(&mine);
    if (rc != 0) return rc;
    if (hdr.magic != mine.magic || hdr.version != mine.version) return fail(FX_E_ARG, "snapshot: not a state image of this library version");
    // (every field is checked before any of them enters an address: the image may be a damaged file)
    if (hdr.iSlots < 0 || hdr.xSlots < 0 || hdr.n < n_ || mine.channels != hdr.channels || mine.nRegs != hdr.nRegs || mine.stateRows != hdr.stateRows ||
        hdr.iSlots > mine.iSlots || hdr.xSlots > mine.xSlots)
        return fail(FX_E_ARG, "snapshot: the image is of another program (registers, channels or delay lines differ)");
    waitLastLaunch();
    hipError_t e = hipStreamSynchronize(stream_);
    const uint8_t* rows = image + sizeof(SnapshotHeader);
    if (e == hipSuccess)
        e = hipMemcpy2D(dState_, (size_t)nPad_ * 4, rows + (size_t)first * 4, (size_t)hdr.n * 4, (size_t)n_ * 4, (size_t)stateRows_, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hipFail(e, "snapshot: state rows");
    // what the host knows about the registers follows the image: a register every instance holds the same value of is a
    // broadcast write of that value, any other one a per-instance write (as if the caller had made them)
    coldSetChanged();
    for (int r = 0; r < hdr.nRegs; ++r) {
        if (tracked(r) || intrinsicLane(r)) continue;
        const uint32_t* row = reinterpret_cast<const uint32_t*>(rows + ((size_t)r * (size_t)hdr.n + (size_t)first) * 4);
        bool same = true;
        for (int64_t i = 1; i < n_ && same; ++i) same = row[i] == row[0];
        float v;
        std::memcpy(&v, &row[0], 4);
        if (same) {
            const bool moved = bitsOf(hostValue_[(size_t)r]) != row[0];
            hostValue_[(size_t)r] = v;
            if (forcedLane_[(size_t)r]) {
                if (laneWritten_[(size_t)r] && !(controlMode_ && declaredControl(r))) { forcedLane_[(size_t)r] = 0; lowDirty_ = true; }
            } else if (moved && readByProgram(r)) {
                lowDirty_ = true;   // (compiled in: the next block is generated with the image's value - loading a snapshot is not the audio path)
            }
            laneWritten_[(size_t)r] = 0;
        } else {
            // (not noteRegisterWritten: the cold set has been marked changed once, above, for the whole image)
            if (!forcedLane_[(size_t)r] && readByProgram(r)) { forcedLane_[(size_t)r] = 1; lowDirty_ = true; }
            laneWritten_[(size_t)r] = 1;
        }
    }
    const uint8_t* sec = rows + (size_t)hdr.stateRows * (size_t)hdr.n * 4;
    for (int which = 0; which < 2; ++which) {
        float* dev = which ? dXTram_ : dITram_;
        const int alloc = which ? xSlotsAlloc_ : iSlotsAlloc_, slots = which ? hdr.xSlots : hdr.iSlots;
        const float* in = reinterpret_cast<const float*>(sec);
        sec += (size_t)hdr.n * (size_t)slots * 4;
        if (alloc == 0) continue;
        const size_t cols = 64 * (size_t)instPerLane_, waveFloats = (size_t)alloc * cols;
        const size_t waves = ((size_t)n_ + cols - 1) / cols, chunk = std::max<size_t>(1, kTramChunkBytes / (waveFloats * 4));
        std::vector<float> tmp(std::min(waves, chunk) * waveFloats);
        for (size_t w0 = 0; w0 < waves; w0 += chunk) {
            const size_t nw = std::min(chunk, waves - w0);
            std::fill(tmp.begin(), tmp.begin() + (long)(nw * waveFloats), 0.0f);
            for (size_t w = 0; w < nw; ++w)
                for (size_t j = 0; j < cols; ++j) {
                    const size_t inst = (w0 + w) * cols + j;
                    if (inst >= (size_t)n_) break;
                    const float* line = in + ((size_t)first + inst) * (size_t)slots;
                    float* dst = tmp.data() + w * waveFloats + j;
                    for (int s = 0; s < slots; ++s) dst[(size_t)s * cols] = line[s];
                }
            e = hipMemcpy(dev + w0 * waveFloats, tmp.data(), nw * waveFloats * 4, hipMemcpyHostToDevice);
            if (e != hipSuccess) return hipFail(e, "snapshot: delay memory");
        }
    }
    return 0;
}

int Batch::getTramAt(int which, int64_t inst, float* out, int nSlots) {
    (void)hipSetDevice(device_);
    if (inst < 0 || inst >= n_ || !out || nSlots < 0 || which < 0 || which > 1) return fail(FX_E_ARG, "get_tram: bad argument");
    int rc = ensureLowered();
    if (rc != 0) return rc;
    waitLastLaunch();
    const float* dev = which ? dXTram_ : dITram_;
    const int alloc = which ? xSlotsAlloc_ : iSlotsAlloc_;
    for (int s = 0; s < nSlots; ++s) out[s] = 0.0f;   // (slots the program cannot reach are not allocated: zero, as in a fresh reference object)
    const int take = std::min(nSlots, alloc);
    if (take <= 0) return 0;
    const size_t cols = 64 * (size_t)instPerLane_;
    const float* src = dev + ((size_t)inst / cols) * (size_t)alloc * cols + (size_t)inst % cols;
    hipError_t e = hipMemcpy2D(out, 4, src, cols * 4, 4, (size_t)take, hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : hipFail(e, "get_tram");
}

int Batch::getCursorsAt(int64_t inst, int32_t out4[4]) {
    (void)hipSetDevice(device_);
    if (inst < 0 || inst >= n_ || !out4 || !dState_) return fail(FX_E_ARG, "get_cursors: bad argument");
    waitLastLaunch();
    hipError_t e = hipMemcpy2D(out4, 4, dState_ + (size_t)stateLayout_.cursorBase * nPad_ + inst, (size_t)nPad_ * 4, 4, 4, hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : hipFail(e, "get_cursors");
}

int64_t Batch::instructionCounter() {
    (void)hipSetDevice(device_);
    if (!dState_) return 0;
    waitLastLaunch();
    unsigned long long zero[2] = {0, 0};
    unsigned long long* dSum = reinterpret_cast<unsigned long long*>(dScratch_);
    uint32_t* dOr = dScratch_ + 2;
    if (hipMemcpy(dSum, zero, 16, hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (launchReduceRow(dState_, nPad_, n_, stateLayout_.countLo, stateLayout_.countHi, stateLayout_.oodRow, dSum, dOr, stream_) != hipSuccess) return -1;
    if (hipStreamSynchronize(stream_) != hipSuccess) return -1;
    unsigned long long res[2] = {0, 0};
    if (hipMemcpy(res, dSum, 16, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)res[0];
}

uint32_t Batch::oodFlags() {
    (void)hipSetDevice(device_);
    if (!dState_) return 0;
    waitLastLaunch();
    unsigned long long zero[2] = {0, 0};
    unsigned long long* dSum = reinterpret_cast<unsigned long long*>(dScratch_);
    uint32_t* dOr = dScratch_ + 2;
    if (hipMemcpy(dSum, zero, 16, hipMemcpyHostToDevice) != hipSuccess) return ~0u;
    if (launchReduceRow(dState_, nPad_, n_, stateLayout_.countLo, stateLayout_.countHi, stateLayout_.oodRow, dSum, dOr, stream_) != hipSuccess) return ~0u;
    if (hipStreamSynchronize(stream_) != hipSuccess) return ~0u;
    uint32_t res[4] = {0, 0, 0, 0};
    if (hipMemcpy(res, dSum, 16, hipMemcpyDeviceToHost) != hipSuccess) return ~0u;
    return res[2];
}

int64_t Batch::instructionCounterAt(int64_t inst) {
    (void)hipSetDevice(device_);
    if (!dState_ || inst < 0 || inst >= n_) return 0;
    waitLastLaunch();
    uint32_t lo = 0, hi = 0;
    (void)hipMemcpy(&lo, dState_ + (size_t)stateLayout_.countLo * nPad_ + inst, 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&hi, dState_ + (size_t)stateLayout_.countHi * nPad_ + inst, 4, hipMemcpyDeviceToHost);
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}

float Batch::lastKernelMs() {
    (void)hipSetDevice(device_);
    if (!timed_) return -1.0f;
    if (hipEventSynchronize(ev1_) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ev0_, ev1_) != hipSuccess) return -1.0f;
    return ms;
}

// ---- output meters (fx_meter.hpp): accumulator rows in device memory, carried from launch to launch ---------------------------------

int Batch::meterReset() {
    waitLastLaunch();
    hipError_t e = hipMemsetAsync(dMeter_, 0, meterChannelBytes(nPad_) * (size_t)prog_.numChannels, stream_);
    // (all six: the match rows of a target as well; the target position stays)
    if (e == hipSuccess && dMatch_) e = hipMemsetAsync(dMatch_, 0, matchChannelBytes(nPad_) * (size_t)prog_.numChannels, stream_);
    // (... and the two level rows; the mode and its parameters stay)
    if (e == hipSuccess && dLevel_) e = hipMemsetAsync(dLevel_, 0, levelChannelBytes(nPad_) * (size_t)prog_.numChannels, stream_);
    // (... and the tone rows behind their header; the mode and its coefficients stay)
    if (e == hipSuccess && dTone_) e = hipMemsetAsync(static_cast<char*>(dTone_) + kToneHeaderBytes, 0, toneRowsBytes(nPad_, prog_.numChannels, toneCount_), stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    meterSamples_ = 0;
    return e == hipSuccess ? 0 : hipFail(e, "zeroing the meter rows");
}

int Batch::meterEnable(bool on) {
    (void)hipSetDevice(device_);
    if (on == (dMeter_ != nullptr)) return 0;   // (on twice: the values stay)
    waitLastLaunch();
    (void)hipStreamSynchronize(stream_);
    if (!on) {
        (void)clearMeterTarget();
        (void)clearMeterLevel();
        (void)clearMeterTones();
        (void)hipFree(dMeter_);
        dMeter_ = nullptr;
        meterSamples_ = 0;
        return 0;
    }
    const hipError_t e = hipMalloc(&dMeter_, meterChannelBytes(nPad_) * (size_t)prog_.numChannels);
    if (e != hipSuccess) { dMeter_ = nullptr; return hipFail(hipErrorOutOfMemory, "hipMalloc meter rows"); }
    const int rc = meterReset();
    if (rc != 0) {
        (void)hipFree(dMeter_);
        dMeter_ = nullptr;
    }
    return rc;
}

int Batch::meterRead(double* energy, float* peak, uint32_t* fullScale, uint32_t* nonfinite, bool reset, int64_t rowPitch) {
    (void)hipSetDevice(device_);
    if (!dMeter_) return fail(FX_E_ARG, "meters: metering is off (fxb_meter_enable)");
    if (rowPitch <= 0) rowPitch = n_;
    if (rowPitch < n_) return fail(FX_E_ARG, "meters: row pitch below the instance count");
    int rc = sync();
    if (rc != 0) return rc;
    const char* rows = static_cast<const char*>(dMeter_);
    hipError_t e = hipSuccess;
    for (int c = 0; c < prog_.numChannels && e == hipSuccess; ++c) {
        const char* ch = rows + (size_t)c * meterChannelBytes(nPad_);
        const size_t at = (size_t)c * (size_t)rowPitch;
        if (energy) e = hipMemcpy(energy + at, ch + meterEnergyOff(nPad_), (size_t)n_ * 8, hipMemcpyDeviceToHost);
        if (peak && e == hipSuccess) e = hipMemcpy(peak + at, ch + meterPeakOff(nPad_), (size_t)n_ * 4, hipMemcpyDeviceToHost);
        if (fullScale && e == hipSuccess) e = hipMemcpy(fullScale + at, ch + meterFullScaleOff(nPad_), (size_t)n_ * 4, hipMemcpyDeviceToHost);
        if (nonfinite && e == hipSuccess) e = hipMemcpy(nonfinite + at, ch + meterNonfiniteOff(nPad_), (size_t)n_ * 4, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return hipFail(e, "reading the meter rows");
    return reset ? meterReset() : 0;
}

#ifdef FX_DIAGNOSTICS
int Batch::readEndStamps(uint32_t* out, int64_t nWords) {
    (void)hipSetDevice(device_);
    if (!out || nWords < 0) return fail(FX_E_ARG, "end stamps: bad argument");
    if (!dStamps_) return fail(FX_E_NOTREADY, "end stamps: no unstaged translated launch with FX_XLATE_ENDSTAMP set has run");
    waitLastLaunch();
    const size_t take = std::min((size_t)nWords, stampWords_);
    const hipError_t e = hipMemcpy(out, dStamps_, take * 4, hipMemcpyDeviceToHost);
    return e == hipSuccess ? (int)std::min<size_t>(take, 0x7fffffff) : hipFail(e, "end stamps");
}
#endif

// "translated to gfx950 code (fx_xlate_v128, 8 stages)" / "interpreter (fx_interp_v96): <why the translation failed>" / "HIP C++
// kernel: <why not an assembly tier>" - of the code in force (before the first block: nothing has been lowered yet)
std::string Batch::tierNote() const {
    // (never in the release library: fx_knobs.hpp)
    return kDiagnosticsBuild ? "DIAGNOSTICS BUILD (environment knobs may change or corrupt results): " + tierNotePlain() : tierNotePlain();
}

std::string Batch::tierNotePlain() const {
    static const char* const regs[ASM_VARIANTS] = {"lds", "v64", "v72", "v80", "v96", "v128", "v168", "v256"};
    if (!loaded_) return "no program loaded";
    if (c_.key.empty() && !c_.useAsm && c_.low.steady.empty()) return "not lowered yet (the first block, fxb_prepare or an fxb_info query does it)";
    if (c_.useAsm && c_.useXlate)
        return std::string("translated to gfx950 code (fx_xlate_") + regs[c_.variant] + (c_.stages > 1 ? ", " + std::to_string(c_.stages) + " stages" : "") +
               (c_.stages <= 1 && c_.prioritySlices ? ", wavefronts of a SIMD by turns" : "") + (c_.quiet ? ", quiet loop" : "") + ")";
    if (c_.useAsm) return std::string("interpreter (fx_interp_") + regs[c_.variant] + "): " + (c_.xlateWhyNot.empty() ? "no translation asked for" : c_.xlateWhyNot);
    return "HIP C++ kernel (" + std::to_string(c_.low.instPerLane) + " instance(s) per lane): " + (c_.asmWhyNot.empty() ? "no assembly tier asked for" : c_.asmWhyNot);
}

// wavefronts of the last launch that left the quiet loop: exit words below the block length (a wavefront that never entered the
// loop - a block of one sample, state rows outside their class - leaves its word at 0xFFFFFFFF)
int64_t Batch::quietLeft() {
    if (!lastLaunchQuiet_ || !dQuietLeft_) return 0;
    (void)hipSetDevice(device_);
    waitLastLaunch();
    const size_t stride = lastLaunchSums_ ? 2 : 1;
    const size_t waves = std::min(quietLeftWords_ / 2, ((size_t)n_ + 63) / 64);
    std::vector<uint32_t> words(waves * stride);
    if (hipMemcpy(words.data(), dQuietLeft_, words.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    int64_t left = 0;
    for (size_t k = 0; k < waves; ++k) left += words[k * stride] < (uint32_t)lastLaunchSamples_;
    return left;
}
// repairs of the last launch's sum groups, summed over its wavefronts: the second word of each pair (a wavefront that never
// entered the loop leaves it at 0xFFFFFFFF: no repair)
int64_t Batch::quietRepairs() {
    if (!lastLaunchSums_ || !dQuietLeft_) return 0;
    (void)hipSetDevice(device_);
    waitLastLaunch();
    const size_t waves = std::min(quietLeftWords_ / 2, ((size_t)n_ + 63) / 64);
    std::vector<uint32_t> words(waves * 2);
    if (hipMemcpy(words.data(), dQuietLeft_, words.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    int64_t repairs = 0;
    for (size_t k = 0; k < waves; ++k) repairs += words[2 * k + 1] == 0xffffffffu ? 0 : words[2 * k + 1];
    return repairs;
}

int64_t Batch::info(int what) {
    if (what == FXB_INFO_DEVICE) return device_;
    if (what == FXB_INFO_NUM_INSTRUCTIONS) return (int64_t)prog_.instrs.size();
    if (what == FXB_INFO_NUM_REGISTERS) return (int64_t)prog_.regs.size();
    if (what == FXB_INFO_GRID) return lastGrid_;
    if (what == FXB_INFO_HOST_STAGED_BLOCKS) return hostStagedBlocks_;
    if (what == FXB_INFO_HOST_INPLACE_BLOCKS) return hostInplaceBlocks_;
    if (what == FXB_INFO_BUS_BLOCKS) return busBlocks_;
    if (what == FXB_INFO_METER_LAUNCHES) return meterLaunches_;
    if (what == FXB_INFO_BUS_GAIN_BLOCKS) return busGainBlocks_;
    if (what == FXB_INFO_BUS_TAP_BLOCKS) return busTapBlocks_;
    if (what == FXB_INFO_BUS_SEND_BLOCKS) return busSendBlocks_;
    if (what == FXB_INFO_BUS_FEED_BLOCKS) return busFeedBlocks_;
    if (what == FXB_INFO_IMAJOR_BLOCKS) return imajorBlocks_;
    if (what == FXB_INFO_INSTANCE_GATHERS) return instGathers_;
    if (what == FXB_INFO_INSTANCE_SCATTERS) return instScatters_;
    if (what == FXB_INFO_INSTANCE_ROTATIONS) return instRotations_;
    if (what == FXB_INFO_GAIN_LIST_SETS) return gainListSets_;
    if (what == FXB_INFO_REGISTER_LIST_SETS) return regListSets_;
    if (what == FXB_INFO_REGISTER_LIST_GETS) return regListGets_;
    if (what == FXB_INFO_TRAM_LIST_SETS) return tramListSets_;
    if (what == FXB_INFO_TRAM_LIST_GETS) return tramListGets_;
    if (what == FXB_INFO_METER_SELECTS) return meterSelects_;
    if (what == FXB_INFO_METER_LIST_READS) return meterListReads_;
    if (what == FXB_INFO_METER_LIST_RESETS) return meterListResets_;
    if (what == FXB_INFO_TRACK_LIST_EXPANDS) return trackListExpands_;
    if (what == FXB_INFO_METER_TARGET_LAUNCHES) return meterTargetLaunches_;
    if (what == FXB_INFO_METER_MATCH_SELECTS) return matchSelects_;
    if (what == FXB_INFO_METER_MATCH_BESTS) return matchBests_;
    if (what == FXB_INFO_METER_LEVEL_LAUNCHES) return meterLevelLaunches_;
    if (what == FXB_INFO_METER_LEVEL_SELECTS) return levelSelects_;
    if (what == FXB_INFO_METER_LEVEL_LIST_READS) return levelListReads_;
    if (what == FXB_INFO_METER_RANKS) return meterRanks_;
    if (what == FXB_INFO_METER_MATCH_RANKS) return matchRanks_;
    if (what == FXB_INFO_METER_LEVEL_RANKS) return levelRanks_;
    if (what == FXB_INFO_BANK_SLOTS) return bankSlots_;
    if (what == FXB_INFO_BANK_STORES) return bankStores_;
    if (what == FXB_INFO_BANK_RECALLS) return bankRecalls_;
    if (what == FXB_INFO_BANK_BYTES) return bankSlots_ * bankWords_ * 4;
    if (what == FXB_INFO_METER_TONE_LAUNCHES) return meterToneLaunches_;
    if (what == FXB_INFO_METER_TONE_SELECTS) return toneSelects_;
    if (what == FXB_INFO_METER_TONE_LIST_READS) return toneListReads_;
    if (what == FXB_INFO_METER_TONE_RANKS) return toneRanks_;
    if (what == FXB_INFO_WAVES_PER_WG) return (c_.useAsm && c_.useXlate) ? c_.stages : 1;
    if (ensureLowered() != 0) return -1;
    switch (what) {
        case FXB_INFO_INST_PER_LANE: return instPerLane_;
        case FXB_INFO_INSTANCE_WORDS: return (int64_t)stateRows_ + iSlotsAlloc_ + xSlotsAlloc_;
        case FXB_INFO_INSTANCE_RINGS: return (ringLine(0).ring() ? 1 : 0) | (ringLine(1).ring() ? 2 : 0);
        case FXB_INFO_KERNEL: return c_.useAsm ? (c_.useXlate ? 8 + (int)c_.variant : 1 + (int)c_.variant) : 0;
        case FXB_INFO_XLATE_CODE_BYTES: return c_.useXlate ? (int64_t)c_.codeBytes : 0;
        case FXB_INFO_XLATE_INLINED: return c_.useXlate ? c_.inlined : 0;
        case FXB_INFO_XLATE_CALLED: return c_.useXlate ? c_.called : 0;
        case FXB_INFO_XLATE_BUILDS: return xlateBuilds_;
        case FXB_INFO_XLATE_BACKGROUND_BUILDS: return backgroundBuilds_;
        case FXB_INFO_CONTROL_ROWS: {
            if (c_.key.empty() || lowDirty_) return -1;   // (nothing in force yet / about to change)
            int64_t rows = 0;
            for (size_t r = 0; r < declared_.size() && r < c_.low.rowOfReg.size(); ++r) rows += declared_[r] && !intrinsicLane((int)r) && c_.low.rowOfReg[r] >= 0;
            return rows;
        }
        case FXB_INFO_STAGE_TRIALS: { int64_t n = 0; for (const Tuner& t : tune_) n += t.trials; return n; }
        case FXB_INFO_XLATE_CODE_HASH: return c_.useXlate ? (int64_t)c_.codeHash : 0;
        case FXB_INFO_XLATE_QUIET: return (c_.useXlate && c_.quiet) ? 1 : 0;
        case FXB_INFO_XLATE_QUIET_LEFT: return quietLeft();
        case FXB_INFO_XLATE_QUIET_REPAIRS: return quietRepairs();
        case FXB_INFO_XLATE_SUM_GROUPS: return (c_.useXlate && c_.sumGroups) ? c_.sumGroupCount : 0;
        case FXB_INFO_XLATE_SUM_LINKS: return (c_.useXlate && c_.sumGroups) ? c_.sumLinkCount : 0;
        case FXB_INFO_CODE_CACHE_HITS: return cacheHits_;
        case FXB_INFO_CODE_CACHED: return (int64_t)cache_.size() + (c_.key.empty() ? 0 : 1);
        case FXB_INFO_XLATE_UNSATURATED: return c_.useXlate ? c_.unsaturated : 0;
        case FXB_INFO_XLATE_VALU: return c_.useXlate ? c_.valu : 0;
        case FXB_INFO_XLATE_VALU_SLOW: return c_.useXlate ? c_.valuSlow : 0;
        case FXB_INFO_XLATE_VALU_CLOCKS: return c_.useXlate ? c_.valuClocks : 0;
        case FXB_INFO_XLATE_VGPR_CONSTANTS: return c_.useXlate ? c_.vgprConstants : 0;
        case FXB_INFO_NUM_LANE_REGS: return c_.low.nLaneRegs;
        case FXB_INFO_NUM_UNIFORM_REGS: return c_.low.nUniformRegs;
        case FXB_INFO_LDS_BYTES_PER_WG: return (c_.useAsm && c_.variant != ASM_LDS) ? (c_.useXlate ? (int64_t)c_.ldsBytes : 0) : (int64_t)c_.low.nRows * 256 * instPerLane_;
        case FXB_INFO_NUM_ROWS: return c_.low.nRows;
        case FXB_INFO_NUM_MICROOPS: return (int64_t)c_.low.steady.size();
        case FXB_INFO_ITRAM_SLOTS: return iSlotsAlloc_;
        case FXB_INFO_XTRAM_SLOTS: return xSlotsAlloc_;
        case FXB_INFO_TRAM_OPS: return c_.low.tramOpsPerSample;
        case FXB_INFO_MULTIPASS: return c_.low.multipass ? 1 : 0;
        case FXB_INFO_NUM_SHADOWED: return c_.low.nShadowed;
        case FXB_INFO_NUM_CCR_LIVE: return c_.low.nCcrLive;
        default: return -1;
    }
}

}  // namespace fx
