// fx_batch_bus_gain.cpp — the per-instance mix gains of bus blocks: the state of one batch (fx_batch.hpp "Bus gains", kernel:
// fx_bus_mix_gain in fx_bus.hip, where it is launched: Batch::runBus).
//
// Two device blocks [channels][n]; gainRamp_ (fx_batch_bus_side.hpp RampPair, shared with the send gains) names the one that is
// b, the other one is a and means something only while a ramp is pending.  A set copies the caller's columns into pinned staging on the host (the caller's array is free on return) and from
// there, on the handle's stream, into the block that becomes b:
//   gains off -> on        block 0 = b; with ramp the other block is filled with 1.0f (a while gains are off);
//   ramp, none pending     a counts as the old b: the two blocks swap roles, the new values go into the block that was a;
//   anything else          the values replace b where it is (ramp = 0 also drops the pending flag; a is stale from then on).
// The copy waits for evBus_ - every bus block queued so far, on whatever stream, has read the blocks it was queued with - and
// evGain_ is recorded behind it: runBus makes a later block's stream wait for that.  The staging is reused, so a set first waits
// on the HOST for the previous set's copy (which waited for the block in front of it: two sets behind one running block cost the
// caller the rest of that block).  Nothing here allocates outside busReserveGains.
#include "fx_batch.hpp"

#include <cmath>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

bool Batch::gainsFinite(const float* gains, int channels, int64_t n, int64_t rowPitch) {
    // the exponent field on the integer view (all ones: Inf or NaN), OR-ed over a row without a branch, so that the scan vectorises
    for (int c = 0; c < channels; ++c) {
        const float* row = gains + (size_t)c * (size_t)rowPitch;
        uint32_t bad = 0;
        for (int64_t i = 0; i < n; ++i) {
            uint32_t u;
            std::memcpy(&u, row + i, 4);
            bad |= (uint32_t)((u & 0x7F800000u) == 0x7F800000u);
        }
        if (bad) return false;
    }
    return true;
}

int Batch::busReserveGains() {
    (void)hipSetDevice(device_);
    const bool had[4] = {dGain_[0] != nullptr, dGain_[1] != nullptr, hGain_ != nullptr, evGain_ != nullptr};
    const size_t bytes = gainFloats() * 4;
    hipError_t e = hipSuccess;
    const char* what = "";
    for (int k = 0; k < 2 && e == hipSuccess; ++k)
        if (!dGain_[k] && (e = hipMalloc(reinterpret_cast<void**>(&dGain_[k]), bytes)) != hipSuccess) { dGain_[k] = nullptr; what = "hipMalloc bus gains"; }
    if (e == hipSuccess && !hGain_ && (e = hipHostMalloc(reinterpret_cast<void**>(&hGain_), bytes * 2, hipHostMallocDefault)) != hipSuccess) { hGain_ = nullptr; what = "pinned staging of the bus gains"; }
    if (e == hipSuccess && !evGain_ && (e = hipEventCreateWithFlags(&evGain_, hipEventDisableTiming)) != hipSuccess) { evGain_ = nullptr; what = "bus gain event"; }
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    // what this call allocated goes again: the handle is as it was
    for (int k = 0; k < 2; ++k)
        if (!had[k] && dGain_[k]) { (void)hipFree(dGain_[k]); dGain_[k] = nullptr; }
    if (!had[2] && hGain_) { (void)hipHostFree(hGain_); hGain_ = nullptr; }
    if (!had[3] && evGain_) { (void)hipEventDestroy(evGain_); evGain_ = nullptr; }
    return hipFail(hipErrorOutOfMemory, what);   // (FX_E_MEMORY: an event that cannot be had is a resource that ran out, too)
}

void Batch::busReleaseGains() {
    if (gainsOn_) return;
    (void)hipSetDevice(device_);
    if (gainCopied_) (void)hipEventSynchronize(evGain_);
    gainCopied_ = false;
    for (int k = 0; k < 2; ++k) {
        (void)hipFree(dGain_[k]);
        dGain_[k] = nullptr;
    }
    if (hGain_) (void)hipHostFree(hGain_);
    hGain_ = nullptr;
    if (evGain_) (void)hipEventDestroy(evGain_);
    evGain_ = nullptr;
}

int Batch::busSetGains(const float* gains, int64_t rowPitch, int ramp, bool checked) {
    (void)hipSetDevice(device_);
    if (ramp != 0 && ramp != 1) return fail(FX_E_ARG, "bus gains: ramp must be 0 or 1");
    if (!gains) {
        if (!gainsOn_) return 0;
        const int rc = sync();   // (blocks queued with the gains still read them)
        if (rc != 0) return rc;  // (a failing call changes nothing: the gains stay on and their blocks stay allocated)
        gainsOn_ = false;
        gainRamp_.consume();
        busReleaseGains();
        return 0;
    }
    if (rowPitch <= 0) rowPitch = n_;
    if (rowPitch < n_) return fail(FX_E_ARG, "bus gains: row pitch below the instance count");
    const int ch = prog_.numChannels;
    if (!checked && !gainsFinite(gains, ch, n_, rowPitch)) return fail(FX_E_ARG, "bus gains: every gain must be finite");
    int rc = busReserveGains();
    if (rc != 0) return rc;
    hipError_t e = hipSuccess;
    if (gainCopied_ && (e = hipEventSynchronize(evGain_)) != hipSuccess) return hipFail(e, "bus gains: waiting for the previous set");
    gainCopied_ = false;
    const size_t block = gainFloats();
    for (int c = 0; c < ch; ++c) std::memcpy(hGain_ + (size_t)c * (size_t)n_, gains + (size_t)c * (size_t)rowPitch, (size_t)n_ * 4);
    const bool fromOff = !gainsOn_;
    const int target = fromOff ? 0 : gainRamp_.writeTarget(ramp);
    if (busLaunched_ && (e = hipStreamWaitEvent(stream_, evBus_, 0)) != hipSuccess) return hipFail(e, "bus gains: ordering behind the queued bus blocks");
    if (fromOff && ramp) {
        for (size_t i = 0; i < block; ++i) hGain_[block + i] = 1.0f;
        e = hipMemcpyAsync(dGain_[target ^ 1], hGain_ + block, block * 4, hipMemcpyHostToDevice, stream_);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(dGain_[target], hGain_, block * 4, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = hipEventRecord(evGain_, stream_);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream_);   // (nothing may still read the staging)
        return hipFail(e, "bus gains: copying to the device");
    }
    gainCopied_ = true;
    gainRamp_ = RampPair{target, ramp != 0};
    gainsOn_ = true;
    return 0;
}

int Batch::busGetGains(float* gains, int64_t rowPitch) {
    (void)hipSetDevice(device_);
    if (!gainsOn_) return fail(FX_E_ARG, "bus gains: gains are off (fxb_bus_set_gains)");
    if (!gains) return fail(FX_E_ARG, "null buffer");
    if (rowPitch <= 0) rowPitch = n_;
    if (rowPitch < n_) return fail(FX_E_ARG, "bus gains: row pitch below the instance count");
    const int rc = sync();
    if (rc != 0) return rc;
    gainCopied_ = false;   // (the handle's stream has drained)
    // the gains in force: a while a ramp waits for its block, else b (a consumed ramp has left its target in force)
    const float* from = dGain_[gainRamp_.inForce()];
    hipError_t e = hipSuccess;
    for (int c = 0; c < prog_.numChannels && e == hipSuccess; ++c)
        e = hipMemcpy(gains + (size_t)c * (size_t)rowPitch, from + (size_t)c * (size_t)n_, (size_t)n_ * 4, hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : hipFail(e, "reading the bus gains");
}

}  // namespace fx
