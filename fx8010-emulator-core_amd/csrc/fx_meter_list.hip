// fx_meter_list.hip — the kernels behind the meter queries by list (fx_meter_list.hpp): an ordered stream compaction of the
// instances whose meter passes a threshold, a gather of the accumulators of listed instances (with their zeroing), and a kernel
// that only zeroes them.  gfx950, wave64, workgroups of 256 lanes.  Plain HIP C++, vector loads and stores only.
//
// The select.  A lane owns one instance of the range.  It reads the one accumulator row the query names for each of the up to
// four channels - a wavefront access is 512 contiguous bytes of an energy row, 256 of the others - and takes the maximum.  The
// compare is done in fp64: the energy is an fp64 word already, a peak (the bits of a non-negative finite float) and a counter (a
// uint32) convert to fp64 without rounding, the maximum of fp64 values is one of them, and the threshold is the caller's double
// as it came.  No accumulator is ever NaN (fx_meter.hip never writes one) and the runtime refuses a NaN threshold, so V >= t and
// V < t are each other's complement and equal the compare of the real numbers.  That was preferred over turning the threshold into
// a bit-pattern bound on the host: one rule for four formats, and nothing to get wrong at the ends of a format's range.
//
// The compaction is three launches and no workgroup ever waits for another one:
//   fx_meter_count  a ballot and a popcount give each wavefront its count, LDS adds the four of a workgroup: offsets[chunk];
//   fx_meter_scan   ONE workgroup of kMeterScanWidth lanes: a lane sums the ceil(chunks / 256) consecutive counts it owns, an
//                   inclusive scan of the 256 lane sums in LDS, then the lane rewrites its counts as their exclusive scan; the
//                   total M goes behind them.  Up to 256 chunks (65 536 instances) a lane has at most one count; above, it loops;
//   fx_meter_emit   recomputes the predicate (the rows cannot have changed: the call is synchronous) and writes the instance number
//                   firstGlobal + i at offsets[chunk] + rank, the rank being the matches in the wavefronts in front plus those in
//                   the lanes below, where that is below cap.  A chunk whose offset has reached cap returns at once.
// The position of a number depends on counts only, never on the order of atomics - there are none: ascending, and the same bits
// run to run.  Columns at and beyond n never match, whatever the padding of the rows holds; first and nRange need no alignment
// (a chunk is 256 instances FROM `first`).
//
// The gather and the zero: one lane per list entry, which walks the channels.  The instance's words are one segment per lane and
// row - the list decides; the packed side is written 256 (energy: 512) contiguous bytes per wavefront.  With `reset` the lane that
// has read a column stores its zeros: the read and the zeroing are one lane's program order.  An entry outside [0, n) is skipped.
//
// Resource usage (-O3, gfx950, from -Rpass-analysis=kernel-resource-usage), VGPRs / scratch bytes per lane / LDS bytes per
// workgroup: fx_meter_count 14 / 0 / 16, fx_meter_scan 16 / 0 / 2 048, fx_meter_emit 16 / 0 / 16, fx_meter_gather 33 / 0 / 0,
// fx_meter_zero 18 / 0 / 0; eight wavefronts per SIMD each.
//
// The queries over the match rows of a target (fx_meter_list.hpp, second half).  fx_match_count / fx_match_emit are the bodies of
// fx_meter_count / fx_meter_emit with another predicate - V is the SUM over the channels of one fp64 row, added in channel order -
// picked by the type of the argument struct (matchesRange is overloaded); the scan is shared as it is.  fx_meter_best gives a
// group of instances to one wavefront: a strided pass keeps the best (V, n) per lane under the total order "V, then n", a
// butterfly of five-plus-one shuffles reduces the pairs, lane 0 stores.  Only compares decide, and the minimum under a total
// order does not depend on the shape of the tree.  A group below 64 instances leaves lanes idle: the known cliff of one
// wavefront per group, as for the mix of small groups.  fx_match_zero stores +0.0 into the listed columns.  Resource usage as
// above: fx_match_count 8 / 0 / 16, fx_match_emit 14 / 0 / 16, fx_meter_best 20 / 0 / 0, fx_match_zero 6 / 0 / 0; eight wavefronts
// per SIMD each.
//
// The queries over the level rows (fx_meter_list.hpp, third part).  fx_level_count / fx_level_emit are the same two bodies with a
// third predicate, picked by LevelSelectArgs: V is the maximum over the channels of the envelope or the MINIMUM over the channels of
// the quiet run, both exact in fp64.  fx_level_gather / fx_level_zero are the one-lane-per-list-entry form of meterColumns on the
// two level rows: the lane that has read a column stores its zeros.  Resource usage as above: fx_level_count 10 / 0 / 16,
// fx_level_emit 14 / 0 / 16, fx_level_gather 11 / 0 / 0, fx_level_zero 6 / 0 / 0; eight wavefronts per SIMD each.
//
// The select over the tone rows (fx_meter_tone.hpp): fx_tone_count / fx_tone_emit are the two bodies with a fourth predicate,
// picked by ToneSelectArgs: V is the maximum over the channels of tonePower.  Resource usage as above: fx_tone_count 14 / 0 / 16,
// fx_tone_emit 16 / 0 / 16; eight wavefronts per SIMD each.
#include <hip/hip_runtime.h>

#include "fx_meter.hpp"
#include "fx_meter_list.hpp"
#include "fx_meter_value.hpp"

namespace fx {

namespace {

constexpr int kLanes = kMeterSelectChunk;
constexpr int kWaves = kLanes / 64;
static_assert(kMeterScanWidth == kLanes, "the scan is one workgroup of that many lanes");

// whether instance first + i of the range matches; i is the lane's index in the range.  V(n) is taken by fx_meter_value.hpp, the
// one place that defines it for the selects, fx_meter_best and the ranks (fx_meter_rank.hip)
__device__ __forceinline__ bool meterMatches(const MeterSelectArgs& a, long long i) {
    if (i >= a.nRange) return false;
    const long long col = a.first + i;
    if (col >= a.n) return false;   // (cannot be: first + nRange <= n.  The padding never matches.)
    const double best = meterValue(a.rows, a.nPad, a.channels, a.stat, col);
    return a.below ? best < a.threshold : best >= a.threshold;
}

// (the bodies of the count and the emit take the predicate through their argument type: matchesRange is overloaded, so the
// select over the match rows of a target - MatchSelectArgs, below - runs the same code with the channel-sum predicate)
__device__ __forceinline__ bool matchesRange(const MeterSelectArgs& a, long long i) { return meterMatches(a, i); }

__device__ __forceinline__ bool matchesRange(const MatchSelectArgs& a, long long i) {
    if (i >= a.nRange) return false;
    const long long col = a.first + i;
    if (col >= a.n) return false;
    const double v = matchValue(a.rows, a.nPad, a.channels, a.stat, col);
    return a.below ? v < a.threshold : v >= a.threshold;
}

// V(n) over the level rows: the maximum of the envelopes, the MINIMUM of the quiet runs - both exact in fp64
__device__ __forceinline__ bool matchesRange(const LevelSelectArgs& a, long long i) {
    if (i >= a.nRange) return false;
    const long long col = a.first + i;
    if (col >= a.n) return false;
    const double best = levelValue(a.rows, a.nPad, a.channels, a.stat, col);
    return a.below ? best < a.threshold : best >= a.threshold;
}

// V(n) over the tone rows: the maximum over the channels of P of tone `stat`
__device__ __forceinline__ bool matchesRange(const ToneSelectArgs& a, long long i) {
    if (i >= a.nRange) return false;
    const long long col = a.first + i;
    if (col >= a.n) return false;
    const double best = toneValue(a.rows, a.nPad, a.channels, a.stat, col);
    return a.below ? best < a.threshold : best >= a.threshold;
}

template <class Args>
__device__ __forceinline__ void selectCount(const Args& a) {
    __shared__ unsigned waveCount[kWaves];
    const unsigned t = threadIdx.x;
    const bool match = matchesRange(a, (long long)blockIdx.x * kLanes + t);
    const unsigned long long mask = __ballot(match);
    if ((t & 63u) == 0) waveCount[t >> 6] = (unsigned)__popcll(mask);
    __syncthreads();
    if (t == 0) {
        unsigned sum = 0;
        for (int w = 0; w < kWaves; ++w) sum += waveCount[w];
        a.offsets[blockIdx.x] = sum;
    }
}

__global__ __launch_bounds__(kLanes) void fx_meter_count(MeterSelectArgs a) { selectCount(a); }
__global__ __launch_bounds__(kLanes) void fx_match_count(MatchSelectArgs a) { selectCount(a); }
__global__ __launch_bounds__(kLanes) void fx_level_count(LevelSelectArgs a) { selectCount(a); }
__global__ __launch_bounds__(kLanes) void fx_tone_count(ToneSelectArgs a) { selectCount(a); }

// one workgroup: offsets[0 .. chunks - 1] counts -> their exclusive scan, offsets[chunks] = the total.  Lane t owns the `per`
// consecutive counts from t * per on: the loads of one lane are independent, so their latencies overlap
__global__ __launch_bounds__(kLanes) void fx_meter_scan(unsigned long long* offsets, long long chunks) {
    __shared__ unsigned long long s[kLanes];
    const unsigned t = threadIdx.x;
    const long long per = (chunks + kLanes - 1) / kLanes;
    const long long lo = (long long)t * per < chunks ? (long long)t * per : chunks, hi = lo + per < chunks ? lo + per : chunks;
    unsigned long long mine = 0;
    for (long long k = lo; k < hi; ++k) mine += offsets[k];
    s[t] = mine;
    __syncthreads();
    // Hillis-Steele over the lane sums, inclusive: after the step of width d, s[t] is the sum of the 2d sums ending at t
    for (unsigned d = 1; d < (unsigned)kLanes; d <<= 1) {
        const unsigned long long add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    unsigned long long run = s[t] - mine;   // the matches in front of this lane's counts
    for (long long k = lo; k < hi; ++k) {
        const unsigned long long c = offsets[k];
        offsets[k] = run;
        run += c;
    }
    if (t == kLanes - 1) offsets[chunks] = s[t];
}

template <class Args>
__device__ __forceinline__ void selectEmit(const Args& a) {
    __shared__ unsigned waveCount[kWaves];
    const unsigned long long offset = a.offsets[blockIdx.x];
    if (offset >= (unsigned long long)a.cap) return;   // (the whole workgroup: nothing of this chunk fits)
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const long long i = (long long)blockIdx.x * kLanes + t;
    const bool match = matchesRange(a, i);
    const unsigned long long mask = __ballot(match);
    if (lane == 0) waveCount[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    unsigned rank = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    for (unsigned w = 0; w < wave; ++w) rank += waveCount[w];
    const unsigned long long pos = offset + rank;
    if (match && pos < (unsigned long long)a.cap) a.list[pos] = a.firstGlobal + i;
}

__global__ __launch_bounds__(kLanes) void fx_meter_emit(MeterSelectArgs a) { selectEmit(a); }
__global__ __launch_bounds__(kLanes) void fx_match_emit(MatchSelectArgs a) { selectEmit(a); }
__global__ __launch_bounds__(kLanes) void fx_level_emit(LevelSelectArgs a) { selectEmit(a); }
__global__ __launch_bounds__(kLanes) void fx_tone_emit(ToneSelectArgs a) { selectEmit(a); }

// fx_meter_best: wavefront w of the grid owns group firstGroup + w.  Its local members are the columns lo .. hi - 1; lane l
// looks at lo + l, lo + l + 64, ... and keeps the best (V, n).  kNone marks a lane that has seen no member (a group below 64).
constexpr long long kNone = 0x7fffffffffffffffll;
__device__ __forceinline__ bool bestBeats(double v, long long k, double bv, long long bk, bool largest) {
    if (k == kNone) return false;
    if (bk == kNone) return true;
    if (v != bv) return largest ? v > bv : v < bv;
    return k < bk;
}

__global__ __launch_bounds__(kLanes) void fx_meter_best(MeterBestArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const long long g = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);   // (uniform in a wavefront)
    if (g >= a.groups) return;
    const long long from = (a.firstGroup + g) * a.group - a.firstGlobal;   // may lie in front of this batch's columns
    const long long lo = from > 0 ? from : 0, hi = from + a.group < a.n ? from + a.group : a.n;
    const bool largest = a.largest != 0;
    double bv = 0.0;
    long long bk = kNone;
    for (long long col = lo + lane; col < hi; col += 64) {
        const double v = matchValue(a.rows, a.nPad, a.channels, a.stat, col);
        if (bestBeats(v, col, bv, bk, largest)) {
            bv = v;
            bk = col;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(bv, d, 64);
        const long long ok = __shfl_xor(bk, d, 64);
        if (bestBeats(ov, ok, bv, bk, largest)) {
            bv = ov;
            bk = ok;
        }
    }
    if (lane == 0) {
        a.winner[g] = bk == kNone ? -1 : a.firstGlobal + bk;
        a.value[g] = bv;
    }
}

// the match rows of the listed columns: stores only
__global__ __launch_bounds__(kLanes) void fx_match_zero(MeterListArgs a) {
    const long long k = (long long)blockIdx.x * kLanes + threadIdx.x;
    if (k >= a.count) return;
    const long long inst = a.list[k];
    if (inst < 0 || inst >= a.n) return;
    char* ch = static_cast<char*>(a.rows);
    for (int c = 0; c < a.channels; ++c, ch += matchChannelBytes(a.nPad)) {
        reinterpret_cast<double*>(ch + matchErrOff(a.nPad))[inst] = 0.0;
        reinterpret_cast<double*>(ch + matchCrossOff(a.nPad))[inst] = 0.0;
    }
}

template <bool kGather>
__device__ __forceinline__ void meterColumns(const MeterListArgs& a) {
    const long long k = (long long)blockIdx.x * kLanes + threadIdx.x;
    if (k >= a.count) return;
    const long long inst = a.list[k];
    if (inst < 0 || inst >= a.n) return;
    const size_t rowWords = (size_t)a.channels * (size_t)a.count;
    double* const pEnergy = static_cast<double*>(a.packed);
    uint32_t* const pPeak = reinterpret_cast<uint32_t*>(static_cast<char*>(a.packed) + rowWords * 8);
    uint32_t* const pFull = pPeak + rowWords;
    uint32_t* const pNon = pFull + rowWords;
    char* ch = static_cast<char*>(a.rows);
    for (int c = 0; c < a.channels; ++c, ch += meterChannelBytes(a.nPad)) {
        double* energy = reinterpret_cast<double*>(ch + meterEnergyOff(a.nPad)) + inst;
        uint32_t* peak = reinterpret_cast<uint32_t*>(ch + meterPeakOff(a.nPad)) + inst;
        uint32_t* fullScale = reinterpret_cast<uint32_t*>(ch + meterFullScaleOff(a.nPad)) + inst;
        uint32_t* nonfinite = reinterpret_cast<uint32_t*>(ch + meterNonfiniteOff(a.nPad)) + inst;
        if (kGather) {
            const size_t at = (size_t)c * (size_t)a.count + (size_t)k;
            const double e = *energy;
            const uint32_t p = *peak, f = *fullScale, q = *nonfinite;
            pEnergy[at] = e;
            pPeak[at] = p;
            pFull[at] = f;
            pNon[at] = q;
        }
        if (!kGather || a.reset) {
            *energy = 0.0;
            *peak = 0u;
            *fullScale = 0u;
            *nonfinite = 0u;
        }
    }
}

__global__ __launch_bounds__(kLanes) void fx_meter_gather(MeterListArgs a) { meterColumns<true>(a); }
__global__ __launch_bounds__(kLanes) void fx_meter_zero(MeterListArgs a) { meterColumns<false>(a); }

// meterColumns on the two level rows: the packed side is level [channels][count], then quiet [channels][count]
template <bool kGather>
__device__ __forceinline__ void levelColumns(const MeterListArgs& a) {
    const long long k = (long long)blockIdx.x * kLanes + threadIdx.x;
    if (k >= a.count) return;
    const long long inst = a.list[k];
    if (inst < 0 || inst >= a.n) return;
    const size_t rowWords = (size_t)a.channels * (size_t)a.count;
    uint32_t* const pLevel = static_cast<uint32_t*>(a.packed);
    uint32_t* const pQuiet = pLevel + rowWords;
    char* ch = static_cast<char*>(a.rows);
    for (int c = 0; c < a.channels; ++c, ch += levelChannelBytes(a.nPad)) {
        uint32_t* level = reinterpret_cast<uint32_t*>(ch + levelLevelOff(a.nPad)) + inst;
        uint32_t* quiet = reinterpret_cast<uint32_t*>(ch + levelQuietOff(a.nPad)) + inst;
        if (kGather) {
            const size_t at = (size_t)c * (size_t)a.count + (size_t)k;
            const uint32_t l = *level, q = *quiet;
            pLevel[at] = l;
            pQuiet[at] = q;
        }
        if (!kGather || a.reset) {
            *level = 0u;
            *quiet = 0u;
        }
    }
}

__global__ __launch_bounds__(kLanes) void fx_level_gather(MeterListArgs a) { levelColumns<true>(a); }
__global__ __launch_bounds__(kLanes) void fx_level_zero(MeterListArgs a) { levelColumns<false>(a); }

inline bool badList(const MeterListArgs& a, bool gather) {
    if (!a.rows || !a.list || a.count < 1 || a.count >= ((long long)1 << 31) || a.n < 1 || a.nPad < a.n) return true;
    if (a.channels < 1 || a.channels > 4) return true;
    return gather && !a.packed;
}

}  // namespace

hipError_t launchMeterSelect(const MeterSelectArgs& a, hipStream_t stream) {
    if (!a.rows || !a.offsets || a.n < 1 || a.nPad < a.n || a.channels < 1 || a.channels > 4 || a.stat < 0 || a.stat > 3) return hipErrorInvalidValue;
    if (a.first < 0 || a.nRange < 1 || a.first > a.n - a.nRange || a.cap < 0 || (a.cap > 0 && !a.list) || a.threshold != a.threshold) return hipErrorInvalidValue;
    const long long chunks = meterSelectChunks(a.nRange);
    if (chunks >= ((long long)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_meter_count, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fx_meter_scan, dim3(1), dim3(kLanes), 0, stream, a.offsets, chunks);
    if ((e = hipGetLastError()) != hipSuccess || a.cap == 0) return e;   // (a count query emits nothing)
    hipLaunchKernelGGL(fx_meter_emit, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchMatchSelect(const MatchSelectArgs& a, hipStream_t stream) {
    if (!a.rows || !a.offsets || a.n < 1 || a.nPad < a.n || a.channels < 1 || a.channels > 4 || a.stat < 0 || a.stat > 1) return hipErrorInvalidValue;
    if (a.first < 0 || a.nRange < 1 || a.first > a.n - a.nRange || a.cap < 0 || (a.cap > 0 && !a.list) || a.threshold != a.threshold) return hipErrorInvalidValue;
    const long long chunks = meterSelectChunks(a.nRange);
    if (chunks >= ((long long)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_match_count, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fx_meter_scan, dim3(1), dim3(kLanes), 0, stream, a.offsets, chunks);
    if ((e = hipGetLastError()) != hipSuccess || a.cap == 0) return e;   // (a count query emits nothing)
    hipLaunchKernelGGL(fx_match_emit, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchLevelSelect(const LevelSelectArgs& a, hipStream_t stream) {
    if (!a.rows || !a.offsets || a.n < 1 || a.nPad < a.n || a.channels < 1 || a.channels > 4 || a.stat < 0 || a.stat > 1) return hipErrorInvalidValue;
    if (a.first < 0 || a.nRange < 1 || a.first > a.n - a.nRange || a.cap < 0 || (a.cap > 0 && !a.list) || a.threshold != a.threshold) return hipErrorInvalidValue;
    const long long chunks = meterSelectChunks(a.nRange);
    if (chunks >= ((long long)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_level_count, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fx_meter_scan, dim3(1), dim3(kLanes), 0, stream, a.offsets, chunks);
    if ((e = hipGetLastError()) != hipSuccess || a.cap == 0) return e;   // (a count query emits nothing)
    hipLaunchKernelGGL(fx_level_emit, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchToneSelect(const ToneSelectArgs& a, hipStream_t stream) {
    if (!a.rows || !a.offsets || a.n < 1 || a.nPad < a.n || a.channels < 1 || a.channels > 4 || a.stat < 0 || a.stat >= kMeterMaxTones) return hipErrorInvalidValue;
    if (a.first < 0 || a.nRange < 1 || a.first > a.n - a.nRange || a.cap < 0 || (a.cap > 0 && !a.list) || a.threshold != a.threshold) return hipErrorInvalidValue;
    const long long chunks = meterSelectChunks(a.nRange);
    if (chunks >= ((long long)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_tone_count, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fx_meter_scan, dim3(1), dim3(kLanes), 0, stream, a.offsets, chunks);
    if ((e = hipGetLastError()) != hipSuccess || a.cap == 0) return e;   // (a count query emits nothing)
    hipLaunchKernelGGL(fx_tone_emit, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchLevelGather(const MeterListArgs& a, hipStream_t stream) {
    if (badList(a, true)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_level_gather, dim3((unsigned)((a.count + kLanes - 1) / kLanes)), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchLevelZero(const MeterListArgs& a, hipStream_t stream) {
    if (badList(a, false)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_level_zero, dim3((unsigned)((a.count + kLanes - 1) / kLanes)), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchMeterBest(const MeterBestArgs& a, hipStream_t stream) {
    if (!a.rows || !a.winner || !a.value || a.n < 1 || a.nPad < a.n || a.channels < 1 || a.channels > 4 || a.stat < 0 || a.stat > 1) return hipErrorInvalidValue;
    if (a.group < 1 || a.firstGlobal < 0 || a.firstGroup != a.firstGlobal / a.group || a.groups != (a.firstGlobal + a.n - 1) / a.group - a.firstGroup + 1) return hipErrorInvalidValue;
    const long long blocks = (a.groups + kWaves - 1) / kWaves;
    if (blocks >= ((long long)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_meter_best, dim3((unsigned)blocks), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchMatchZero(const MeterListArgs& a, hipStream_t stream) {
    if (badList(a, false)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_match_zero, dim3((unsigned)((a.count + kLanes - 1) / kLanes)), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchMeterGather(const MeterListArgs& a, hipStream_t stream) {
    if (badList(a, true)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_meter_gather, dim3((unsigned)((a.count + kLanes - 1) / kLanes)), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchMeterZero(const MeterListArgs& a, hipStream_t stream) {
    if (badList(a, false)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_meter_zero, dim3((unsigned)((a.count + kLanes - 1) / kLanes)), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fx
