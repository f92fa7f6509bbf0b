// fx_meter_rank.hip — the kernels behind the meter ranks (fx_meter_rank.hpp): the first k candidates of a range under the order
// (V, n), chosen on the device - V of one of four families (fx_meter_value.hpp).  gfx950, wave64, workgroups of 256 lanes, a chunk of 256 instances per workgroup as in the selects.
// Plain HIP C++, vector loads and stores only.
//
// The key.  V + 0.0 (so that -0.0 cannot appear), its bits with the sign-flip transform - a negative value has all bits
// complemented, any other its sign bit set - give a 64-bit unsigned key that is monotone in the real order; `largest` complements
// the key, so that every kernel only ever looks for the SMALLEST keys.  No V is NaN.  A lane recomputes V, the predicate and the
// key in every kernel: the rows cannot change (the call is synchronous), and the values never travel through memory.
//
// The selection.  With K = min(k, M), T is the key of the K-th candidate in key order.  The eight digits of T are found most
// significant first.  fx_rank_hist of pass p counts digit p of the candidates whose digits in front equal the prefix found so far:
// a histogram of 256 bins in LDS per workgroup, its non-zero bins added to the pass's bins in device memory with integer atomic
// adds - sums, which no order of arrival can change.  The PICK of pass p - an inclusive scan of the 256 bins, one per lane, and the
// one lane whose bin holds the remainder-th candidate - is done again by EVERY workgroup of the next kernel, from the same words to
// the same result; workgroup 0 also stores it (slots) for the kernel behind.  So a pass is one launch, and no workgroup waits for
// another.  The pick of pass 0 sees M (the sum of all bins) and starts the remainder at K; with K == 0 no lane picks, the prefix
// stays 0, T == 0 and nothing is below it or taken: M == 0, k == 0 and M <= k (T is then the largest key and all its equals are
// taken) come out of the same launches.
//
// The winners are the candidates with key < T and the first `take` BY INSTANCE NUMBER of those with key == T, `take` being the
// remainder after the last pick.  fx_rank_count writes both counts per chunk; fx_rank_scan, one workgroup, scans the equals to clamp
// each chunk's share of `take`, then scans the winners per chunk; fx_rank_emit recomputes, ranks the lanes by ballots and writes
// (firstGlobal + i, the bits of V) at offset + rank.  Positions depend on counts only: ascending by instance, the same bits run to
// run.  The host sorts the R pairs into rank order.
//
// Resource usage (-O3, gfx950, from -Rpass-analysis=kernel-resource-usage), VGPRs / SGPRs / scratch bytes per lane / LDS bytes per
// workgroup: fx_rank_hist 24 / 44 / 0 / 3 088, fx_rank_count 20 / 41 / 0 / 2 096, fx_rank_scan 26 / 34 / 0 / 2 048, fx_rank_emit
// 38 / 44 / 0 / 32; eight wavefronts per SIMD each (with the fourth family, the tone rows of fx_meter_tone.hpp, compiled in; 17,
// 16, 26 and 38 VGPRs with three).
#include <hip/hip_runtime.h>

#include "fx_meter.hpp"
#include "fx_meter_rank.hpp"
#include "fx_meter_value.hpp"

namespace fx {

namespace {

constexpr int kLanes = kMeterSelectChunk;
constexpr int kWaves = kLanes / 64;
static_assert(kMeterScanWidth == kLanes && kMeterRankBins == kLanes, "one workgroup of that many lanes scans, one lane per bin");

struct RankLane {
    bool cand;                 // a candidate of the range
    unsigned long long key;    // smaller wins
    double v;
};

__device__ __forceinline__ RankLane rankLane(const MeterRankArgs& a, long long i) {
    RankLane r{false, 0ull, 0.0};
    if (i >= a.nRange) return r;
    const long long col = a.first + i;
    if (col >= a.n) return r;   // (cannot be: first + nRange <= n.  The padding is never a candidate.)
    const double v = a.family == kRankMeter ? meterValue(a.rows, a.nPad, a.channels, a.stat, col)
                     : a.family == kRankMatch ? matchValue(a.rows, a.nPad, a.channels, a.stat, col)
                     : a.family == kRankLevel ? levelValue(a.rows, a.nPad, a.channels, a.stat, col) : toneValue(a.rows, a.nPad, a.channels, a.stat, col);
    r.cand = a.below ? v < a.threshold : v >= a.threshold;
    unsigned long long u = (unsigned long long)__double_as_longlong(v + 0.0);
    u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    r.key = a.largest ? ~u : u;
    r.v = v;
    return r;
}

// inclusive scan of one word per lane over the workgroup (Hillis-Steele in LDS, as fx_meter_scan): s[t] on return
__device__ __forceinline__ unsigned long long scanLanes(unsigned long long* s, unsigned long long mine) {
    const unsigned t = threadIdx.x;
    __syncthreads();   // (whoever still reads s from an earlier use)
    s[t] = mine;
    __syncthreads();
    for (unsigned d = 1; d < (unsigned)kLanes; d <<= 1) {
        const unsigned long long add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    return s[t];
}

// The pick of pass p, by the whole workgroup: (prefix, rem) in front of pass p -> (prefix, rem) behind it.  Lane b owns bin b.
// Workgroup 0 stores the result for the kernel behind: slot p + 1, or T and `take` in the result words after the last pass; the
// pick of pass 0 also stores M and R.
__device__ __forceinline__ void rankPick(const MeterRankArgs& a, int p, unsigned long long* prefixOut, unsigned long long* remOut) {
    __shared__ unsigned long long s[kLanes];
    __shared__ unsigned long long picked[2];
    const unsigned t = threadIdx.x;
    const unsigned long long mine = a.stage[rankHistOff(a.room) + (size_t)p * kMeterRankBins + t];
    const unsigned long long incl = scanLanes(s, mine), excl = incl - mine;
    unsigned long long* const slots = a.stage + rankSlotsOff(a.room);
    unsigned long long prefix = 0, rem;
    if (p == 0) {
        const unsigned long long m = s[kLanes - 1];
        rem = m < (unsigned long long)a.k ? m : (unsigned long long)a.k;
        if (blockIdx.x == 0 && t == 0) {
            a.stage[0] = m;
            a.stage[1] = rem;
        }
    } else {
        prefix = slots[2 * p];
        rem = slots[2 * p + 1];
    }
    if (t == 0) {   // (rem == 0: no lane picks, the digit is 0 and the remainder stays 0)
        picked[0] = prefix;
        picked[1] = 0;
    }
    __syncthreads();
    if (rem >= 1 && excl < rem && rem <= incl) {   // exactly one lane: the bins in front hold fewer than rem, with this one enough
        picked[0] = prefix | ((unsigned long long)t << (64 - kMeterRankDigitBits * (p + 1)));
        picked[1] = rem - excl;
    }
    __syncthreads();
    *prefixOut = picked[0];
    *remOut = picked[1];
    if (blockIdx.x == 0 && t == 0) {
        unsigned long long* const to = p + 1 < kMeterRankPasses ? slots + 2 * (p + 1) : a.stage + 2;
        to[0] = picked[0];
        to[1] = picked[1];
    }
}

__global__ __launch_bounds__(kLanes) void fx_rank_hist(MeterRankArgs a, int p) {
    __shared__ unsigned bins[kLanes];
    const unsigned t = threadIdx.x;
    unsigned long long prefix = 0, rem = 0;
    if (p > 0) rankPick(a, p - 1, &prefix, &rem);
    bins[t] = 0;
    __syncthreads();
    const RankLane r = rankLane(a, (long long)blockIdx.x * kLanes + t);
    const int high = 64 - kMeterRankDigitBits * p;   // bits below the digits in front: 64 in pass 0, where every candidate counts
    if (r.cand && (p == 0 || (r.key >> high) == (prefix >> high))) atomicAdd(&bins[(unsigned)(r.key >> (high - kMeterRankDigitBits)) & (unsigned)(kMeterRankBins - 1)], 1u);
    __syncthreads();
    if (bins[t] != 0) atomicAdd(a.stage + rankHistOff(a.room) + (size_t)p * kMeterRankBins + t, (unsigned long long)bins[t]);
}

// below / equal of a chunk from the lanes' flags: ballots and popcounts per wavefront, LDS adds the four
__global__ __launch_bounds__(kLanes) void fx_rank_count(MeterRankArgs a) {
    __shared__ unsigned waveBelow[kWaves], waveEqual[kWaves];
    const unsigned t = threadIdx.x;
    unsigned long long key = 0, take = 0;
    rankPick(a, kMeterRankPasses - 1, &key, &take);
    const RankLane r = rankLane(a, (long long)blockIdx.x * kLanes + t);
    const unsigned long long below = __ballot(r.cand && r.key < key), equal = __ballot(r.cand && r.key == key);
    if ((t & 63u) == 0) {
        waveBelow[t >> 6] = (unsigned)__popcll(below);
        waveEqual[t >> 6] = (unsigned)__popcll(equal);
    }
    __syncthreads();
    if (t == 0) {
        unsigned b = 0, e = 0;
        for (int w = 0; w < kWaves; ++w) {
            b += waveBelow[w];
            e += waveEqual[w];
        }
        a.stage[rankBelowOff(a.room) + blockIdx.x] = b;
        a.stage[rankEqualOff(a.nRange, a.room) + blockIdx.x] = e;
    }
}

// one workgroup.  Lane t owns the `per` consecutive chunks from t * per on, as in fx_meter_scan.  First the equals: with E the
// equals in the chunks in front, a chunk's share is what is left of `take` there, at most its own count.  Then the winners of a
// chunk - below + share - are scanned: below[chunk] becomes their exclusive scan, equal[chunk] the share.
__global__ __launch_bounds__(kLanes) void fx_rank_scan(unsigned long long* below, unsigned long long* equal, const unsigned long long* result, long long chunks) {
    __shared__ unsigned long long s[kLanes];
    const unsigned t = threadIdx.x;
    const unsigned long long take = result[3];
    const long long per = (chunks + kLanes - 1) / kLanes;
    const long long lo = (long long)t * per < chunks ? (long long)t * per : chunks, hi = lo + per < chunks ? lo + per : chunks;
    unsigned long long mine = 0;
    for (long long c = lo; c < hi; ++c) mine += equal[c];
    unsigned long long run = scanLanes(s, mine) - mine;   // the equals in front of this lane's chunks
    mine = 0;
    for (long long c = lo; c < hi; ++c) {
        const unsigned long long e = equal[c], left = run < take ? take - run : 0, share = e < left ? e : left;
        run += e;
        equal[c] = share;
        below[c] += share;
        mine += below[c];
    }
    run = scanLanes(s, mine) - mine;   // the winners in front of this lane's chunks
    for (long long c = lo; c < hi; ++c) {
        const unsigned long long w = below[c];
        below[c] = run;
        run += w;
    }
}

__global__ __launch_bounds__(kLanes) void fx_rank_emit(MeterRankArgs a) {
    __shared__ unsigned waveEqual[kWaves], waveWin[kWaves];
    const unsigned long long offset = a.stage[rankBelowOff(a.room) + blockIdx.x];
    if (offset >= (unsigned long long)a.room) return;   // (the whole workgroup: every pair is written by the chunks in front)
    const unsigned long long share = a.stage[rankEqualOff(a.nRange, a.room) + blockIdx.x], key = a.stage[2];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned long long lower = (1ull << lane) - 1ull;
    const long long i = (long long)blockIdx.x * kLanes + t;
    const RankLane r = rankLane(a, i);
    const bool isEqual = r.cand && r.key == key;
    const unsigned long long equalMask = __ballot(isEqual);
    if (lane == 0) waveEqual[wave] = (unsigned)__popcll(equalMask);
    __syncthreads();
    unsigned long long equalRank = (unsigned long long)__popcll(equalMask & lower);
    for (unsigned w = 0; w < wave; ++w) equalRank += waveEqual[w];
    const bool win = r.cand && (r.key < key || (isEqual && equalRank < share));
    const unsigned long long winMask = __ballot(win);
    if (lane == 0) waveWin[wave] = (unsigned)__popcll(winMask);
    __syncthreads();
    unsigned long long pos = offset + (unsigned long long)__popcll(winMask & lower);
    for (unsigned w = 0; w < wave; ++w) pos += waveWin[w];
    if (win && pos < (unsigned long long)a.room) {
        unsigned long long* const pair = a.stage + rankPairsOff() + 2 * pos;
        pair[0] = (unsigned long long)(a.firstGlobal + i);
        pair[1] = (unsigned long long)__double_as_longlong(r.v);
    }
}

}  // namespace

hipError_t launchMeterRank(const MeterRankArgs& a, hipStream_t stream) {
    if (!a.rows || !a.stage || a.n < 1 || a.nPad < a.n || a.channels < 1 || a.channels > 4 || a.family < kRankMeter || a.family > kRankTone) return hipErrorInvalidValue;
    if (a.stat < 0 || a.stat > (a.family == kRankMeter ? 3 : a.family == kRankTone ? kMeterMaxTones - 1 : 1)) return hipErrorInvalidValue;
    if (a.first < 0 || a.nRange < 1 || a.first > a.n - a.nRange || a.k < 0 || a.room != (a.k < a.nRange ? a.k : a.nRange) || a.threshold != a.threshold) return hipErrorInvalidValue;
    const long long chunks = meterSelectChunks(a.nRange);
    if (chunks >= ((long long)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipError_t e = hipMemsetAsync(a.stage + rankHistOff(a.room), 0, (rankBelowOff(a.room) - rankHistOff(a.room)) * 8, stream);
    for (int p = 0; p < kMeterRankPasses && e == hipSuccess; ++p) {
        hipLaunchKernelGGL(fx_rank_hist, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a, p);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fx_rank_count, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(fx_rank_scan, dim3(1), dim3(kLanes), 0, stream, a.stage + rankBelowOff(a.room), a.stage + rankEqualOff(a.nRange, a.room), a.stage, chunks);
    if ((e = hipGetLastError()) != hipSuccess || a.room == 0) return e;   // (a count query emits nothing)
    hipLaunchKernelGGL(fx_rank_emit, dim3((unsigned)chunks), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

// (the tone family, fx_meter_tone.hpp: the same launches)
hipError_t launchToneRank(const MeterRankArgs& a, hipStream_t stream) { return a.family == kRankTone ? launchMeterRank(a, stream) : hipErrorInvalidValue; }

}  // namespace fx
