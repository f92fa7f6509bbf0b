// fx_bus.hip — the kernels around the emulation launch of a bus block (fx_bus.hpp): expand a per-group input to the
// per-instance scratch, mix the scratch down to one word per group - plain (fx_bus_mix) or with per-instance gains (fx_bus_mix_gain) -
// gather a list of its columns into a narrow monitor side (fx_bus_tap), sum member lists of them onto aux buses (fx_bus_send_*), and
// build the scratch from per-instance lists of the columns of a narrow source block (fx_bus_feed).  gfx950, wave64, one wavefront per workgroup.  The narrow side,
// which may be pinned host memory behind PCIe, sees exactly one 256-byte access per wavefront and row.  The wide side: the expand
// stores 1 KiB per wavefront access; the mix loads 256 contiguous bytes per access for groups of 64 instances and more, and ONE
// PARTIAL access of K * 4 bytes per group for K < 64 (each followed by the whole shuffle tree: short groups are slow - K = 1 spends
// 64 trees on 256 bytes; packing several short groups into one load with a segmented tree of the same bits is open).  Groups above
// 64 are summed by one wavefront, four loads in flight: a group of a whole row (K = N) is one wavefront walking the row.
// Shared: treeSum, walkSum; weightOf, termOf, rampAt, RampRows; badRamp, byRampShape.  The plain and the weighted mix stay two
// written-out kernels: as entries over one inlined body they compile to more VGPRs (35 -> 38, 43 -> 47, 108 -> 120).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fx_bus.hpp"

namespace fx {

namespace {

constexpr unsigned kExpandSpan = 2048;   // floats of a row one wavefront writes: 8 stores of 1 KiB

__device__ __forceinline__ uint32_t laneWord(uint32_t v, unsigned src) { return (uint32_t)__shfl((int)v, (int)(src & 63u)); }

// grid.x = blocks of 64 groups x slices of kExpandSpan instances, grid.y strides over the rows.  Words are moved as bits: a NaN
// keeps its payload.
__global__ __launch_bounds__(64) void fx_bus_expand(BusArgs a, unsigned slices) {
    const unsigned lane = threadIdx.x;
    const unsigned K = (unsigned)a.group, n = (unsigned)a.n;
    const long long g0 = (long long)(blockIdx.x / slices) * 64;
    const long long lo = g0 * (long long)K + (long long)(blockIdx.x % slices) * kExpandSpan;
    long long hi = (g0 + 64) * (long long)K;
    if (hi > (long long)n) hi = n;
    if (hi > lo + (long long)kExpandSpan) hi = lo + kExpandSpan;
    if (lo >= hi) return;   // (the whole wavefront)
    const unsigned first = (unsigned)lo, end = (unsigned)hi, gFirst = (unsigned)g0;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.narrowIn);
    uint32_t* wide = reinterpret_cast<uint32_t*>(a.wide);
    for (long long row = blockIdx.y; row < a.rows; row += gridDim.y) {
        uint32_t v = 0;
        if (g0 + lane < a.groups) v = src[row * a.narrowPitch + g0 + lane];   // one 256-byte load
        uint32_t* dst = wide + row * a.n;
        // up to three words in front of the first 16-byte boundary, then whole uint4 stores, the ragged end word by word
        const unsigned head = (unsigned)((4u - (unsigned)((reinterpret_cast<uintptr_t>(dst + first) >> 2) & 3u)) & 3u);
        {
            const unsigned i = first + lane;
            const uint32_t w = laneWord(v, i / K - gFirst);
            if (lane < head && i < end) dst[i] = w;
        }
        for (unsigned base = first + head; base < end; base += 256u) {
            const unsigned i = base + lane * 4u;
            const unsigned at = i < end ? i : end - 1u;
            unsigned q = at / K, r = at - q * K;
            uint32_t w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                w[e] = laneWord(v, q - gFirst);
                if (++r == K) { r = 0; ++q; }
            }
            if (i + 4u <= end) {
                *reinterpret_cast<uint4*>(dst + i) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i + (unsigned)e < end) dst[i + e] = w[e];
            }
        }
    }
}

// the 64-lane shuffle-down tree; lanes at and beyond 64 - step take a value nobody reads
__device__ __forceinline__ float treeSum(float p) {
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) p = p + __shfl_down(p, step);
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p)));
}

// The long walk of the published sum order: the whole wavefront sums the `count` words load(m), four 256-byte loads in flight,
// then the tree (the plain mix above 64 members, the fold of the sends above one chunk).  Idx is the caller's index type.
template <class Idx, class Load>
__device__ __forceinline__ float walkSum(const Idx count, const unsigned lane, Load load) {
    float p = 0.0f;
    for (Idx m0 = 0; m0 < count; m0 += 256) {
        float v[4];
        bool have[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const Idx m = m0 + (Idx)(u * 64) + (Idx)lane;
            have[u] = m < count;
            v[u] = have[u] ? load(m) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) p = have[u] ? p + v[u] : p;
    }
    return treeSum(p);
}

// ---- the weights (fx_bus.hpp BusRampArgs), shared by the weighted mix, the sends and the feeds ---------------------------------
// The weight: (b - a), * t, a + ... and w * y are four roundings (the file is built with -ffp-contract=off); the mute is a
// select on w in front of the add, so a NaN or Inf of a muted member never reaches the sum.
template <bool kRamp>
__device__ __forceinline__ float weightOf(float a, float b, float t, bool atTarget) {
    if (!kRamp) return b;
    const float d = b - a;
    const float m = d * t;
    const float w = a + m;
    return atTarget ? b : w;
}

__device__ __forceinline__ float termOf(float w, float y) {
    const float prod = w * y;
    return w == 0.0f ? 0.0f : prod;
}

// where a row of the piece is on the ramp: t of weightOf, and whether it is the last sample of the CALL (exactly b there)
__device__ __forceinline__ void rampAt(const BusRampArgs& r, const long long row, float& t, bool& atTarget) {
    const long long s = row / r.channels + r.sample0;   // the sample of the CALL this row belongs to
    t = (float)(s + 1) * r.r;
    atTarget = s == (long long)r.samples - 1;
}

// The ramp-row frame of the kernels that keep kRows = 8 rows in flight (sends, feeds): per row its place on the ramp and whether it
// exists (kFull: all do, no predicate anywhere), and the gain rows the group reads.  Row groups begin at a multiple of eight rows,
// so with kCh = 1 or 2 channels row u is channel u % kCh; kCh = 0 is every other channel count, one gain row per row: gainOf(u).
template <int kRows, int kCh, bool kFull>
struct RampRows {
    static constexpr int kGains = kCh > 0 ? kCh : kRows;
    float t[kRows];
    bool atTarget[kRows], rowOk[kRows];
    long long gainRow[kGains];
    static constexpr int gainOf(int u) { return kCh > 0 ? u % kGains : u; }
};
template <int kRows, int kCh, bool kFull>
__device__ __forceinline__ RampRows<kRows, kCh, kFull> rampRows(const BusRampArgs& r, const long long gainPitch, const long long rows, const long long row0) {
    RampRows<kRows, kCh, kFull> f;
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
        rampAt(r, row0 + u, f.t[u], f.atTarget[u]);
        f.rowOk[u] = kFull || row0 + u < rows;
        if (kCh == 0) f.gainRow[u] = ((row0 + u) % r.channels) * gainPitch;
    }
#pragma unroll
    for (int c = 0; kCh > 0 && c < decltype(f)::kGains; ++c) f.gainRow[c] = (long long)c * gainPitch;
    return f;
}

// grid.x = blocks of 64 groups, grid.y strides over the rows: group g0 + k's sum ends in lane k, one 256-byte store per row
__global__ __launch_bounds__(64) void fx_bus_mix(BusArgs a) {
    const unsigned lane = threadIdx.x;
    const long long K = a.group;
    const long long g0 = (long long)blockIdx.x * 64;
    const int here = (int)(a.groups - g0 < 64 ? a.groups - g0 : 64);
    for (long long row = blockIdx.y; row < a.rows; row += gridDim.y) {
        const float* y = a.wide + row * a.n;
        float res = 0.0f;
        if (K <= 64) {
            // a group is one partial wavefront load: eight of them in flight at a time
            for (int k0 = 0; k0 < here; k0 += 8) {
                float v[8];
                bool have[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const long long first = (g0 + k0 + u) * K;
                    const long long count = a.n - first < K ? a.n - first : K;
                    have[u] = k0 + u < here && (long long)lane < count;
                    v[u] = have[u] ? y[first + lane] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    float p = 0.0f;
                    p = have[u] ? p + v[u] : p;
                    const float sum = treeSum(p);
                    if ((int)lane == k0 + u) res = sum;
                }
            }
        } else {
            for (int k = 0; k < here; ++k) {
                const long long first = (g0 + k) * K;
                const long long count = a.n - first < K ? a.n - first : K;
                const float sum = walkSum(count, lane, [&](const long long m) { return y[first + m]; });   // 256 contiguous bytes per load
                if ((int)lane == k) res = sum;
            }
        }
        if ((int)lane < here) a.narrowOut[row * a.narrowPitch + g0 + lane] = res;
    }
}

// ---- the weighted mix (fx_bus.hpp BusGainArgs): fx_bus_mix with every member multiplied by its weight first --------------------
//
// Same geometry, same loads of y, same trees, same one 256-byte store per row; a gain word is loaded beside every y word, with
// the same lane addressing (gain[c][first + lane]: 256 contiguous bytes per access for K >= 64, one partial access per short
// group).  The gain words of a wavefront's groups do not depend on the sample, but a workgroup handles ONE row unless a block has
// more than 65 535 of them (grid.y = rows), so there is nothing to keep in registers across rows: every row re-reads its gains,
// [C][n] words that 2 * S rows share and the L2 / Infinity Cache hold.  kRamp = false loads the target block only.
template <bool kRamp>
__global__ __launch_bounds__(64) void fx_bus_mix_gain(BusArgs a, BusGainArgs g) {
    const unsigned lane = threadIdx.x;
    const long long K = a.group;
    const long long g0 = (long long)blockIdx.x * 64;
    const int here = (int)(a.groups - g0 < 64 ? a.groups - g0 : 64);
    for (long long row = blockIdx.y; row < a.rows; row += gridDim.y) {
        const float* y = a.wide + row * a.n;
        const long long gainRow = (row % g.channels) * g.gainPitch;    // the row's channel's row of the gain blocks
        float t;
        bool atTarget;
        rampAt(g, row, t, atTarget);
        float res = 0.0f;
        if (K <= 64) {
            for (int k0 = 0; k0 < here; k0 += 8) {
                // (all loads of the eight groups are issued before the first weight is computed)
                float v[8], ga[8], gb[8];
                bool have[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const long long first = (g0 + k0 + u) * K;
                    const long long count = a.n - first < K ? a.n - first : K;
                    have[u] = k0 + u < here && (long long)lane < count;
                    v[u] = ga[u] = gb[u] = 0.0f;
                    if (have[u]) {
                        v[u] = y[first + lane];
                        gb[u] = g.target[gainRow + first + lane];
                        if (kRamp) ga[u] = g.current[gainRow + first + lane];
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    float p = 0.0f;
                    p = have[u] ? p + termOf(weightOf<kRamp>(ga[u], gb[u], t, atTarget), v[u]) : p;
                    const float sum = treeSum(p);
                    if ((int)lane == k0 + u) res = sum;
                }
            }
        } else {
            for (int k = 0; k < here; ++k) {
                const long long first = (g0 + k) * K;
                const long long count = a.n - first < K ? a.n - first : K;
                float p = 0.0f;
                for (long long m0 = 0; m0 < count; m0 += 256) {
                    float v[4], ga[4], gb[4];
                    bool have[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const long long m = m0 + u * 64 + lane;
                        have[u] = m < count;
                        v[u] = ga[u] = gb[u] = 0.0f;
                        if (have[u]) {   // 256 contiguous bytes per load, of y and of each gain block
                            v[u] = y[first + m];
                            gb[u] = g.target[gainRow + first + m];
                            if (kRamp) ga[u] = g.current[gainRow + first + m];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) p = have[u] ? p + termOf(weightOf<kRamp>(ga[u], gb[u], t, atTarget), v[u]) : p;
                }
                const float sum = treeSum(p);
                if ((int)lane == k) res = sum;
            }
        }
        if ((int)lane < here) a.narrowOut[row * a.narrowPitch + g0 + lane] = res;
    }
}

// ---- the taps (fx_bus.hpp BusTapArgs): columns idx[t] of the scratch block to a narrow side, as bit patterns --------------------
//
// One wavefront per workgroup; grid.x = blocks of 64 taps, grid.y = chunks of kTapRows rows (a loop where a block has more chunks
// than a grid may have).  A lane owns one tap: it reads its instance number (and its column) once and then, per chunk, issues
// kTapRows independent loads - one per row, a 32-bit byte stride of n * 4 apart - before the first store.  Per row the 64 stores
// of a wavefront are contiguous (identity columns), which is what the narrow side wants when it is pinned host memory; the loads
// are a gather - wherever the list points, T words per row out of a block the emulation has just written.  With S * C = 32 rows
// and T = 64 that is four wavefronts of eight loads each; nothing here scales with n.  No LDS, no floating-point instruction.
constexpr int kTapRows = 8;   // row loads in flight per lane

__global__ __launch_bounds__(64) void fx_bus_tap(BusTapArgs a) {
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= a.taps) return;
    const uint32_t inst = a.idx[t];
    const uint32_t column = a.col ? a.col[t] : (uint32_t)t;
    const uint32_t loadStride = (uint32_t)a.n * 4u, storeStride = (uint32_t)a.tapPitch * 4u;   // (both below 2^32: launchBusTap)
    const long long chunks = (a.rows + kTapRows - 1) / kTapRows;
    for (long long chunk = blockIdx.y; chunk < chunks; chunk += gridDim.y) {
        const long long row0 = chunk * kTapRows;
        const char* p = reinterpret_cast<const char*>(a.wide + row0 * a.n + inst);
        char* q = reinterpret_cast<char*>(a.tapOut + row0 * a.tapPitch + column);
        if (row0 + kTapRows <= a.rows) {
            uint32_t v[kTapRows];
#pragma unroll
            for (int u = 0; u < kTapRows; ++u) {
                v[u] = *reinterpret_cast<const uint32_t*>(p);
                p += loadStride;
            }
#pragma unroll
            for (int u = 0; u < kTapRows; ++u) {
                *reinterpret_cast<uint32_t*>(q) = v[u];
                q += storeStride;
            }
        } else {
            for (long long row = row0; row < a.rows; ++row) {
                *reinterpret_cast<uint32_t*>(q) = *reinterpret_cast<const uint32_t*>(p);
                p += loadStride;
                q += storeStride;
            }
        }
    }
}

// ---- the sends (fx_bus.hpp BusSendArgs): aux buses by member list, summed chunk by chunk --------------------------------------
//
// fx_bus_send_chunks: grid.x = the chunks of the host-built table, grid.y = groups of kSendRows rows (a loop where a block has
// more groups than a grid may have).  A chunk is at most 1 024 consecutive entries of ONE bus: sixteen 64-lane steps.  Per step a
// lane loads its instance number and its gain words once (256 contiguous bytes per wavefront each) and then issues the eight
// rows' gathers wide[row][idx] - a 32-bit byte stride of n * 4 apart - before the first add, as fx_bus_tap does; eight partial
// sums stay in registers.  After the last step come eight trees, and lanes 0..7 store the eight chunk sums to partial[row][chunk].
// The gain words depend on the row's channel (RampRows): kCh = 1 and 2 load one and two words per block and step, kCh = 0 per row.
// A ragged last group predicates its loads and stores by row: nothing outside the block's rows is read.  The index and the gain
// words of step j + 1 are requested behind the gathers of step j, so that only a chunk's first step waits for them.
constexpr int kSendRows = 8;

// one chunk over the eight rows from row0 on; kFull: all eight exist (no predicate anywhere)
template <bool kRamp, int kCh, bool kFull>
__device__ __forceinline__ void sendRowGroup(const BusSendArgs& a, const BusSendChunk ck, const long long row0, const unsigned lane) {
    const uint32_t loadStride = (uint32_t)a.n * 4u;   // (below 2^32: launchBusSend)
    const auto f = rampRows<kSendRows, kCh, kFull>(a, a.gainPitch, a.rows, row0);
    constexpr int kGains = decltype(f)::kGains;
    float p[kSendRows];
#pragma unroll
    for (int u = 0; u < kSendRows; ++u) p[u] = 0.0f;
    const char* base = reinterpret_cast<const char*>(a.wide + row0 * a.n);
    // a step's instance number and gain words (lanes beyond the chunk's end read its first entry and add nothing)
    auto fetch = [&](uint32_t m0, uint32_t& inst, float (&ga)[kGains], float (&gb)[kGains]) {
        const uint32_t m = m0 + lane;
        const uint32_t e = ck.first + (m < ck.count ? m : 0u);
        inst = a.idx[e];
#pragma unroll
        for (int c = 0; c < kGains; ++c) {
            const bool need = kCh > 0 || f.rowOk[c];
            gb[c] = need ? a.target[f.gainRow[c] + e] : 0.0f;
            ga[c] = (kRamp && need) ? a.current[f.gainRow[c] + e] : 0.0f;
        }
    };
    uint32_t inst;
    float ga[kGains], gb[kGains];
    fetch(0u, inst, ga, gb);
    for (uint32_t m0 = 0; m0 < ck.count; m0 += 64u) {
        const bool have = m0 + lane < ck.count;
        float y[kSendRows];
        const char* q = base + (size_t)inst * 4u;
#pragma unroll
        for (int u = 0; u < kSendRows; ++u) {
            y[u] = f.rowOk[u] ? *reinterpret_cast<const float*>(q) : 0.0f;
            q += loadStride;
        }
        // the next step's index and gains go out behind this step's gathers, so that only the first step waits for them
        uint32_t instNext = inst;
        float gaNext[kGains], gbNext[kGains];
#pragma unroll
        for (int c = 0; c < kGains; ++c) gaNext[c] = gbNext[c] = 0.0f;
        if (m0 + 64u < ck.count) fetch(m0 + 64u, instNext, gaNext, gbNext);
#pragma unroll
        for (int u = 0; u < kSendRows; ++u) {
            const int c = f.gainOf(u);
            const float term = termOf(weightOf<kRamp>(ga[c], gb[c], f.t[u], f.atTarget[u]), y[u]);
            p[u] = have ? p[u] + term : p[u];
        }
        inst = instNext;
#pragma unroll
        for (int c = 0; c < kGains; ++c) {
            ga[c] = gaNext[c];
            gb[c] = gbNext[c];
        }
    }
    float mine = 0.0f;
#pragma unroll
    for (int u = 0; u < kSendRows; ++u) {
        const float sum = treeSum(p[u]);
        if ((int)lane == u) mine = sum;
    }
    if (lane < (unsigned)kSendRows && (kFull || row0 + lane < a.rows)) a.partial[(row0 + lane) * a.chunks + blockIdx.x] = mine;
}

template <bool kRamp, int kCh>
__global__ __launch_bounds__(64) void fx_bus_send_chunks(BusSendArgs a) {
    const unsigned lane = threadIdx.x;
    const BusSendChunk ck = a.chunk[blockIdx.x];
    const long long groups = (a.rows + kSendRows - 1) / kSendRows;
    for (long long grp = blockIdx.y; grp < groups; grp += gridDim.y) {
        const long long row0 = grp * kSendRows;
        if (row0 + kSendRows <= a.rows) sendRowGroup<kRamp, kCh, true>(a, ck, row0, lane);
        else sendRowGroup<kRamp, kCh, false>(a, ck, row0, lane);
    }
}

// fx_bus_send_fold: the ragged fx_bus_mix over partial.  grid.x = blocks of 64 buses, grid.y strides over the rows.  Lane k takes
// bus g0 + k: +0.0f for an empty one, a copy of its chunk sum for one chunk (all such lanes in one gather); a bus of more chunks
// is walked by the whole wavefront, 256 contiguous bytes per load, one tree, and its word lands in lane k.  One 256-byte store per
// wavefront and row to the narrow side (identity columns), or to the columns of the table.
__global__ __launch_bounds__(64) void fx_bus_send_fold(BusSendArgs a) {
    const unsigned lane = threadIdx.x;
    const long long g0 = (long long)blockIdx.x * 64;
    const bool mineHere = g0 + lane < a.buses;
    BusSendBus b{0u, 0u, 0u};
    if (mineHere) b = a.bus[g0 + lane];
    const uint32_t column = a.columns ? b.column : (uint32_t)(g0 + lane);
    const unsigned long long wideBuses = __ballot(mineHere && b.chunks > 1u);
    for (long long row = blockIdx.y; row < a.rows; row += gridDim.y) {
        const float* c = a.partial + row * a.chunks;
        float res = 0.0f;
        if (mineHere && b.chunks == 1u) res = c[b.firstChunk];
        for (unsigned long long left = wideBuses; left != 0ull; left &= left - 1ull) {
            const int k = __ffsll((long long)left) - 1;
            const uint32_t first = laneWord(b.firstChunk, (unsigned)k), count = laneWord(b.chunks, (unsigned)k);
            const float sum = walkSum(count, lane, [&](const uint32_t m) { return c[first + m]; });
            if ((int)lane == k) res = sum;
        }
        if (mineHere) a.auxOut[row * a.auxPitch + column] = res;
    }
}

// ---- the feeds (fx_bus.hpp BusFeedArgs): the scratch block built from per-instance lists of source columns -------------------
//
// fx_bus_feed: grid.x = spans of kFeedSpan instances, grid.y = groups of kFeedRows rows (a loop where a block has more groups than
// a grid may have).  A lane owns FOUR consecutive instances of a row, the same four in every row of a group: it loads their
// offsets, source columns and gain words once per group (one 16-byte access per table, 1 KiB contiguous per wavefront) and issues
// the gathers src[row][idx] of all eight rows - a 32-bit byte stride of m * 4 apart, out of a block of m * 4 bytes per row that
// the L2 holds - before the first add.  The wide side is written as fx_bus_expand writes it: one aligned uint4 store per lane and
// row, 1 KiB per wavefront.  Where a row's span does not begin on a 16-byte boundary (n not a multiple of 4: the boundary moves
// from row to row) a lane's quad is the tail of its own four words and the head of its neighbour's, fetched by three shuffles;
// the words in front of the first boundary and at the ragged end go one by one.
//   kMap:  every instance has exactly one entry, entry i is instance i's: no offsets, no loop.
//   else:  CSR; a lane walks entry j of its four instances together, up to the longest of their lists.
//   kMode: 0 unweighted (words move as bit patterns), 1 weighted, 2 weighted with a ramp pending.  kCh as fx_bus_send_chunks.
// A ragged last group predicates its loads and stores by row: nothing outside the block's rows is read or written.
constexpr int kFeedRows = 8;
constexpr unsigned kFeedSpan = 256;   // instances of a row one wavefront writes: one store of 1 KiB

// the words w of instances i .. i + 3 (i = the span's first + lane * 4) to one row; end: behind the span's last instance
__device__ __forceinline__ void feedStoreRow(uint32_t* dstRow, const unsigned i, const unsigned end, const uint32_t (&w)[4], const unsigned lane) {
    // the words in front of the lane's 16-byte boundary: the same number in every lane
    const unsigned h = (unsigned)__builtin_amdgcn_readfirstlane((int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(dstRow + i) >> 2) & 3u)) & 3u));
    if (h == 0u) {
        if (i + 4u <= end) {
            *reinterpret_cast<uint4*>(dstRow + i) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + (unsigned)e < end) dstRow[i + e] = w[e];
        }
        return;
    }
    // the aligned quad i + h .. i + h + 3: this lane's last 4 - h words and the next lane's first h
    const uint32_t n0 = (uint32_t)__shfl_down((int)w[0], 1), n1 = (uint32_t)__shfl_down((int)w[1], 1), n2 = (uint32_t)__shfl_down((int)w[2], 1);
    uint4 q;
    if (h == 1u) q = make_uint4(w[1], w[2], w[3], n0);
    else if (h == 2u) q = make_uint4(w[2], w[3], n0, n1);
    else q = make_uint4(w[3], n0, n1, n2);
    // the h words in front belong to the previous lane's quad - which lane 0 has none of, and a lane at the ragged end neither
    if (lane == 0u || i + h > end) {
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if ((unsigned)e < h && i + (unsigned)e < end) dstRow[i + e] = w[e];
    }
    if (lane < 63u && i + h + 4u <= end) {
        *reinterpret_cast<uint4*>(dstRow + i + h) = q;
    } else {
#pragma unroll
        for (int e = 1; e < 4; ++e)
            if ((unsigned)e >= h && i + (unsigned)e < end) dstRow[i + e] = w[e];
    }
}

// one span over the eight rows from row0 on; kFull: all eight exist (no row predicate anywhere)
template <bool kMap, int kMode, int kCh, bool kFull>
__device__ __forceinline__ void feedRowGroup(const BusFeedArgs& a, const long long row0, const unsigned lane, const unsigned i, const unsigned end) {
    constexpr bool kWeighted = kMode > 0, kRamp = kMode == 2;
    const uint32_t srcStride = (uint32_t)a.m * 4u;   // (below 2^32: launchBusFeed)
    RampRows<kFeedRows, kCh, kFull> f;   // (filled here: built by rampRows, the instantiation <false, 2, 0> takes a VGPR more)
    constexpr int kGains = f.kGains;
#pragma unroll
    for (int u = 0; u < kFeedRows; ++u) {
        rampAt(a, row0 + u, f.t[u], f.atTarget[u]);
        f.rowOk[u] = kFull || row0 + u < a.rows;
        if (kCh == 0) f.gainRow[u] = ((row0 + u) % a.channels) * a.gainPitch;
    }
#pragma unroll
    for (int c = 0; kCh > 0 && c < kGains; ++c) f.gainRow[c] = (long long)c * a.gainPitch;
    uint32_t w[kFeedRows][4];
#pragma unroll
    for (int u = 0; u < kFeedRows; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) w[u][k] = 0u;
    const char* base = reinterpret_cast<const char*>(a.src + row0 * a.m);
    if (i < end) {
        if (kMap) {
            const uint4 ix4 = *reinterpret_cast<const uint4*>(a.idx + i);
            const uint32_t ix[4] = {ix4.x, ix4.y, ix4.z, ix4.w};
            float ga[kGains][4], gb[kGains][4];
#pragma unroll
            for (int c = 0; c < kGains; ++c) {
                float4 b4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a4 = b4;
                if (kWeighted && (kCh > 0 || f.rowOk[c])) {
                    b4 = *reinterpret_cast<const float4*>(a.target + f.gainRow[c] + i);
                    if (kRamp) a4 = *reinterpret_cast<const float4*>(a.current + f.gainRow[c] + i);
                }
                gb[c][0] = b4.x; gb[c][1] = b4.y; gb[c][2] = b4.z; gb[c][3] = b4.w;
                ga[c][0] = a4.x; ga[c][1] = a4.y; ga[c][2] = a4.z; ga[c][3] = a4.w;
            }
            uint32_t x[kFeedRows][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const char* p = base + (size_t)ix[k] * 4u;
#pragma unroll
                for (int u = 0; u < kFeedRows; ++u) {
                    x[u][k] = f.rowOk[u] ? *reinterpret_cast<const uint32_t*>(p) : 0u;
                    p += srcStride;
                }
            }
#pragma unroll
            for (int u = 0; u < kFeedRows; ++u) {
                const int c = f.gainOf(u);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    w[u][k] = kWeighted ? __builtin_bit_cast(uint32_t, termOf(weightOf<kRamp>(ga[c][k], gb[c][k], f.t[u], f.atTarget[u]), __builtin_bit_cast(float, x[u][k])))
                                        : x[u][k];
            }
        } else {
            const uint4 o4 = *reinterpret_cast<const uint4*>(a.off + i);
            const uint32_t o[5] = {o4.x, o4.y, o4.z, o4.w, a.off[i + 4u]};
            uint32_t count[4], longest = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                count[k] = o[k + 1] - o[k];
                longest = count[k] > longest ? count[k] : longest;
            }
            float acc[kFeedRows][4];
            // entry j of the lane's four instances: index and gain words, the 32 gathers, then the adds - the first term starts the sum
            auto step = [&](const uint32_t j, auto first) {
                uint32_t ix[4];
                bool has[4];
                float ga[kGains][4], gb[kGains][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    has[k] = j < count[k];
                    const uint32_t e = o[k] + j;
                    ix[k] = has[k] ? a.idx[e] : 0u;
#pragma unroll
                    for (int c = 0; c < kGains; ++c) {
                        const bool need = kWeighted && has[k] && (kCh > 0 || f.rowOk[c]);
                        gb[c][k] = need ? a.target[f.gainRow[c] + e] : 0.0f;
                        ga[c][k] = (kRamp && need) ? a.current[f.gainRow[c] + e] : 0.0f;
                    }
                }
                uint32_t x[kFeedRows][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const char* p = base + (size_t)ix[k] * 4u;
#pragma unroll
                    for (int u = 0; u < kFeedRows; ++u) {
                        x[u][k] = (has[k] && f.rowOk[u]) ? *reinterpret_cast<const uint32_t*>(p) : 0u;
                        p += srcStride;
                    }
                }
#pragma unroll
                for (int u = 0; u < kFeedRows; ++u) {
                    const int c = f.gainOf(u);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float xf = __builtin_bit_cast(float, x[u][k]);
                        const float term = kWeighted ? termOf(weightOf<kRamp>(ga[c][k], gb[c][k], f.t[u], f.atTarget[u]), xf) : xf;
                        if (decltype(first)::value) acc[u][k] = has[k] ? term : 0.0f;
                        else acc[u][k] = has[k] ? acc[u][k] + term : acc[u][k];
                    }
                }
            };
            step(0u, std::true_type{});
            for (uint32_t j = 1u; j < longest; ++j) step(j, std::false_type{});
#pragma unroll
            for (int u = 0; u < kFeedRows; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) w[u][k] = __builtin_bit_cast(uint32_t, acc[u][k]);
        }
    }
    uint32_t* dst = a.wide + row0 * a.n;
#pragma unroll
    for (int u = 0; u < kFeedRows; ++u) {
        if (f.rowOk[u]) feedStoreRow(dst, i, end, w[u], lane);   // (the same rows in every lane)
        dst += a.n;
    }
}

template <bool kMap, int kMode, int kCh>
__global__ __launch_bounds__(64) void fx_bus_feed(BusFeedArgs a) {
    const unsigned lane = threadIdx.x;
    const unsigned first = blockIdx.x * kFeedSpan, n = (unsigned)a.n;
    const unsigned end = n - first < kFeedSpan ? n : first + kFeedSpan;
    const unsigned i = first + lane * 4u;
    const long long groups = (a.rows + kFeedRows - 1) / kFeedRows;
    for (long long grp = blockIdx.y; grp < groups; grp += gridDim.y) {
        const long long row0 = grp * kFeedRows;
        if (row0 + kFeedRows <= a.rows) feedRowGroup<kMap, kMode, kCh, true>(a, row0, lane, i, end);
        else feedRowGroup<kMap, kMode, kCh, false>(a, row0, lane, i, end);
    }
}

// ---- gain sets by list (fx_bus.hpp GainScatterArgs): the moved faders of a block, scattered into the gain blocks ------------------
//
// One wavefront per workgroup, one lane per list entry: grid.x = blocks of 64 entries.  A lane loads its position once, then per
// channel one word of the staged values - consecutive lanes read consecutive words, 256 bytes per wavefront - and stores it at its
// position in b, and in a where the set writes both.  The stores go wherever the list points; no two lanes share a word (the host
// refuses a repeated index), so there is nothing to order.  Plain 32-bit loads and stores: no LDS, no atomics, no floating point.
__global__ __launch_bounds__(64) void fx_gain_scatter(GainScatterArgs g) {
    const long long k = (long long)blockIdx.x * 64 + threadIdx.x;
    if (k >= g.count) return;
    const uint32_t i = g.idx[k];
    if ((long long)i >= g.pitch) return;   // (never, behind the host's range check: a word outside the blocks is not written whatever the list holds)
    const uint32_t* v = g.val + k;
    uint32_t* b = g.b + i;
    uint32_t* a = g.a ? g.a + i : nullptr;
    for (int c = 0; c < g.channels; ++c) {
        const uint32_t w = *v;
        *b = w;
        if (a) {
            *a = w;
            a += g.pitch;
        }
        v += g.count;
        b += g.pitch;
    }
}

inline bool badArgs(const BusArgs& a) { return a.rows < 1 || a.n < 1 || a.group < 1 || a.group > a.n || a.groups != (a.n + a.group - 1) / a.group || a.narrowPitch < a.groups || !a.wide; }

// the ramp block of a launch over `rows` rows: whole samples always; weighted, the piece lies inside the caller's block and a
// pending ramp has its a block (haveCurrent); unweighted (feeds only) nothing else is read, and a ramp is refused
inline bool badRamp(const BusRampArgs& r, long long rows, bool weighted, bool haveCurrent) {
    if (r.channels < 1 || rows % r.channels != 0) return true;
    if (!weighted) return r.ramp != 0;
    return r.samples < 1 || r.sample0 < 0 || (long long)r.sample0 + rows / r.channels > (long long)r.samples || (r.ramp && !haveCurrent);
}

// the one ladder from (ramp pending, channels) to a kernel's <kRamp, kCh> instantiation: launch(kRamp, kCh), as integral_constants
template <class Launch>
void byRampShape(const BusRampArgs& r, Launch launch) {
    const auto byChannels = [&](auto kRamp) {
        if (r.channels == 1) launch(kRamp, std::integral_constant<int, 1>{});
        else if (r.channels == 2) launch(kRamp, std::integral_constant<int, 2>{});
        else launch(kRamp, std::integral_constant<int, 0>{});
    };
    if (r.ramp) byChannels(std::true_type{});
    else byChannels(std::false_type{});
}

}  // namespace

hipError_t launchBusExpand(const BusArgs& a, hipStream_t stream) {
    if (badArgs(a) || !a.narrowIn || a.n >= ((long long)1 << 31)) return hipErrorInvalidValue;
    const long long blocks = (a.groups + 63) / 64;
    const long long widest = 64 * a.group < a.n ? 64 * a.group : a.n;   // instances of a block of 64 groups
    const long long slices = (widest + kExpandSpan - 1) / kExpandSpan;
    if (blocks * slices >= ((long long)1 << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(blocks * slices), (unsigned)(a.rows < 65535 ? a.rows : 65535));
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_bus_expand, grid, dim3(64), 0, stream, a, (unsigned)slices);
    return hipGetLastError();
}

// either mix: g null is the plain one
static hipError_t launchMix(const BusArgs& a, const BusGainArgs* g, hipStream_t stream) {
    if (badArgs(a) || !a.narrowOut) return hipErrorInvalidValue;
    if (g && (!g->target || g->gainPitch < a.n || badRamp(*g, a.rows, true, g->current != nullptr))) return hipErrorInvalidValue;
    const long long blocks = (a.groups + 63) / 64;
    if (blocks >= ((long long)1 << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)(a.rows < 65535 ? a.rows : 65535));
    (void)hipGetLastError();
    if (!g) hipLaunchKernelGGL(fx_bus_mix, grid, dim3(64), 0, stream, a);
    else if (g->ramp) hipLaunchKernelGGL(fx_bus_mix_gain<true>, grid, dim3(64), 0, stream, a, *g);
    else hipLaunchKernelGGL(fx_bus_mix_gain<false>, grid, dim3(64), 0, stream, a, *g);
    return hipGetLastError();
}
hipError_t launchBusMix(const BusArgs& a, hipStream_t stream) { return launchMix(a, nullptr, stream); }
hipError_t launchBusMixGain(const BusArgs& a, const BusGainArgs& g, hipStream_t stream) { return launchMix(a, &g, stream); }

hipError_t launchBusTap(const BusTapArgs& a, hipStream_t stream) {
    constexpr long long kMostTaps = 65536;
    if (!a.wide || !a.tapOut || !a.idx || a.rows < 1 || a.n < 1 || a.n >= ((long long)1 << 30) || a.taps < 1 || a.taps > kMostTaps ||
        a.tapPitch < a.taps || a.tapPitch > kMostTaps)
        return hipErrorInvalidValue;
    const long long chunks = (a.rows + kTapRows - 1) / kTapRows;
    const dim3 grid((unsigned)((a.taps + 63) / 64), (unsigned)(chunks < 65535 ? chunks : 65535));
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_bus_tap, grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchBusSend(const BusSendArgs& a, hipStream_t stream) {
    constexpr long long kMostBuses = 65536, kMostEntries = (long long)1 << 24;
    if (!a.wide || !a.bus || !a.auxOut || a.rows < 1 || a.n < 1 || a.n >= ((long long)1 << 30) || a.buses < 1 || a.buses > kMostBuses || a.auxPitch < a.buses ||
        a.auxPitch > kMostBuses || a.entries < 0 || a.entries > kMostEntries || a.chunks < 0 || a.chunks > a.entries || a.chunks > kMostEntries / kSendChunk + kMostBuses ||
        (a.entries > 0) != (a.chunks > 0) || badRamp(a, a.rows, true, a.current || a.chunks == 0))   // (without a chunk nothing reads a)
        return hipErrorInvalidValue;
    if (a.chunks > 0 && (!a.idx || !a.target || !a.chunk || !a.partial || a.gainPitch < a.entries)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    if (a.chunks > 0) {
        const long long groups = (a.rows + kSendRows - 1) / kSendRows;
        const dim3 grid((unsigned)a.chunks, (unsigned)(groups < 65535 ? groups : 65535));
        byRampShape(a, [&](auto kRamp, auto kCh) {
            hipLaunchKernelGGL((fx_bus_send_chunks<decltype(kRamp)::value, decltype(kCh)::value>), grid, dim3(64), 0, stream, a);
        });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((a.buses + 63) / 64), (unsigned)(a.rows < 65535 ? a.rows : 65535));
    hipLaunchKernelGGL(fx_bus_send_fold, grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchBusFeed(const BusFeedArgs& a, hipStream_t stream) {
    constexpr long long kMostEntries = (long long)1 << 24;
    const auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const bool map = !a.off;
    const long long n4 = (a.n + 3) / 4 * 4;
    if (!a.src || !a.wide || a.rows < 1 || a.n < 1 || a.n >= ((long long)1 << 30) || a.m < 1 || a.m >= ((long long)1 << 30) || a.entries < 0 || a.entries > kMostEntries ||
        (map && a.entries != a.n) || (a.entries > 0 && !a.idx) || !aligned16(a.off) || !aligned16(a.idx) || badRamp(a, a.rows, a.target != nullptr, a.current != nullptr))
        return hipErrorInvalidValue;
    if (a.target && (a.gainPitch < a.entries || (map && (a.gainPitch < n4 || a.gainPitch % 4 != 0 || !aligned16(a.target) || !aligned16(a.current))))) return hipErrorInvalidValue;
    const long long groups = (a.rows + kFeedRows - 1) / kFeedRows;
    const dim3 grid((unsigned)((a.n + kFeedSpan - 1) / kFeedSpan), (unsigned)(groups < 65535 ? groups : 65535));
    (void)hipGetLastError();
    // unweighted: one instantiation; weighted: kMode = 1 or 2 by the ramp, on the ladder of the sends
    const auto launch = [&](auto kMap) {
        constexpr bool kM = decltype(kMap)::value;
        if (!a.target) hipLaunchKernelGGL((fx_bus_feed<kM, 0, 1>), grid, dim3(64), 0, stream, a);
        else byRampShape(a, [&](auto kRamp, auto kCh) {
            hipLaunchKernelGGL((fx_bus_feed<kM, decltype(kRamp)::value ? 2 : 1, decltype(kCh)::value>), grid, dim3(64), 0, stream, a);
        });
    };
    if (map) launch(std::true_type{});
    else launch(std::false_type{});
    return hipGetLastError();
}

hipError_t launchGainScatter(const GainScatterArgs& a, hipStream_t stream) {
    if (!a.idx || !a.val || !a.b || a.count < 1 || a.pitch < 1 || a.count > a.pitch || a.pitch >= ((long long)1 << 32) || a.channels < 1) return hipErrorInvalidValue;
    const long long blocks = (a.count + 63) / 64;
    if (blocks >= ((long long)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_gain_scatter, dim3((unsigned)blocks), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fx
