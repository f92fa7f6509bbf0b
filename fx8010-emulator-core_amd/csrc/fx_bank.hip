// fx_bank.hip — the kernels behind the record bank (fx_bank.hpp): the gather of fx_instances.hip with the packed side in the bank
// (fx_bank_gather), the rotations of a recall worked out on the device (fx_bank_rotations), and the rotating scatter of
// fx_instances.hip with the bank as its source and a gate in front (fx_bank_scatter_rot).  gfx950, wave64, workgroups of 256 lanes.
//
// The tile scheme is that of fx_instances.hip, access for access: 64 list entries x 64 record words through LDS as [64][64 + 1]
// dwords, lanes along the entries on the batch side, lanes along the words on the packed side.  The packed side is
// bank[slot[e] * W + w]: a wavefront's 64 lanes hold ONE entry there (64 consecutive words of a pass belong to one entry), so the
// slot is wave-uniform and the 256-byte accesses stay whole.  The slot words of the tile's 64 entries are loaded once per
// workgroup, into LDS.
//
// Every access is one dword moved as a bit pattern, every offset is 64-bit (nSlots * W * 4 passes 2^32 easily).  Lanes beyond
// `count` or beyond the W words touch no memory; an entry outside [0, n) or a slot outside [0, nSlots) - the runtime refuses such
// lists before it launches - is skipped rather than followed.
//
// THE GATE.  fx_bank_rotations adds to cells[kBankCellFaults] with a vector atomic for every record the rule refuses.  The
// scatter is a later kernel on the same stream: it reads the cell with a plain load, and every workgroup leaves in front of its
// first store when the cell is not zero - a refused recall changes no word of the batch.  Workgroup (0, 0) notes the refusal in the
// kept cells; it is the only writer of those, and the host reads them behind the stream.
#include <hip/hip_runtime.h>

#include "fx_bank.hpp"

namespace fx {

namespace {

constexpr int kLanes = 256;
constexpr int kTI = 64;                          // list entries of a tile
constexpr int kTW = 64;                          // record words of a tile
constexpr int kPasses = kTI * kTW / kLanes;      // loads in flight per lane
constexpr int kRowsPerPass = kLanes / kTI;       // batch side: words of one entry column covered by a pass

// where word w of the lane's instance lives: stateAt = inst, iAt / xAt = its column in slot 0 of its wavefront tile
__device__ __forceinline__ uint32_t* wordOf(const InstArgs& a, long long w, long long stateAt, long long iAt, long long xAt) {
    if (w < a.stateRows) return a.state + w * a.nPad + stateAt;
    w -= a.stateRows;
    if (w < a.iSlots) return a.itram + iAt + w * a.cols;
    return a.xtram + xAt + (w - a.iSlots) * a.cols;
}

// the slot of a slot word, or -1 for one outside the bank
__device__ __forceinline__ long long slotOf(long long word, long long nSlots) {
    const long long s = word & 0xffffffffll;
    return s < nSlots ? s : -1;
}

// grid.x = tiles of kTI list entries, grid.y strides over the tiles of kTW record words
__global__ __launch_bounds__(kLanes) void fx_bank_gather(BankArgs b) {
    __shared__ uint32_t tile[kTI * (kTW + 1)];
    __shared__ long long slotAt[kTI];
    const InstArgs& a = b.base;
    const unsigned t = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * kTI;
    const long long W = (long long)a.stateRows + a.iSlots + a.xSlots;
    if (t < kTI) slotAt[t] = e0 + t < a.count ? slotOf(b.slots[e0 + t], b.nSlots) : -1;
    const unsigned c = t % kTI, q = t / kTI;
    long long inst = -1;
    if (e0 + c < a.count) inst = a.list[e0 + c];
    const bool listed = inst >= 0 && inst < a.n;
    const long long wave = listed ? inst / a.cols : 0, col = listed ? inst % a.cols : 0;
    const long long iAt = wave * a.iSlots * a.cols + col, xAt = wave * a.xSlots * a.cols + col;
    __syncthreads();
    for (long long w0 = (long long)blockIdx.y * kTW; w0 < W; w0 += (long long)gridDim.y * kTW) {
        uint32_t v[kPasses];
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const long long w = w0 + k * kRowsPerPass + q;
            v[k] = (listed && w < W) ? *wordOf(a, w, inst, iAt, xAt) : 0u;
        }
#pragma unroll
        for (int k = 0; k < kPasses; ++k) tile[c * (kTW + 1) + k * kRowsPerPass + q] = v[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
            const long long w = w0 + wl, slot = slotAt[el];
            if (slot >= 0 && w < W) b.bank[slot * W + w] = tile[el * (kTW + 1) + wl];
        }
        __syncthreads();   // (the tile is refilled by the next turn of the loop)
    }
}

// One lane per (entry, line): two words of the record, two of the destination's position rows, the pair, and the fault cells.
__global__ __launch_bounds__(kLanes) void fx_bank_rotations(BankRotArgs r) {
    const InstArgs& a = r.bank.base;
    const long long at = (long long)blockIdx.x * kLanes + threadIdx.x, e = at >> 1;
    const int which = (int)(at & 1);
    if (e >= a.count) return;
    const BankLine l = r.line[which];
    const long long W = (long long)a.stateRows + a.iSlots + a.xSlots;
    const long long word = r.bank.slots[e], slot = slotOf(word, r.bank.nSlots), inst = a.list[e];
    int d = 0, fault = 0;
    // (the program has no memory on this line: nothing to rotate, nothing reads the positions)
    if (l.slots > 0 && l.size >= 1 && slot >= 0 && inst >= 0 && inst < a.n) {
        const uint32_t* rec = r.bank.bank + slot * W + r.cursorBase + which * 2;
        const uint32_t* dst = a.state + (long long)(r.cursorBase + which * 2) * a.nPad + inst;
        const long long Z = l.size;
        long long found = -1;
        // kind 0: the write position, kind 1: the read position (the DANE model has one counter, in the write word)
        for (int kind = 0; kind < (r.dane ? 1 : 2) && !fault; ++kind) {
            const long long s = rec[kind], t = dst[(long long)kind * a.nPad];
            if (s >= Z) { fault = kBankBadPosition; break; }
            if (!r.dane && !(kind ? l.reads : l.writes)) continue;   // (never moves: does not count)
            const long long dk = (((t - s) % Z) + Z) % Z;
            if (found >= 0 && dk != found) fault = kBankPhase;
            found = dk;
        }
        if (!fault && found > 0 && !l.ring) fault = kBankNoRing;
        d = (fault || found < 0) ? 0 : (int)found;
    }
    r.pairs[e * 2 + which] = d;
    if (fault) {
        const unsigned long long entry = (unsigned long long)word >> 32;
        const unsigned long long key = entry << 3 | (unsigned long long)which << 2 | (unsigned long long)fault;
        atomicAdd(&r.cells[kBankCellFaults], 1ull);
        atomicMax(&r.cells[kBankCellLowest], ~key);
    }
}

// fx_inst_scatter_rot with records[k] = bank[slot[k]], behind the gate.  pairs == null: no rotation, no gate.
__global__ __launch_bounds__(kLanes) void fx_bank_scatter_rot(BankRotArgs r) {
    __shared__ uint32_t tile[kTI * (kTW + 1)];
    __shared__ long long slotAt[kTI];
    __shared__ int rotOf[kTI * 2];
    const InstArgs& a = r.bank.base;
    const unsigned t = threadIdx.x;
    if (r.pairs && r.cells[kBankCellFaults] != 0) {   // (uniform over the grid: nobody stores)
        if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) {
            r.cells[kBankCellRefused] += 1;
            r.cells[kBankCellLastKey] = ~r.cells[kBankCellLowest];
            r.cells[kBankCellLastCall] = (unsigned long long)r.serial;
        }
        return;
    }
    const long long e0 = (long long)blockIdx.x * kTI;
    const long long iBase = a.stateRows, xBase = iBase + a.iSlots, W = xBase + a.xSlots;
    const int iSize = r.line[0].ring ? a.iSlots : 0, xSize = r.line[1].ring ? a.xSlots : 0;
    if (t < kTI) slotAt[t] = e0 + t < a.count ? slotOf(r.bank.slots[e0 + t], r.bank.nSlots) : -1;
    if (t < 2 * kTI) {
        const long long e = e0 + t / 2;
        const int size = (t & 1) ? xSize : iSize;
        const int d = (r.pairs && e < a.count) ? r.pairs[e * 2 + (t & 1)] : 0;
        rotOf[t] = (d > 0 && d < size) ? d : 0;
    }
    const unsigned c = t % kTI, q = t / kTI;
    long long inst = -1;
    if (e0 + c < a.count) inst = a.list[e0 + c];
    const bool listed = inst >= 0 && inst < a.n;
    const long long wave = listed ? inst / a.cols : 0, col = listed ? inst % a.cols : 0;
    const long long iAt = wave * a.iSlots * a.cols + col, xAt = wave * a.xSlots * a.cols + col;
    __syncthreads();
    // (an entry whose slot lies outside the bank keeps what it holds)
    const bool take = listed && slotAt[c] >= 0;
    for (long long w0 = (long long)blockIdx.y * kTW; w0 < W; w0 += (long long)gridDim.y * kTW) {
        uint32_t v[kPasses];
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
            const long long w = w0 + wl, slot = slotAt[el];
            long long from = w;
            if (w >= iBase) {
                const int line = w >= xBase ? 1 : 0;
                const long long base = line ? xBase : iBase, size = line ? xSize : iSize, j = w - base;
                if (j < size) {
                    const long long back = j - rotOf[el * 2 + line];
                    from = base + (back < 0 ? back + size : back);
                }
            }
            v[k] = (slot >= 0 && w < W) ? r.bank.bank[slot * W + from] : 0u;
        }
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const unsigned flat = (unsigned)k * kLanes + t, el = flat / kTW, wl = flat % kTW;
            tile[el * (kTW + 1) + wl] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const long long w = w0 + k * kRowsPerPass + q;
            if (take && w < W && !(w >= a.skipLo && w < a.skipHi)) *wordOf(a, w, inst, iAt, xAt) = tile[c * (kTW + 1) + k * kRowsPerPass + q];
        }
        __syncthreads();   // (the tile is refilled by the next turn of the loop)
    }
}

inline bool badArgs(const BankArgs& b) {
    const InstArgs& a = b.base;
    if (!a.state || !a.list || !b.bank || !b.slots || b.nSlots < 1 || b.nSlots >= ((long long)1 << 31)) return true;
    if (a.count < 1 || a.count >= ((long long)1 << 31) || a.n < 1 || a.nPad < a.n) return true;
    if (a.stateRows < 1 || a.iSlots < 0 || a.xSlots < 0 || (a.iSlots > 0 && !a.itram) || (a.xSlots > 0 && !a.xtram)) return true;
    if (a.cols != 64 && a.cols != 128 && a.cols != 256) return true;
    return a.skipLo < 0 || a.skipHi < a.skipLo || a.skipHi > a.stateRows;
}

inline bool badRotArgs(const BankRotArgs& r) {
    if (badArgs(r.bank)) return true;
    if (!r.pairs) return false;
    if (!r.cells || r.cursorBase < 0 || r.cursorBase + 4 > r.bank.base.stateRows) return true;
    for (int which = 0; which < 2; ++which) {
        const BankLine& l = r.line[which];
        if (l.size < 0 || l.slots != (which ? r.bank.base.xSlots : r.bank.base.iSlots) || (l.ring != 0) != (l.slots > 0 && l.slots == l.size)) return true;
    }
    return false;
}

inline dim3 tileGrid(const InstArgs& a) {
    const long long across = (a.count + kTI - 1) / kTI, down = (instanceWords(a) + kTW - 1) / kTW;
    return dim3((unsigned)across, (unsigned)(down < 65535 ? down : 65535));
}

}  // namespace

hipError_t launchBankGather(const BankArgs& a, hipStream_t stream) {
    if (badArgs(a)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_bank_gather, tileGrid(a.base), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchBankRotations(const BankRotArgs& r, hipStream_t stream) {
    if (badRotArgs(r) || !r.pairs) return hipErrorInvalidValue;
    const long long lanes = r.bank.base.count * 2;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_bank_rotations, dim3((unsigned)((lanes + kLanes - 1) / kLanes)), dim3(kLanes), 0, stream, r);
    return hipGetLastError();
}

hipError_t launchBankScatterRot(const BankRotArgs& r, hipStream_t stream) {
    if (badRotArgs(r)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fx_bank_scatter_rot, tileGrid(r.bank.base), dim3(kLanes), 0, stream, r);
    return hipGetLastError();
}

}  // namespace fx
