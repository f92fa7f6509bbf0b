// fx_batch_bus_feed.cpp — the feeds of bus blocks: the state of one batch (fx_batch.hpp "Bus feeds", kernel: fx_bus_feed in
// fx_bus.hip, launched by launchFeed from Batch::runBus).
//
// The sends over again on the input side.  The structure lives twice: on the host (feed_, what busGetFeeds reads - the weights a
// and b included) and in ONE device block of 32-bit words: the offsets [n + 1] of the CSR form (the map form - one entry per
// instance - has none), the source columns [E] and the two gain blocks [C][E] whose roles swap from ramp to ramp (feedRamp_,
// fx_batch_bus_side.hpp RampPair).  Every table begins on a 16-byte boundary and is padded to whole quads of words, so that a lane
// of fx_bus_feed reads the words of its four instances with one access (fx_bus.hpp BusFeedArgs).  A set is two steps so that
// several shards can be all-or-nothing: busReserveFeeds allocates the block of the set to come and touches nothing else,
// busSetFeeds waits for everything queued on the handle, takes the reserved block and fills it with a synchronous copy.
// busSetFeedGains waits the same way and copies into the gain block that becomes b.  The only other allocation is the device copy
// of a source block that is not device memory (planFeedRoute), made in front of a block's first launch.
#include "fx_batch.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/fx8010_amd.h"

namespace fx {

namespace {
inline size_t quads(size_t words) { return (words + 3) / 4 * 4; }
}  // namespace

bool Batch::FeedSet::isMap() const {
    for (size_t i = 0; i < offsets.size(); ++i)
        if (offsets[i] != (int64_t)i) return false;
    return true;
}

// words of the device block of a structure of `entries` entries; off4: where the four tables begin and the pitch of a gain row
size_t Batch::feedBlockWords(int64_t entries, bool map, size_t* off4) const {
    const size_t ch = (size_t)prog_.numChannels, n4 = quads((size_t)n_);
    const size_t pitch = map ? n4 : quads((size_t)entries);
    size_t at = map ? 0 : quads(n4 + 1);
    off4[0] = 0;
    off4[1] = at;
    at += pitch;
    off4[2] = at;
    at += ch * pitch;
    off4[3] = at;
    at += ch * pitch;
    off4[4] = pitch;
    return at;
}

int Batch::busReserveFeeds(int64_t sources, int64_t entries, bool map) {
    (void)hipSetDevice(device_);
    if (sources < 0 || entries < 0 || entries > kMaxFeedEntries) return fail(FX_E_ARG, "bus feeds: counts out of range");
    size_t off4[5];
    return reserveBlock(feedBlock_, sources == 0 ? 0 : feedBlockWords(entries, map, off4), "hipMalloc bus feeds");
}

void Batch::busReleaseFeeds() { releaseBlock(feedBlock_); }

int Batch::busSetFeeds(FeedSet&& set) {
    (void)hipSetDevice(device_);
    const size_t ch = (size_t)prog_.numChannels;
    const int64_t entries = (int64_t)set.columns.size();
    if (set.sources == 0) {   // off: waits, frees
        const int rc = sync();
        if (rc != 0) return rc;
        takeUpBlock(feedBlock_, false);
        freeBlock(feedSrc_, false);
        feed_ = FeedSet{};
        feedRamp_ = RampPair{};
        return 0;
    }
    if (set.sources < 0 || (uint64_t)ch * (uint64_t)set.sources * 4u >= ((uint64_t)1 << 32) || set.offsets.size() != (size_t)n_ + 1 || set.offsets.front() != 0 ||
        set.offsets.back() != entries || set.first < 0 || set.totalEntries < set.first + entries || set.totalEntries > kMaxFeedEntries ||
        set.gain[0].size() != ch * (size_t)entries)
        return fail(FX_E_ARG, "bus feeds: a structure that does not hold together");
    for (int64_t i = 0; i < n_; ++i)
        if (set.offsets[(size_t)i + 1] < set.offsets[(size_t)i]) return fail(FX_E_ARG, "bus feeds: offsets must not decrease");
    for (int64_t c : set.columns)
        if (c < 0 || c >= set.sources) return fail(FX_E_ARG, "bus feeds: a source outside 0..M-1");
    const bool map = set.isMap();
    size_t off4[5];
    const size_t words = feedBlockWords(entries, map, off4);
    if (feedBlock_.reservedWords < words) {
        const int rc = busReserveFeeds(set.sources, entries, map);
        if (rc != 0) return rc;
    }
    // the image of the device block, on the host first: from here on nothing can run out of memory but these vectors (bad_alloc
    // leaves the handle as it was: nothing has been touched yet)
    std::vector<uint32_t> image(words, 0u);
    if (!map) {
        const size_t n4 = quads((size_t)n_);
        for (size_t i = 0; i <= n4; ++i) image[off4[0] + i] = (uint32_t)set.offsets[std::min(i, (size_t)n_)];
    }
    for (int64_t e = 0; e < entries; ++e) image[off4[1] + (size_t)e] = (uint32_t)set.columns[(size_t)e];
    for (size_t c = 0; c < ch && entries > 0; ++c) {
        std::memcpy(&image[off4[2] + c * off4[4]], &set.gain[0][c * (size_t)entries], (size_t)entries * 4);
        std::memcpy(&image[off4[3] + c * off4[4]], &set.gain[0][c * (size_t)entries], (size_t)entries * 4);
    }
    set.gain[1] = set.gain[0];
    const int rc = sync();   // (blocks queued with the old structure still read it)
    if (rc != 0) return rc;
    const hipError_t e = hipMemcpy(feedBlock_.reserved, image.data(), words * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hipFail(e, "bus feeds: copying the structure to the device");
    takeUpBlock(feedBlock_, true);
    for (int k = 0; k < 4; ++k) feedOff_[k] = off4[k];
    feedGainPitch_ = off4[4];
    feedMap_ = map;
    feed_ = std::move(set);
    feedRamp_ = RampPair{};   // a = b, and a ramp that was waiting for its block is gone
    return 0;
}

int Batch::busSetFeedGains(const float* gains, int ramp) {
    (void)hipSetDevice(device_);
    if (ramp != 0 && ramp != 1) return fail(FX_E_ARG, "bus feeds: ramp must be 0 or 1");
    if (feed_.sources < 1) return fail(FX_E_ARG, "bus feeds: feeds are off (fxb_bus_set_feeds)");
    const size_t ch = (size_t)prog_.numChannels, mine = feed_.columns.size(), all = (size_t)feed_.totalEntries;
    // this batch's run of the caller's [C][E], as the device holds it: [C][pitch]
    std::vector<float> next(ch * mine, 1.0f);
    if (gains)
        for (size_t c = 0; c < ch && mine > 0; ++c) std::memcpy(&next[c * mine], gains + c * all + (size_t)feed_.first, mine * 4);
    std::vector<float> image(ch * feedGainPitch_, 0.0f);
    for (size_t c = 0; c < ch && mine > 0; ++c) std::memcpy(&image[c * feedGainPitch_], &next[c * mine], mine * 4);
    const int rc = sync();   // (blocks queued with the old weights still read them)
    if (rc != 0) return rc;
    // null: back to unweighted - both blocks hold 1.0f again, which is what a later ramp starts from
    const int target = gains ? feedRamp_.writeTarget(ramp) : 0;
    for (int k = 0; k < (gains ? 1 : 2) && !image.empty(); ++k) {
        const hipError_t e = hipMemcpy(feedBlock_.cur + feedOff_[2 + (target ^ k)], image.data(), image.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hipFail(e, "bus feeds: copying the gains to the device");
    }
    if (!gains) feed_.gain[1] = next;
    feed_.gain[target].swap(next);
    feed_.weighted = gains != nullptr;
    feedRamp_ = gains ? RampPair{target, ramp != 0} : RampPair{};
    return 0;
}

void Batch::busGetFeeds(int64_t* offsets, int64_t offCap, int64_t* sources, float* gains, int64_t cap, int64_t firstInstance) const {
    if (feed_.sources < 1) return;
    const size_t ch = (size_t)prog_.numChannels, mine = feed_.columns.size(), all = (size_t)feed_.totalEntries;
    const std::vector<float>& g = feed_.gain[feedRamp_.inForce()];
    if (offsets)
        for (int64_t i = 0; i <= n_ && firstInstance + i < offCap; ++i) offsets[firstInstance + i] = feed_.first + feed_.offsets[(size_t)i];
    for (size_t e = 0; e < mine && feed_.first + (int64_t)e < cap; ++e) {
        const size_t to = (size_t)feed_.first + e;
        if (sources) sources[to] = feed_.columns[e];
        if (gains)
            for (size_t c = 0; c < ch; ++c) gains[c * all + to] = g[c * mine + e];
    }
}

// Where the feed kernel of a block gathers from, decided - and the device copy allocated - before the block's first launch.
// devSrc: the caller's rows where they are memory of this device, else null.
int Batch::planFeedRoute(const float* src, const void* devSrc, size_t rows, FeedRoute* route) {
    *route = FeedRoute{};
    if (devSrc) {
        route->dev = static_cast<const uint32_t*>(devSrc);
        return 0;
    }
    const size_t words = rows * (size_t)feed_.sources;
    if (words > feedSrc_.cap) {
        if (busLaunched_) (void)hipEventSynchronize(evBus_);   // (a block on the caller's stream may still be gathering from the old one)
        (void)hipStreamSynchronize(stream_);
        const int rc = growBlock(feedSrc_, words, false, "hipMalloc bus feed source rows");
        if (rc != 0) return rc;
    }
    route->host = src;
    return 0;
}

// the launch of one piece (Batch::runBus): rows [first, first + rows) of the block, sample0 the piece's first sample
hipError_t Batch::launchFeed(const FeedRoute& route, size_t first, long long rows, int nSamples, int sample0, hipStream_t s) {
    const size_t m = (size_t)feed_.sources;
    const uint32_t* src = route.dev;
    if (!src) {   // the piece's source rows, pinned or pageable, into device memory: every word of them is gathered many times
        const hipError_t e = hipMemcpyAsync(feedSrc_.p + first * m, route.host + first * m, (size_t)rows * m * 4, hipMemcpyDefault, s);
        if (e != hipSuccess) return e;
        src = feedSrc_.p;
    }
    BusFeedArgs a{};
    const uint32_t* words = feedBlock_.cur;
    a.src = src + first * m;
    a.wide = reinterpret_cast<uint32_t*>(bus_.p);
    a.off = feedMap_ ? nullptr : words + feedOff_[0];
    a.idx = words + feedOff_[1];
    if (feed_.weighted) {
        a.target = reinterpret_cast<const float*>(words + feedOff_[2 + feedRamp_.target]);
        a.current = feedRamp_.pending ? reinterpret_cast<const float*>(words + feedOff_[2 + (feedRamp_.target ^ 1)]) : nullptr;
    }
    a.rows = rows;
    a.n = n_;
    a.m = feed_.sources;
    a.entries = (long long)feed_.columns.size();
    a.gainPitch = (long long)feedGainPitch_;
    setRamp(a, feed_.weighted ? feedRamp_ : RampPair{}, nSamples, sample0);   // (unweighted: never a ramp)
    return launchBusFeed(a, s);
}

}  // namespace fx
