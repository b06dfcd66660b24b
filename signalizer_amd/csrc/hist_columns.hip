// hist_columns.hip -- the histogram lane's reduction: one sgz_hist_record (the samples of 106 buckets of |v|, an octave in four linear parts;
// beside them the count, the NaNs, the negative samples, the peak and the OR and the AND of the quantised words) per column of m samples
// and channel of a linear planar stream, with a carried open column (sgz.h, "The histogram lane"); and the lane's host helpers: the bucket
// edges, the fold of kept records, the percentile and the readout of one.  gfx950 only.  The reference has no counterpart.
// What the column lanes share -- the shape of a call, the bounds, the quantiser, the staging of a row, the stage call's front, the fold's
// frame -- is column_lanes.hpp; this file is the histogram.
//   v = the quantiser's (quantiseMarked); a NaN is skipped; a = |v|; the bucket is found from the position of a's leading bit and the two
//   bits below it (integer clz: a conversion to float rounds above 2^24 and would misfile the upper edges there).  Every field folds by an
//   associative and commutative rule -- add, max, or, and --, so any cut of the stream (calls with a carry) or of a column (lanes, waves,
//   slices) gives the same bytes.  The identity is NOT all-zero: bits_and of no sample is 0xffffffff.
// A histogram is a scatter, and this one is built as one: a table of kHsWords words per column in LDS, every lane adds 1 to its sample's
// bucket with a no-return LDS add (4 clocks a wave-instruction where the lanes' addresses differ, 2 clocks for every lane that shares one:
// tools/ubench/lds_atomics.hip).  The contended case -- digital silence puts all 64 lanes on bucket 0 -- is taken out in front of the add:
// the lanes whose table word is the first active lane's are counted by a ballot, and where they are kHsPrefold or more of the wave one lane
// adds their number and they are done (preFoldAdd).  The other six fields never touch the table while samples are taken: they stay in
// registers, are folded across the lanes of a column and written once.
//   m <= kHsSwitch (1024)   histTileKernel: one workgroup per (channel, tile); a tile is min(kHsTile / m, kHsTables) whole columns.  The row
//                           goes to LDS quantised (stageRow, padded), the tile's tables are zeroed behind it, then groups of G lanes (a
//                           power of two near m / 16) take a column each.  A record is complete in its table (words 106 .. 111 from the
//                           group's first lane); the workgroup folds the carry into column 0 and stores the records word by word, 448
//                           contiguous bytes each.
//   else, or slices >= 2    histSliceKernel: workgroup (column, channel, slice) scans its part of the column from memory (16-byte loads
//                           between the 16-byte boundaries) into a table PER WAVE, the register fields carried along -> partial records
//                           [slices][columns][channels] in scratch; histEmitKernel, a launch of its own behind it, folds the slices and
//                           the carry with one lane per (column, channel, word), each word by its own rule.  A flush without samples is
//                           the emit kernel alone, on the carry.
// Every sample is read from memory once.  Nothing is waited for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>

#include "column_lanes.hpp"

using namespace sgz;

namespace {

constexpr int kHsThreads = 256;
constexpr int kHsWaves = kHsThreads / 64;
constexpr uint32_t kHsTile = 4096;               // samples of a tile's row (16 KiB of LDS and the padding)
constexpr uint32_t kHsTables = 64;               // tables of a tile: 28 KiB beside the row, three workgroups a CU
constexpr uint32_t kHsSwitch = 1024;             // the switch-over: columns longer than this take the sliced form (a full tile of the longest
                                                 // tile-form columns has one for every wave)
constexpr uint32_t kHsMaxChannels = 64;
constexpr int kHsUnroll = 4;                     // 16-byte loads a lane of the tile form issues before the first store to LDS
constexpr int kHsScan = 4;                       // 16-byte loads a lane of the sliced form has in flight
constexpr uint32_t kHsPerLane = 16;              // samples of a column a lane of the tile form takes at most
constexpr uint32_t kHsBatch = 4;                 // reads of LDS a lane of the tile form issues in front of their adds
constexpr uint32_t kHsTileWords = kHsTile + 4 + 4 * ((kHsTile + 4) / 64 + 1);      // the lead, and four words of padding per 64 (tileWord)
constexpr uint32_t kHsWords = sizeof(sgz_hist_record) / 4;                        // a record, and a table, as words
constexpr int32_t kHsNaN = kQuantNaN;            // a NaN in LDS
// "most of the wave": the lanes of one add that share the first active lane's table word, from which on one lane adds for all of them.
// The bits do not depend on it (NOTES.md, "The histogram lane", has the values it was chosen from; -DSGZ_HIST_PREFOLD=65 is no pre-fold)
#ifndef SGZ_HIST_PREFOLD
#define SGZ_HIST_PREFOLD 32
#endif
constexpr uint32_t kHsPrefold = SGZ_HIST_PREFOLD;
// the tables of the sliced form's workgroup: one per wave, or 1 -- one for all four (NOTES.md has both)
#ifndef SGZ_HIST_SLICE_TABLES
#define SGZ_HIST_SLICE_TABLES 4
#endif
constexpr uint32_t kHsSliceTables = SGZ_HIST_SLICE_TABLES;
static_assert(kHsSliceTables == 1 || kHsSliceTables == kHsWaves, "one table, or one per wave");
// the words of a record behind the buckets, and how each folds: add below kHsPeak, then max, or, and
constexpr uint32_t kHsCount = SGZ_HIST_BUCKETS, kHsSkipped = kHsCount + 1, kHsNegative = kHsCount + 2, kHsPeak = kHsCount + 3,
                   kHsOr = kHsCount + 4, kHsAnd = kHsCount + 5;
static_assert(SGZ_HIST_BUCKETS == 106 && sizeof(sgz_hist_record) == 448 && kHsWords == 112 && kHsAnd == kHsWords - 1, "sgz.h documents 448 bytes");
static_assert(offsetof(sgz_hist_record, count) == 4 * kHsCount && offsetof(sgz_hist_record, skipped) == 4 * kHsSkipped &&
              offsetof(sgz_hist_record, negative) == 4 * kHsNegative && offsetof(sgz_hist_record, peak) == 4 * kHsPeak &&
              offsetof(sgz_hist_record, bits_or) == 4 * kHsOr && offsetof(sgz_hist_record, bits_and) == 4 * kHsAnd, "the record as words");
static_assert(kHsTile == 4u * kHsThreads * kHsUnroll, "a lane moves kHsUnroll 16-byte chunks of a tile's row");
static_assert(kHsSwitch <= kHsTile && kHsSwitch * kHsWaves <= kHsTile && kHsTile / kHsSwitch <= kHsTables, "a full tile of the longest columns");
static_assert(kHsSwitch <= 64 * kHsPerLane, "a group of at most 64 lanes takes a column of the tile form");
static_assert(kHsTileWords * 4 + kHsTables * kHsWords * 4 <= 48 * 1024, "three workgroups a CU");

struct HistParams {
    const float *planar;                 // [channels][stride]
    size_t stride;
    long n;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t m, held, channels;
    uint32_t perTile;                    // columns of a tile = min(kHsTile / m, kHsTables)
    uint32_t group;                      // lanes per column in the tile form
    uint32_t slices;
    const sgz_hist_record *carryIn;      // [channels]: column 0's `held` earlier samples (read iff held > 0)
    sgz_hist_record *carryOut;           // [channels]: the open column
    sgz_hist_record *hist;               // [closed][channels]
    sgz_hist_record *partial;            // [slices][columns][channels]
};

// the bucket of a = |v| <= 2^26: 0 for a = 0, else 1 + 4 e + s with e the leading bit's position and s the two bits below it (for e < 2:
// what there is of them, shifted up).  Integer throughout
__host__ __device__ __forceinline__ uint32_t bucketOf(uint32_t a)
{
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t z = uint32_t(__clz(int(a | 1u)));
#else
    const uint32_t z = uint32_t(__builtin_clz(a | 1u));
#endif
    const uint32_t top = a << z;                                            // the leading bit at bit 31
    return a ? 1u + 4u * (31u - z) + ((top >> 29) & 3u) : 0u;
}

// how word w of a record folds
__host__ __device__ __forceinline__ uint32_t foldWord(uint32_t w, uint32_t acc, uint32_t v)
{
    return w < kHsPeak ? acc + v : w == kHsPeak ? (acc > v ? acc : v) : w == kHsOr ? (acc | v) : (acc & v);
}
__host__ __device__ __forceinline__ uint32_t identityWord(uint32_t w) { return w == kHsAnd ? 0xffffffffu : 0u; }

// One add of a wave to the table words `key` of its lanes (has: the lane has a sample; a lane without one carries a key no table has).
// The lanes that share the first active lane's word are counted; kHsPrefold or more: the first of them adds their number, and they are
// done.  The rest take the plain add.  An uncontended add pays the broadcast, the compare and the ballot
__device__ __forceinline__ void preFoldAdd(uint32_t *tables, uint32_t key, bool has)
{
    const uint32_t first = uint32_t(__builtin_amdgcn_readfirstlane(int(key)));
    const bool same = has && key == first;
    const unsigned long long mask = __ballot(same);
    if (uint32_t(__popcll(mask)) >= kHsPrefold) {                           // (the same in every lane of the wave)
        if (same && (threadIdx.x & 63u) == uint32_t(__ffsll(mask)) - 1u)
            (void)__hip_atomic_fetch_add(tables + first, uint32_t(__popcll(mask)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        has = has && !same;
    }
    if (has) (void)__hip_atomic_fetch_add(tables + key, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// a lane's part of the six fields that stay in registers
struct Fields {
    uint32_t count, skipped, negative, peak, bitsOr, bitsAnd;
    // v: a quantised sample or the NaN mark, where `valid`; table: the first word of the column's table in `tables`.  Called by whole waves
    __device__ __forceinline__ void take(int32_t v, bool valid, uint32_t *tables, uint32_t table)
    {
        const bool has = valid && v != kHsNaN;
        const uint32_t a = has ? uint32_t(abs(v)) : 0u;
        count += has ? 1u : 0u;
        skipped += (valid && !has) ? 1u : 0u;
        negative += (has && v < 0) ? 1u : 0u;
        peak = max(peak, a);
        bitsOr |= has ? uint32_t(v) : 0u;
        bitsAnd &= has ? uint32_t(v) : 0xffffffffu;                         // (a NaN leaves both untouched: the identities)
        preFoldAdd(tables, has ? table + bucketOf(a) : 0xffffffffu, has);
    }
    __device__ __forceinline__ void foldLane(int o)
    {
        count += __shfl_xor(count, o);
        skipped += __shfl_xor(skipped, o);
        negative += __shfl_xor(negative, o);
        peak = max(peak, __shfl_xor(peak, o));
        bitsOr |= __shfl_xor(bitsOr, o);
        bitsAnd &= __shfl_xor(bitsAnd, o);
    }
    // into words 106 .. 111 of a table that no other lane writes to
    __device__ __forceinline__ void foldInto(uint32_t *table) const
    {
        table[kHsCount] += count;
        table[kHsSkipped] += skipped;
        table[kHsNegative] += negative;
        table[kHsPeak] = max(table[kHsPeak], peak);
        table[kHsOr] |= bitsOr;
        table[kHsAnd] &= bitsAnd;
    }
    // ... and of a table that other waves fold into as well
    __device__ __forceinline__ void foldIntoShared(uint32_t *table) const
    {
        (void)__hip_atomic_fetch_add(table + kHsCount, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        (void)__hip_atomic_fetch_add(table + kHsSkipped, skipped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        (void)__hip_atomic_fetch_add(table + kHsNegative, negative, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        (void)__hip_atomic_fetch_max(table + kHsPeak, peak, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        (void)__hip_atomic_fetch_or(table + kHsOr, bitsOr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        (void)__hip_atomic_fetch_and(table + kHsAnd, bitsAnd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};
__device__ __forceinline__ Fields noSamples() { return Fields{0u, 0u, 0u, 0u, 0u, 0xffffffffu}; }

// where word w of (column, channel)'s record goes: the output (a closed column) or the carry (the open column)
__device__ __forceinline__ uint32_t *recordWord(const HistParams &prm, long col, uint32_t ch, uint32_t w)
{
    sgz_hist_record *to = col < prm.closed ? prm.hist + size_t(col) * prm.channels + ch : prm.carryOut + ch;
    return reinterpret_cast<uint32_t *>(to) + w;
}

// the tile's row and tables in LDS, then groups of prm.group lanes per column
__global__ void __launch_bounds__(kHsThreads)
histTileKernel(const HistParams prm)
{
    __shared__ __attribute__((aligned(16))) int32_t row[kHsTileWords];
    __shared__ uint32_t tables[kHsTables * kHsWords];
    const uint32_t tid = threadIdx.x, ch = blockIdx.y;
    TileBounds t;
    tileBounds(prm, t);
    const long c0 = t.c0, c1 = t.c1, a = t.a, b = t.b;
    const uint32_t count = uint32_t(b - a);                                 // <= perTile * m <= kHsTile
    const uint32_t cols = uint32_t(c1 - c0);                                // <= perTile <= kHsTables
    const float *g = prm.planar + size_t(ch) * prm.stride + size_t(a);
    const uint32_t lead = uint32_t(reinterpret_cast<uintptr_t>(g) >> 2) & 3u;
    stageRow<true, kHsThreads, kHsUnroll>(g, count, lead, row);
    for (uint32_t w = tid; w < cols * kHsWords; w += kHsThreads) tables[w] = identityWord(w % kHsWords);
    __syncthreads();
    const uint32_t G = prm.group, sub = tid & (G - 1u), grp = tid / G, groups = uint32_t(kHsThreads) / G;
    const uint32_t trips = (prm.m + G - 1u) / G;                            // (<= kHsPerLane)
    for (uint32_t base = 0; base < cols; base += groups) {                  // (the same trips in every lane: the cross-lane steps see whole waves)
        const uint32_t lc = base + grp;
        const bool mine = lc < cols;
        uint32_t begin = 0, end = 0;
        if (mine) {
            long ca, cb;
            columnSamples(prm, c0 + long(lc), ca, cb);
            begin = uint32_t(ca - a);
            end = uint32_t(cb - a);
        }
        Fields k = noSamples();
        for (uint32_t j = 0; j < trips; j += kHsBatch) {                     // (a trip past the last one is past the column's end: not valid)
            int32_t v[kHsBatch];
            bool valid[kHsBatch];
#pragma unroll
            for (uint32_t q = 0; q < kHsBatch; ++q) {                       // the batch's reads of LDS in front of its adds
                const uint32_t i = begin + sub + (j + q) * G;
                valid[q] = i < end;
                v[q] = valid[q] ? row[tileWord(lead + i)] : 0;
            }
#pragma unroll
            for (uint32_t q = 0; q < kHsBatch; ++q) k.take(v[q], valid[q], tables, lc * kHsWords);
        }
        for (uint32_t o = G >> 1; o > 0; o >>= 1) k.foldLane(int(o));
        if (mine && sub == 0) k.foldInto(tables + lc * kHsWords);           // (one group per column: no other lane has these six words)
    }
    __syncthreads();
    for (uint32_t w = tid; w < cols * kHsWords; w += kHsThreads) {
        const uint32_t lc = w / kHsWords, word = w - lc * kHsWords;
        const long col = c0 + long(lc);
        uint32_t v = tables[w];
        if (col == 0 && prm.held) v = foldWord(word, v, reinterpret_cast<const uint32_t *>(prm.carryIn + ch)[word]);
        *recordWord(prm, col, ch, word) = v;
    }
}

// slice blockIdx.z of column blockIdx.x's samples of channel blockIdx.y (an empty slice -- more slices than samples -- leaves the identity)
__global__ void __launch_bounds__(kHsThreads)
histSliceKernel(const HistParams prm)
{
    __shared__ uint32_t tables[kHsSliceTables * kHsWords];
    const long col = long(blockIdx.x);
    const uint32_t ch = blockIdx.y, s = blockIdx.z, tid = threadIdx.x, table = kHsSliceTables == 1 ? 0u : (tid >> 6) * kHsWords;
    for (uint32_t w = tid; w < kHsSliceTables * kHsWords; w += kHsThreads) tables[w] = identityWord(w % kHsWords);
    __syncthreads();
    long a, b, sa, sb;
    columnSamples(prm, col, a, b);
    sliceSamples(prm, a, b, s, sa, sb);
    Fields k = noSamples();
    if (sb > sa) {                                                          // (sa, sb: the workgroup's)
        const float *g = prm.planar + size_t(ch) * prm.stride + size_t(sa);
        const size_t count = size_t(sb - sa);
        uint32_t head;
        size_t vecs, tail;
        splitAligned(g, count, head, vecs, tail);
        // up to three samples on either side of the 16-byte part (every lane takes part in every add: the ballots see whole waves)
        const bool front = tid < head, back = tid < count - tail;
        k.take(front ? quantiseMarked(__float_as_uint(g[tid])) : 0, front, tables, table);
        k.take(back ? quantiseMarked(__float_as_uint(g[tail + tid])) : 0, back, tables, table);
        const uint4 *gv = reinterpret_cast<const uint4 *>(g + head);
        for (size_t at = 0; at < vecs; at += size_t(kHsThreads) * kHsScan) {
            uint4 q[kHsScan];
            bool valid[kHsScan];
#pragma unroll
            for (int j = 0; j < kHsScan; ++j) {
                const size_t i = at + size_t(j) * kHsThreads + tid;
                valid[j] = i < vecs;
                q[j] = valid[j] ? gv[i] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int j = 0; j < kHsScan; ++j) {
                k.take(quantiseMarked(q[j].x), valid[j], tables, table);
                k.take(quantiseMarked(q[j].y), valid[j], tables, table);
                k.take(quantiseMarked(q[j].z), valid[j], tables, table);
                k.take(quantiseMarked(q[j].w), valid[j], tables, table);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k.foldLane(o);
    if ((tid & 63u) == 0) {
        if constexpr (kHsSliceTables == 1) k.foldIntoShared(tables);
        else k.foldInto(tables + table);                                    // (a wave's own table, words no add touches)
    }
    __syncthreads();
    if (tid < kHsWords) {
        uint32_t v = tables[tid];
#pragma unroll
        for (uint32_t wv = 1; wv < kHsSliceTables; ++wv) v = foldWord(tid, v, tables[wv * kHsWords + tid]);
        reinterpret_cast<uint32_t *>(prm.partial + (size_t(s) * size_t(prm.columns) + size_t(col)) * prm.channels + ch)[tid] = v;
    }
}

// one lane per (column, channel, word): the fold over the slices (none: a flush of the carry alone) from the identity, the carry, the store
__global__ void __launch_bounds__(kHsThreads)
histEmitKernel(const HistParams prm)
{
    const size_t at = size_t(blockIdx.x) * kHsThreads + threadIdx.x, cell = at / kHsWords, perSlice = size_t(prm.columns) * prm.channels;
    const uint32_t word = uint32_t(at - cell * kHsWords);
    if (cell >= perSlice) return;
    const long col = long(cell / prm.channels);
    const uint32_t ch = uint32_t(cell % prm.channels);
    uint32_t v = identityWord(word);
    for (uint32_t sl = 0; sl < prm.slices; ++sl)
        v = foldWord(word, v, reinterpret_cast<const uint32_t *>(prm.partial + size_t(sl) * perSlice + cell)[word]);
    if (col == 0 && prm.held) v = foldWord(word, v, reinterpret_cast<const uint32_t *>(prm.carryIn + ch)[word]);
    *recordWord(prm, col, ch, word) = v;
}

// ---- the host helpers -----------------------------------------------------------------------------------------------------------------------
// the integers of bucket b: [lo, hi], empty where lo > hi
void edgesOf(uint32_t b, uint32_t &lo, uint32_t &hi)
{
    if (b == 0) { lo = hi = 0; return; }
    const uint32_t e = (b - 1) / 4, s = (b - 1) % 4;
    // ceil((4 + s) 2^(e - 2)) and ceil((5 + s) 2^(e - 2)) - 1
    const auto scaled = [e](uint32_t x) { return e >= 2 ? x << (e - 2) : (x + (1u << (2 - e)) - 1u) >> (2 - e); };
    lo = scaled(4 + s);
    hi = b == SGZ_HIST_BUCKETS - 1 ? (1u << 26) : scaled(5 + s) - 1u;
}

}  // namespace

namespace sgz {

ColumnsShape histColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices)
{
    return columnsShape(channels, nsamples, m, held, flush, slices, kHsSwitch, sizeof(sgz_hist_record), 0);
}

sgz_status runHistColumns(const ColumnsShape &sh, const float *d_planar, size_t channelStride, uint32_t channels, size_t nsamples, uint32_t m,
                          uint32_t held, const sgz_hist_record *carryIn, sgz_hist_record *carryOut, sgz_hist_record *d_hist, void *scratch,
                          hipStream_t stream)
{
    if (!sh.launch) return SGZ_OK;
    HistParams prm{};
    fillGrid(prm, sh, d_planar, channelStride, nsamples, m, held);
    prm.channels = channels;
    prm.carryIn = carryIn; prm.carryOut = carryOut;
    prm.hist = d_hist; prm.partial = static_cast<sgz_hist_record *>(scratch);
    return launchPlainLane(histTileKernel, histSliceKernel, histEmitKernel, kHsThreads, "histogram", prm, sh, channels, nsamples, kHsWords, [m](HistParams &p) {
        p.perTile = std::min(kHsTile / m, kHsTables);                      // (a tile of very short columns has fewer than kHsTile samples)
        p.group = pow2AtLeast((m + kHsPerLane - 1) / kHsPerLane);          // (1 .. 64: at most sixteen samples a lane)
    }, stream);
}

}  // namespace sgz

extern "C" {

void sgz_hist_columns_limits(uint32_t *switch_over, uint32_t *tile_samples)
{
    if (switch_over) *switch_over = kHsSwitch;
    if (tile_samples) *tile_samples = kHsTile;
}

sgz_status sgz_stage_hist_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, uint32_t m, uint32_t held,
                                  int flush, uint32_t slices, sgz_hist_record *d_carry, sgz_hist_record *d_hist, void *stream)
{
    const StageFront front{"sgz_stage_hist_columns", "channels", kHsMaxChannels, "d_hist", 16, false, 62};
    return stageColumns(front, SGZ_OK, d_planar, channel_stride, channels, nsamples, m, held, flush, 0, 0, slices, d_carry, d_hist, stream, histColumnsShape,
                        size_t(channels) * sizeof(sgz_hist_record), noStep, [&](const ColumnsShape &sh, const void *carryIn, void *scratch, hipStream_t s) {
                            return runHistColumns(sh, d_planar, channel_stride, channels, nsamples, m, held, static_cast<const sgz_hist_record *>(carryIn), d_carry, d_hist, scratch, s);
                        });
}

void sgz_hist_edges(uint32_t lo[SGZ_HIST_BUCKETS], uint32_t hi[SGZ_HIST_BUCKETS])
{
    for (uint32_t b = 0; b < SGZ_HIST_BUCKETS; ++b) {
        uint32_t l, h;
        edgesOf(b, l, h);
        if (lo) lo[b] = l;
        if (hi) hi[b] = h;
    }
}

sgz_status sgz_hist_fold(const sgz_hist_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns, sgz_hist_record *out)
{
    return foldColumns(
        "sgz_hist_fold", "channels", " samples", in, n, channels, x0, x1, out_columns, out,
        [](const sgz_hist_record *in, size_t count, size_t stride) {
            uint64_t tally[2] = {0, 0};                                    // (count bounds every bucket and `negative`)
            for (size_t j = 0; j < count; ++j) {
                tally[0] += in[j * stride].count;
                tally[1] += in[j * stride].skipped;
            }
            return tally[0] <= 0xffffffffull && tally[1] <= 0xffffffffull;
        },
        [](const sgz_hist_record *in, size_t count, size_t stride) {
            sgz_hist_record r;
            uint32_t *acc = reinterpret_cast<uint32_t *>(&r);
            for (uint32_t w = 0; w < kHsWords; ++w) acc[w] = identityWord(w);
            for (size_t j = 0; j < count; ++j) {
                const uint32_t *v = reinterpret_cast<const uint32_t *>(in + j * stride);
                for (uint32_t w = 0; w < kHsWords; ++w) acc[w] = foldWord(w, acc[w], v[w]);
            }
            return r;
        });
}

sgz_status sgz_hist_percentile(const sgz_hist_record *rec, double q, uint32_t *bucket, double *lo, double *hi)
{
    if (!rec || !bucket || !lo || !hi) return fail(SGZ_EINVAL, "sgz_hist_percentile: null argument");
    if (!(q >= 0.0 && q <= 1.0)) return fail(SGZ_EINVAL, "sgz_hist_percentile: 0 <= q <= 1");
    if (rec->count == 0) return fail(SGZ_EINVAL, "sgz_hist_percentile: a record without samples has no percentile");
    const double want = std::ceil(q * double(rec->count));                 // the least integer >= q count; one fp64 multiply
    const uint64_t r = want < 1.0 ? 1u : want > double(rec->count) ? uint64_t(rec->count) : uint64_t(want);
    uint64_t below = 0;
    uint32_t b = 0;
    for (; b < SGZ_HIST_BUCKETS - 1; ++b) {
        below += rec->bucket[b];
        if (below >= r) break;
    }
    uint32_t l, h;
    edgesOf(b, l, h);
    *bucket = b;
    *lo = double(l) / 0x1p23;
    *hi = double(h) / 0x1p23;
    return SGZ_OK;
}

sgz_status sgz_hist_readout(const sgz_hist_record *rec, sgz_hist_reading *out)
{
    if (!rec || !out) return fail(SGZ_EINVAL, "sgz_hist_readout: null argument");
    const double nan = std::numeric_limits<double>::quiet_NaN(), count = double(rec->count);
    out->zero_share = rec->count ? double(rec->bucket[0]) / count : nan;
    out->negative_share = rec->count ? double(rec->negative) / count : nan;
    out->peak = double(rec->peak) / 0x1p23;
    out->peak_db = rec->count ? 20.0 * std::log10(out->peak) : nan;        // (log10(0) = -inf)
    out->median_db = nan;
    if (rec->count) {
        uint32_t b = 0;
        double lo = 0, hi = 0;
        if (sgz_status st = sgz_hist_percentile(rec, 0.5, &b, &lo, &hi); st != SGZ_OK) return st;
        out->median_db = 20.0 * std::log10(hi);
    }
    out->toggling = rec->bits_or & ~rec->bits_and;
    out->effective_bits = 0;
    if (rec->bits_or) {
        const int bits = 24 - __builtin_ctz(rec->bits_or);
        out->effective_bits = bits > 0 ? uint32_t(bits) : 0u;
    }
    return SGZ_OK;
}

}  // extern "C"
