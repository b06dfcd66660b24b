// level_columns.hip -- the level lane's reduction: one sgz_level_record (sums of squares, cross term, sums, counts, overs) per column of m
// samples and channel pair of a linear planar stream, with a carried open column (sgz.h, "The level lane"); and the lane's host helpers, the
// fold of kept records and the readout of one.  gfx950 only.  The reference has no counterpart: its meters are live one-pole filters.
// What the column lanes share -- the shape of a call, the bounds, the quantiser, the staging of a row, the stage call's front, the fold's
// frame -- is column_lanes.hpp; this file is the record's arithmetic.
//   v = the quantiser's (quantiseMarked), a NaN takes no part; every field is a sum of integers, so any cut of the stream (calls with a
//   carry) or of a column (lanes, slices) gives the same bits.
// The kernels keep a NaN as v = 0 beside a count of 0: it then adds nothing to any sum.
//   m <= kLvSwitch (1024)   levelTileKernel: one workgroup per (pair, tile) of BOTH rows of the pair.  Each row goes to LDS once, quantised
//                           on the way (stageRow, padded; the two rows of a pair need not share an alignment, each keeps its own offset
//                           within 16 bytes).  Then groups of G lanes (a power of two near m / 16) take a column each: the lanes stride the
//                           column in LDS with 64-bit accumulators (Narrow: a column holds at most 1024 samples; a lane's own sums of v, at
//                           most 16 of them, in 32 bits), log2 G cross-lane steps, the group's first lane widens, folds the carry (column
//                           0) and stores the record -- or the carry (the open column).
//   else, or slices >= 2    levelSliceKernel: workgroup (column, pair, slice) scans its part of the column from memory (16-byte loads where
//                           both rows share an alignment, 4-byte loads otherwise) into 128-bit accumulators -> partial records
//                           [slices][columns][pairs] in scratch; levelEmitKernel, a launch of its own behind it, folds the slices and the
//                           carry and stores.  A flush without samples is the emit kernel alone, on the carry.
// Every sample is read from memory once.  Nothing is waited for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "column_lanes.hpp"

using namespace sgz;

namespace {

typedef unsigned __int128 u128;
typedef __int128 i128;

constexpr int kLvThreads = 256;
constexpr uint32_t kLvTile = 4096;              // samples per row of a tile (two rows: 32 KiB of LDS and the padding)
constexpr uint32_t kLvSwitch = 1024;            // the switch-over: columns longer than this take the sliced form
constexpr uint32_t kLvMaxPairs = 32;
constexpr int kLvUnroll = 4;                    // 16-byte loads per row a lane of the tile form issues before the first store to LDS
constexpr int kLvScan = 2;                      // loads per row a lane of the sliced form has in flight (two rows: four)
constexpr uint32_t kLvTileWords = kLvTile + 4 + 4 * ((kLvTile + 4) / 64 + 1);      // the lead, and four words of padding per 64 (tileWord)
constexpr int32_t kLvFull = 1 << 23;            // |v| of full scale: an over
constexpr int32_t kLvClamp = 1 << 26;           // the quantiser's range
constexpr int32_t kLvNaN = kQuantNaN;           // a NaN in LDS
static_assert(kLvTile == 4u * kLvThreads * kLvUnroll, "a lane moves kLvUnroll 16-byte chunks of a tile's row");
static_assert(kLvSwitch <= kLvTile, "a short column fits a tile");
// The 64-bit accumulators: a term v^2 or |v_L v_R| is at most 2^52, so fewer than 2048 terms stay below 2^63, the signed cross term's limit.
// A Narrow takes a column of the tile form (at most kLvSwitch terms) or a batch of the sliced form (4 * kLvScan); everything wider is 128-bit.
constexpr uint64_t kLvTerm = uint64_t(kLvClamp) * uint64_t(kLvClamp);
constexpr uint32_t kLvNarrowTerms = 2047;
static_assert(kLvTerm == (uint64_t(1) << 52) && kLvTerm * kLvNarrowTerms < (uint64_t(1) << 63), "2047 terms of 2^52 stay below 2^63");
static_assert(kLvSwitch <= kLvNarrowTerms && 4 * kLvScan <= kLvNarrowTerms, "what goes into one Narrow");
static_assert(kLvSwitch < (1u << 16), "a Narrow tallies count and overs in 16 bits each");
// The 32-bit sums of v: |v| <= 2^26, so fewer than 32 terms stay below 2^31.  A lane takes that few between two calls of Narrow::settle: at
// most kLvPerLane sample frames of a column in the tile form (the group has at least m / kLvPerLane lanes), one batch in the sliced form.
constexpr uint32_t kLvPerLane = 16, kLvLaneTerms = 31;
static_assert(uint64_t(kLvClamp) * kLvLaneTerms < (uint64_t(1) << 31), "31 terms of 2^26 stay below 2^31");
static_assert(kLvPerLane <= kLvLaneTerms && 4 * kLvScan <= kLvLaneTerms, "what goes into a lane's 32-bit sums");
static_assert(sizeof(sgz_level_record) == 80, "sgz.h documents 80 bytes");

struct LevelParams {
    const float *planar;                 // [2 pairs][stride]
    size_t stride;
    long n;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t m, held, pairs;
    uint32_t perTile;                    // columns of a tile = kLvTile / m
    uint32_t group;                      // lanes per column in the tile form
    uint32_t slices;
    const sgz_level_record *carryIn;     // [pairs]: column 0's `held` earlier samples (read iff held > 0)
    sgz_level_record *carryOut;          // [pairs]: the open column
    sgz_level_record *level;             // [closed][pairs]
    sgz_level_record *partial;           // [slices][columns][pairs]
};

// at most kLvNarrowTerms sample frames of a pair (the static_asserts above)
struct Narrow {
    uint64_t sq[2];
    int64_t cross, sum[2];
    uint32_t tally[2];                   // count | overs << 16
    int32_t lane[2];                     // the sums of v since the last settle(): at most kLvLaneTerms terms
    __device__ __forceinline__ void take(int32_t l, int32_t r)
    {
        const bool hasL = l != kLvNaN, hasR = r != kLvNaN;
        l = hasL ? l : 0;
        r = hasR ? r : 0;
        sq[0] += uint64_t(int64_t(l) * int64_t(l));
        sq[1] += uint64_t(int64_t(r) * int64_t(r));
        cross += int64_t(l) * int64_t(r);
        lane[0] += l;
        lane[1] += r;
        tally[0] += uint32_t(hasL) + (uint32_t(abs(l) >= kLvFull) << 16);
        tally[1] += uint32_t(hasR) + (uint32_t(abs(r) >= kLvFull) << 16);
    }
    __device__ __forceinline__ void settle()
    {
        sum[0] += lane[0];
        sum[1] += lane[1];
        lane[0] = lane[1] = 0;
    }
    __device__ __forceinline__ void foldLane(int o)                      // (of settled lanes)
    {
        sq[0] += __shfl_xor((unsigned long long)sq[0], o);
        sq[1] += __shfl_xor((unsigned long long)sq[1], o);
        cross += __shfl_xor((long long)cross, o);
        sum[0] += __shfl_xor((long long)sum[0], o);
        sum[1] += __shfl_xor((long long)sum[1], o);
        tally[0] += __shfl_xor(tally[0], o);
        tally[1] += __shfl_xor(tally[1], o);
    }
};
__device__ __forceinline__ Narrow noSamples() { return Narrow{{0, 0}, 0, {0, 0}, {0, 0}, {0, 0}}; }

// any number of sample frames: the record's own widths (|sum| < 2^58 and count < 2^32 for a column of up to 2^32 - 1 samples, sgz.h)
struct Wide {
    u128 sq[2];
    i128 cross;
    int64_t sum[2];
    uint32_t count[2], overs[2];
    __device__ __forceinline__ void add(const Narrow &k)
    {
        sq[0] += k.sq[0];
        sq[1] += k.sq[1];
        cross += i128(k.cross);
        sum[0] += k.sum[0] + k.lane[0];
        sum[1] += k.sum[1] + k.lane[1];
        count[0] += k.tally[0] & 0xffffu;
        count[1] += k.tally[1] & 0xffffu;
        overs[0] += k.tally[0] >> 16;
        overs[1] += k.tally[1] >> 16;
    }
    __device__ __forceinline__ void add(const sgz_level_record &r)
    {
        sq[0] += u128(r.sumsq[0][1]) << 64 | r.sumsq[0][0];
        sq[1] += u128(r.sumsq[1][1]) << 64 | r.sumsq[1][0];
        cross += i128(u128(r.cross[1]) << 64 | r.cross[0]);
        sum[0] += r.sum[0];
        sum[1] += r.sum[1];
        count[0] += r.count[0];
        count[1] += r.count[1];
        overs[0] += r.overs[0];
        overs[1] += r.overs[1];
    }
    __device__ __forceinline__ void store(sgz_level_record *to) const
    {
        sgz_level_record r;
        r.sumsq[0][0] = uint64_t(sq[0]); r.sumsq[0][1] = uint64_t(sq[0] >> 64);
        r.sumsq[1][0] = uint64_t(sq[1]); r.sumsq[1][1] = uint64_t(sq[1] >> 64);
        r.cross[0] = uint64_t(u128(cross)); r.cross[1] = uint64_t(u128(cross) >> 64);
        r.sum[0] = sum[0]; r.sum[1] = sum[1];
        r.count[0] = count[0]; r.count[1] = count[1];
        r.overs[0] = overs[0]; r.overs[1] = overs[1];
        *to = r;
    }
};
__device__ __forceinline__ Wide nothing() { return Wide{{0, 0}, 0, {0, 0}, {0, 0}, {0, 0}}; }

// what a (column, pair) does with its sums: the carry into column 0, then the record to the output (a closed column) or to the carry
__device__ __forceinline__ void emitColumn(const LevelParams &prm, long col, uint32_t p, Wide w)
{
    if (col == 0 && prm.held) w.add(prm.carryIn[p]);
    w.store(col < prm.closed ? prm.level + size_t(col) * prm.pairs + p : prm.carryOut + p);
}

// the tile's two rows through LDS, then groups of prm.group lanes per column
__global__ void __launch_bounds__(kLvThreads)
levelTileKernel(const LevelParams prm)
{
    __shared__ __attribute__((aligned(16))) int32_t tile[2][kLvTileWords];
    const uint32_t tid = threadIdx.x, p = blockIdx.y;
    TileBounds t;
    tileBounds(prm, t);
    const long c0 = t.c0, c1 = t.c1, a = t.a, b = t.b;
    const uint32_t count = uint32_t(b - a);                                 // <= perTile * m <= kLvTile
    const float *gL = prm.planar + size_t(2 * p) * prm.stride + size_t(a), *gR = gL + prm.stride;
    const uint32_t leadL = uint32_t(reinterpret_cast<uintptr_t>(gL) >> 2) & 3u, leadR = uint32_t(reinterpret_cast<uintptr_t>(gR) >> 2) & 3u;
    stageRow<true, kLvThreads, kLvUnroll>(gL, count, leadL, tile[0]);
    stageRow<true, kLvThreads, kLvUnroll>(gR, count, leadR, tile[1]);
    __syncthreads();
    const uint32_t G = prm.group, sub = tid & (G - 1u), grp = tid / G, groups = uint32_t(kLvThreads) / G;
    const uint32_t cols = uint32_t(c1 - c0);
    for (uint32_t base = 0; base < cols; base += groups) {                  // (the same trips in every lane: the cross-lane steps see whole waves)
        const uint32_t lc = base + grp;
        const bool mine = lc < cols;
        Narrow k = noSamples();                                             // (a column's samples: at most m <= kLvSwitch terms, kLvPerLane of them this lane's)
        if (mine) {
            long ca, cb;
            columnSamples(prm, c0 + long(lc), ca, cb);
            const uint32_t end = uint32_t(cb - a);
#pragma unroll 4
            for (uint32_t i = uint32_t(ca - a) + sub; i < end; i += G) k.take(tile[0][tileWord(leadL + i)], tile[1][tileWord(leadR + i)]);
        }
        k.settle();
        for (uint32_t o = G >> 1; o > 0; o >>= 1) k.foldLane(int(o));
        if (mine && sub == 0) {
            Wide w = nothing();
            w.add(k);
            emitColumn(prm, c0 + long(lc), p, w);
        }
    }
}

// this lane's share of the sums of sample frames [a, b) of a pair's rows, `lanes` lanes side by side.  Where both rows begin equally far from
// a 16-byte boundary: 16-byte loads between the first and the last boundary, kLvScan per row in flight, up to three scalar loads on either
// side; else 4-byte loads, lane after lane.  A batch of loads goes into a Narrow (4 * kLvScan terms at most), the Narrow into the Wide.
__device__ __forceinline__ Wide scanLanes(const float *rowL, const float *rowR, long a, long b, uint32_t lane, uint32_t lanes)
{
    Wide w = nothing();
    if (b <= a) return w;
    const float *gL = rowL + a, *gR = rowR + a;
    const size_t count = size_t(b - a);
    const uint32_t qnan = 0x7fc00000u;                                      // (a NaN takes no part)
    if (((reinterpret_cast<uintptr_t>(gL) ^ reinterpret_cast<uintptr_t>(gR)) & 15u) == 0) {
        uint32_t head;
        size_t vecs, tail;
        splitAligned(gL, count, head, vecs, tail);
        Narrow k = noSamples();
        if (lane < head) k.take(quantiseMarked(__float_as_uint(gL[lane])), quantiseMarked(__float_as_uint(gR[lane])));
        if (lane < count - tail) k.take(quantiseMarked(__float_as_uint(gL[tail + lane])), quantiseMarked(__float_as_uint(gR[tail + lane])));
        w.add(k);
        const uint4 *vL = reinterpret_cast<const uint4 *>(gL + head), *vR = reinterpret_cast<const uint4 *>(gR + head);
        for (size_t i = lane; i < vecs; i += size_t(lanes) * kLvScan) {
            uint4 l[kLvScan], r[kLvScan];
#pragma unroll
            for (int j = 0; j < kLvScan; ++j) {
                const size_t at = i + size_t(j) * lanes;
                l[j] = at < vecs ? vL[at] : make_uint4(qnan, qnan, qnan, qnan);
                r[j] = at < vecs ? vR[at] : make_uint4(qnan, qnan, qnan, qnan);
            }
            k = noSamples();
#pragma unroll
            for (int j = 0; j < kLvScan; ++j) {
                k.take(quantiseMarked(l[j].x), quantiseMarked(r[j].x));
                k.take(quantiseMarked(l[j].y), quantiseMarked(r[j].y));
                k.take(quantiseMarked(l[j].z), quantiseMarked(r[j].z));
                k.take(quantiseMarked(l[j].w), quantiseMarked(r[j].w));
            }
            w.add(k);
        }
        return w;
    }
    const uint32_t *sL = reinterpret_cast<const uint32_t *>(gL), *sR = reinterpret_cast<const uint32_t *>(gR);
    for (size_t i = lane; i < count; i += size_t(lanes) * 4 * kLvScan) {
        uint32_t l[4 * kLvScan], r[4 * kLvScan];
#pragma unroll
        for (int j = 0; j < 4 * kLvScan; ++j) {
            const size_t at = i + size_t(j) * lanes;
            l[j] = at < count ? sL[at] : qnan;
            r[j] = at < count ? sR[at] : qnan;
        }
        Narrow k = noSamples();
#pragma unroll
        for (int j = 0; j < 4 * kLvScan; ++j) k.take(quantiseMarked(l[j]), quantiseMarked(r[j]));
        w.add(k);
    }
    return w;
}

__device__ __forceinline__ uint64_t shuffleXor(uint64_t v, int o) { return __shfl_xor((unsigned long long)v, o); }

// every lane ends with the sums of all 64
__device__ __forceinline__ Wide waveFold(Wide w)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        for (int c = 0; c < 2; ++c) {
            w.sq[c] += u128(shuffleXor(uint64_t(w.sq[c] >> 64), o)) << 64 | shuffleXor(uint64_t(w.sq[c]), o);
            w.sum[c] += int64_t(shuffleXor(uint64_t(w.sum[c]), o));
            w.count[c] += __shfl_xor(w.count[c], o);
            w.overs[c] += __shfl_xor(w.overs[c], o);
        }
        w.cross += i128(u128(shuffleXor(uint64_t(u128(w.cross) >> 64), o)) << 64 | shuffleXor(uint64_t(u128(w.cross)), o));
    }
    return w;
}

// slice blockIdx.z of column blockIdx.x's samples of pair blockIdx.y (an empty slice -- more slices than samples -- leaves the zero record)
__global__ void __launch_bounds__(kLvThreads)
levelSliceKernel(const LevelParams prm)
{
    __shared__ sgz_level_record lds[kLvThreads / 64];
    const long col = long(blockIdx.x);
    const uint32_t p = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
    long a, b, sa, sb;
    columnSamples(prm, col, a, b);
    sliceSamples(prm, a, b, s, sa, sb);
    const float *rowL = prm.planar + size_t(2 * p) * prm.stride;
    Wide w = waveFold(scanLanes(rowL, rowL + prm.stride, sa, sb, tid, uint32_t(kLvThreads)));
    if ((tid & 63u) == 0) w.store(&lds[tid >> 6]);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < kLvThreads / 64; ++v) w.add(lds[v]);
        w.store(prm.partial + (size_t(s) * size_t(prm.columns) + size_t(col)) * prm.pairs + p);
    }
}

// one thread per (column, pair): the sum over the slices (none: a flush of the carry alone), the carry, the store
__global__ void __launch_bounds__(kLvThreads)
levelEmitKernel(const LevelParams prm)
{
    const size_t at = size_t(blockIdx.x) * kLvThreads + threadIdx.x, perSlice = size_t(prm.columns) * prm.pairs;
    if (at >= perSlice) return;
    Wide w = nothing();
    for (uint32_t s = 0; s < prm.slices; ++s) w.add(prm.partial[size_t(s) * perSlice + at]);
    emitColumn(prm, long(at / prm.pairs), uint32_t(at % prm.pairs), w);
}

// ---- the host helpers' 128-bit arithmetic: two words with carry ---------------------------------------------------------------------------
void addWords(uint64_t acc[2], const uint64_t v[2])
{
    const uint64_t lo = acc[0] + v[0];
    acc[1] += v[1] + (lo < acc[0] ? 1u : 0u);
    acc[0] = lo;
}

// the magnitude (lo, hi) as a double: hi is exact below 2^53 (any column's is below 2^20), lo rounds once, the sum once
double wordsToDouble(uint64_t lo, uint64_t hi) { return std::ldexp(double(hi), 64) + double(lo); }

}  // namespace

namespace sgz {

ColumnsShape levelColumnsShape(uint32_t pairs, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices)
{
    return columnsShape(pairs, nsamples, m, held, flush, slices, kLvSwitch, sizeof(sgz_level_record), 0);
}

sgz_status runLevelColumns(const ColumnsShape &sh, const float *d_planar, size_t channelStride, uint32_t pairs, size_t nsamples, uint32_t m,
                           uint32_t held, const sgz_level_record *carryIn, sgz_level_record *carryOut, sgz_level_record *d_level, void *scratch,
                           hipStream_t stream)
{
    if (!sh.launch) return SGZ_OK;
    LevelParams prm{};
    fillGrid(prm, sh, d_planar, channelStride, nsamples, m, held);
    prm.pairs = pairs;
    prm.carryIn = carryIn; prm.carryOut = carryOut;
    prm.level = d_level; prm.partial = static_cast<sgz_level_record *>(scratch);
    return launchPlainLane(levelTileKernel, levelSliceKernel, levelEmitKernel, kLvThreads, "level", prm, sh, pairs, nsamples, 1, [m](LevelParams &p) {
        p.perTile = kLvTile / m;
        p.group = pow2AtLeast((m + kLvPerLane - 1) / kLvPerLane);     // (1 .. 64: at most sixteen sample frames a lane)
    }, stream);
}

}  // namespace sgz

extern "C" {

void sgz_level_columns_limits(uint32_t *switch_over, uint32_t *tile_samples)
{
    if (switch_over) *switch_over = kLvSwitch;
    if (tile_samples) *tile_samples = kLvTile;
}

sgz_status sgz_stage_level_columns(const float *d_planar, size_t channel_stride, uint32_t pairs, size_t nsamples, uint32_t m, uint32_t held,
                                   int flush, uint32_t slices, sgz_level_record *d_carry, sgz_level_record *d_level, void *stream)
{
    const StageFront front{"sgz_stage_level_columns", "pairs", kLvMaxPairs, "d_level", 16, false, 62};
    return stageColumns(front, SGZ_OK, d_planar, channel_stride, pairs, nsamples, m, held, flush, 0, 0, slices, d_carry, d_level, stream, levelColumnsShape,
                        size_t(pairs) * sizeof(sgz_level_record), noStep, [&](const ColumnsShape &sh, const void *carryIn, void *scratch, hipStream_t s) {
                            return runLevelColumns(sh, d_planar, channel_stride, pairs, nsamples, m, held, static_cast<const sgz_level_record *>(carryIn), d_carry, d_level, scratch, s);
                        });
}

sgz_status sgz_level_fold(const sgz_level_record *in, size_t n, uint32_t pairs, size_t x0, size_t x1, uint32_t out_columns, sgz_level_record *out)
{
    return foldColumns(
        "sgz_level_fold", "pairs", " samples", in, n, pairs, x0, x1, out_columns, out,
        [](const sgz_level_record *v, size_t count, size_t stride) {
            uint64_t tally[2] = {0, 0};
            for (size_t j = 0; j < count; ++j)
                for (int c = 0; c < 2; ++c) tally[c] += v[j * stride].count[c];
            return tally[0] <= 0xffffffffull && tally[1] <= 0xffffffffull;
        },
        [](const sgz_level_record *in, size_t count, size_t stride) {
            sgz_level_record r;
            std::memset(&r, 0, sizeof r);
            for (size_t j = 0; j < count; ++j) {
                const sgz_level_record &v = in[j * stride];
                addWords(r.sumsq[0], v.sumsq[0]);
                addWords(r.sumsq[1], v.sumsq[1]);
                addWords(r.cross, v.cross);                        // (two's complement adds as unsigned)
                for (int c = 0; c < 2; ++c) {
                    r.sum[c] = int64_t(uint64_t(r.sum[c]) + uint64_t(v.sum[c]));
                    r.count[c] += v.count[c];
                    r.overs[c] += v.overs[c];
                }
            }
            return r;
        });
}

sgz_status sgz_level_readout(const sgz_level_record *rec, sgz_level_reading *out)
{
    if (!rec || !out) return fail(SGZ_EINVAL, "sgz_level_readout: null argument");
    double sq[2];
    for (int c = 0; c < 2; ++c) {
        sq[c] = wordsToDouble(rec->sumsq[c][0], rec->sumsq[c][1]);
        const double meanSquare = sq[c] / (double(rec->count[c]) * 0x1p46);                    // (0 / 0: NaN for a column without samples)
        out->rms[c] = std::sqrt(meanSquare);
        out->rms_db[c] = 10.0 * std::log10(meanSquare);
        out->dc[c] = double(rec->sum[c]) / (double(rec->count[c]) * 0x1p23);
    }
    uint64_t lo = rec->cross[0], hi = rec->cross[1];
    const bool negative = (hi >> 63) != 0;
    if (negative) {                                                // the magnitude: two's complement negation of (lo, hi)
        lo = ~lo + 1u;
        hi = ~hi + (lo == 0 ? 1u : 0u);
    }
    const double cross = negative ? -wordsToDouble(lo, hi) : wordsToDouble(lo, hi);
    out->correlation = (sq[0] == 0.0 || sq[1] == 0.0) ? 0.0 : cross / std::sqrt(sq[0] * sq[1]);
    return SGZ_OK;
}

}  // extern "C"
