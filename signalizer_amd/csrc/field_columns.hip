// field_columns.hip -- the stereo-field lane's reduction: one sgz_field_record (a histogram over 32 sectors of stereo direction: the sum and the
// maximum of the radius and the frame count per sector, beside the silent and the skipped frames) per column of m sample frames and channel
// pair of a linear planar stream, with a carried open column (sgz.h, "The stereo-field lane"); and the lane's host helpers: the boundary
// table, the fold of kept records and the readout of one.  gfx950 only.  The reference's polar plot is live (drawPolarPlot); the lane takes
// its geometry from it -- direction from (L + R, L - R), radius = max(|L|, |R|), left at negative angles -- and nothing else.
// What the column lanes share -- the shape of a call, the bounds, the quantiser, the staging of a row, the stage call's front, the fold's
// frame -- is column_lanes.hpp; this file is the histogram.
//   v = the quantiser's (quantiseMarked); a frame with a NaN on either side is skipped, one with vL = vR = 0 is silent; every other frame adds its
//   radius to the sector its direction falls in, found by exact 64-bit tests against the 32 integer boundary directions (kFdDirs).  All fields
//   are integer sums and maxima, so any cut of the stream (calls with a carry) or of a column (lanes, slices) gives the same bytes.
// A histogram is a scatter: lanes that add to one address serialise, and real music piles its frames into two or three sectors.  Nothing is
// scattered here.  A tile's frames become one packed word each in LDS (sector << 27 | radius; two words no frame makes for silent and
// skipped), and then a LANE IS A SECTOR: a half-wave of 32 lanes reads a column's words one after another -- every lane the same word, a
// broadcast -- and each lane keeps count, sum and peak of its own sector in registers.  No table in LDS, no atomics, nothing to zero or to
// fold inside a column, and the rate is the same whatever the signal: an all-mono file costs what noise costs (DESIGN.md section 4 has the
// measurements, and what the broadcast costs: every word is looked at by 32 lanes).
//   m <= kFdSwitch (512)    fieldTileKernel: one workgroup per (pair, tile); a tile is kFdTile / m whole columns of both rows of the pair.  The
//                           rows go to LDS quantised (stageRow, plain: nothing strides these rows), the frames are packed in place, and each of the workgroup's eight half-waves takes a column
//                           at a time.  The lanes of the half-wave store the record: lane b its sector's three fields.  A tile of the
//                           shortest columns holds kFdTile of them (m = 1): there is no table per column to bound that number.
//   else, or slices >= 2    fieldSliceKernel: workgroup (column, pair, slice) takes its part of the column through LDS a tile at a time, the
//                           eight half-waves an eighth of every tile each, the sums in registers from tile to tile -> partial records
//                           [slices][columns][pairs] in scratch; fieldEmitKernel, a launch of its own behind it, folds the slices and the carry
//                           with one lane per (column, pair, sector).  A flush without samples is the emit kernel alone, on the carry.
// Every sample is read from memory once.  Nothing is waited for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "column_lanes.hpp"

using namespace sgz;

namespace {

constexpr int kFdThreads = 256;
constexpr int kFdHalves = kFdThreads / 32;       // half-waves of a workgroup: 32 lanes, one per sector
constexpr uint32_t kFdTile = 4096;               // sample frames of a tile (two rows of quantised samples: 32 KiB of LDS)
constexpr uint32_t kFdSwitch = 512;              // the switch-over: columns longer than this take the sliced form (a full tile of shorter ones
                                                 // has a column for every half-wave)
constexpr uint32_t kFdMaxPairs = 32;
constexpr int kFdUnroll = 4;                     // 16-byte loads per row a lane issues before the first store to LDS
constexpr uint32_t kFdRowWords = kFdTile + 4;    // a row of the tile and its lead: the row's own offset within 16 bytes
constexpr int32_t kFdClamp = 1 << 26;            // the quantiser's range, and the greatest radius
constexpr int32_t kFdNaN = kQuantNaN;            // a NaN in LDS
// a frame in LDS: sector << 27 | radius with 1 <= radius <= 2^26, or one of two words whose radius field is above 2^26 in every sector
constexpr uint32_t kFdSilent = 0xffffffffu, kFdSkipped = 0xfffffffeu;
static_assert(SGZ_FIELD_SECTORS == 32, "a lane of a half-wave per sector, five bits of a packed frame");
static_assert(kFdTile == 4u * kFdThreads * kFdUnroll, "a lane moves kFdUnroll 16-byte chunks of a tile's row");
static_assert(kFdSwitch * kFdHalves <= kFdTile, "a full tile of short columns has one for every half-wave");
static_assert(uint64_t(kFdClamp) < (1u << 27) && (kFdSilent & 0x7ffffffu) > uint32_t(kFdClamp) && (kFdSkipped & 0x7ffffffu) > uint32_t(kFdClamp),
              "a radius fits 27 bits, and the two marks are no frame's word");
// the radius sum: 2^26 a frame and at most 2^32 - 1 frames a column stay below 2^58; the 32-bit counts bound nothing below that
static_assert((uint64_t(kFdClamp) << 32) == (uint64_t(1) << 58), "a column's radius sums fit 64 bits");
static_assert(sizeof(sgz_field_record) == 528 && sizeof(sgz_field_record) % 16 == 0, "sgz.h documents 528 bytes");

// The boundaries (sgz.h has the same literal, and it is the normative one): (C_k, S_k) = (rint(cos g_k 2^30), rint(sin g_k 2^30)),
// g_k = (k - 15.5) pi / 32
#define SGZ_FD_DIRS                                                                                                                              \
    {{52686014, -1072448455}, {157550647, -1062120190}, {260897982, -1041563127}, {361732726, -1010975242}, {459083786, -970651112},               \
     {552013618, -920979082}, {639627258, -862437520}, {721080937, -795590213}, {795590213, -721080937}, {862437520, -639627258},                  \
     {920979082, -552013618}, {970651112, -459083786}, {1010975242, -361732726}, {1041563127, -260897982}, {1062120190, -157550647},               \
     {1072448455, -52686014}, {1072448455, 52686014}, {1062120190, 157550647}, {1041563127, 260897982}, {1010975242, 361732726},                   \
     {970651112, 459083786}, {920979082, 552013618}, {862437520, 639627258}, {795590213, 721080937}, {721080937, 795590213},                       \
     {639627258, 862437520}, {552013618, 920979082}, {459083786, 970651112}, {361732726, 1010975242}, {260897982, 1041563127},                     \
     {157550647, 1062120190}, {52686014, 1072448455}}
constexpr int32_t kFdDirs[32][2] = SGZ_FD_DIRS;
__device__ const int32_t kFdDirsDevice[32][2] = SGZ_FD_DIRS;
#undef SGZ_FD_DIRS

// what the sector search relies on: the table is symmetric, every entry is at most 2^30 (so a product with |M|, |X| <= 2^27 is at most 2^57
// and the difference of two fits 64 bits), and the rounded directions still increase strictly in angle (the cross product of neighbours is
// positive), so the true tests form a prefix
constexpr bool dirsAreSound()
{
    for (int k = 0; k < 32; ++k) {
        if (kFdDirs[31 - k][0] != kFdDirs[k][0] || kFdDirs[31 - k][1] != -kFdDirs[k][1]) return false;
        if (kFdDirs[k][0] <= 0 || kFdDirs[k][0] > (1 << 30) || kFdDirs[k][1] > (1 << 30) || kFdDirs[k][1] < -(1 << 30)) return false;
        if (k < 31 && int64_t(kFdDirs[k][0]) * kFdDirs[k + 1][1] - int64_t(kFdDirs[k][1]) * kFdDirs[k + 1][0] <= 0) return false;
    }
    return true;
}
static_assert(dirsAreSound(), "the boundary table");

struct FieldParams {
    const float *planar;                 // [2 pairs][stride]
    size_t stride;
    long n;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t m, held, pairs;
    uint32_t perTile;                    // columns of a tile = kFdTile / m
    uint32_t slices;
    const sgz_field_record *carryIn;     // [pairs]: column 0's `held` earlier samples (read iff held > 0)
    sgz_field_record *carryOut;          // [pairs]: the open column
    sgz_field_record *field;             // [closed][pairs]
    sgz_field_record *partial;           // [slices][columns][pairs]
};

// A frame's word.  n = #{k : C_k X - S_k M >= 0} by binary search over the tests 0 .. 30 (they form a prefix), then test 31 where all of
// those hold: n = 32 is sector 0 again, the antiphase line from its other end.  Every product is a v_mad_i64_i32, exact.
__device__ __forceinline__ uint32_t packFrame(int32_t l, int32_t r, const int2 *dirs)
{
    const bool skipped = l == kFdNaN || r == kFdNaN;
    l = skipped ? 0 : l;
    r = skipped ? 0 : r;
    int32_t M = l + r, X = r - l;                                          // |.| <= 2^27
    if (M < 0) { M = -M; X = -X; }
    const auto holds = [&](uint32_t k) { const int2 d = dirs[k]; return int64_t(d.x) * int64_t(X) - int64_t(d.y) * int64_t(M) >= 0; };
    uint32_t n = 0;
#pragma unroll
    for (uint32_t step = 16; step > 0; step >>= 1)
        if (holds(n + step - 1)) n += step;
    if (n == 31 && holds(31)) n = 0;
    const uint32_t radius = uint32_t(max(abs(l), abs(r)));
    return skipped ? kFdSkipped : radius == 0 ? kFdSilent : (n << 27 | radius);
}

// a sector's sums in the lane that is the sector: any number of frames (the record's own widths)
struct Sector {
    uint64_t radius;
    uint32_t count, peak;
    __device__ __forceinline__ void take(uint32_t word, uint32_t key)      // key: the lane's sector << 27
    {
        const uint32_t x = word ^ key;                                      // this sector's frame: its radius; any other word: above 2^26
        const bool hit = x <= uint32_t(kFdClamp);
        const uint32_t r = hit ? x : 0u;
        radius += r;
        count += hit ? 1u : 0u;
        peak = max(peak, r);
    }
};

// The tile of one (pair, sample range) in LDS.  load: `count` frames at gL / gR -> a packed word per frame in row 0, frame j at words()[j]
// (the workgroup's call; it ends behind a barrier).  Each row keeps its own offset within 16 bytes, so the rows of a pair need not share one
struct Tile {
    int32_t row[2][kFdRowWords];
    int2 dirs[32];
    uint32_t lead;                                                          // row 0's: written by every lane with the same value

    __device__ __forceinline__ void load(const float *gL, const float *gR, uint32_t count)
    {
        const uint32_t tid = threadIdx.x;
        const uint32_t leadL = uint32_t(reinterpret_cast<uintptr_t>(gL) >> 2) & 3u, leadR = uint32_t(reinterpret_cast<uintptr_t>(gR) >> 2) & 3u;
        if (tid < 32) dirs[tid] = make_int2(kFdDirsDevice[tid][0], kFdDirsDevice[tid][1]);
        if (tid == 0) lead = leadL;
        stageRow<false, kFdThreads, kFdUnroll>(gL, count, leadL, row[0]);      // (plain rows: nothing strides them)
        stageRow<false, kFdThreads, kFdUnroll>(gR, count, leadR, row[1]);
        __syncthreads();
        for (uint32_t i = tid; i < count; i += kFdThreads)                  // (a lane packs the frames it reads: in place)
            row[0][leadL + i] = int32_t(packFrame(row[0][leadL + i], row[1][leadR + i], dirs));
        __syncthreads();
    }
    // frames [i0, i1) of the tile into the lane's sector: every lane of the half-wave reads the same words, 16 bytes at a time between the
    // 16-byte boundaries of LDS
    __device__ __forceinline__ void scan(uint32_t i0, uint32_t i1, uint32_t key, Sector &s) const
    {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(row[0]);
        uint32_t i = lead + i0;
        const uint32_t end = lead + i1;
        for (; i < end && (i & 3u); ++i) s.take(w[i], key);
        for (; i + 4 <= end; i += 4) {
            const uint4 q = *reinterpret_cast<const uint4 *>(w + i);
            s.take(q.x, key);
            s.take(q.y, key);
            s.take(q.z, key);
            s.take(q.w, key);
        }
        for (; i < end; ++i) s.take(w[i], key);
    }
    // this lane's share of the silent and skipped frames among [i0, i1): the 32 lanes of the half-wave side by side
    __device__ __forceinline__ void marks(uint32_t i0, uint32_t i1, uint32_t lane, uint32_t &silent, uint32_t &skipped) const
    {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(row[0]) + lead;
        for (uint32_t i = i0 + lane; i < i1; i += 32) {
            const uint32_t v = w[i];
            silent += v == kFdSilent ? 1u : 0u;
            skipped += v == kFdSkipped ? 1u : 0u;
        }
    }
};

// the sum over the 32 lanes of a half-wave, in every one of them (called by whole waves)
__device__ __forceinline__ uint32_t halfWaveSum(uint32_t v)
{
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// what lane `b` of a (column, pair) does with its sector's sums (lane 0 also with the marks): the carry into column 0, then the fields to the
// output (a closed column) or to the carry (the open column)
__device__ __forceinline__ void emitColumn(const FieldParams &prm, long col, uint32_t p, uint32_t b, Sector s, uint32_t silent, uint32_t skipped)
{
    if (col == 0 && prm.held) {
        const sgz_field_record *c = prm.carryIn + p;
        s.radius += c->radius[b];
        s.count += c->count[b];
        s.peak = max(s.peak, c->peak[b]);
        if (b == 0) { silent += c->silent; skipped += c->skipped; }
    }
    sgz_field_record *to = col < prm.closed ? prm.field + size_t(col) * prm.pairs + p : prm.carryOut + p;
    to->radius[b] = s.radius;
    to->count[b] = s.count;
    to->peak[b] = s.peak;
    if (b == 0) { to->silent = silent; to->skipped = skipped; to->reserved = 0; }
}

// the tile's frames packed in LDS, then a half-wave per column
__global__ void __launch_bounds__(kFdThreads)
fieldTileKernel(const FieldParams prm)
{
    __shared__ __attribute__((aligned(16))) Tile tile;
    const uint32_t tid = threadIdx.x, p = blockIdx.y;
    TileBounds t;
    tileBounds(prm, t);
    const long c0 = t.c0, c1 = t.c1, a = t.a, b = t.b;
    const float *gL = prm.planar + size_t(2 * p) * prm.stride + size_t(a);
    tile.load(gL, gL + prm.stride, uint32_t(b - a));                        // (b - a <= perTile * m <= kFdTile)
    const uint32_t lane = tid & 31u, half = tid >> 5, cols = uint32_t(c1 - c0);
    for (uint32_t base = 0; base < cols; base += kFdHalves) {               // (the same trips in every lane: the cross-lane steps see whole waves)
        const uint32_t lc = base + half;
        const bool mine = lc < cols;
        Sector s{0, 0, 0};
        uint32_t silent = 0, skipped = 0;
        if (mine) {
            long ca, cb;
            columnSamples(prm, c0 + long(lc), ca, cb);
            tile.scan(uint32_t(ca - a), uint32_t(cb - a), lane << 27, s);
            tile.marks(uint32_t(ca - a), uint32_t(cb - a), lane, silent, skipped);
        }
        silent = halfWaveSum(silent);
        skipped = halfWaveSum(skipped);
        if (mine) emitColumn(prm, c0 + long(lc), p, lane, s, silent, skipped);
    }
}

// slice blockIdx.z of column blockIdx.x's samples of pair blockIdx.y (an empty slice -- more slices than samples -- leaves the zero record)
__global__ void __launch_bounds__(kFdThreads)
fieldSliceKernel(const FieldParams prm)
{
    __shared__ __attribute__((aligned(16))) Tile tile;
    __shared__ uint64_t foldRadius[kFdHalves][32];
    __shared__ uint32_t foldCount[kFdHalves][32], foldPeak[kFdHalves][32], foldMarks[kFdHalves][2];
    const long col = long(blockIdx.x);
    const uint32_t p = blockIdx.y, sl = blockIdx.z, tid = threadIdx.x, lane = tid & 31u, half = tid >> 5;
    long a, b, sa, sb;
    columnSamples(prm, col, a, b);
    sliceSamples(prm, a, b, sl, sa, sb);
    const float *rowL = prm.planar + size_t(2 * p) * prm.stride;
    Sector s{0, 0, 0};
    uint32_t silent = 0, skipped = 0;
    for (long at = sa; at < sb; at += long(kFdTile)) {                      // (sa, sb: the workgroup's, so every lane meets every barrier)
        const uint32_t count = uint32_t(sb - at < long(kFdTile) ? sb - at : long(kFdTile));
        if (at != sa) __syncthreads();                                      // the tile before this one has been read
        tile.load(rowL + at, rowL + prm.stride + at, count);
        const uint32_t i0 = count * half / kFdHalves, i1 = count * (half + 1) / kFdHalves;     // an eighth of the tile a half-wave
        tile.scan(i0, i1, lane << 27, s);
        tile.marks(i0, i1, lane, silent, skipped);
    }
    silent = halfWaveSum(silent);
    skipped = halfWaveSum(skipped);
    foldRadius[half][lane] = s.radius;
    foldCount[half][lane] = s.count;
    foldPeak[half][lane] = s.peak;
    if (lane == 0) { foldMarks[half][0] = silent; foldMarks[half][1] = skipped; }
    __syncthreads();
    if (tid < 32) {
#pragma unroll
        for (int h = 1; h < kFdHalves; ++h) {
            s.radius += foldRadius[h][lane];
            s.count += foldCount[h][lane];
            s.peak = max(s.peak, foldPeak[h][lane]);
            silent += foldMarks[h][0];
            skipped += foldMarks[h][1];
        }
        sgz_field_record *to = prm.partial + (size_t(sl) * size_t(prm.columns) + size_t(col)) * prm.pairs + p;
        to->radius[lane] = s.radius;
        to->count[lane] = s.count;
        to->peak[lane] = s.peak;
        if (lane == 0) { to->silent = silent; to->skipped = skipped; to->reserved = 0; }
    }
}

// one lane per (column, pair, sector): the fold over the slices (none: a flush of the carry alone), the carry, the store
__global__ void __launch_bounds__(kFdThreads)
fieldEmitKernel(const FieldParams prm)
{
    const size_t at = size_t(blockIdx.x) * kFdThreads + threadIdx.x, cell = at >> 5, perSlice = size_t(prm.columns) * prm.pairs;
    const uint32_t b = uint32_t(at & 31u);
    if (cell >= perSlice) return;
    Sector s{0, 0, 0};
    uint32_t silent = 0, skipped = 0;
    for (uint32_t sl = 0; sl < prm.slices; ++sl) {
        const sgz_field_record *r = prm.partial + size_t(sl) * perSlice + cell;
        s.radius += r->radius[b];
        s.count += r->count[b];
        s.peak = max(s.peak, r->peak[b]);
        if (b == 0) { silent += r->silent; skipped += r->skipped; }
    }
    emitColumn(prm, long(cell / prm.pairs), uint32_t(cell % prm.pairs), b, s, silent, skipped);
}

}  // namespace

namespace sgz {

ColumnsShape fieldColumnsShape(uint32_t pairs, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices)
{
    return columnsShape(pairs, nsamples, m, held, flush, slices, kFdSwitch, sizeof(sgz_field_record), 0);
}

sgz_status runFieldColumns(const ColumnsShape &sh, const float *d_planar, size_t channelStride, uint32_t pairs, size_t nsamples, uint32_t m,
                           uint32_t held, const sgz_field_record *carryIn, sgz_field_record *carryOut, sgz_field_record *d_field, void *scratch,
                           hipStream_t stream)
{
    if (!sh.launch) return SGZ_OK;
    FieldParams prm{};
    fillGrid(prm, sh, d_planar, channelStride, nsamples, m, held);
    prm.pairs = pairs;
    prm.carryIn = carryIn; prm.carryOut = carryOut;
    prm.field = d_field; prm.partial = static_cast<sgz_field_record *>(scratch);
    return launchPlainLane(fieldTileKernel, fieldSliceKernel, fieldEmitKernel, kFdThreads, "field", prm, sh, pairs, nsamples, 32,
                           [m](FieldParams &p) { p.perTile = kFdTile / m; }, stream);
}

}  // namespace sgz

extern "C" {

void sgz_field_columns_limits(uint32_t *switch_over, uint32_t *tile_samples)
{
    if (switch_over) *switch_over = kFdSwitch;
    if (tile_samples) *tile_samples = kFdTile;
}

void sgz_field_boundaries(int32_t cs[32][2]) { std::memcpy(cs, kFdDirs, sizeof kFdDirs); }

sgz_status sgz_stage_field_columns(const float *d_planar, size_t channel_stride, uint32_t pairs, size_t nsamples, uint32_t m, uint32_t held,
                                   int flush, uint32_t slices, sgz_field_record *d_carry, sgz_field_record *d_field, void *stream)
{
    const StageFront front{"sgz_stage_field_columns", "pairs", kFdMaxPairs, "d_field", 16, false, 62};
    return stageColumns(front, SGZ_OK, d_planar, channel_stride, pairs, nsamples, m, held, flush, 0, 0, slices, d_carry, d_field, stream, fieldColumnsShape,
                        size_t(pairs) * sizeof(sgz_field_record), noStep, [&](const ColumnsShape &sh, const void *carryIn, void *scratch, hipStream_t s) {
                            return runFieldColumns(sh, d_planar, channel_stride, pairs, nsamples, m, held, static_cast<const sgz_field_record *>(carryIn), d_carry, d_field, scratch, s);
                        });
}

sgz_status sgz_field_fold(const sgz_field_record *in, size_t n, uint32_t pairs, size_t x0, size_t x1, uint32_t out_columns, sgz_field_record *out)
{
    return foldColumns(
        "sgz_field_fold", "pairs", " frames", in, n, pairs, x0, x1, out_columns, out,
        [](const sgz_field_record *in, size_t count, size_t stride) {
            uint64_t tally[SGZ_FIELD_SECTORS + 2] = {};
            for (size_t j = 0; j < count; ++j) {
                const sgz_field_record &v = in[j * stride];
                for (int k = 0; k < SGZ_FIELD_SECTORS; ++k) tally[k] += v.count[k];
                tally[SGZ_FIELD_SECTORS] += v.silent;
                tally[SGZ_FIELD_SECTORS + 1] += v.skipped;
            }
            return std::all_of(tally, tally + SGZ_FIELD_SECTORS + 2, [](uint64_t t) { return t <= 0xffffffffull; });
        },
        [](const sgz_field_record *in, size_t count, size_t stride) {
            sgz_field_record r;
            std::memset(&r, 0, sizeof r);
            for (size_t j = 0; j < count; ++j) {
                const sgz_field_record &v = in[j * stride];
                for (int k = 0; k < SGZ_FIELD_SECTORS; ++k) {
                    r.radius[k] += v.radius[k];
                    r.count[k] += v.count[k];
                    r.peak[k] = std::max(r.peak[k], v.peak[k]);
                }
                r.silent += v.silent;
                r.skipped += v.skipped;
            }
            return r;
        });
}

sgz_status sgz_field_readout(const sgz_field_record *rec, sgz_field_reading *out)
{
    if (!rec || !out) return fail(SGZ_EINVAL, "sgz_field_readout: null argument");
    const double pi = 3.14159265358979323846;
    double frames = 0, weight = 0, c2 = 0, s2 = 0;
    for (int b = 0; b < SGZ_FIELD_SECTORS; ++b) frames += double(rec->count[b]);
    for (int b = 0; b < SGZ_FIELD_SECTORS; ++b) {
        const double w = double(rec->radius[b]), theta = double(b - 16) * pi / 32.0;
        out->share[b] = frames > 0 ? double(rec->count[b]) / frames : 0.0;
        out->mean[b] = rec->count[b] ? w / (double(rec->count[b]) * 0x1p23) : 0.0;
        out->peak[b] = double(rec->peak[b]) / 0x1p23;
        weight += w;
        c2 += w * std::cos(2.0 * theta);
        s2 += w * std::sin(2.0 * theta);
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    out->direction = weight > 0 ? 0.5 * std::atan2(s2, c2) : nan;
    out->spread = weight > 0 ? 1.0 - std::hypot(s2, c2) / weight : nan;
    out->silent_share = frames + double(rec->silent) > 0 ? double(rec->silent) / (frames + double(rec->silent)) : 0.0;
    return SGZ_OK;
}

}  // extern "C"
