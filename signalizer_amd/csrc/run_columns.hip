// run_columns.hip -- the run lane's reduction: one sgz_run_record (for each of three predicates -- hot, quiet, flat -- the samples that have
// it, the runs that begin, the longest run and where it starts, the runs at either end; beside them the length, the NaNs and the sign
// changes) per column of m samples and channel of a linear planar stream, with a carried open column and a carried two-sample history
// (sgz.h, "The run lane"); and the lane's host helpers: the defaults, the fold of kept records and the readout of one.  gfx950 only.  The
// reference has no counterpart.
// What the column lanes share -- the shape of a call, the bounds, the quantiser, the staging of a row, the stage call's front with the
// carry's snapshot, the fold's frame -- is column_lanes.hpp; this file is the ordered fold.
//   v = the quantiser's (quantiseMarked: a NaN is a mark no sample equals).  A sample's predicates need v[i], v[i - 1] and -- for "a flat
//   run begins here" -- v[i - 2]: sample k < 0 of a call is the carry's prev[-1 - k] (marks when the stream begins here).  With them every
//   lane knows its sample's predicates AND whether a run begins at it, so the sums (count, runs, crossings, skipped) are plain sums; only
//   head, tail, longest and at depend on order.
// The fold is associative and NOT commutative: A followed by B is foldRec(A, B), never the other way round.  The element the kernels fold is
// not a sample but 64 consecutive ones: a wave's lanes take sample p + lane, eight __ballot's turn the predicates into 64-bit masks (bit j
// is sample p + j), and a segment [shift, shift + L) of the masks becomes a record by bit arithmetic (ofMask): popcounts, trailing and
// leading ones, and "x &= x << 1 until nothing is left" for the longest run -- the last x that was not 0 marks where runs of that length
// end, so its lowest bit is the earliest of them.  Elements are then folded strictly left to right; no butterfly, no atomics.
//   m <= kRnSwitch (1024)   runTileKernel: one workgroup per (channel, tile of kRnTile / m whole columns).  The tile goes to LDS quantised
//                           (stageRow, plain) behind a two-word halo.  m <= 32: a wave takes 64 / m columns at a time, one set of masks,
//                           and lane j cuts column j's segment out of them.  Longer columns: a wave takes a column and walks it 64
//                           samples a step, folding as it goes (takeStep: a predicate that none of the 64 has costs one move).
//                           Column 0 is folded behind the carry's open column.  The last tile's workgroup writes the rest of the
//                           carry.
//   else, or slices >= 2    runSliceKernel: workgroup (column, channel, slice); wave w walks quarter w of the slice straight from memory
//                           (the two samples before a lane's come from its neighbours, for lanes 0 and 1 from the step before or the
//                           halo), the four quarters are folded in order -> partial records [slices][columns][channels] in scratch;
//                           runEmitKernel, a launch of its own behind it, folds carry, slice 0, slice 1, .. in that order, stores, and
//                           writes the rest of the carry.  A flush without samples is the emit kernel alone, on the carry.
// Every sample is read from memory once, but for the halos.  Nothing is waited for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>

#include "column_lanes.hpp"

using namespace sgz;

namespace {

constexpr int kRnThreads = 256;
constexpr int kRnWaves = kRnThreads / 64;
constexpr uint32_t kRnTile = 4096;               // samples of a tile's row
constexpr uint32_t kRnSwitch = 1024;             // the switch-over: columns longer than this take the sliced form
constexpr uint32_t kRnMaxChannels = 64;
constexpr int kRnUnroll = 4;                     // 16-byte loads a lane of the tile form issues before the first store to LDS
constexpr int kRnScan = 8;                       // loads a lane of the sliced form has in flight
constexpr uint32_t kRnBase = 4;                  // where the tile's 16-byte grid begins in LDS: room for the halo in front, a multiple of 4
constexpr uint32_t kRnRowWords = kRnBase + 4 + kRnTile;      // the halo's room, the lead (the base's offset within 16 bytes), the tile
constexpr uint32_t kRnPacked = 32;               // columns up to here share a wave's masks
constexpr uint32_t kRnWords = sizeof(sgz_run_record) / 4;
constexpr int32_t kRnNaN = kQuantNaN;
constexpr uint32_t kRnMaxHot = 1u << 26;         // the quantiser's range
static_assert(sizeof(sgz_run_record) == 96 && sizeof(sgz_run_carry) == 112 && kRnWords == 24, "sgz.h documents 96 and 112 bytes");
static_assert(offsetof(sgz_run_record, of) == 16 && sizeof(sgz_run_of) == 24 && offsetof(sgz_run_carry, prev) == 96, "the record as words");
static_assert(SGZ_RUN_NAN == kQuantNaN, "the carry's mark is the quantiser's");
static_assert(kRnTile == 4u * kRnThreads * kRnUnroll, "a lane moves kRnUnroll 16-byte chunks of a tile's row");
static_assert(kRnSwitch <= kRnTile && kRnBase % 4 == 0 && kRnBase >= 2, "a short column fits a tile; the halo lies in front of it");

struct RunParams {
    const float *planar;                 // [channels][stride]
    size_t stride;
    long n;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t m, held, channels;
    uint32_t continued;                  // carryIn's prev holds the two samples before this call (else marks)
    uint32_t perTile;                    // columns of a tile = kRnTile / m
    uint32_t slices;
    uint32_t hot, quiet;                 // the thresholds (sgz_run_params)
    const sgz_run_carry *carryIn;        // [channels]: the history (continued) and column 0's `held` earlier samples (held > 0)
    sgz_run_carry *carryOut;             // [channels]: written whole by every call with samples
    sgz_run_record *runs;                // [closed][channels]
    sgz_run_record *partial;             // [slices][columns][channels]
};

// a column's, a segment's or a slice's record in registers
struct Of { uint32_t count, runs, longest, at, head, tail; };
struct Rec {
    uint32_t len, skipped, crossings;
    Of of[3];
};

__host__ __device__ __forceinline__ Of foldOf(const Of &A, uint32_t lenA, const Of &B, uint32_t lenB)
{
    Of r;
    r.count = A.count + B.count;
    r.runs = A.runs + B.runs;
    r.head = A.head == lenA ? lenA + B.head : A.head;
    r.tail = B.tail == lenB ? lenB + A.tail : B.tail;
    // the three candidates: A's, the run across the cut, B's; the greatest, and among equals the least position
    const uint32_t l2 = A.tail + B.head, p2 = lenA - A.tail, l3 = B.longest, p3 = lenA + B.at;
    uint32_t best = A.longest, at = A.at;
    if (l2 > best || (l2 == best && p2 < at)) { best = l2; at = p2; }
    if (l3 > best || (l3 == best && p3 < at)) { best = l3; at = p3; }
    r.longest = best;
    r.at = best ? at : 0u;
    return r;
}

// A followed by B
__host__ __device__ __forceinline__ Rec foldRec(const Rec &A, const Rec &B)
{
    Rec r;
    r.len = A.len + B.len;
    r.skipped = A.skipped + B.skipped;
    r.crossings = A.crossings + B.crossings;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.of[k] = foldOf(A.of[k], A.len, B.of[k], B.len);
    return r;
}

__host__ __device__ __forceinline__ Rec fromRecord(const sgz_run_record &s)
{
    Rec r;
    r.len = s.len; r.skipped = s.skipped; r.crossings = s.crossings;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.of[k] = Of{s.of[k].count, s.of[k].runs, s.of[k].longest, s.of[k].at, s.of[k].head, s.of[k].tail};
    return r;
}

__host__ __device__ __forceinline__ sgz_run_record toRecord(const Rec &r)
{
    sgz_run_record s;
    s.len = r.len; s.skipped = r.skipped; s.crossings = r.crossings; s.reserved0 = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s.of[k].count = r.of[k].count; s.of[k].runs = r.of[k].runs; s.of[k].longest = r.of[k].longest;
        s.of[k].at = r.of[k].at; s.of[k].head = r.of[k].head; s.of[k].tail = r.of[k].tail;
    }
    s.reserved[0] = s.reserved[1] = 0;
    return s;
}

__device__ __forceinline__ Rec nothing()
{
    Rec r;
    r.len = r.skipped = r.crossings = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.of[k] = Of{0, 0, 0, 0, 0, 0};
    return r;
}

// all 96 bytes of a record (aligned to 16: the output, the carry, the scratch), six 16-byte stores
__device__ __forceinline__ void storeRec(const Rec &r, sgz_run_record *to)
{
    uint4 *p = reinterpret_cast<uint4 *>(to);
    p[0] = make_uint4(r.len, r.skipped, r.crossings, 0u);
    p[1] = make_uint4(r.of[0].count, r.of[0].runs, r.of[0].longest, r.of[0].at);
    p[2] = make_uint4(r.of[0].head, r.of[0].tail, r.of[1].count, r.of[1].runs);
    p[3] = make_uint4(r.of[1].longest, r.of[1].at, r.of[1].head, r.of[1].tail);
    p[4] = make_uint4(r.of[2].count, r.of[2].runs, r.of[2].longest, r.of[2].at);
    p[5] = make_uint4(r.of[2].head, r.of[2].tail, 0u, 0u);
}

// what the predicates see at sample k of the call, k >= -2: the call's own sample, or the carried history in front of it
__device__ __forceinline__ int32_t sampleAt(const RunParams &prm, uint32_t ch, long k)
{
    if (k >= 0) return quantiseMarked(__float_as_uint(prm.planar[size_t(ch) * prm.stride + size_t(k)]));
    return prm.continued ? prm.carryIn[ch].prev[-1 - k] : kRnNaN;
}

// the predicates of 64 consecutive samples as masks: bit j is the sample of lane j
struct Masks {
    uint64_t is[3], starts[3], cross, nan;
};

__device__ __forceinline__ uint32_t magnitude(int32_t v) { return v < 0 ? 0u - uint32_t(v) : uint32_t(v); }

// v0, v1, v2: the lane's sample and the two before it (marks where there is none); has: the lane has a sample.  Called by whole waves.
// Most steps of most material have no hot, quiet or flat sample and no NaN: one ballot says so, and the seven that would all be 0 are
// not taken (the branch is the wave's: a ballot is the same in every lane)
__device__ __forceinline__ Masks masksOf(const RunParams &prm, int32_t v0, int32_t v1, int32_t v2, bool has)
{
    const bool ok0 = has && v0 != kRnNaN, ok1 = v1 != kRnNaN;
    const uint32_t a0 = magnitude(v0), a1 = magnitude(v1);
    const bool is0[3] = {ok0 && a0 >= prm.hot, ok0 && a0 <= prm.quiet, ok0 && v0 == v1};
    Masks k;
    k.cross = __ballot(ok0 && ok1 && ((v0 < 0) != (v1 < 0)));
    if (__ballot(is0[0] || is0[1] || is0[2] || (has && !ok0)) == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) k.is[q] = k.starts[q] = 0;
        k.nan = 0;
        return k;
    }
    const bool is1[3] = {ok1 && a1 >= prm.hot, ok1 && a1 <= prm.quiet, ok1 && v1 == v2};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        k.is[q] = __ballot(is0[q]);
        k.starts[q] = __ballot(is0[q] && !is1[q]);
    }
    k.nan = __ballot(has && !ok0);
    return k;
}

// One predicate of the L <= 64 samples whose bits are the low L of `seg` (nothing above them); starts: the runs that begin among them
__device__ __forceinline__ Of ofMask(uint64_t seg, uint64_t starts, uint32_t L, uint64_t low)
{
    Of o;
    if (seg == 0) return Of{0, 0, 0, 0, 0, 0};                              // no sample has it -- most segments of most material
    o.count = uint32_t(__popcll(seg));
    o.runs = uint32_t(__popcll(starts));
    if (seg == low) {                                                    // every sample has it (or there is none): one run, the whole of it
        o.longest = o.head = o.tail = L;
        o.at = 0;
        return o;
    }
    // (a bit below L is 0 from here on, and L >= 1)
    o.head = uint32_t(__ffsll((long long)~seg)) - 1u;                      // the trailing ones
    o.tail = uint32_t(__clzll((long long)~(seg << (64u - L))));             // the leading ones, counted from bit L - 1
    uint64_t x = seg, last = 0;
    uint32_t r = 0;
    while (x) {                                                             // after t steps bit j of x: bits j - t .. j of seg are all set
        last = x;
        x &= x << 1;
        ++r;
    }
    o.longest = r;
    o.at = r ? uint32_t(__ffsll((long long)last)) - r : 0u;                // the lowest end of a run of r, less r - 1
    return o;
}

// the record of the samples [shift, shift + L) of a wave's masks (shift + L <= 64); shift and L may differ from lane to lane
__device__ __forceinline__ Rec recOf(const Masks &k, uint32_t shift, uint32_t L)
{
    const uint64_t low = L >= 64u ? ~uint64_t(0) : (uint64_t(1) << L) - 1u;
    Rec r;
    r.len = L;
    r.skipped = uint32_t(__popcll((k.nan >> shift) & low));
    r.crossings = uint32_t(__popcll((k.cross >> shift) & low));
#pragma unroll
    for (int q = 0; q < 3; ++q) r.of[q] = ofMask((k.is[q] >> shift) & low, (k.starts[q] >> shift) & low, L, low);
    return r;
}

// acc followed by the L >= 1 samples at the low bits of a wave's masks: foldRec(acc, recOf(k, 0, L)), with the fold by a predicate that no
// sample of them has written out, for that is most steps of most material.  B = nothing of L samples adds nothing to count and runs, leaves
// the head (A.head == A.len gives A.len + 0), ends the tail, and of the three candidates for the longest run the joined one is A's own tail
// -- no longer than A's longest and, where as long, no earlier: `at` is the least position -- and B's is empty.  (acc is built here from
// nothing, so its `at` is the least position; the carry's open column, which is the caller's, goes through foldRec in emitColumn)
__device__ __forceinline__ void takeStep(Rec &acc, const Masks &k, uint32_t L)
{
    const uint64_t low = L >= 64u ? ~uint64_t(0) : (uint64_t(1) << L) - 1u;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const uint64_t seg = k.is[q] & low;
        if (seg == 0) acc.of[q].tail = 0;
        else acc.of[q] = foldOf(acc.of[q], acc.len, ofMask(seg, k.starts[q] & low, L, low), L);
    }
    acc.len += L;
    acc.skipped += uint32_t(__popcll(k.nan & low));
    acc.crossings += uint32_t(__popcll(k.cross & low));
}

// what a (column, channel) does with its record: behind the carry's open column (column 0), then to the output (a closed column) or to the
// carry's open column
__device__ __forceinline__ void emitColumn(const RunParams &prm, long col, uint32_t ch, Rec k)
{
    if (col == 0 && prm.held) k = foldRec(fromRecord(prm.carryIn[ch].open), k);
    storeRec(k, col < prm.closed ? prm.runs + size_t(col) * prm.channels + ch : &prm.carryOut[ch].open);
}

// the carry of a call with samples but for an open column's record: lane 0 and 1 write the new history -- the last two of (the old history,
// the call's samples) --, lane 2 the reserved words, lane 3 an all-zero open column where none stays open
__device__ __forceinline__ void writeCarry(const RunParams &prm, uint32_t ch, uint32_t t)
{
    if (t < 2u) prm.carryOut[ch].prev[t] = sampleAt(prm, ch, prm.n - 1 - long(t));
    if (t == 2u) prm.carryOut[ch].reserved[0] = prm.carryOut[ch].reserved[1] = 0u;
    if (t == 3u && prm.closed == prm.columns) storeRec(nothing(), &prm.carryOut[ch].open);
}

// the tile through LDS, then a wave per group of short columns or per column
__global__ void __launch_bounds__(kRnThreads)
runTileKernel(const RunParams prm)
{
    __shared__ __attribute__((aligned(16))) int32_t row[kRnRowWords];
    const uint32_t tid = threadIdx.x, ch = blockIdx.y, wave = tid >> 6, lane = tid & 63u;
    TileBounds t;
    tileBounds(prm, t);
    const long c0 = t.c0, c1 = t.c1, a = t.a, b = t.b;
    const float *g = prm.planar + size_t(ch) * prm.stride + size_t(a);
    const uint32_t first = kRnBase + (uint32_t(reinterpret_cast<uintptr_t>(g) >> 2) & 3u);     // where sample a lies in the row
    stageRow<false, kRnThreads, kRnUnroll>(g, uint32_t(b - a), first, row);                     // (b - a <= perTile * m <= kRnTile)
    if (tid < 2u) row[first - 1u - tid] = sampleAt(prm, ch, a - 1 - long(tid));                 // the halo: samples a - 1 and a - 2
    if (c1 == prm.columns) writeCarry(prm, ch, tid);                                            // (the last tile's workgroup; carryOut is not carryIn)
    __syncthreads();
    const uint32_t cols = uint32_t(c1 - c0);
    // (the loops below make the same trips in every lane of a wave: the ballots see whole waves)
    if (prm.m <= kRnPacked) {
        const uint32_t G = 64u / prm.m;                                     // columns that share a wave's 64 samples
        for (uint32_t lc0 = wave * G; lc0 < cols; lc0 += kRnWaves * G) {
            long ga, gb;
            columnSamples(prm, c0 + long(lc0), ga, gb);
            const long i = ga + long(lane);
            const bool has = i < b;
            const int32_t *at = row + first + uint32_t(ga - a) + lane;
            const Masks k = masksOf(prm, has ? at[0] : kRnNaN, has ? at[-1] : kRnNaN, has ? at[-2] : kRnNaN, has);
            const uint32_t lc = lc0 + lane;
            if (lane < G && lc < cols) {
                long ca, cb;
                columnSamples(prm, c0 + long(lc), ca, cb);
                emitColumn(prm, c0 + long(lc), ch, recOf(k, uint32_t(ca - ga), uint32_t(cb - ca)));       // (cb - ga <= G m <= 64)
            }
        }
    } else {
        for (uint32_t lc = wave; lc < cols; lc += kRnWaves) {
            long ca, cb;
            columnSamples(prm, c0 + long(lc), ca, cb);
            Rec acc = nothing();
            for (long p = ca; p < cb; p += 64) {
                const uint32_t L = uint32_t(cb - p < 64 ? cb - p : 64);
                const bool has = lane < L;
                const int32_t *at = row + first + uint32_t(p - a) + lane;
                const Masks k = masksOf(prm, has ? at[0] : kRnNaN, has ? at[-1] : kRnNaN, has ? at[-2] : kRnNaN, has);
                takeStep(acc, k, L);
            }
            if (lane == 0) emitColumn(prm, c0 + long(lc), ch, acc);
        }
    }
}

// slice blockIdx.z of column blockIdx.x's samples of channel blockIdx.y (an empty slice -- more slices than samples -- leaves the zero record)
__global__ void __launch_bounds__(kRnThreads)
runSliceKernel(const RunParams prm)
{
    __shared__ __attribute__((aligned(16))) sgz_run_record waves[kRnWaves];
    const long col = long(blockIdx.x);
    const uint32_t ch = blockIdx.y, s = blockIdx.z, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    long a, b, sa, sb;
    columnSamples(prm, col, a, b);
    sliceSamples(prm, a, b, s, sa, sb);
    // quarter `wave` of the slice, a multiple of 64 samples but for the last
    const long per = (((sb - sa) + kRnWaves - 1) / kRnWaves + 63) & ~long(63);
    const long wa = sa + long(wave) * per < sb ? sa + long(wave) * per : sb, wb = wa + per < sb ? wa + per : sb;
    const float *g = prm.planar + size_t(ch) * prm.stride;
    Rec acc = nothing();
    if (wa < wb) {                                                          // (wa, wb: the wave's)
        int32_t p1 = sampleAt(prm, ch, wa - 1), p2 = sampleAt(prm, ch, wa - 2);                // the two samples before the step's first
        for (long p = wa; p < wb; p += 64 * kRnScan) {
            uint32_t x[kRnScan];
#pragma unroll
            for (int j = 0; j < kRnScan; ++j) {
                const long i = p + 64 * j + long(lane);
                x[j] = i < wb ? __float_as_uint(g[i]) : 0u;
            }
#pragma unroll
            for (int j = 0; j < kRnScan; ++j) {
                const long q = p + 64 * j;
                if (q < wb) {                                               // (the same in every lane of the wave)
                    const uint32_t L = uint32_t(wb - q < 64 ? wb - q : 64);
                    const bool has = lane < L;
                    const int32_t v0 = has ? quantiseMarked(x[j]) : kRnNaN;
                    const int32_t u1 = __shfl_up(v0, 1), u2 = __shfl_up(v0, 2);
                    const int32_t v1 = lane >= 1u ? u1 : p1, v2 = lane >= 2u ? u2 : lane == 1u ? p1 : p2;
                    const Masks k = masksOf(prm, v0, v1, v2, has);
                    takeStep(acc, k, L);
                    p1 = __shfl(v0, 63);                                    // (a step of fewer than 64 samples is the wave's last)
                    p2 = __shfl(v0, 62);
                }
            }
        }
    }
    if (lane == 0) storeRec(acc, &waves[wave]);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kRnWaves; ++w) acc = foldRec(acc, fromRecord(waves[w]));          // (acc: wave 0's; then 1, 2, 3, in order)
        storeRec(acc, prm.partial + (size_t(s) * size_t(prm.columns) + size_t(col)) * prm.channels + ch);
    }
}

// one thread per (column, channel): the carry (column 0), then the slices in order (none: a flush of the carry alone), the store; the last
// column's thread of a call with samples writes the rest of the carry
__global__ void __launch_bounds__(kRnThreads)
runEmitKernel(const RunParams prm)
{
    const size_t at = size_t(blockIdx.x) * kRnThreads + threadIdx.x, perSlice = size_t(prm.columns) * prm.channels;
    if (at >= perSlice) return;
    const long col = long(at / prm.channels);
    const uint32_t ch = uint32_t(at % prm.channels);
    Rec k = nothing();
    for (uint32_t s = 0; s < prm.slices; ++s) k = foldRec(k, fromRecord(prm.partial[size_t(s) * perSlice + at]));
    emitColumn(prm, col, ch, k);
    if (prm.n > 0 && col == prm.columns - 1)
        for (uint32_t t = 0; t < 4u; ++t) writeCarry(prm, ch, t);
}

bool paramsOk(const sgz_run_params &p) { return p.hot >= 1u && p.hot <= kRnMaxHot && p.quiet < p.hot; }

sgz_status checkParams(const sgz_run_params *p, const char *who)
{
    if (!p) return fail(SGZ_EINVAL, std::string(who) + ": null params");
    if (!paramsOk(*p)) return fail(SGZ_EINVAL, std::string(who) + ": 1 <= hot <= 2^26 and quiet < hot");
    return SGZ_OK;
}

}  // namespace

namespace sgz {

sgz_status runParamsCheck(const sgz_run_params *p, const char *who) { return checkParams(p, who); }

ColumnsShape runColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices)
{
    return columnsShape(channels, nsamples, m, held, flush, slices, kRnSwitch, sizeof(sgz_run_record), 0);
}

sgz_status runRunColumns(const ColumnsShape &sh, const sgz_run_params &p, const float *d_planar, size_t channelStride, uint32_t channels,
                         size_t nsamples, uint32_t m, uint32_t held, uint32_t continued, const sgz_run_carry *carryIn, sgz_run_carry *carryOut,
                         sgz_run_record *d_runs, void *scratch, hipStream_t stream)
{
    if (!sh.launch) return SGZ_OK;
    RunParams prm{};
    fillGrid(prm, sh, d_planar, channelStride, nsamples, m, held);
    prm.channels = channels; prm.continued = continued;
    prm.hot = p.hot; prm.quiet = p.quiet;
    prm.carryIn = carryIn; prm.carryOut = carryOut;
    prm.runs = d_runs; prm.partial = static_cast<sgz_run_record *>(scratch);
    return launchPlainLane(runTileKernel, runSliceKernel, runEmitKernel, kRnThreads, "run", prm, sh, channels, nsamples, 1,
                           [m](RunParams &t) { t.perTile = kRnTile / m; }, stream);
}

}  // namespace sgz

extern "C" {

void sgz_run_columns_limits(uint32_t *switch_over, uint32_t *tile_samples)
{
    if (switch_over) *switch_over = kRnSwitch;
    if (tile_samples) *tile_samples = kRnTile;
}

void sgz_run_params_default(sgz_run_params *params)
{
    if (!params) return;
    params->hot = (1u << 23) - (1u << 8);                                   // the positive full scale of 16-bit PCM
    params->quiet = 0;
}

sgz_status sgz_stage_run_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, const sgz_run_params *params,
                                 uint32_t m, uint32_t held, int flush, uint32_t continued, uint32_t slices, sgz_run_carry *d_carry,
                                 sgz_run_record *d_runs, void *stream)
{
    const StageFront front{"sgz_stage_run_columns", "channels", kRnMaxChannels, "d_runs", 16, true, 62};
    const sgz_status filter = d_planar ? checkParams(params, "sgz_stage_run_columns") : SGZ_OK;
    return stageColumns(front, filter, d_planar, channel_stride, channels, nsamples, m, held, flush, continued, 0, slices, d_carry, d_runs, stream, runColumnsShape,
                        size_t(channels) * sizeof(sgz_run_carry), noStep, [&](const ColumnsShape &sh, const void *carryIn, void *scratch, hipStream_t s) {
                            return runRunColumns(sh, *params, d_planar, channel_stride, channels, nsamples, m, held, continued, static_cast<const sgz_run_carry *>(carryIn), d_carry,
                                                 d_runs, scratch, s);
                        });
}

sgz_status sgz_run_fold(const sgz_run_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns, sgz_run_record *out)
{
    return foldColumns(
        "sgz_run_fold", "channels", " samples", in, n, channels, x0, x1, out_columns, out,
        [](const sgz_run_record *v, size_t count, size_t stride) {
            uint64_t len = 0;                                              // (len bounds every other field)
            for (size_t j = 0; j < count; ++j) len += v[j * stride].len;
            return len <= 0xffffffffull;
        },
        [](const sgz_run_record *v, size_t count, size_t stride) {         // the source columns in their order: the fold is not commutative
            Rec r = fromRecord(sgz_run_record{});
            for (size_t j = 0; j < count; ++j) r = foldRec(r, fromRecord(v[j * stride]));
            return toRecord(r);
        });
}

sgz_status sgz_run_readout(const sgz_run_record *rec, double rate, sgz_run_reading *out)
{
    if (!rec || !out) return fail(SGZ_EINVAL, "sgz_run_readout: null argument");
    if (!(rate > 0.0) || !std::isfinite(rate)) return fail(SGZ_EINVAL, "sgz_run_readout: rate > 0");
    const double nan = std::numeric_limits<double>::quiet_NaN(), len = double(rec->len);
    for (int k = 0; k < 3; ++k) {
        out->share[k] = rec->len ? double(rec->of[k].count) / len : nan;
        out->longest_seconds[k] = double(rec->of[k].longest) / rate;
        out->at_seconds[k] = double(rec->of[k].at) / rate;
    }
    out->crossing_hz = rec->len ? double(rec->crossings) * rate / (2.0 * len) : nan;
    return SGZ_OK;
}

}  // extern "C"
