// truepeak_columns.hip -- the true-peak lane's reduction: one sgz_truepeak_record (the peak of the 4x oversampled signal, the count, the overs)
// per column of m samples and channel of a linear planar stream, with a carried open column and a carried filter history (sgz.h, "The
// true-peak lane"); and the lane's host helpers, the tap table, the fold of kept records and the readout of one.  gfx950 only.  The reference
// has no counterpart: its meters are live one-pole filters.
// What the column lanes share -- the shape of a call, the bounds, the quantiser, the aligned split, the stage call's front with the carry's
// snapshot, the fold's frame -- is column_lanes.hpp; this file is the filter and the halo it needs.
//   v = the quantiser's (quantiseMarked), a NaN is v = 0 and is not counted;  y[i][q] = sum_j c[q][j] v[i - j], 12 taps per phase,
//   4 phases, integer taps at 2^20: every y is an exact integer below 2^47, the record a maximum and two integer sums, so any cut of the
//   stream (calls with a carry) or of a column (lanes, slices) gives the same bits.
// The multiply-adds come in two forms with the same bits, chosen at build time by SGZ_TP_FP64: 32 x 32 -> 64-bit integer multiply-adds
// (v_mad_i64_i32) and FMAs on integer-valued doubles, exact below 2^53 -- every operand is an integer, so fp contraction cannot change a bit
// either way.  Which one is built and what both cost: DESIGN.md section 8, row b8.
// Sample k < 0 of a call is word 11 + k of the carried history (zeros when the stream begins here).
//   m <= kTpSwitch (1024)   truePeakTileKernel: one workgroup per (channel, tile); a tile is kTpTile / m whole columns of the call (column 0
//                           counts as one, whatever is left of it).  The tile goes to LDS once, quantised on the way (16-byte loads between
//                           the row's first and last 16-byte boundary, scalar loads on either side, the base only 4-byte aligned), behind an
//                           11-word halo: the call's samples before the tile, the history before those.  Groups of G lanes (a power of two
//                           near m / 16) take a column each; a lane takes a RUN of at most 16 consecutive samples and slides a 12-sample
//                           register window along it (R + 11 LDS reads for R samples).  LDS carries one word of padding behind every 16,
//                           so that runs 16 words apart begin on different banks.  log2 G cross-lane steps (max, add, add), the group's
//                           first lane folds the carry (column 0) and stores the record -- or the carry's open column.  The workgroup of
//                           the last tile writes the history.
//   else, or slices >= 2    truePeakSliceKernel: workgroup (column, channel, slice) takes its part of the column through LDS in chunks of
//                           kTpTile samples, each behind its own halo, a run of 16 per lane -> partial records [slices][columns][channels]
//                           in scratch; truePeakEmitKernel, a launch of its own behind it, folds the slices and the carry, stores, and
//                           writes the history (no hand-off between workgroups inside a launch).  A flush without samples is the emit
//                           kernel alone, on the carry.
// Every sample is read from memory once, but for the halos.  Nothing is waited for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "column_lanes.hpp"

using namespace sgz;

namespace {

// ---- the filter (sgz.h: the table is normative) --------------------------------------------------------------------------------------------
// c[q][j] = rint(2^20 L(j - 6 + q / 4)), L(t) = sinc(t) sinc(t / 6) for |t| < 6; phase 0 is the delayed sample itself, phase 3 is phase 1
// reversed, phase 2 is symmetric.  Literals: nothing is computed at start-up.
#define SGZ_TP_PHASE1 -1780, 12162, -29613, 59093, -116769, 306657, 941356, -175616, 82260, -42310, 19798, -6258
#define SGZ_TP_PHASE2 -5454, 22259, -50264, 98518, -200334, 659945, 659945, -200334, 98518, -50264, 22259, -5454
#define SGZ_TP_PHASE3 -6258, 19798, -42310, 82260, -175616, 941356, 306657, -116769, 59093, -29613, 12162, -1780
constexpr int kTpTaps = 12, kTpPhases = 4, kTpHist = kTpTaps - 1;
constexpr int32_t kTpTable[kTpPhases][kTpTaps] = {{0, 0, 0, 0, 0, 0, 1 << 20, 0, 0, 0, 0, 0}, {SGZ_TP_PHASE1}, {SGZ_TP_PHASE2}, {SGZ_TP_PHASE3}};
constexpr int32_t kTpClamp = 1 << 26;           // the quantiser's range
constexpr uint64_t kTpFull = uint64_t(1) << 43; // |y| of full scale: 2^23 of the quantiser times 2^20 of the taps
constexpr uint64_t absSum(int q)
{
    uint64_t s = 0;
    for (int j = 0; j < kTpTaps; ++j) s += uint64_t(kTpTable[q][j] < 0 ? -kTpTable[q][j] : kTpTable[q][j]);
    return s;
}
constexpr bool mirrored()
{
    for (int j = 0; j < kTpTaps; ++j)
        if (kTpTable[3][j] != kTpTable[1][kTpTaps - 1 - j] || kTpTable[2][j] != kTpTable[2][kTpTaps - 1 - j]) return false;
    return true;
}
// The 64-bit accumulators: |y| <= 2^26 sum |c|, and the greatest sum |c| is phase 2's.  Every partial sum of a phase is bounded likewise.
static_assert(absSum(0) == 1048576 && absSum(1) == 1793672 && absSum(2) == 2073548 && absSum(3) == 1793672, "the sums of |c| per phase (sgz.h)");
static_assert(uint64_t(kTpClamp) * absSum(2) < (uint64_t(1) << 47), "|y| < 2^47: exact in int64, and in fp64 (below 2^53)");
static_assert(mirrored(), "phase 3 is phase 1 reversed and phase 2 is symmetric: the kernels fold phase 2's taps in pairs");
// phase 2 adds the two samples of a tap pair first, in 32 bits: 2 * 2^26 < 2^31
static_assert(2 * int64_t(kTpClamp) < (int64_t(1) << 31), "the sum of two quantised samples fits 32 bits");
static_assert(sizeof(sgz_truepeak_record) == 16 && sizeof(sgz_truepeak_carry) == 64, "sgz.h documents 16 and 64 bytes");
static_assert(sizeof(((sgz_truepeak_carry *)nullptr)->hist) == kTpHist * sizeof(int32_t), "the history is the filter's 11 earlier samples");

constexpr int kTpThreads = 256;
constexpr uint32_t kTpTile = 4096;              // samples of a tile
constexpr uint32_t kTpSwitch = 1024;            // the switch-over: columns longer than this take the sliced form
constexpr uint32_t kTpMaxChannels = 64;
constexpr uint32_t kTpRun = 16;                 // the most samples a lane walks in one run
constexpr int kTpUnroll = 4;                    // 16-byte loads a lane issues before the first store to LDS
constexpr uint32_t kTpBase = 12;                // where the tile's 16-byte grid begins in LDS: room for the halo in front, a multiple of 4
constexpr int32_t kTpNaN = kQuantNaN;           // a NaN in LDS
// where sample word i lies in LDS: one word of padding behind every 16, so that runs 16 words apart start on different banks
__host__ __device__ constexpr uint32_t padWord(uint32_t i) { return i + (i >> 4); }
constexpr uint32_t kTpTileWords = padWord(kTpBase + 3 + kTpTile) + 1;      // the halo, the lead (the base's offset within 16 bytes), the tile
static_assert(kTpTile == 4u * kTpThreads * kTpUnroll, "a lane moves kTpUnroll 16-byte chunks of a tile");
static_assert(kTpTile == kTpThreads * kTpRun, "the sliced form: a run per lane and chunk");
static_assert(kTpSwitch <= kTpTile, "a short column fits a tile");
static_assert(kTpBase % 4 == 0 && kTpBase >= uint32_t(kTpHist), "the halo lies in front of the tile's first word");

struct TruePeakParams {
    const float *planar;                 // [channels][stride]
    size_t stride;
    long n;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t m, held, channels;
    uint32_t continued;                  // the history in carryIn holds the samples before this call (else zeros)
    uint32_t perTile;                    // columns of a tile = kTpTile / m
    uint32_t group, run;                 // lanes per column in the tile form, and the samples of a lane's run = ceil(m / group) <= kTpRun
    uint32_t slices;
    const sgz_truepeak_carry *carryIn;   // [channels]: the history (continued) and column 0's `held` earlier samples (held > 0)
    sgz_truepeak_carry *carryOut;        // [channels]: written whole by every call with samples
    sgz_truepeak_record *peaks;          // [closed][channels]
    sgz_truepeak_record *partial;        // [slices][columns][channels]
};

__device__ __forceinline__ int32_t silenceForNaN(int32_t v) { return v == kTpNaN ? 0 : v; }

// what the filter sees at sample k of the call, k >= -11: the call's own sample, or the carried history in front of it
__device__ __forceinline__ int32_t filterInput(const TruePeakParams &prm, uint32_t ch, long k)
{
    if (k >= 0) return silenceForNaN(quantiseMarked(__float_as_uint(prm.planar[size_t(ch) * prm.stride + size_t(k)])));
    return prm.continued ? prm.carryIn[ch].hist[kTpHist + k] : 0;
}

// a column's, a lane's or a slice's part of a record
struct Acc {
    uint64_t peak;
    uint32_t count, overs;
    __device__ __forceinline__ void add(const Acc &o)
    {
        peak = o.peak > peak ? o.peak : peak;
        count += o.count;
        overs += o.overs;
    }
    __device__ __forceinline__ void add(const sgz_truepeak_record &r) { add(Acc{r.peak, r.count, r.overs}); }
    __device__ __forceinline__ void foldLane(int o)
    {
        add(Acc{__shfl_xor((unsigned long long)peak, o), __shfl_xor(count, o), __shfl_xor(overs, o)});
    }
    __device__ __forceinline__ void store(sgz_truepeak_record *to) const
    {
        sgz_truepeak_record r;
        r.peak = peak; r.count = count; r.overs = overs;
        *to = r;
    }
};
__device__ __forceinline__ Acc nothing() { return Acc{0, 0, 0}; }

// One sample's four phases from its window w[t] = v[i - 11 + t], t = 0 .. 11: phase 0 is the sample six back, phase 2 folds its symmetric
// taps in pairs, phase 3 is phase 1's taps on the reversed window.  Two forms of the same integers (SGZ_TP_FP64, below):
//   Int64Form   32 x 32 -> 64-bit multiply-adds; `peak` is the greatest |y| so far
//   Fp64Form    FMAs on integer-valued doubles: every operand and every partial sum is an integer below 2^53 in magnitude, so each FMA is
//               exact and contraction or its absence cannot change a bit; `peak` is a double that holds an integer
struct Int64Form {
    typedef int32_t Word;
    typedef uint64_t Peak;
    static __device__ __forceinline__ Word word(int32_t v) { return v; }
    static __device__ __forceinline__ uint64_t integer(Peak p) { return p; }
    static __device__ __forceinline__ Peak sample(const Word *w)
    {
        constexpr int32_t c1[kTpTaps] = {SGZ_TP_PHASE1}, c2[kTpTaps] = {SGZ_TP_PHASE2};
        int64_t y1 = 0, y2 = 0, y3 = 0;
#pragma unroll
        for (int j = 0; j < kTpTaps; ++j) {                               // y[q] = sum_j c[q][j] v[i - j], v[i - j] = w[11 - j]
            y1 += int64_t(c1[j]) * int64_t(w[kTpHist - j]);
            y3 += int64_t(c1[kTpHist - j]) * int64_t(w[kTpHist - j]);
        }
#pragma unroll
        for (int j = 0; j < kTpTaps / 2; ++j) y2 += int64_t(c2[j]) * int64_t(w[kTpHist - j] + w[j]);
        const uint64_t a0 = uint64_t(uint32_t(abs(w[5]))) << 20;          // c[0][6] v[i - 6]
        const uint64_t a1 = uint64_t(y1 < 0 ? -y1 : y1), a2 = uint64_t(y2 < 0 ? -y2 : y2), a3 = uint64_t(y3 < 0 ? -y3 : y3);
        const uint64_t p01 = a0 > a1 ? a0 : a1, p23 = a2 > a3 ? a2 : a3;
        return p01 > p23 ? p01 : p23;
    }
    static __device__ __forceinline__ bool over(Peak p) { return p >= kTpFull; }
    static __device__ __forceinline__ Peak greater(Peak a, Peak b) { return a > b ? a : b; }
};
struct Fp64Form {
    typedef double Word;
    typedef double Peak;
    static __device__ __forceinline__ Word word(int32_t v) { return double(v); }
    static __device__ __forceinline__ uint64_t integer(Peak p) { return uint64_t(p); }      // (exact: an integer below 2^47)
    static __device__ __forceinline__ Peak sample(const Word *w)
    {
        constexpr int32_t c1[kTpTaps] = {SGZ_TP_PHASE1}, c2[kTpTaps] = {SGZ_TP_PHASE2};
        double y1 = 0.0, y2 = 0.0, y3 = 0.0;
#pragma unroll
        for (int j = 0; j < kTpTaps; ++j) {
            y1 = __builtin_fma(double(c1[j]), w[kTpHist - j], y1);
            y3 = __builtin_fma(double(c1[kTpHist - j]), w[kTpHist - j], y3);
        }
#pragma unroll
        for (int j = 0; j < kTpTaps / 2; ++j) y2 = __builtin_fma(double(c2[j]), w[kTpHist - j] + w[j], y2);
        const double a0 = __builtin_fabs(w[5]) * 0x1p20;
        return __builtin_fmax(__builtin_fmax(a0, __builtin_fabs(y1)), __builtin_fmax(__builtin_fabs(y2), __builtin_fabs(y3)));
    }
    static __device__ __forceinline__ bool over(Peak p) { return p >= 0x1p43; }
    static __device__ __forceinline__ Peak greater(Peak a, Peak b) { return __builtin_fmax(a, b); }
};
#ifndef SGZ_TP_FP64
#define SGZ_TP_FP64 1                   // chosen by measurement: the fp64 form is 13-18 % faster cold; both forms give the definition's bits
#endif
#if SGZ_TP_FP64
typedef Fp64Form Form;
#else
typedef Int64Form Form;
#endif

// LDS sample words [from, to) of a tile (at least 11 words lie in front of `from`): the 12-sample window slides along the run in registers,
// four samples a step -- their LDS reads go out together, and the window moves once per step -- and one sample a step for the rest.
__device__ __forceinline__ void walkRun(const int32_t *tile, uint32_t from, uint32_t to, Acc &k)
{
    constexpr int kStep = 4;
    if (from >= to) return;
    Form::Word w[kTpHist + kStep];                                        // w[t] = v[i - 11 + t]
    Form::Peak peak = Form::Peak(0);
#pragma unroll
    for (int t = 0; t < kTpHist; ++t) w[t] = Form::word(silenceForNaN(tile[padWord(from - uint32_t(kTpHist) + uint32_t(t))]));
    uint32_t i = from;
    for (; i + kStep <= to; i += kStep) {
        int32_t x[kStep];
#pragma unroll
        for (int s = 0; s < kStep; ++s) x[s] = tile[padWord(i + uint32_t(s))];
#pragma unroll
        for (int s = 0; s < kStep; ++s) w[kTpHist + s] = Form::word(silenceForNaN(x[s]));
#pragma unroll
        for (int s = 0; s < kStep; ++s) {
            const Form::Peak p = Form::sample(w + s);
            peak = Form::greater(peak, p);
            k.count += uint32_t(x[s] != kTpNaN);
            k.overs += uint32_t(Form::over(p));
        }
#pragma unroll
        for (int t = 0; t < kTpHist; ++t) w[t] = w[t + kStep];
    }
    for (; i < to; ++i) {
        const int32_t x = tile[padWord(i)];
        w[kTpHist] = Form::word(silenceForNaN(x));
        const Form::Peak p = Form::sample(w);
        peak = Form::greater(peak, p);
        k.count += uint32_t(x != kTpNaN);
        k.overs += uint32_t(Form::over(p));
#pragma unroll
        for (int t = 0; t < kTpHist; ++t) w[t] = w[t + 1];
    }
    const uint64_t run = Form::integer(peak);
    k.peak = run > k.peak ? run : k.peak;
}

// what a (column, channel) does with its record: the carry into column 0, then to the output (a closed column) or to the carry's open column
__device__ __forceinline__ void emitColumn(const TruePeakParams &prm, long col, uint32_t ch, Acc k)
{
    if (col == 0 && prm.held) k.add(prm.carryIn[ch].open);
    k.store(col < prm.closed ? prm.peaks + size_t(col) * prm.channels + ch : &prm.carryOut[ch].open);
}

// the carry of a call with samples but for an open column's record: lane t < 11 writes word t of the new history -- the last 11 of (the old
// history, the call's samples) --, lane 11 the reserved word, lane 12 an all-zero open column where none stays open
__device__ __forceinline__ void writeCarry(const TruePeakParams &prm, uint32_t ch, uint32_t t)
{
    if (t < uint32_t(kTpHist)) prm.carryOut[ch].hist[t] = filterInput(prm, ch, prm.n - long(kTpHist) + long(t));
    if (t == uint32_t(kTpHist)) prm.carryOut[ch].reserved = 0;
    if (t == uint32_t(kTpHist) + 1 && prm.closed == prm.columns) nothing().store(&prm.carryOut[ch].open);
}

// samples [a, a + count) of channel ch (count <= kTpTile), quantised, into the tile behind their 11-word halo; returns where sample a lies
// (LDS sample word kTpBase + lead: the tile keeps the row's offset within 16 bytes, so a 16-byte chunk of memory is four words of one
// 16-word block of LDS).  The caller puts a barrier behind it.
__device__ __forceinline__ uint32_t stageTile(const TruePeakParams &prm, uint32_t ch, long a, uint32_t count, int32_t *tile)
{
    const uint32_t tid = threadIdx.x;
    const float *g = prm.planar + size_t(ch) * prm.stride + size_t(a);
    const uint32_t lead = uint32_t(reinterpret_cast<uintptr_t>(g) >> 2) & 3u, first = kTpBase + lead;
    uint32_t head, vecs, tail;
    splitAligned(g, count, head, vecs, tail);
    if (tid < uint32_t(kTpHist)) tile[padWord(first - uint32_t(kTpHist) + tid)] = filterInput(prm, ch, a - long(kTpHist) + long(tid));
    if (tid < head) tile[padWord(first + tid)] = quantiseMarked(__float_as_uint(g[tid]));
    if (tid < count - tail) tile[padWord(first + tail + tid)] = quantiseMarked(__float_as_uint(g[tail + tid]));
    const uint4 *gv = reinterpret_cast<const uint4 *>(g + head);
    uint4 v[kTpUnroll];
#pragma unroll
    for (int j = 0; j < kTpUnroll; ++j)
        v[j] = tid + uint32_t(j) * kTpThreads < vecs ? gv[tid + uint32_t(j) * kTpThreads] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int j = 0; j < kTpUnroll; ++j)                                     // (first + head is a multiple of 4 wherever vecs > 0: the four words share a block)
        if (tid + uint32_t(j) * kTpThreads < vecs) {
            int32_t *to = tile + padWord(first + head + 4u * (tid + uint32_t(j) * kTpThreads));
            to[0] = quantiseMarked(v[j].x); to[1] = quantiseMarked(v[j].y); to[2] = quantiseMarked(v[j].z); to[3] = quantiseMarked(v[j].w);
        }
    return first;
}

// the tile through LDS, then groups of prm.group lanes per column, a run of prm.run samples per lane
__global__ void __launch_bounds__(kTpThreads)
truePeakTileKernel(const TruePeakParams prm)
{
    __shared__ int32_t tile[kTpTileWords];
    const uint32_t tid = threadIdx.x, ch = blockIdx.y;
    TileBounds t;
    tileBounds(prm, t);
    const long c0 = t.c0, c1 = t.c1, a = t.a, b = t.b;
    const uint32_t first = stageTile(prm, ch, a, uint32_t(b - a), tile);   // (b - a <= perTile * m <= kTpTile)
    if (c1 == prm.columns) writeCarry(prm, ch, tid);                        // (the last tile's workgroup; carryOut is not carryIn)
    __syncthreads();
    const uint32_t G = prm.group, sub = tid & (G - 1u), grp = tid / G, groups = uint32_t(kTpThreads) / G;
    const uint32_t cols = uint32_t(c1 - c0);
    for (uint32_t base = 0; base < cols; base += groups) {                  // (the same trips in every lane: the cross-lane steps see whole waves)
        const uint32_t lc = base + grp;
        const bool mine = lc < cols;
        Acc k = nothing();
        if (mine) {
            long ca, cb;
            columnSamples(prm, c0 + long(lc), ca, cb);
            const uint32_t from = first + uint32_t(ca - a), end = first + uint32_t(cb - a);
            const uint32_t ra = from + sub * prm.run, rb = ra + prm.run;
            walkRun(tile, ra, rb < end ? rb : end, k);
        }
        for (uint32_t o = G >> 1; o > 0; o >>= 1) k.foldLane(int(o));
        if (mine && sub == 0) emitColumn(prm, c0 + long(lc), ch, k);
    }
}

// slice blockIdx.z of column blockIdx.x's samples of channel blockIdx.y (an empty slice -- more slices than samples -- leaves the zero record)
__global__ void __launch_bounds__(kTpThreads)
truePeakSliceKernel(const TruePeakParams prm)
{
    __shared__ int32_t tile[kTpTileWords];
    __shared__ sgz_truepeak_record waves[kTpThreads / 64];
    const long col = long(blockIdx.x);
    const uint32_t ch = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
    long a, b, sa, sb;
    columnSamples(prm, col, a, b);
    sliceSamples(prm, a, b, s, sa, sb);
    Acc k = nothing();
    for (long at = sa; at < sb; at += long(kTpTile)) {                      // (the same trips in every lane: the barriers see the whole workgroup)
        const uint32_t count = uint32_t(sb - at < long(kTpTile) ? sb - at : long(kTpTile));
        const uint32_t first = stageTile(prm, ch, at, count, tile);
        __syncthreads();
        const uint32_t ra = tid * kTpRun, rb = ra + kTpRun;
        walkRun(tile, first + (ra < count ? ra : count), first + (rb < count ? rb : count), k);
        __syncthreads();                                                    // (the next chunk overwrites the tile)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k.foldLane(o);
    if ((tid & 63u) == 0) k.store(&waves[tid >> 6]);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < kTpThreads / 64; ++v) k.add(waves[v]);
        k.store(prm.partial + (size_t(s) * size_t(prm.columns) + size_t(col)) * prm.channels + ch);
    }
}

// one thread per (column, channel): the fold of the slices (none: a flush of the carry alone), the carry, the store; the last column's thread
// of a call with samples writes the rest of the carry
__global__ void __launch_bounds__(kTpThreads)
truePeakEmitKernel(const TruePeakParams prm)
{
    const size_t at = size_t(blockIdx.x) * kTpThreads + threadIdx.x, perSlice = size_t(prm.columns) * prm.channels;
    if (at >= perSlice) return;
    const long col = long(at / prm.channels);
    const uint32_t ch = uint32_t(at % prm.channels);
    Acc k = nothing();
    for (uint32_t s = 0; s < prm.slices; ++s) k.add(prm.partial[size_t(s) * perSlice + at]);
    emitColumn(prm, col, ch, k);
    if (prm.n > 0 && col == prm.columns - 1)
        for (uint32_t t = 0; t < uint32_t(kTpHist) + 2; ++t) writeCarry(prm, ch, t);
}

}  // namespace

namespace sgz {

ColumnsShape truePeakColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices)
{
    return columnsShape(channels, nsamples, m, held, flush, slices, kTpSwitch, sizeof(sgz_truepeak_record), 0);
}

sgz_status runTruePeakColumns(const ColumnsShape &sh, const float *d_planar, size_t channelStride, uint32_t channels, size_t nsamples,
                              uint32_t m, uint32_t held, uint32_t continued, const sgz_truepeak_carry *carryIn, sgz_truepeak_carry *carryOut,
                              sgz_truepeak_record *d_peaks, void *scratch, hipStream_t stream)
{
    if (!sh.launch) return SGZ_OK;
    TruePeakParams prm{};
    fillGrid(prm, sh, d_planar, channelStride, nsamples, m, held);
    prm.channels = channels; prm.continued = continued;
    prm.carryIn = carryIn; prm.carryOut = carryOut;
    prm.peaks = d_peaks; prm.partial = static_cast<sgz_truepeak_record *>(scratch);
    return launchPlainLane(truePeakTileKernel, truePeakSliceKernel, truePeakEmitKernel, kTpThreads, "true-peak", prm, sh, channels, nsamples, 1, [m](TruePeakParams &p) {
        p.perTile = kTpTile / m;
        p.group = pow2AtLeast((m + kTpRun - 1) / kTpRun);             // (1 .. 64)
        p.run = (m + p.group - 1) / p.group;                          // (<= kTpRun; group * run >= m)
    }, stream);
}

}  // namespace sgz

extern "C" {

void sgz_truepeak_columns_limits(uint32_t *switch_over, uint32_t *tile_samples)
{
    if (switch_over) *switch_over = kTpSwitch;
    if (tile_samples) *tile_samples = kTpTile;
}

void sgz_truepeak_taps(int32_t taps[4][12])
{
    if (taps) std::memcpy(taps, kTpTable, sizeof kTpTable);
}

sgz_status sgz_stage_truepeak_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, uint32_t m, uint32_t held,
                                      int flush, uint32_t continued, uint32_t slices, sgz_truepeak_carry *d_carry, sgz_truepeak_record *d_peaks,
                                      void *stream)
{
    const StageFront front{"sgz_stage_truepeak_columns", "channels", kTpMaxChannels, "d_peaks", 16, true, 62};
    return stageColumns(front, SGZ_OK, d_planar, channel_stride, channels, nsamples, m, held, flush, continued, 0, slices, d_carry, d_peaks, stream, truePeakColumnsShape,
                        size_t(channels) * sizeof(sgz_truepeak_carry), noStep, [&](const ColumnsShape &sh, const void *carryIn, void *scratch, hipStream_t s) {
                            return runTruePeakColumns(sh, d_planar, channel_stride, channels, nsamples, m, held, continued, static_cast<const sgz_truepeak_carry *>(carryIn), d_carry,
                                                      d_peaks, scratch, s);
                        });
}

sgz_status sgz_truepeak_fold(const sgz_truepeak_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns,
                             sgz_truepeak_record *out)
{
    return foldColumns(
        "sgz_truepeak_fold", "channels", "", in, n, channels, x0, x1, out_columns, out,
        [](const sgz_truepeak_record *v, size_t count, size_t stride) {
            uint64_t tally = 0, overs = 0;
            for (size_t j = 0; j < count; ++j) {
                tally += v[j * stride].count;
                overs += v[j * stride].overs;
            }
            return tally <= 0xffffffffull && overs <= 0xffffffffull;
        },
        [](const sgz_truepeak_record *v, size_t count, size_t stride) {
            sgz_truepeak_record r{0, 0, 0};
            for (size_t j = 0; j < count; ++j) {
                r.peak = std::max(r.peak, v[j * stride].peak);
                r.count += v[j * stride].count;
                r.overs += v[j * stride].overs;
            }
            return r;
        });
}

sgz_status sgz_truepeak_readout(const sgz_truepeak_record *rec, double *peak, double *dbtp)
{
    if (!rec) return fail(SGZ_EINVAL, "sgz_truepeak_readout: null argument");
    const double p = double(rec->peak) * 0x1p-43;                  // (exact: a peak is below 2^47)
    if (peak) *peak = p;
    if (dbtp) *dbtp = p == 0.0 ? -std::numeric_limits<double>::infinity() : 20.0 * std::log10(p);
    return SGZ_OK;
}

}  // extern "C"
