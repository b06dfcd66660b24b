// overview_pct.hip -- the percentile overview: the distribution of k frames of line results per image column (sgz.h, "The percentile
// overview").  gfx950 only.  The sixth reduction of the overview render, over the mean overview's input x = L[f][p][0][i].x and its columns:
//   word(x) = 66 for a NaN, else the bucket: 0 for x < 0, 65 for x >= 1, otherwise 1 + floor(64 x) (exact in fp32; -0 in bucket 1);
//   per (column, pair, pixel) the record { bucket[66], nans, reserved = 0 } -- counts, so every word adds and any split of the frames
//   (slices, calls, slabs, feeds) gives the same bytes;  the quantile q of a record is read from the cumulative counts (pctRank / pctValue);
//   the pixel is blendColour / toRgba8 of decay_body.hpp at quantile 0's value (called, not copied).
// A record is 68 words, too many for registers: a lane keeps its table in LDS.  A workgroup is ONE wave of 64 lanes and its table is
// [68 words][64 lanes] with a row stride of 65 words (17 680 bytes: nine workgroups a CU).  A lane owns column `lane` of it, so counting needs
// no atomicity for correctness; the increment is a no-return ds_add_u32, which spares the read-modify-write round trip.  Lane l's word w lies
// in bank (w + l) mod 64: the counting step sees chance conflicts only.  The three shapes of overview_stats.hip, for its reasons:
//   overviewPctColumnsKernel   one lane per (column, pixel): pairs outermost (the blend order), the column's frames inside, 4 row loads in
//                              flight before the bucket arithmetic (8 in the slice kernel); then the carry, the quantiles (one cumulative
//                              walk of the lane's table), the colour, and the wave's 64 records as ONE contiguous run of 64 x 272 bytes:
//                              chunk c of the run, 16 bytes, is words 4 (c mod 17) .. + 3 of record c / 17, read across the table and
//                              stored as a dwordx4.
//   overviewPctSliceKernel     few columns of many frames: slice s of a column's frames -> partial records [slices][columns][pairs][P] in
//   overviewPctEmitKernel      plan scratch; then the fold over the slices and the carry (the run read back as it was written, added into
//                              the table), the quantiles, the colour, the stores -- a launch of its own behind it on the stream.
// A wave's lanes exchange table columns only in the run transfers; a __syncthreads() stands on either side of each (one wave: no s_barrier
// is left of it, the LDS counter wait is).  Nothing is waited for on the host; scratch grows on demand; everything runs on the caller's stream.
// From overview_kinds.hpp: the step of a call, the column and slice bounds, a workgroup's cells, the launch front (with this kind's slice rule,
// pctAutoSlices, and its 64-thread workgroup) and the host fold's frame.  The kernel bodies are this file's own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "runtime.hpp"
#include "decay_body.hpp"

#pragma clang fp contract(off)

#include "overview_kinds.hpp"   // behind the pragma: its templates are parsed without contraction

using namespace sgz;

static_assert(sizeof(sgz_overview_pct_record) == 272 && alignof(sgz_overview_pct_record) == 4, "sgz_overview_pct_record: 272 bytes");
static_assert(offsetof(sgz_overview_pct_record, bucket) == 0 && offsetof(sgz_overview_pct_record, nans) == 264 &&
              offsetof(sgz_overview_pct_record, reserved) == 268, "sgz_overview_pct_record: the layout sgz.h documents");
static_assert(SGZ_OVERVIEW_PCT_BUCKETS == 66 && SGZ_OVERVIEW_PCT_MAX_QUANTILES == 8, "the kernels' table and argument block");

namespace {

using Record = sgz_overview_pct_record;

constexpr int kPctThreads = 64;                          // one wave
constexpr int kPctUnroll = 4;                            // frames whose loads are issued before the first increment, where a column is emitted
constexpr int kPctSliceUnroll = 8;                       // ... and in the slice kernel (in the columns kernel 8 spill twelve scalar registers to lanes)
constexpr int kPctBuckets = SGZ_OVERVIEW_PCT_BUCKETS;
constexpr int kPctNans = kPctBuckets;                    // the table's word 66; word 67 is `reserved` and stays 0
constexpr int kPctWords = sizeof(Record) / 4;            // 68
constexpr int kPctChunks = kPctWords / 4;                // 17 16-byte chunks a record
constexpr int kPctStride = kPctThreads + 1;
constexpr int kMaxQ = SGZ_OVERVIEW_PCT_MAX_QUANTILES;
constexpr size_t kPctPartialBytes = size_t(64) << 20;    // what the automatic choice lets the partial records take (sgz.h)
constexpr uint32_t kPctSliceFrames = 64;                 // the fewest frames of a slice: its partial record, written and read, is 68 row loads

// ---- the definition, for the host and the device -------------------------------------------------------------------------------------------
// the table word of a value's bits: the tests on the bits hold whatever the denormal mode; 64 x is exact, the conversion truncates a value
// in [0, 64) to its floor
__host__ __device__ inline uint32_t pctWord(uint32_t bits)
{
    const uint32_t mag = bits & 0x7fffffffu;
    if (mag > 0x7f800000u) return uint32_t(kPctNans);
    if ((bits >> 31) && mag) return 0u;                  // x < 0; -0 is not
    if (mag >= 0x3f800000u) return uint32_t(kPctBuckets - 1);   // x >= 1, +inf
#ifdef __HIP_DEVICE_COMPILE__
    const float x = __uint_as_float(mag);
#else
    float x;
    std::memcpy(&x, &mag, sizeof x);
#endif
    return 1u + uint32_t(64.f * x);
}

// r: the least integer >= q count, clamped to [1, count]; one fp64 multiply (sgz_hist_percentile's rule).  count >= 1
__host__ __device__ inline uint32_t pctRank(double q, uint32_t count)
{
    const double want = ceil(q * double(count));
    return want < 1.0 ? 1u : want > double(count) ? count : uint32_t(want);
}

// the value of rank r in bucket b, which holds n values behind `before` lower ones
__host__ __device__ inline float pctValue(uint32_t b, uint32_t r, uint32_t before, uint32_t n)
{
    if (b == 0u) return -0.015625f;
    if (b == uint32_t(kPctBuckets - 1)) return 1.0f;
    return float((double(b - 1u) + (double(r - before) - 0.5) / double(n)) * 0.015625);
}

// ---- what every emitting kernel writes -----------------------------------------------------------------------------------------------------
struct PctOut {
    uint32_t C, P, nq;
    uchar4 *rgba;                        // [columns][P] or null
    Record *records;                     // [columns][C][P] or null
    float *values[kMaxQ];                // plane j: [columns][C][P]; all null or the first nq set
    double q[kMaxQ];
    const float *colourTables;
    DeviceScalars sc;
};

struct PctParams {
    const float2 *lines;                 // [frames][C][G][P]
    long frames;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t k, held, blocks, slices;
    const Record *carryIn;               // [C][P]: the record of column 0's `held` earlier frames (read iff held > 0)
    Record *carryOut;                    // [C][P]: the record of the open column
    Record *partial;                     // [slices][columns][C][P]
    PctOut out;
};

// ---- the lane's table ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tabZero(uint32_t *tab, uint32_t lane)
{
#pragma unroll
    for (int w = 0; w < kPctWords; ++w) tab[w * kPctStride + lane] = 0u;
}

__device__ __forceinline__ void tabAdd(uint32_t *tab, uint32_t at, uint32_t v)
{
    (void)__hip_atomic_fetch_add(tab + at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      // result unused: ds_add_u32
}

// frames [a, b) of (pair, pixel) into the lane's table: graph 0's row of every frame, independent loads first (a and b are the wave's)
template <int kUnroll>
__device__ __forceinline__ void tabCount(uint32_t *tab, uint32_t lane, const PctParams &prm, long a, long b, uint32_t pair, uint32_t pixel)
{
    const size_t perFrame = size_t(prm.out.C) * G * prm.out.P;
    const float2 *row = prm.lines + size_t(pair) * G * prm.out.P + pixel;
    const uint32_t n = uint32_t(b > a ? b - a : 0);              // (at most k)
    row += size_t(a) * perFrame;
    for (uint32_t f = 0; f < n; f += kUnroll) {
        uint32_t bits[kUnroll];
#pragma unroll
        for (uint32_t j = 0; j < kUnroll; ++j, row += perFrame) bits[j] = f + j < n ? __float_as_uint(row->x) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < kUnroll; ++j)
            if (f + j < n) tabAdd(tab, pctWord(bits[j]) * kPctStride + lane, 1u);
    }
}

// The wave's records as one run: `run` is lane 0's record, n <= 64 of them exist.  Chunk c, 16 bytes, is words 4 (c mod 17) .. + 3 of
// record c / 17.
__device__ __forceinline__ void tabStoreRun(const uint32_t *tab, uint32_t lane, Record *run, uint32_t n)
{
    uint4 *dst = reinterpret_cast<uint4 *>(run);
    const uint32_t chunks = n * kPctChunks;
#pragma nounroll
    for (uint32_t c = lane; c < chunks; c += kPctThreads) {
        const uint32_t rec = c / kPctChunks, at = 4u * (c % kPctChunks) * kPctStride + rec;
        dst[c] = make_uint4(tab[at], tab[at + kPctStride], tab[at + 2 * kPctStride], tab[at + 3 * kPctStride]);
    }
}

// ... and a run of records added into the table (no two lanes meet in a word)
__device__ __forceinline__ void tabFoldRun(uint32_t *tab, uint32_t lane, const Record *run, uint32_t n)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(run);
    const uint32_t chunks = n * kPctChunks;
#pragma nounroll
    for (uint32_t c = lane; c < chunks; c += kPctThreads) {
        const uint4 v = src[c];
        const uint32_t rec = c / kPctChunks, at = 4u * (c % kPctChunks) * kPctStride + rec;
        tabAdd(tab, at, v.x);
        tabAdd(tab, at + kPctStride, v.y);
        tabAdd(tab, at + 2 * kPctStride, v.z);
        tabAdd(tab, at + 3 * kPctStride, v.w);
    }
}

// The nq quantiles of the lane's table by one cumulative walk; count: the sum of its buckets.  The ranks and what the walk finds are in
// registers, picked by compare chains; the loops over the quantiles are not unrolled and index the launch arguments where they lie, so the
// eight quantiles and the eight plane pointers never stand in scalar registers together.  at: the value's index within its plane.
// Returns quantile 0's value
__device__ __forceinline__ float tabQuantiles(const uint32_t *tab, uint32_t lane, uint32_t count, const PctOut &o, size_t at)
{
    constexpr uint32_t kNone = 0xffffffffu;
    uint32_t r[kMaxQ], b[kMaxQ], before[kMaxQ], n[kMaxQ];
#pragma unroll
    for (int i = 0; i < kMaxQ; ++i) { r[i] = kNone; b[i] = kNone; before[i] = 0u; n[i] = 1u; }
    if (count) {
#pragma nounroll
        for (uint32_t j = 0; j < o.nq; ++j) {
            const uint32_t rank = pctRank(o.q[j], count);
#pragma unroll
            for (int i = 0; i < kMaxQ; ++i) r[i] = uint32_t(i) == j ? rank : r[i];
        }
    }
    uint32_t below = 0;
#pragma unroll 2
    for (int w = 0; w < kPctBuckets; ++w) {
        const uint32_t x = tab[w * kPctStride + lane], upTo = below + x;
#pragma unroll
        for (int i = 0; i < kMaxQ; ++i) {
            const bool hit = b[i] == kNone && upTo >= r[i];      // (a rank that is not asked for, kNone, is above every count)
            b[i] = hit ? uint32_t(w) : b[i];
            before[i] = hit ? below : before[i];
            n[i] = hit ? x : n[i];
        }
        below = upTo;
    }
    float first = 0.f;
#pragma nounroll
    for (uint32_t j = 0; j < o.nq; ++j) {
        uint32_t rj = kNone, bj = kNone, beforej = 0u, nj = 1u;
#pragma unroll
        for (int i = 0; i < kMaxQ; ++i)
            if (uint32_t(i) == j) { rj = r[i]; bj = b[i]; beforej = before[i]; nj = n[i]; }
        const float value = bj == kNone ? __uint_as_float(0x7fc00000u) : pctValue(bj, rj, beforej, nj);
        if (o.values[0]) o.values[j][at] = value;
        first = j == 0u ? value : first;
    }
    return first;
}

// What a wave does with a (column, pair) whose frames are in its table, behind a __syncthreads(): a closed column's values, its part of the
// blend and its records, or the open column's carry.  total: the frames the table holds, the carry's `held` included -- the lane's count is
// what is left of them beside its NaNs.  run: the index of lane 0's record within a [C][P] plane; live: records of the wave that exist
__device__ __forceinline__ void emitPair(const uint32_t *tab, uint32_t lane, const PctParams &prm, long col, uint32_t pair, uint32_t pixel, size_t run,
                                         uint32_t live, uint32_t total, float (&cb)[3])
{
    const PctOut &o = prm.out;
    if (col >= prm.closed) { tabStoreRun(tab, lane, prm.carryOut + run, live); return; }
    const size_t plane = size_t(col) * o.C * o.P;
    if ((o.values[0] || o.rgba) && lane < live) {
        const uint32_t count = total - tab[kPctNans * kPctStride + lane];
        const float first = tabQuantiles(tab, lane, count, o, plane + size_t(pair) * o.P + pixel);
        if (o.rgba) blendColour(cb, first, o.colourTables + size_t(pair) * NC * 3, o.sc);
    }
    if (o.records) tabStoreRun(tab, lane, o.records + plane + run, live);
}

__device__ __forceinline__ void emitPixel(const PctParams &prm, long col, uint32_t pixel, uint32_t lane, uint32_t live, const float (&cb)[3])
{
    if (prm.out.rgba && col < prm.closed && lane < live) prm.out.rgba[size_t(col) * prm.out.P + pixel] = toRgba8(cb);
}

__global__ void __launch_bounds__(kPctThreads)
overviewPctColumnsKernel(const PctParams prm)
{
    __shared__ uint32_t tab[kPctWords * kPctStride];
    long col;
    uint32_t first;
    blockCells<kPctThreads>(prm, col, first);
    const uint32_t lane = threadIdx.x, pixel = first + lane;
    const uint32_t live = min(uint32_t(kPctThreads), prm.out.P - first);
    long a, b;
    columnFrames(prm, col, a, b);
    const bool carried = col == 0 && prm.held;
    const uint32_t total = uint32_t(b > a ? b - a : 0) + (carried ? prm.held : 0u);
    float cb[3] = {0.f, 0.f, 0.f};
    for (uint32_t pair = 0; pair < prm.out.C; ++pair) {
        const size_t run = size_t(pair) * prm.out.P + first;
        tabZero(tab, lane);
        if (lane < live) tabCount<kPctUnroll>(tab, lane, prm, a, b, pair, pixel);
        if (carried) {
            __syncthreads();
            tabFoldRun(tab, lane, prm.carryIn + run, live);
        }
        __syncthreads();
        emitPair(tab, lane, prm, col, pair, pixel, run, live, total, cb);
        __syncthreads();
    }
    emitPixel(prm, col, pixel, lane, live, cb);
}

// slice blockIdx.y of every column's frames (an empty slice -- more slices than frames -- leaves an empty record)
__global__ void __launch_bounds__(kPctThreads)
overviewPctSliceKernel(const PctParams prm)
{
    __shared__ uint32_t tab[kPctWords * kPctStride];
    long col;
    uint32_t first;
    blockCells<kPctThreads>(prm, col, first);
    const uint32_t lane = threadIdx.x, pixel = first + lane;
    const uint32_t live = min(uint32_t(kPctThreads), prm.out.P - first);
    long a, b, sa, sb;
    columnFrames(prm, col, a, b);
    sliceRange(prm, a, b, b > a ? b - a : 0, sa, sb);
    for (uint32_t pair = 0; pair < prm.out.C; ++pair) {
        tabZero(tab, lane);
        if (lane < live) tabCount<kPctSliceUnroll>(tab, lane, prm, sa, sb, pair, pixel);
        __syncthreads();
        tabStoreRun(tab, lane, prm.partial + ((size_t(blockIdx.y) * size_t(prm.columns) + size_t(col)) * prm.out.C + pair) * prm.out.P + first, live);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kPctThreads)
overviewPctEmitKernel(const PctParams prm)
{
    __shared__ uint32_t tab[kPctWords * kPctStride];
    long col;
    uint32_t first;
    blockCells<kPctThreads>(prm, col, first);
    const uint32_t lane = threadIdx.x, pixel = first + lane;
    const uint32_t live = min(uint32_t(kPctThreads), prm.out.P - first);
    const size_t perSlice = size_t(prm.columns) * prm.out.C * prm.out.P;
    long a, b;
    columnFrames(prm, col, a, b);
    const uint32_t total = uint32_t(b > a ? b - a : 0) + (col == 0 ? prm.held : 0u);
    float cb[3] = {0.f, 0.f, 0.f};
    for (uint32_t pair = 0; pair < prm.out.C; ++pair) {
        const size_t run = size_t(pair) * prm.out.P + first;
        tabZero(tab, lane);
        __syncthreads();
        for (uint32_t s = 0; s < prm.slices; ++s) tabFoldRun(tab, lane, prm.partial + size_t(s) * perSlice + size_t(col) * prm.out.C * prm.out.P + run, live);
        if (col == 0 && prm.held) tabFoldRun(tab, lane, prm.carryIn + run, live);
        __syncthreads();
        emitPair(tab, lane, prm, col, pair, pixel, run, live, total, cb);
        __syncthreads();
    }
    emitPixel(prm, col, pixel, lane, live, cb);
}

// The library's choice of form: slices only where the launch would leave CUs idle, no slice shorter than kPctSliceFrames frames, and no
// more partial records than kPctPartialBytes hold
uint32_t pctAutoSlices(const Plan &p, uint64_t columns, uint32_t blocks, uint32_t k, size_t frames)
{
    uint64_t s = overviewAutoSlices(long(columns), blocks, k, frames, 4 * numCUs());      // (its unit is a 256-lane workgroup)
    s = std::min<uint64_t>(s, std::min<uint64_t>(k, frames) / kPctSliceFrames);
    s = std::min<uint64_t>(s, kPctPartialBytes / (columns * p.C * p.P * sizeof(Record)));
    return uint32_t(std::max<uint64_t>(s, 1));
}

}  // namespace

namespace sgz {

bool validPctQuantiles(const double *q, uint32_t nq)
{
    if (!q || nq < 1 || nq > uint32_t(kMaxQ)) return false;
    for (uint32_t j = 0; j < nq; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return false;
    return true;
}

// sgz_stage_overview_pct behind its argument checks (the plan's tables are uploaded).  d_lines [frames][C][G][P] float2; planes: where the
// call's first column of every value plane goes, all null for none.
sgz_status runOverviewPctColumns(Plan &p, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices, const double *q,
                                 uint32_t nq, sgz_overview_pct_record *d_carry, uint8_t *d_rgba, sgz_overview_pct_record *d_records,
                                 const PctPlanes &planes, hipStream_t stream)
{
    PctParams prm{};
    prm.lines = reinterpret_cast<const float2 *>(d_lines);
    PctOut &o = prm.out;
    o.C = p.C; o.P = p.P; o.nq = nq;
    o.rgba = reinterpret_cast<uchar4 *>(d_rgba); o.records = d_records;
    for (uint32_t j = 0; j < nq; ++j) { o.values[j] = planes.p[j]; o.q[j] = q[j]; }
    o.colourTables = p.d_colourTables; o.sc = p.scalars;
    return launchOverviewColumns(p, kOvPct, prm, frames, k, held, flush, slices, d_carry, p.P, kPctThreads,
                                 [&](uint64_t columns, uint32_t blocks) { return pctAutoSlices(p, columns, blocks, k, frames); },
                                 overviewPctColumnsKernel, overviewPctSliceKernel, overviewPctEmitKernel, stream);
}

}  // namespace sgz

struct sgz_plan { Plan impl; };

extern "C" sgz_status sgz_stage_overview_pct(sgz_plan *plan, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                             const double *q, uint32_t nq, sgz_overview_pct_record *d_carry, uint8_t *d_rgba,
                                             sgz_overview_pct_record *d_records, float *d_values, void *stream)
{
    if (!plan || !d_lines) return fail(SGZ_EINVAL, "null argument");
    if (sgz_status st = checkOverviewStep(k, held, frames); st != SGZ_OK) return st;
    if (slices > kOvMaxSlices) return fail(SGZ_EINVAL, "sgz_stage_overview_pct: slices 0 (automatic) or 1 .. 64");
    if (!validPctQuantiles(q, nq)) return fail(SGZ_EINVAL, "sgz_stage_overview_pct: 1 .. 8 quantiles, each in [0, 1]");
    if (!d_rgba && !d_records && !d_values) return fail(SGZ_EINVAL, "sgz_stage_overview_pct: an image, the records, the values or any of them");
    if (reinterpret_cast<uintptr_t>(d_carry) % 16 || reinterpret_cast<uintptr_t>(d_records) % 16)
        return fail(SGZ_EINVAL, "sgz_stage_overview_pct: d_carry and d_records are aligned to 16 bytes");
    const OverviewStep sh = overviewStepShape(k, held, frames, flush);
    if (!d_carry && (held || sh.open)) return fail(SGZ_EINVAL, "sgz_stage_overview_pct: d_carry is read (held > 0) or written (frames stay open)");
    if (!sh.launch) return SGZ_OK;
    Plan &p = plan->impl;
    if (sgz_status st = uploaded(p); st != SGZ_OK) return st;
    return runOverviewPctColumns(p, d_lines, frames, k, held, flush, slices, q, nq, d_carry, d_rgba, d_records,
                                 pctPlanes(d_values, 0, size_t(sh.closed) * p.C * p.P, nq), reinterpret_cast<hipStream_t>(stream));
}

// ---- the host helpers (no GPU) ----------------------------------------------------------------------------------------------------------------
extern "C" sgz_status sgz_overview_pct_bucket(float x, uint32_t *b)
{
    if (!b) return fail(SGZ_EINVAL, "sgz_overview_pct_bucket: null argument");
    if (x != x) return fail(SGZ_EINVAL, "sgz_overview_pct_bucket: a NaN has no bucket (it is counted in nans)");
    uint32_t bits;
    std::memcpy(&bits, &x, sizeof bits);
    *b = pctWord(bits);
    return SGZ_OK;
}

extern "C" sgz_status sgz_overview_pct_fold(const sgz_overview_pct_record *in, size_t n, size_t width, size_t x0, size_t x1, uint32_t out_columns,
                                            sgz_overview_pct_record *out)
{
    struct Wide { uint64_t w[kPctWords] = {}; };                // every word wide enough to see it pass 2^32 - 1
    return foldKeptColumns<Wide>(
        {"sgz_overview_pct_fold: null argument", "sgz_overview_pct_fold: width >= 1 records per column",
         "sgz_overview_pct_fold: a folded word counts more than 2^32 - 1 frames"},
        in, n, width, x0, x1, out_columns, out,
        [](Wide &acc, const Record &r) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(&r);
            for (int x = 0; x <= kPctNans; ++x) acc.w[x] += w[x];
        },
        [](const Wide &acc) { return std::all_of(acc.w, acc.w + kPctNans + 1, [](uint64_t c) { return c <= 0xffffffffull; }); },
        [](const Wide &acc, Record &r) {
            uint32_t *o = reinterpret_cast<uint32_t *>(&r);
            for (int x = 0; x <= kPctNans; ++x) o[x] = uint32_t(acc.w[x]);
            o[kPctWords - 1] = 0u;
        });
}

extern "C" sgz_status sgz_overview_pct_readout(const sgz_overview_pct_record *records, size_t count, const double *q, uint32_t nq, float *values)
{
    if ((!records && count) || !values) return fail(SGZ_EINVAL, "sgz_overview_pct_readout: null argument");
    if (!validPctQuantiles(q, nq)) return fail(SGZ_EINVAL, "sgz_overview_pct_readout: 1 .. 8 quantiles, each in [0, 1]");
    const auto countOf = [](const Record &rec) { uint64_t total = 0; for (uint32_t c : rec.bucket) total += c; return total; };
    for (size_t i = 0; i < count; ++i)
        if (countOf(records[i]) > 0xffffffffull) return fail(SGZ_EINVAL, "sgz_overview_pct_readout: a record counts more than 2^32 - 1 frames");
    for (size_t i = 0; i < count; ++i) {
        const Record &rec = records[i];
        const uint64_t total = countOf(rec);
        for (uint32_t j = 0; j < nq; ++j) {
            float v;
            if (total == 0) { const uint32_t bits = 0x7fc00000u; std::memcpy(&v, &bits, sizeof v); }
            else {
                const uint32_t r = pctRank(q[j], uint32_t(total));
                uint64_t below = 0;
                uint32_t b = 0;
                for (; b < uint32_t(kPctBuckets) - 1; ++b) {
                    if (below + rec.bucket[b] >= r) break;
                    below += rec.bucket[b];
                }
                v = pctValue(b, r, uint32_t(below), rec.bucket[b]);
            }
            values[size_t(j) * count + i] = v;
        }
    }
    return SGZ_OK;
}
