// overview_stats.hip -- the mean overview: mean and range of k frames of line results per image column (sgz.h, "The mean overview").  gfx950
// only.  The reduction beside overview.hip's peak hold, over the same line results and the same columns:
//   q(x) = rint(x 2^20) clamped to +-(2^31 - 1), a NaN left out and counted; per (column, pair, pixel) the record
//   { sum = sum of q, count, nans, lo, hi }  -- integers and an order's extremes, so every field folds associatively and commutatively
//   and any split of the frames (slices, calls, slabs, feeds) gives the same bytes;  mean = (float)((double)sum / (double)count 2^-20);
//   the pixel is blendColour / toRgba8 of decay_body.hpp at the mean (called, not copied).
// The kernels keep an accumulator: the sum, the counts, hi as a key (0: no value yet) and lo as key - 1 (0xFFFFFFFF: no value yet;
// order_key.hpp), and turn it into a record where it leaves the registers.  This file holds the kind (struct Stats: the record, the
// accumulator's operations, a record's load and store, emitClosed) and the named entry points; the six kernel bodies, the bounds, the batched
// folds, the launch front and the host fold's frame are overview_kinds.hpp's.  The three shapes of overview.hip, for its reasons:
//   overviewStatsColumnsKernel   one thread per (column, pixel): pairs outermost (the blend order), the column's frames inside, 8 loads in
//                                flight before the quantiser and the updates; then the carry, the mean, the colour, the stores.
//   overviewStatsSliceKernel     few columns of many frames: slice s of a column's frames -> partial records [slices][columns][pairs][P] in
//   overviewStatsEmitKernel      plan scratch; then the fold over the slices and the carry, the mean, the colour, the stores -- a launch of its
//                                own behind it on the stream (no hand-off between workgroups inside a launch).
//   overviewStatsViewKernel, overviewStatsViewSliceKernel, overviewStatsViewEmitKernel   the same fold on kept records [n][pairs][P].
// A record leaves a lane by per-field stores, not through LDS staging: the listing shows them merged into one global_store_dwordx2 (sum) and
// one global_store_dwordx4 at offset 8 (count, nans, lo, hi) -- consecutive lanes are 24 bytes apart, so a wave's 64 records are one
// contiguous 1536-byte run that the two stores cover between them; records are read the same way ("The mean overview").
// In the frame loop the only 64-bit integer operation is the add; the fp64 division happens once per (column, pair, pixel).
// Nothing is waited for; scratch grows on demand (only growth synchronises); everything runs on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "runtime.hpp"
#include "decay_body.hpp"
#include "order_key.hpp"       // orderKey / keyBits / orderKeyMin / keyBitsMin

#pragma clang fp contract(off)

#include "overview_kinds.hpp"   // behind the pragma: its templates are parsed without contraction

using namespace sgz;

static_assert(sizeof(sgz_overview_stat_record) == 24 && alignof(sgz_overview_stat_record) == 8, "sgz_overview_stat_record: 24 bytes, 8-aligned");
static_assert(offsetof(sgz_overview_stat_record, sum) == 0 && offsetof(sgz_overview_stat_record, count) == 8 &&
              offsetof(sgz_overview_stat_record, nans) == 12 && offsetof(sgz_overview_stat_record, lo) == 16 &&
              offsetof(sgz_overview_stat_record, hi) == 20, "sgz_overview_stat_record: the layout sgz.h documents");

namespace {

using Record = sgz_overview_stat_record;

constexpr double kQuantum = 1048576.0;   // 2^20 steps per unit of the dB axis
constexpr double kQMost = 2147483647.0;  // 2^31 - 1

// ---- the definition, for the host and the device -------------------------------------------------------------------------------------------
// q of a non-NaN value: the product is exact, +-inf stays +-inf and clamps; rint of a clamped t is the clamp itself.  No branch: a wave's
// lanes hold different pixels, and a NaN handed in (the caller masks its q) takes the same instructions
__host__ __device__ inline int32_t statQuantise(float x)
{
    const double t = double(x) * kQuantum;
    return int32_t(rint(fmin(fmax(t, -kQMost), kQMost)));
}

// the mean's bits: two conversions, one division, one exact scaling, one conversion, each to nearest even
__host__ __device__ inline uint32_t statMeanBits(int64_t sum, uint32_t count)
{
    if (count == 0) return 0x7fc00000u;
    const float mean = float((double(sum) / double(count)) * (1.0 / kQuantum));
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(mean);
#else
    return hostBits(mean);
#endif
}

// ---- what every emitting kernel writes -----------------------------------------------------------------------------------------------------
struct StatsOut {
    uint32_t C, P;
    uchar4 *rgba;                        // [columns][P] or null
    Record *stats;                       // [columns][C][P] or null
    float *means;                        // [columns][C][P] or null
    const float *colourTables;
    DeviceScalars sc;
};

// the direct form: k frames of line results per column
struct StatsParams {
    const float2 *lines;                 // [frames][C][G][P]
    long frames;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t k, held, blocks, slices;
    const Record *carryIn;               // [C][P]: the record of column 0's `held` earlier frames (read iff held > 0)
    Record *carryOut;                    // [C][P]: the record of the open column
    Record *partial;                     // [slices][columns][C][P]
    StatsOut out;
};

// the view of kept records (sgz.h, "The mean overview"): records [n][pairs][P] as any stats call writes them
struct StatsViewParams {
    const Record *src;                   // [m][C][P]: the range's first source column
    long m, cols;
    uint32_t blocks, slices;
    Record *partial;                     // [slices][cols][C][P]
    StatsOut out;
};

// ---- the kind (overview_kinds.hpp, section 3) ------------------------------------------------------------------------------------------------
struct Stats {
    using Record = ::Record;
    using Params = StatsParams;
    using ViewParams = StatsViewParams;
    static constexpr int kThreads = 256;

    struct Acc {
        long long sum = 0;
        uint32_t count = 0, nans = 0;
        uint32_t hi = 0u;                // the greatest orderKey; 0: no value yet
        uint32_t lo = 0xffffffffu;       // the least orderKeyMin; 0xFFFFFFFF: no value yet
    };

    static __device__ __forceinline__ uint32_t cells(const StatsOut &o) { return o.P; }
    static __device__ __forceinline__ LinesRow row(const Params &prm, uint32_t pair, uint32_t pixel)
    {
        return linesRow(prm.lines, prm.out.C, prm.out.P, pair, pixel);
    }

    static __device__ __forceinline__ void accFrame(Acc &a, uint32_t bits)
    {
        const uint32_t key = orderKey(bits);                     // 0 for a NaN: it moves neither hi nor, as key - 1 = 0xFFFFFFFF, lo
        const bool nan = key == 0u;
        a.sum += nan ? 0ll : (long long)statQuantise(__uint_as_float(bits));
        a.count += nan ? 0u : 1u;
        a.nans += nan ? 1u : 0u;
        a.hi = max(a.hi, key);
        a.lo = min(a.lo, key - 1u);
    }
    static __device__ __forceinline__ void accUnfill(Acc &a, uint32_t n) { a.nans -= n; }

    // field-wise: a record without values carries NaNs in lo and hi, whose keys are the two empty markers
    static __device__ __forceinline__ void accFold(Acc &a, const Record &r)
    {
        a.sum += r.sum;
        a.count += r.count;
        a.nans += r.nans;
        a.hi = max(a.hi, orderKey(__float_as_uint(r.hi)));
        a.lo = min(a.lo, orderKeyMin(__float_as_uint(r.lo)));
    }

    static __device__ __forceinline__ Record accRecord(const Acc &a)
    {
        Record r;
        r.sum = a.sum; r.count = a.count; r.nans = a.nans;
        r.lo = __uint_as_float(keyBitsMin(a.lo));
        r.hi = __uint_as_float(keyBits(a.hi));
        return r;
    }

    // a record as three 8-byte words, for loads that are issued together (the compiler merges the last two: dwordx2 + dwordx4)
    struct Words { uint2 w[3]; };
    static __device__ __forceinline__ Words loadWords(const Record *p)
    {
        const uint2 *q = reinterpret_cast<const uint2 *>(p);
        return Words{{q[0], q[1], q[2]}};
    }
    static __device__ __forceinline__ Record wordsRecord(const Words &x)
    {
        Record r;
        r.sum = (long long)((unsigned long long)x.w[0].x | ((unsigned long long)x.w[0].y << 32));
        r.count = x.w[1].x; r.nans = x.w[1].y;
        r.lo = __uint_as_float(x.w[2].x); r.hi = __uint_as_float(x.w[2].y);
        return r;
    }
    static __device__ __forceinline__ void storeRecord(Record *p, const Record &r)
    {
        uint2 *q = reinterpret_cast<uint2 *>(p);
        q[0] = make_uint2(uint32_t((unsigned long long)r.sum), uint32_t((unsigned long long)r.sum >> 32));
        q[1] = make_uint2(r.count, r.nans);
        q[2] = make_uint2(__float_as_uint(r.lo), __float_as_uint(r.hi));
    }

    // a closed column of a pixel: the records, the means and the blend at the means in pair order
    template <typename AccOf>
    static __device__ __forceinline__ void emitClosed(const StatsOut &o, long col, uint32_t pixel, AccOf accOf)
    {
        float cb[3] = {0.f, 0.f, 0.f};
        for (uint32_t pair = 0; pair < o.C; ++pair) {
            const Acc acc = accOf(pair);
            const size_t at = (size_t(col) * o.C + pair) * o.P + pixel;
            if (o.stats) storeRecord(o.stats + at, accRecord(acc));
            if (!o.means && !o.rgba) continue;
            const float mean = __uint_as_float(statMeanBits(acc.sum, acc.count));
            if (o.means) o.means[at] = mean;
            if (o.rgba) blendColour(cb, mean, o.colourTables + size_t(pair) * NC * 3, o.sc);
        }
        if (o.rgba) o.rgba[size_t(col) * o.P + pixel] = toRgba8(cb);
    }
};

__global__ void __launch_bounds__(Stats::kThreads) overviewStatsColumnsKernel(const StatsParams prm) { overviewColumnsBody<Stats>(prm); }
__global__ void __launch_bounds__(Stats::kThreads) overviewStatsSliceKernel(const StatsParams prm) { overviewSliceBody<Stats>(prm); }
__global__ void __launch_bounds__(Stats::kThreads) overviewStatsEmitKernel(const StatsParams prm) { overviewEmitBody<Stats>(prm); }
__global__ void __launch_bounds__(Stats::kThreads) overviewStatsViewKernel(const StatsViewParams prm) { overviewViewBody<Stats>(prm); }
__global__ void __launch_bounds__(Stats::kThreads) overviewStatsViewSliceKernel(const StatsViewParams prm) { overviewViewSliceBody<Stats>(prm); }
__global__ void __launch_bounds__(Stats::kThreads) overviewStatsViewEmitKernel(const StatsViewParams prm) { overviewViewEmitBody<Stats>(prm); }

StatsOut statsOut(const Plan &p, uint8_t *d_rgba, Record *d_stats, float *d_means)
{
    StatsOut o{};
    o.C = p.C; o.P = p.P;
    o.rgba = reinterpret_cast<uchar4 *>(d_rgba); o.stats = d_stats; o.means = d_means;
    o.colourTables = p.d_colourTables; o.sc = p.scalars;
    return o;
}

// host: the accumulator of sgz_overview_stats_fold, with counts wide enough to see them pass 2^32 - 1
struct HostAcc { int64_t sum = 0; uint64_t count = 0, nans = 0; uint32_t hi = 0u, lo = 0xffffffffu; };

}  // namespace

namespace sgz {

// sgz_stage_overview_stats behind its argument checks (the plan's tables are uploaded).  d_lines [frames][C][G][P] float2.
sgz_status runOverviewStatsColumns(Plan &p, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                   sgz_overview_stat_record *d_carry, uint8_t *d_rgba, sgz_overview_stat_record *d_stats, float *d_means,
                                   hipStream_t stream)
{
    StatsParams prm{};
    prm.lines = reinterpret_cast<const float2 *>(d_lines);
    prm.out = statsOut(p, d_rgba, d_stats, d_means);
    return launchOverviewColumns(p, kOvStats, prm, frames, k, held, flush, slices, d_carry, p.P, Stats::kThreads,
                                 [&](uint64_t columns, uint32_t blocks) { return overviewAutoSlices(long(columns), blocks, k, frames, numCUs()); },
                                 overviewStatsColumnsKernel, overviewStatsSliceKernel, overviewStatsEmitKernel, stream);
}

// sgz_stage_overview_stats_view behind its argument checks (the plan's tables are uploaded).  d_src [m][C][P]: the range's first source column.
sgz_status runOverviewStatsView(Plan &p, const sgz_overview_stat_record *d_src, size_t m, size_t cols, uint32_t slices, uint8_t *d_rgba,
                                sgz_overview_stat_record *d_statsOut, float *d_means, hipStream_t stream)
{
    StatsViewParams prm{};
    prm.src = d_src;
    prm.out = statsOut(p, d_rgba, d_statsOut, d_means);
    return launchOverviewView(p, kOvStats, prm, m, cols, slices, p.P, Stats::kThreads, overviewStatsViewKernel, overviewStatsViewSliceKernel,
                              overviewStatsViewEmitKernel, stream);
}

}  // namespace sgz

struct sgz_plan { Plan impl; };

extern "C" sgz_status sgz_stage_overview_stats(sgz_plan *plan, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                               sgz_overview_stat_record *d_carry, uint8_t *d_rgba, sgz_overview_stat_record *d_stats, float *d_means,
                                               void *stream)
{
    if (!plan || !d_lines) return fail(SGZ_EINVAL, "null argument");
    if (sgz_status st = checkOverviewStep(k, held, frames); st != SGZ_OK) return st;
    if (slices > kOvMaxSlices) return fail(SGZ_EINVAL, "sgz_stage_overview_stats: slices 0 (automatic) or 1 .. 64");
    if (!d_rgba && !d_stats && !d_means) return fail(SGZ_EINVAL, "sgz_stage_overview_stats: an image, the records, the means or any of them");
    const OverviewStep sh = overviewStepShape(k, held, frames, flush);
    if (!d_carry && (held || sh.open)) return fail(SGZ_EINVAL, "sgz_stage_overview_stats: d_carry is read (held > 0) or written (frames stay open)");
    if (!sh.launch) return SGZ_OK;
    Plan &p = plan->impl;
    if (sgz_status st = uploaded(p); st != SGZ_OK) return st;
    return runOverviewStatsColumns(p, d_lines, frames, k, held, flush, slices, d_carry, d_rgba, d_stats, d_means, reinterpret_cast<hipStream_t>(stream));
}

extern "C" sgz_status sgz_stage_overview_stats_view(sgz_plan *plan, const sgz_overview_stat_record *d_stats, size_t n, size_t x0, size_t x1,
                                                    uint32_t out_columns, uint32_t slices, uint8_t *d_rgba, sgz_overview_stat_record *d_stats_out,
                                                    float *d_means, void *stream)
{
    if (!plan || !d_stats) return fail(SGZ_EINVAL, "null argument");
    uint64_t cols = 0;
    if (sgz_status st = checkViewRange(n, x0, x1, out_columns, &cols); st != SGZ_OK) return st;
    if (slices > kOvMaxSlices) return fail(SGZ_EINVAL, "sgz_stage_overview_stats_view: slices 0 (automatic) or 1 .. 64");
    if (!d_rgba && !d_stats_out && !d_means) return fail(SGZ_EINVAL, "sgz_stage_overview_stats_view: an image, the records, the means or any of them");
    Plan &p = plan->impl;
    const size_t column = size_t(p.C) * p.P;                     // records of a source column
    const Record *src = d_stats + x0 * column;
    const size_t srcBytes = (x1 - x0) * column * sizeof(Record);
    if (bytesOverlap(src, srcBytes, d_rgba, size_t(cols) * p.P * 4) || bytesOverlap(src, srcBytes, d_stats_out, size_t(cols) * column * sizeof(Record)) ||
        bytesOverlap(src, srcBytes, d_means, size_t(cols) * column * sizeof(float)))
        return fail(SGZ_EINVAL, "sgz_stage_overview_stats_view: an output overlaps the source columns it is made from");
    if (sgz_status st = uploaded(p); st != SGZ_OK) return st;
    return runOverviewStatsView(p, src, x1 - x0, size_t(cols), slices, d_rgba, d_stats_out, d_means, reinterpret_cast<hipStream_t>(stream));
}

// ---- the host helpers (no GPU) ----------------------------------------------------------------------------------------------------------------
extern "C" sgz_status sgz_overview_stats_fold(const sgz_overview_stat_record *in, size_t n, size_t width, size_t x0, size_t x1, uint32_t out_columns,
                                              sgz_overview_stat_record *out)
{
    return foldKeptColumns<HostAcc>(
        {"sgz_overview_stats_fold: null argument", "sgz_overview_stats_fold: width >= 1 records per column",
         "sgz_overview_stats_fold: a folded column counts more than 2^32 - 1 frames"},
        in, n, width, x0, x1, out_columns, out,
        [](HostAcc &acc, const Record &r) {
            acc.sum = int64_t(uint64_t(acc.sum) + uint64_t(r.sum));
            acc.count += r.count; acc.nans += r.nans;
            acc.hi = std::max(acc.hi, orderKey(hostBits(r.hi)));
            acc.lo = std::min(acc.lo, orderKeyMin(hostBits(r.lo)));
        },
        [](const HostAcc &acc) { return acc.count <= 0xffffffffull && acc.nans <= 0xffffffffull; },
        [](const HostAcc &acc, Record &o) {
            o.sum = acc.sum; o.count = uint32_t(acc.count); o.nans = uint32_t(acc.nans);
            o.lo = hostFloat(keyBitsMin(acc.lo)); o.hi = hostFloat(keyBits(acc.hi));
        });
}

extern "C" sgz_status sgz_overview_stats_readout(const sgz_overview_stat_record *in, size_t count, float *mean, float *lo, float *hi)
{
    if (!in && count) return fail(SGZ_EINVAL, "sgz_overview_stats_readout: null records");
    if (!mean && !lo && !hi) return fail(SGZ_EINVAL, "sgz_overview_stats_readout: the means, the least, the greatest or any of them");
    for (size_t i = 0; i < count; ++i) {
        if (mean) { const uint32_t bits = statMeanBits(in[i].sum, in[i].count); std::memcpy(mean + i, &bits, sizeof bits); }
        if (lo) lo[i] = in[i].lo;
        if (hi) hi[i] = in[i].hi;
    }
    return SGZ_OK;
}
