// overview_power.hip -- the power overview: mean-square spectrum of k frames per image column (sgz.h, "The power overview").  gfx950 only.
// The third reduction over the overview's columns, of the mapped magnitudes M [frames][pairs][sides][P] that K_A leaves in HBM -- the values
// from before the decay and the dB map, so that the mean is a power-domain mean and no K_B launch and no decay state take part:
//   q(x) = rint(x^2 2^60) clamped to 2^64 - 2^11, a NaN left out and counted; per (column, pair, side, pixel) the record
//   { sum[2] = the 128-bit sum of q, count, nans, lo, hi }  -- integers and an order's extremes, so every field folds associatively and
//   commutatively and any split of the frames (slices, calls, slabs, feeds) gives the same bytes;
//   rms = (float)(sqrt(S / count) 2^-30), S = (double)sum[1] 2^64 + (double)sum[0];  level = dbMap(slopeMap[i], rms) of decay_body.hpp (called,
//   not copied) -- K_B's line result for a frame of magnitude rms from a zero decay state;  the pixel is blendColour / toRgba8 at side 0's level.
// The kernels keep an accumulator: the sum as unsigned __int128 (level_columns.hip's way), the counts, hi as a key (0: no value yet) and lo as
// key - 1 (0xFFFFFFFF: no value yet; order_key.hpp), and turn it into a record where it leaves the registers.  This file holds the kind
// (struct Power: the record, the accumulator's operations, a record's load and store, emitClosed) and the named entry points; the six kernel
// bodies, the bounds, the batched folds, the launch front and the host fold's frame are overview_kinds.hpp's.  The three shapes of
// overview_stats.hip, for its reasons, with a column's sides * P values in the place of its P:
//   overviewPowerColumnsKernel   one thread per (column, side * P + pixel): pairs outermost (the blend order), the column's frames inside, 8 loads
//                                in flight before the quantiser and the updates; then the carry, the readout, the level, the colour, the stores.
//   overviewPowerSliceKernel     few columns of many frames: slice s of a column's frames -> partial records [slices][columns][pairs][sides][P]
//   overviewPowerEmitKernel      in plan scratch; then the fold over the slices and the carry and the outputs -- a launch of its own behind it
//                                on the stream (no hand-off between workgroups inside a launch).
//   overviewPowerViewKernel, overviewPowerViewSliceKernel, overviewPowerViewEmitKernel   the same fold on kept records [n][pairs][sides][P].
// The thread of (side 0, pixel i) walks the pairs in order and blends their colours; a side-1 thread writes its records and levels only.
// A record leaves and enters a lane as two 16-byte words: consecutive lanes are 32 bytes apart, a wave's 64 records one contiguous 2 KiB run.
// In the frame loop there is one fp64 product, one scaling, one conversion and the 128-bit add; the fp64 division, the root and dbMap happen
// once per emitted (column, pair, side, pixel).  No LDS, no atomics.  Nothing is waited for; scratch grows on demand (only growth
// synchronises); everything runs on the caller's stream.
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

static_assert(sizeof(sgz_overview_power_record) == 32 && alignof(sgz_overview_power_record) == 8, "sgz_overview_power_record: 32 bytes, 8-aligned");
static_assert(offsetof(sgz_overview_power_record, sum) == 0 && offsetof(sgz_overview_power_record, count) == 16 &&
              offsetof(sgz_overview_power_record, nans) == 20 && offsetof(sgz_overview_power_record, lo) == 24 &&
              offsetof(sgz_overview_power_record, hi) == 28, "sgz_overview_power_record: the layout sgz.h documents");

namespace {

using Record = sgz_overview_power_record;
typedef unsigned __int128 u128;

constexpr double kQuantum = 1152921504606846976.0;      // 2^60 steps per unit of power
constexpr double kQMost = 18446744073709549568.0;       // 2^64 - 2^11, the largest double below 2^64
constexpr double kTwo64 = 18446744073709551616.0;
constexpr double kRmsScale = 9.3132257461547852e-10;    // 2^-30

// ---- the definition, for the host and the device -------------------------------------------------------------------------------------------
// q of a non-NaN value: the square is exact (48 significant bits), the scaling is exact, +inf stays +inf and clamps; rint of the clamp is the
// clamp itself, and it converts exactly.  No branch: a wave's lanes hold different pixels, and a NaN handed in (the caller masks its q) takes
// the same instructions -- fmin drops it for the clamp
__host__ __device__ inline uint64_t powerQuantise(float x)
{
    const double t = double(x) * double(x);
    return uint64_t(rint(fmin(t * kQuantum, kQMost)));
}

// the mean square in units of 2^-60: both conversions, the sum and the division to nearest even (sum[1] 2^64 is exact below 2^96)
__host__ __device__ inline double powerMeanSquare(uint64_t lo, uint64_t hi, uint32_t count)
{
    const double S = double(hi) * kTwo64 + double(lo);
    return S / double(count);
}

// the rms' bits: the root correctly rounded, one exact scaling, one conversion
__host__ __device__ inline uint32_t powerRmsBits(uint64_t lo, uint64_t hi, uint32_t count)
{
    if (count == 0) return 0x7fc00000u;
    const double ms = powerMeanSquare(lo, hi, count);
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(float(__dsqrt_rn(ms) * kRmsScale));
#else
    return hostBits(float(std::sqrt(ms) * kRmsScale));
#endif
}

// ---- what every emitting kernel writes -----------------------------------------------------------------------------------------------------
struct PowerOut {
    uint32_t C, P, SP;                   // pairs, pixels, sides * P: the values of one (frame, pair), and a thread's index among them
    uchar4 *rgba;                        // [columns][P] or null
    Record *power;                       // [columns][C][sides][P] or null
    float *levels;                       // [columns][C][sides][P] or null
    const float *slope;                  // [P]
    const float *colourTables;
    DeviceScalars sc;
};

// the direct form: k frames of mapped magnitudes per column
struct PowerParams {
    const float *mapped;                 // [frames][C][sides][P]
    long frames;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t k, held, blocks, slices;
    const Record *carryIn;               // [C][sides][P]: the record of column 0's `held` earlier frames (read iff held > 0)
    Record *carryOut;                    // [C][sides][P]: the record of the open column
    Record *partial;                     // [slices][columns][C][sides][P]
    PowerOut out;
};

// the view of kept records (sgz.h, "The power overview"): records [n][pairs][sides][P] as any power call writes them
struct PowerViewParams {
    const Record *src;                   // [m][C][sides][P]: the range's first source column
    long m, cols;
    uint32_t blocks, slices;
    Record *partial;                     // [slices][cols][C][sides][P]
    PowerOut out;
};

// the mapped magnitudes of thread j = side * P + pixel of a pair over the frames, as bits
struct MappedRow {
    const uint32_t *first;
    size_t perFrame;
    __device__ __forceinline__ uint32_t bits(long f) const { return first[size_t(f) * perFrame]; }
};

// ---- the kind (overview_kinds.hpp, section 3) ------------------------------------------------------------------------------------------------
struct Power {
    using Record = ::Record;
    using Params = PowerParams;
    using ViewParams = PowerViewParams;
    static constexpr int kThreads = 256;

    struct Acc {
        u128 sum = 0;
        uint32_t count = 0, nans = 0;
        uint32_t hi = 0u;                // the greatest orderKey; 0: no value yet
        uint32_t lo = 0xffffffffu;       // the least orderKeyMin; 0xFFFFFFFF: no value yet
    };

    static __device__ __forceinline__ uint32_t cells(const PowerOut &o) { return o.SP; }
    static __device__ __forceinline__ MappedRow row(const Params &prm, uint32_t pair, uint32_t j)
    {
        return MappedRow{reinterpret_cast<const uint32_t *>(prm.mapped) + size_t(pair) * prm.out.SP + j, size_t(prm.out.C) * prm.out.SP};
    }

    static __device__ __forceinline__ void accFrame(Acc &a, uint32_t bits)
    {
        const uint32_t key = orderKey(bits);                     // 0 for a NaN: it moves neither hi nor, as key - 1 = 0xFFFFFFFF, lo
        const bool nan = key == 0u;
        const uint64_t q = powerQuantise(__uint_as_float(bits));
        a.sum += u128(nan ? 0ull : q);
        a.count += nan ? 0u : 1u;
        a.nans += nan ? 1u : 0u;
        a.hi = max(a.hi, key);
        a.lo = min(a.lo, key - 1u);
    }
    static __device__ __forceinline__ void accUnfill(Acc &a, uint32_t n) { a.nans -= n; }

    // field-wise: a record without values carries NaNs in lo and hi, whose keys are the two empty markers
    static __device__ __forceinline__ void accFold(Acc &a, const Record &r)
    {
        a.sum += (u128(r.sum[1]) << 64) | u128(r.sum[0]);
        a.count += r.count;
        a.nans += r.nans;
        a.hi = max(a.hi, orderKey(__float_as_uint(r.hi)));
        a.lo = min(a.lo, orderKeyMin(__float_as_uint(r.lo)));
    }

    static __device__ __forceinline__ Record accRecord(const Acc &a)
    {
        Record r;
        r.sum[0] = uint64_t(a.sum); r.sum[1] = uint64_t(a.sum >> 64);
        r.count = a.count; r.nans = a.nans;
        r.lo = __uint_as_float(keyBitsMin(a.lo));
        r.hi = __uint_as_float(keyBits(a.hi));
        return r;
    }

    // a record as two 16-byte words, for loads that are issued together
    struct Words { uint4 w[2]; };
    static __device__ __forceinline__ Words loadWords(const Record *p)
    {
        const uint4 *q = reinterpret_cast<const uint4 *>(p);
        return Words{{q[0], q[1]}};
    }
    static __device__ __forceinline__ Record wordsRecord(const Words &x)
    {
        Record r;
        r.sum[0] = uint64_t(x.w[0].x) | (uint64_t(x.w[0].y) << 32);
        r.sum[1] = uint64_t(x.w[0].z) | (uint64_t(x.w[0].w) << 32);
        r.count = x.w[1].x; r.nans = x.w[1].y;
        r.lo = __uint_as_float(x.w[1].z); r.hi = __uint_as_float(x.w[1].w);
        return r;
    }
    static __device__ __forceinline__ void storeRecord(Record *p, const Record &r)
    {
        uint4 *q = reinterpret_cast<uint4 *>(p);
        q[0] = make_uint4(uint32_t(r.sum[0]), uint32_t(r.sum[0] >> 32), uint32_t(r.sum[1]), uint32_t(r.sum[1] >> 32));
        q[1] = make_uint4(r.count, r.nans, __float_as_uint(r.lo), __float_as_uint(r.hi));
    }

    // a closed column of thread j = side * P + pixel: the records, the levels and -- side 0 -- the blend at the levels in pair order
    template <typename AccOf>
    static __device__ __forceinline__ void emitClosed(const PowerOut &o, long col, uint32_t j, AccOf accOf)
    {
        const uint32_t pixel = j < o.P ? j : j - o.P;
        const bool image = o.rgba && j < o.P;
        const bool level = o.levels || image;
        const float slope = level ? o.slope[pixel] : 0.f;
        float cb[3] = {0.f, 0.f, 0.f};
        for (uint32_t pair = 0; pair < o.C; ++pair) {
            const Acc acc = accOf(pair);
            const size_t at = (size_t(col) * o.C + pair) * o.SP + j;
            if (o.power) storeRecord(o.power + at, accRecord(acc));
            if (!level) continue;
            float lv = __uint_as_float(0x7fc00000u);
            if (acc.count) lv = dbMap(slope, __uint_as_float(powerRmsBits(uint64_t(acc.sum), uint64_t(acc.sum >> 64), acc.count)), o.sc);
            if (o.levels) o.levels[at] = lv;
            if (image) blendColour(cb, lv, o.colourTables + size_t(pair) * NC * 3, o.sc);
        }
        if (image) o.rgba[size_t(col) * o.P + pixel] = toRgba8(cb);
    }
};

__global__ void __launch_bounds__(Power::kThreads) overviewPowerColumnsKernel(const PowerParams prm) { overviewColumnsBody<Power>(prm); }
__global__ void __launch_bounds__(Power::kThreads) overviewPowerSliceKernel(const PowerParams prm) { overviewSliceBody<Power>(prm); }
__global__ void __launch_bounds__(Power::kThreads) overviewPowerEmitKernel(const PowerParams prm) { overviewEmitBody<Power>(prm); }
__global__ void __launch_bounds__(Power::kThreads) overviewPowerViewKernel(const PowerViewParams prm) { overviewViewBody<Power>(prm); }
__global__ void __launch_bounds__(Power::kThreads) overviewPowerViewSliceKernel(const PowerViewParams prm) { overviewViewSliceBody<Power>(prm); }
__global__ void __launch_bounds__(Power::kThreads) overviewPowerViewEmitKernel(const PowerViewParams prm) { overviewViewEmitBody<Power>(prm); }

PowerOut powerOut(const Plan &p, uint8_t *d_rgba, Record *d_power, float *d_levels)
{
    PowerOut o{};
    o.C = p.C; o.P = p.P; o.SP = uint32_t(p.sides) * p.P;
    o.rgba = reinterpret_cast<uchar4 *>(d_rgba); o.power = d_power; o.levels = d_levels;
    o.slope = p.d_slope; o.colourTables = p.d_colourTables; o.sc = p.scalars;
    return o;
}

// host: the accumulator of sgz_overview_power_fold, with counts wide enough to see them pass 2^32 - 1
struct HostAcc { u128 sum = 0; uint64_t count = 0, nans = 0; uint32_t hi = 0u, lo = 0xffffffffu; };

}  // namespace

namespace sgz {

// sgz_stage_overview_power behind its argument checks (the plan's tables are uploaded).  d_mapped [frames][C][sides][P] float.
sgz_status runOverviewPowerColumns(Plan &p, const float *d_mapped, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                   sgz_overview_power_record *d_carry, uint8_t *d_rgba, sgz_overview_power_record *d_power, float *d_levels,
                                   hipStream_t stream)
{
    PowerParams prm{};
    prm.mapped = d_mapped;
    prm.out = powerOut(p, d_rgba, d_power, d_levels);
    return launchOverviewColumns(p, kOvPower, prm, frames, k, held, flush, slices, d_carry, prm.out.SP, Power::kThreads,
                                 [&](uint64_t columns, uint32_t blocks) { return overviewAutoSlices(long(columns), blocks, k, frames, numCUs()); },
                                 overviewPowerColumnsKernel, overviewPowerSliceKernel, overviewPowerEmitKernel, stream);
}

// sgz_stage_overview_power_view behind its argument checks (the plan's tables are uploaded).  d_src [m][C][sides][P]: the range's first source column.
sgz_status runOverviewPowerView(Plan &p, const sgz_overview_power_record *d_src, size_t m, size_t cols, uint32_t slices, uint8_t *d_rgba,
                                sgz_overview_power_record *d_powerOut, float *d_levels, hipStream_t stream)
{
    PowerViewParams prm{};
    prm.src = d_src;
    prm.out = powerOut(p, d_rgba, d_powerOut, d_levels);
    return launchOverviewView(p, kOvPower, prm, m, cols, slices, prm.out.SP, Power::kThreads, overviewPowerViewKernel, overviewPowerViewSliceKernel,
                              overviewPowerViewEmitKernel, stream);
}

}  // namespace sgz

struct sgz_plan { Plan impl; };

extern "C" sgz_status sgz_stage_overview_power(sgz_plan *plan, const float *d_mapped, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                               sgz_overview_power_record *d_carry, uint8_t *d_rgba, sgz_overview_power_record *d_power, float *d_levels,
                                               void *stream)
{
    if (!plan || !d_mapped) return fail(SGZ_EINVAL, "null argument");
    if (sgz_status st = checkOverviewStep(k, held, frames); st != SGZ_OK) return st;
    if (slices > kOvMaxSlices) return fail(SGZ_EINVAL, "sgz_stage_overview_power: slices 0 (automatic) or 1 .. 64");
    if (!d_rgba && !d_power && !d_levels) return fail(SGZ_EINVAL, "sgz_stage_overview_power: an image, the records, the levels or any of them");
    const OverviewStep sh = overviewStepShape(k, held, frames, flush);
    if (!d_carry && (held || sh.open)) return fail(SGZ_EINVAL, "sgz_stage_overview_power: d_carry is read (held > 0) or written (frames stay open)");
    if (!sh.launch) return SGZ_OK;
    Plan &p = plan->impl;
    if (sgz_status st = uploaded(p); st != SGZ_OK) return st;
    return runOverviewPowerColumns(p, d_mapped, frames, k, held, flush, slices, d_carry, d_rgba, d_power, d_levels, reinterpret_cast<hipStream_t>(stream));
}

extern "C" sgz_status sgz_stage_overview_power_view(sgz_plan *plan, const sgz_overview_power_record *d_power, size_t n, size_t x0, size_t x1,
                                                    uint32_t out_columns, uint32_t slices, uint8_t *d_rgba, sgz_overview_power_record *d_power_out,
                                                    float *d_levels, void *stream)
{
    if (!plan || !d_power) return fail(SGZ_EINVAL, "null argument");
    uint64_t cols = 0;
    if (sgz_status st = checkViewRange(n, x0, x1, out_columns, &cols); st != SGZ_OK) return st;
    if (slices > kOvMaxSlices) return fail(SGZ_EINVAL, "sgz_stage_overview_power_view: slices 0 (automatic) or 1 .. 64");
    if (!d_rgba && !d_power_out && !d_levels) return fail(SGZ_EINVAL, "sgz_stage_overview_power_view: an image, the records, the levels or any of them");
    Plan &p = plan->impl;
    const size_t column = size_t(p.C) * p.sides * p.P;           // records of a source column
    const Record *src = d_power + x0 * column;
    const size_t srcBytes = (x1 - x0) * column * sizeof(Record);
    if (bytesOverlap(src, srcBytes, d_rgba, size_t(cols) * p.P * 4) || bytesOverlap(src, srcBytes, d_power_out, size_t(cols) * column * sizeof(Record)) ||
        bytesOverlap(src, srcBytes, d_levels, size_t(cols) * column * sizeof(float)))
        return fail(SGZ_EINVAL, "sgz_stage_overview_power_view: an output overlaps the source columns it is made from");
    if (sgz_status st = uploaded(p); st != SGZ_OK) return st;
    return runOverviewPowerView(p, src, x1 - x0, size_t(cols), slices, d_rgba, d_power_out, d_levels, reinterpret_cast<hipStream_t>(stream));
}

// ---- the host helpers (no GPU) ----------------------------------------------------------------------------------------------------------------
extern "C" sgz_status sgz_overview_power_quantise(const float *x, size_t n, uint64_t *q)
{
    if ((!x || !q) && n) return fail(SGZ_EINVAL, "sgz_overview_power_quantise: null argument");
    for (size_t i = 0; i < n; ++i) q[i] = x[i] != x[i] ? 0u : powerQuantise(x[i]);      // (a NaN has no q: it takes no part in a sum)
    return SGZ_OK;
}

extern "C" sgz_status sgz_overview_power_fold(const sgz_overview_power_record *in, size_t n, size_t width, size_t x0, size_t x1, uint32_t out_columns,
                                              sgz_overview_power_record *out)
{
    return foldKeptColumns<HostAcc>(
        {"sgz_overview_power_fold: null argument", "sgz_overview_power_fold: width >= 1 records per column",
         "sgz_overview_power_fold: a folded column counts more than 2^32 - 1 frames"},
        in, n, width, x0, x1, out_columns, out,
        [](HostAcc &acc, const Record &r) {
            acc.sum += (u128(r.sum[1]) << 64) | u128(r.sum[0]);
            acc.count += r.count; acc.nans += r.nans;
            acc.hi = std::max(acc.hi, orderKey(hostBits(r.hi)));
            acc.lo = std::min(acc.lo, orderKeyMin(hostBits(r.lo)));
        },
        [](const HostAcc &acc) { return acc.count <= 0xffffffffull && acc.nans <= 0xffffffffull; },
        [](const HostAcc &acc, Record &o) {
            o.sum[0] = uint64_t(acc.sum); o.sum[1] = uint64_t(acc.sum >> 64);
            o.count = uint32_t(acc.count); o.nans = uint32_t(acc.nans);
            o.lo = hostFloat(keyBitsMin(acc.lo)); o.hi = hostFloat(keyBits(acc.hi));
        });
}

extern "C" sgz_status sgz_overview_power_readout(const sgz_overview_power_record *in, size_t count, double *mean_square, float *rms, float *lo, float *hi)
{
    if (!in && count) return fail(SGZ_EINVAL, "sgz_overview_power_readout: null records");
    if (!mean_square && !rms && !lo && !hi) return fail(SGZ_EINVAL, "sgz_overview_power_readout: the mean squares, the rms values, the least, the greatest or any of them");
    for (size_t i = 0; i < count; ++i) {
        const Record &r = in[i];
        if (mean_square) mean_square[i] = r.count ? powerMeanSquare(r.sum[0], r.sum[1], r.count) * (1.0 / kQuantum) : std::nan("");
        if (rms) { const uint32_t bits = powerRmsBits(r.sum[0], r.sum[1], r.count); std::memcpy(rms + i, &bits, sizeof bits); }
        if (lo) lo[i] = r.lo;
        if (hi) hi[i] = r.hi;
    }
    return SGZ_OK;
}

// the level of every record by the plan's HOST tables: dbMap of decay_body.hpp restated with std::log(float), which is what that function
// reproduces bit for bit (its comment); in [columns][pairs][sides][P], both sides under slopeMap[i]
extern "C" sgz_status sgz_overview_power_levels(const sgz_plan *plan, const sgz_overview_power_record *in, size_t columns, float *levels)
{
    if (!plan || !levels || (!in && columns)) return fail(SGZ_EINVAL, "sgz_overview_power_levels: null argument");
    const Plan &p = plan->impl;
    const DeviceScalars &sc = p.scalars;
    const size_t rows = columns * p.C * size_t(p.sides);
    for (size_t row = 0; row < rows; ++row)
        for (uint32_t i = 0; i < p.P; ++i) {
            const Record &r = in[row * p.P + i];
            uint32_t bits = 0x7fc00000u;
            if (r.count) {
                const float rms = hostFloat(powerRmsBits(r.sum[0], r.sum[1], r.count));
                const float deltaX = p.slope[i] * rms * sc.minFracRecip;
                const float level = deltaX > 0.f ? std::log(deltaX) * sc.deltaYRecip : sc.lowerClip;
                bits = hostBits(level);
            }
            levels[row * p.P + i] = hostFloat(bits);
        }
    return SGZ_OK;
}
