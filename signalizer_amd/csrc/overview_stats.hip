// overview_stats.hip -- the mean overview: mean and range of k frames of line results per image column (sgz.h, "The mean overview").  gfx950
// only.  The reduction beside overview.hip's peak hold, over the same line results and the same columns:
//   q(x) = rint(x 2^20) clamped to +-(2^31 - 1), a NaN left out and counted; per (column, pair, pixel) the record
//   { sum = sum of q, count, nans, lo, hi }  -- integers and an order's extremes, so every field folds associatively and commutatively
//   and any split of the frames (slices, calls, slabs, feeds) gives the same bytes;  mean = (float)((double)sum / (double)count 2^-20);
//   the pixel is blendColour / toRgba8 of decay_body.hpp at the mean (called, not copied).
// The kernels keep an accumulator: the sum, the counts, hi as a key (0: no value yet) and lo as key - 1 (0xFFFFFFFF: no value yet;
// order_key.hpp), and turn it into a record where it leaves the registers.  The three shapes of overview.hip, for its reasons:
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

using namespace sgz;

static_assert(sizeof(sgz_overview_stat_record) == 24 && alignof(sgz_overview_stat_record) == 8, "sgz_overview_stat_record: 24 bytes, 8-aligned");
static_assert(offsetof(sgz_overview_stat_record, sum) == 0 && offsetof(sgz_overview_stat_record, count) == 8 &&
              offsetof(sgz_overview_stat_record, nans) == 12 && offsetof(sgz_overview_stat_record, lo) == 16 &&
              offsetof(sgz_overview_stat_record, hi) == 20, "sgz_overview_stat_record: the layout sgz.h documents");

namespace {

using Record = sgz_overview_stat_record;

constexpr int kOvThreads = 256;
constexpr int kOvUnroll = 8;             // frames (or slices, or source columns) whose loads are issued before the first update
constexpr uint32_t kOvMaxSlices = 64;
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
    uint32_t bits;
    std::memcpy(&bits, &mean, sizeof bits);
    return bits;
#endif
}

// ---- the accumulator ---------------------------------------------------------------------------------------------------------------------
struct Acc {
    long long sum = 0;
    uint32_t count = 0, nans = 0;
    uint32_t hi = 0u;                    // the greatest orderKey; 0: no value yet
    uint32_t lo = 0xffffffffu;           // the least orderKeyMin; 0xFFFFFFFF: no value yet
};

__device__ __forceinline__ void accFrame(Acc &a, uint32_t bits)
{
    const uint32_t key = orderKey(bits);                         // 0 for a NaN: it moves neither hi nor, as key - 1 = 0xFFFFFFFF, lo
    const bool nan = key == 0u;
    a.sum += nan ? 0ll : (long long)statQuantise(__uint_as_float(bits));
    a.count += nan ? 0u : 1u;
    a.nans += nan ? 1u : 0u;
    a.hi = max(a.hi, key);
    a.lo = min(a.lo, key - 1u);
}

// field-wise: a record without values carries NaNs in lo and hi, whose keys are the two empty markers
__device__ __forceinline__ void accFold(Acc &a, const Record &r)
{
    a.sum += r.sum;
    a.count += r.count;
    a.nans += r.nans;
    a.hi = max(a.hi, orderKey(__float_as_uint(r.hi)));
    a.lo = min(a.lo, orderKeyMin(__float_as_uint(r.lo)));
}

__device__ __forceinline__ Record accRecord(const Acc &a)
{
    Record r;
    r.sum = a.sum; r.count = a.count; r.nans = a.nans;
    r.lo = __uint_as_float(keyBitsMin(a.lo));
    r.hi = __uint_as_float(keyBits(a.hi));
    return r;
}

// a record as three 8-byte words, for loads that are issued together (the compiler merges the last two: dwordx2 + dwordx4)
struct Words { uint2 w[3]; };
__device__ __forceinline__ Words loadWords(const Record *p)
{
    const uint2 *q = reinterpret_cast<const uint2 *>(p);
    return Words{{q[0], q[1], q[2]}};
}
__device__ __forceinline__ Record wordsRecord(const Words &x)
{
    Record r;
    r.sum = (long long)((unsigned long long)x.w[0].x | ((unsigned long long)x.w[0].y << 32));
    r.count = x.w[1].x; r.nans = x.w[1].y;
    r.lo = __uint_as_float(x.w[2].x); r.hi = __uint_as_float(x.w[2].y);
    return r;
}
__device__ __forceinline__ void storeRecord(Record *p, const Record &r)
{
    uint2 *q = reinterpret_cast<uint2 *>(p);
    q[0] = make_uint2(uint32_t((unsigned long long)r.sum), uint32_t((unsigned long long)r.sum >> 32));
    q[1] = make_uint2(r.count, r.nans);
    q[2] = make_uint2(__float_as_uint(r.lo), __float_as_uint(r.hi));
}

// the fold of `n` records `stride` apart, independent loads first
__device__ __forceinline__ Acc foldRecords(const Record *first, size_t stride, long n)
{
    Acc acc;
    for (long j = 0; j < n; j += kOvUnroll) {
        Words x[kOvUnroll];
#pragma unroll
        for (int u = 0; u < kOvUnroll; ++u)
            if (j + u < n) x[u] = loadWords(first + size_t(j + u) * stride);
#pragma unroll
        for (int u = 0; u < kOvUnroll; ++u)
            if (j + u < n) accFold(acc, wordsRecord(x[u]));
    }
    return acc;
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

// a closed column of a pixel: the records, the means and the blend at the means in pair order
template <typename AccOf>
__device__ __forceinline__ void emitClosed(const StatsOut &o, long col, uint32_t pixel, AccOf accOf)
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

// ---- the direct form: k frames of line results per column ------------------------------------------------------------------------------------
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

// frames [a, b) of this call that belong to column `col`
__device__ __forceinline__ void columnFrames(const StatsParams &prm, long col, long &a, long &b)
{
    a = col * long(prm.k) - long(prm.held);
    b = a + long(prm.k);
    a = a < 0 ? 0 : a;
    b = b > prm.frames ? prm.frames : b;
}

// the accumulator of (pair, pixel) over frames [a, b): graph 0's row of every frame, independent loads first
__device__ __forceinline__ Acc framesAcc(const StatsParams &prm, long a, long b, uint32_t pair, uint32_t pixel)
{
    const size_t perFrame = size_t(prm.out.C) * G * prm.out.P;
    const float2 *row = prm.lines + size_t(pair) * G * prm.out.P + pixel;
    Acc acc;
    for (long f = a; f < b; f += kOvUnroll) {
        uint32_t bits[kOvUnroll];
#pragma unroll
        for (int j = 0; j < kOvUnroll; ++j) bits[j] = f + j < b ? __float_as_uint(row[size_t(f + j) * perFrame].x) : 0xffffffffu;
#pragma unroll
        for (int j = 0; j < kOvUnroll; ++j) accFrame(acc, bits[j]);
    }
    // the last batch was filled up with NaNs, which moved nothing but their count
    const long n = b > a ? b - a : 0;
    acc.nans -= uint32_t((kOvUnroll - n % kOvUnroll) % kOvUnroll);
    return acc;
}

// what a (column, pixel) does with its accumulators: the carry into column 0, then a closed column's outputs or the open one's carry
template <typename AccOf>
__device__ __forceinline__ void emitColumn(const StatsParams &prm, long col, uint32_t pixel, AccOf accOf)
{
    const auto withCarry = [&](uint32_t pair) {
        Acc acc = accOf(pair);
        if (col == 0 && prm.held) accFold(acc, wordsRecord(loadWords(prm.carryIn + size_t(pair) * prm.out.P + pixel)));
        return acc;
    };
    if (col < prm.closed) { emitClosed(prm.out, col, pixel, withCarry); return; }
    for (uint32_t pair = 0; pair < prm.out.C; ++pair) storeRecord(prm.carryOut + size_t(pair) * prm.out.P + pixel, accRecord(withCarry(pair)));
}

__global__ void __launch_bounds__(kOvThreads)
overviewStatsColumnsKernel(const StatsParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t pixel = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (pixel >= prm.out.P) return;
    long a, b;
    columnFrames(prm, col, a, b);
    emitColumn(prm, col, pixel, [&](uint32_t pair) { return framesAcc(prm, a, b, pair, pixel); });
}

// slice blockIdx.y of every column's frames (an empty slice -- more slices than frames -- leaves an empty record)
__global__ void __launch_bounds__(kOvThreads)
overviewStatsSliceKernel(const StatsParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t pixel = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (pixel >= prm.out.P) return;
    long a, b;
    columnFrames(prm, col, a, b);
    const long n = b > a ? b - a : 0, per = (n + long(prm.slices) - 1) / long(prm.slices);
    const long sa = a + long(blockIdx.y) * per, sb = sa + per < b ? sa + per : b;
    for (uint32_t pair = 0; pair < prm.out.C; ++pair)
        storeRecord(prm.partial + ((size_t(blockIdx.y) * size_t(prm.columns) + size_t(col)) * prm.out.C + pair) * prm.out.P + pixel,
                    accRecord(framesAcc(prm, sa, sb, pair, pixel)));
}

__global__ void __launch_bounds__(kOvThreads)
overviewStatsEmitKernel(const StatsParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t pixel = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (pixel >= prm.out.P) return;
    const size_t perSlice = size_t(prm.columns) * prm.out.C * prm.out.P;
    emitColumn(prm, col, pixel, [&](uint32_t pair) {
        return foldRecords(prm.partial + (size_t(col) * prm.out.C + pair) * prm.out.P + pixel, perSlice, long(prm.slices));
    });
}

// ---- the view of kept records (sgz.h, "The mean overview") ---------------------------------------------------------------------------------
// records [n][pairs][P] as any stats call writes them; output column b is the fold of source columns ceil(b m / cols) <= j < ceil((b + 1) m /
// cols) of the range, m = x1 - x0 -- the boundary rule of the view of kept peaks, and a fold of folds, hence the bytes of the direct call
// wherever the boundaries coincide.
struct StatsViewParams {
    const Record *src;                   // [m][C][P]: the range's first source column
    long m, cols;
    uint32_t blocks, slices;
    Record *partial;                     // [slices][cols][C][P]
    StatsOut out;
};

// source columns [a, b) of output column `col`, relative to the range (m < 2^31 and col <= cols <= m: the products fit)
__device__ __forceinline__ void viewColumns(const StatsViewParams &prm, long col, long &a, long &b)
{
    a = (col * prm.m + prm.cols - 1) / prm.cols;
    b = ((col + 1) * prm.m + prm.cols - 1) / prm.cols;
}

__device__ __forceinline__ Acc viewAcc(const StatsViewParams &prm, long a, long b, uint32_t pair, uint32_t pixel)
{
    const size_t perColumn = size_t(prm.out.C) * prm.out.P;
    return foldRecords(prm.src + size_t(a) * perColumn + size_t(pair) * prm.out.P + pixel, perColumn, b > a ? b - a : 0);
}

__global__ void __launch_bounds__(kOvThreads)
overviewStatsViewKernel(const StatsViewParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t pixel = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (pixel >= prm.out.P) return;
    long a, b;
    viewColumns(prm, col, a, b);
    emitClosed(prm.out, col, pixel, [&](uint32_t pair) { return viewAcc(prm, a, b, pair, pixel); });
}

// slice blockIdx.y of every output column's source columns (an empty slice leaves an empty record)
__global__ void __launch_bounds__(kOvThreads)
overviewStatsViewSliceKernel(const StatsViewParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t pixel = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (pixel >= prm.out.P) return;
    long a, b;
    viewColumns(prm, col, a, b);
    const long per = (b - a + long(prm.slices) - 1) / long(prm.slices);
    const long sa = a + long(blockIdx.y) * per, sb = sa + per < b ? sa + per : b;
    for (uint32_t pair = 0; pair < prm.out.C; ++pair)
        storeRecord(prm.partial + ((size_t(blockIdx.y) * size_t(prm.cols) + size_t(col)) * prm.out.C + pair) * prm.out.P + pixel,
                    accRecord(viewAcc(prm, sa, sb, pair, pixel)));
}

__global__ void __launch_bounds__(kOvThreads)
overviewStatsViewEmitKernel(const StatsViewParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t pixel = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (pixel >= prm.out.P) return;
    const size_t perSlice = size_t(prm.cols) * prm.out.C * prm.out.P;
    emitClosed(prm.out, col, pixel, [&](uint32_t pair) {
        return foldRecords(prm.partial + (size_t(col) * prm.out.C + pair) * prm.out.P + pixel, perSlice, long(prm.slices));
    });
}

constexpr size_t kRecordFloats = sizeof(Record) / sizeof(float);     // plan scratch is counted in floats (ensureCap)

StatsOut statsOut(const Plan &p, uint8_t *d_rgba, Record *d_stats, float *d_means)
{
    StatsOut o{};
    o.C = p.C; o.P = p.P;
    o.rgba = reinterpret_cast<uchar4 *>(d_rgba); o.stats = d_stats; o.means = d_means;
    o.colourTables = p.d_colourTables; o.sc = p.scalars;
    return o;
}

sgz_status uploaded(Plan &p)                                         // the kernels read the plan's colour tables
{
    if (p.uploaded) return SGZ_OK;
    std::string err;
    const sgz_status st = uploadPlan(p, err);
    return st == SGZ_OK ? st : fail(st, err);
}

// host: the accumulator of sgz_overview_stats_fold, with counts wide enough to see them pass 2^32 - 1
struct HostAcc { int64_t sum = 0; uint64_t count = 0, nans = 0; uint32_t hi = 0u, lo = 0xffffffffu; };
uint32_t hostBits(float v) { uint32_t bits; std::memcpy(&bits, &v, sizeof bits); return bits; }
float hostFloat(uint32_t bits) { float v; std::memcpy(&v, &bits, sizeof v); return v; }

}  // namespace

namespace sgz {

// sgz_stage_overview_stats behind its argument checks (the plan's tables are uploaded).  d_lines [frames][C][G][P] float2.
sgz_status runOverviewStatsColumns(Plan &p, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                   sgz_overview_stat_record *d_carry, uint8_t *d_rgba, sgz_overview_stat_record *d_stats, float *d_means,
                                   hipStream_t stream)
{
    const uint64_t t = uint64_t(held) + frames;
    const uint64_t closed = t / k + ((flush && t % k) ? 1u : 0u);
    const bool open = !flush && t % k != 0;
    const uint64_t columns = closed + (open ? 1u : 0u);
    if (frames == 0 && !(flush && held)) return SGZ_OK;          // nothing arrives and no column to flush
    const uint32_t blocks = (p.P + kOvThreads - 1) / kOvThreads;
    if (columns == 0 || blocks == 0) return SGZ_OK;
    if (columns > 0x7fffffffull / blocks || frames > size_t(0x7fffffffffffffffll)) return fail(SGZ_EINVAL, "too many columns for one launch");
    StatsParams prm{};
    prm.lines = reinterpret_cast<const float2 *>(d_lines);
    prm.frames = long(frames); prm.columns = long(columns); prm.closed = long(closed);
    prm.k = k; prm.held = held; prm.blocks = blocks;
    prm.carryIn = d_carry; prm.carryOut = d_carry;
    prm.out = statsOut(p, d_rgba, d_stats, d_means);
    if (held && open && columns > 1) {
        // column 0's threads read the carry while the open column's threads write it: they read a snapshot
        const size_t carryN = size_t(p.C) * p.P;
        if (sgz_status st = ensureCap(&p.ov[kOvStats].d_carryCopy, &p.ov[kOvStats].carryCopyCap, carryN * kRecordFloats); st != SGZ_OK) return st;
        SGZ_HIP(hipMemcpyAsync(p.ov[kOvStats].d_carryCopy, d_carry, carryN * sizeof(Record), hipMemcpyDeviceToDevice, stream));
        prm.carryIn = reinterpret_cast<const Record *>(p.ov[kOvStats].d_carryCopy);
    }
    prm.slices = slices ? slices : overviewAutoSlices(long(columns), blocks, k, frames, numCUs());
    const dim3 grid(unsigned(columns * blocks));
    if (prm.slices <= 1) {
        hipLaunchKernelGGL(overviewStatsColumnsKernel, grid, dim3(kOvThreads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
        return SGZ_OK;
    }
    if (sgz_status st = ensureCap(&p.ov[kOvStats].d_partial, &p.ov[kOvStats].partialCap, size_t(prm.slices) * size_t(columns) * p.C * p.P * kRecordFloats); st != SGZ_OK) return st;
    prm.partial = reinterpret_cast<Record *>(p.ov[kOvStats].d_partial);
    hipLaunchKernelGGL(overviewStatsSliceKernel, dim3(grid.x, prm.slices), dim3(kOvThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(overviewStatsEmitKernel, grid, dim3(kOvThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

// sgz_stage_overview_stats_view behind its argument checks (the plan's tables are uploaded).  d_src [m][C][P]: the range's first source column.
sgz_status runOverviewStatsView(Plan &p, const sgz_overview_stat_record *d_src, size_t m, size_t cols, uint32_t slices, uint8_t *d_rgba,
                                sgz_overview_stat_record *d_statsOut, float *d_means, hipStream_t stream)
{
    const uint32_t blocks = (p.P + kOvThreads - 1) / kOvThreads;
    if (cols == 0 || blocks == 0) return SGZ_OK;
    if (cols > 0x7fffffffull / blocks) return fail(SGZ_EINVAL, "too many columns for one launch");
    StatsViewParams prm{};
    prm.src = d_src; prm.m = long(m); prm.cols = long(cols); prm.blocks = blocks;
    prm.out = statsOut(p, d_rgba, d_statsOut, d_means);
    const uint32_t most = uint32_t((m + cols - 1) / cols);       // source columns of the longest output column
    // the rule of the view of kept peaks (overview.hip runOverviewView)
    prm.slices = slices ? slices : std::min(overviewAutoSlices(long(cols), blocks, most, m, 2 * numCUs()), std::max(1u, most / uint32_t(kOvUnroll)));
    const dim3 grid(unsigned(cols * blocks));
    if (prm.slices <= 1) {
        hipLaunchKernelGGL(overviewStatsViewKernel, grid, dim3(kOvThreads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
        return SGZ_OK;
    }
    if (sgz_status st = ensureCap(&p.ov[kOvStats].d_partial, &p.ov[kOvStats].partialCap, size_t(prm.slices) * cols * p.C * p.P * kRecordFloats); st != SGZ_OK) return st;
    prm.partial = reinterpret_cast<Record *>(p.ov[kOvStats].d_partial);
    hipLaunchKernelGGL(overviewStatsViewSliceKernel, dim3(grid.x, prm.slices), dim3(kOvThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(overviewStatsViewEmitKernel, grid, dim3(kOvThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
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
    const uint64_t t = uint64_t(held) + frames;
    if (!d_carry && (held || (!flush && t % k))) return fail(SGZ_EINVAL, "sgz_stage_overview_stats: d_carry is read (held > 0) or written (frames stay open)");
    if (frames == 0 && !(flush && held)) return SGZ_OK;
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
    if (!in || !out) return fail(SGZ_EINVAL, "sgz_overview_stats_fold: null argument");
    if (width == 0) return fail(SGZ_EINVAL, "sgz_overview_stats_fold: width >= 1 records per column");
    uint64_t cols = 0;
    if (sgz_status st = checkViewRange(n, x0, x1, out_columns, &cols); st != SGZ_OK) return st;
    const uint64_t m = x1 - x0;
    // two passes: nothing is written when any column's count overflows
    for (int pass = 0; pass < 2; ++pass)
        for (uint64_t b = 0; b < cols; ++b) {
            const uint64_t ja = x0 + (b * m + cols - 1) / cols, jb = x0 + ((b + 1) * m + cols - 1) / cols;
            for (size_t i = 0; i < width; ++i) {
                HostAcc acc;
                for (uint64_t j = ja; j < jb; ++j) {
                    const Record &r = in[j * width + i];
                    acc.sum = int64_t(uint64_t(acc.sum) + uint64_t(r.sum));
                    acc.count += r.count; acc.nans += r.nans;
                    acc.hi = std::max(acc.hi, orderKey(hostBits(r.hi)));
                    acc.lo = std::min(acc.lo, orderKeyMin(hostBits(r.lo)));
                }
                if (acc.count > 0xffffffffull || acc.nans > 0xffffffffull)
                    return fail(SGZ_EINVAL, "sgz_overview_stats_fold: a folded column counts more than 2^32 - 1 frames");
                if (pass == 0) continue;
                Record &o = out[b * width + i];
                o.sum = acc.sum; o.count = uint32_t(acc.count); o.nans = uint32_t(acc.nans);
                o.lo = hostFloat(keyBitsMin(acc.lo)); o.hi = hostFloat(keyBits(acc.hi));
            }
        }
    return SGZ_OK;
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
