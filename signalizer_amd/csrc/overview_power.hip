// overview_power.hip -- the power overview: mean-square spectrum of k frames per image column (sgz.h, "The power overview").  gfx950 only.
// The third reduction over the overview's columns, of the mapped magnitudes M [frames][pairs][sides][P] that K_A leaves in HBM -- the values
// from before the decay and the dB map, so that the mean is a power-domain mean and no K_B launch and no decay state take part:
//   q(x) = rint(x^2 2^60) clamped to 2^64 - 2^11, a NaN left out and counted; per (column, pair, side, pixel) the record
//   { sum[2] = the 128-bit sum of q, count, nans, lo, hi }  -- integers and an order's extremes, so every field folds associatively and
//   commutatively and any split of the frames (slices, calls, slabs, feeds) gives the same bytes;
//   rms = (float)(sqrt(S / count) 2^-30), S = (double)sum[1] 2^64 + (double)sum[0];  level = dbMap(slopeMap[i], rms) of decay_body.hpp (called,
//   not copied) -- K_B's line result for a frame of magnitude rms from a zero decay state;  the pixel is blendColour / toRgba8 at side 0's level.
// The kernels keep an accumulator: the sum as unsigned __int128 (level_columns.hip's way), the counts, hi as a key (0: no value yet) and lo as
// key - 1 (0xFFFFFFFF: no value yet; order_key.hpp), and turn it into a record where it leaves the registers.  The three shapes of
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

using namespace sgz;

static_assert(sizeof(sgz_overview_power_record) == 32 && alignof(sgz_overview_power_record) == 8, "sgz_overview_power_record: 32 bytes, 8-aligned");
static_assert(offsetof(sgz_overview_power_record, sum) == 0 && offsetof(sgz_overview_power_record, count) == 16 &&
              offsetof(sgz_overview_power_record, nans) == 20 && offsetof(sgz_overview_power_record, lo) == 24 &&
              offsetof(sgz_overview_power_record, hi) == 28, "sgz_overview_power_record: the layout sgz.h documents");

namespace {

using Record = sgz_overview_power_record;
typedef unsigned __int128 u128;

constexpr int kOvThreads = 256;
constexpr int kOvUnroll = 8;             // frames (or slices, or source columns) whose loads are issued before the first update
constexpr uint32_t kOvMaxSlices = 64;
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
    const float rms = float(std::sqrt(ms) * kRmsScale);
    uint32_t bits;
    std::memcpy(&bits, &rms, sizeof bits);
    return bits;
#endif
}

// ---- the accumulator ---------------------------------------------------------------------------------------------------------------------
struct Acc {
    u128 sum = 0;
    uint32_t count = 0, nans = 0;
    uint32_t hi = 0u;                    // the greatest orderKey; 0: no value yet
    uint32_t lo = 0xffffffffu;           // the least orderKeyMin; 0xFFFFFFFF: no value yet
};

__device__ __forceinline__ void accFrame(Acc &a, uint32_t bits)
{
    const uint32_t key = orderKey(bits);                         // 0 for a NaN: it moves neither hi nor, as key - 1 = 0xFFFFFFFF, lo
    const bool nan = key == 0u;
    const uint64_t q = powerQuantise(__uint_as_float(bits));
    a.sum += u128(nan ? 0ull : q);
    a.count += nan ? 0u : 1u;
    a.nans += nan ? 1u : 0u;
    a.hi = max(a.hi, key);
    a.lo = min(a.lo, key - 1u);
}

// field-wise: a record without values carries NaNs in lo and hi, whose keys are the two empty markers
__device__ __forceinline__ void accFold(Acc &a, const Record &r)
{
    a.sum += (u128(r.sum[1]) << 64) | u128(r.sum[0]);
    a.count += r.count;
    a.nans += r.nans;
    a.hi = max(a.hi, orderKey(__float_as_uint(r.hi)));
    a.lo = min(a.lo, orderKeyMin(__float_as_uint(r.lo)));
}

__device__ __forceinline__ Record accRecord(const Acc &a)
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
__device__ __forceinline__ Words loadWords(const Record *p)
{
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    return Words{{q[0], q[1]}};
}
__device__ __forceinline__ Record wordsRecord(const Words &x)
{
    Record r;
    r.sum[0] = uint64_t(x.w[0].x) | (uint64_t(x.w[0].y) << 32);
    r.sum[1] = uint64_t(x.w[0].z) | (uint64_t(x.w[0].w) << 32);
    r.count = x.w[1].x; r.nans = x.w[1].y;
    r.lo = __uint_as_float(x.w[1].z); r.hi = __uint_as_float(x.w[1].w);
    return r;
}
__device__ __forceinline__ void storeRecord(Record *p, const Record &r)
{
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(uint32_t(r.sum[0]), uint32_t(r.sum[0] >> 32), uint32_t(r.sum[1]), uint32_t(r.sum[1] >> 32));
    q[1] = make_uint4(r.count, r.nans, __float_as_uint(r.lo), __float_as_uint(r.hi));
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
struct PowerOut {
    uint32_t C, P, SP;                   // pairs, pixels, sides * P: the values of one (frame, pair), and a thread's index among them
    uchar4 *rgba;                        // [columns][P] or null
    Record *power;                       // [columns][C][sides][P] or null
    float *levels;                       // [columns][C][sides][P] or null
    const float *slope;                  // [P]
    const float *colourTables;
    DeviceScalars sc;
};

// a closed column of thread j = side * P + pixel: the records, the levels and -- side 0 -- the blend at the levels in pair order
template <typename AccOf>
__device__ __forceinline__ void emitClosed(const PowerOut &o, long col, uint32_t j, AccOf accOf)
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

// ---- the direct form: k frames of mapped magnitudes per column -------------------------------------------------------------------------------
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

// frames [a, b) of this call that belong to column `col`
__device__ __forceinline__ void columnFrames(const PowerParams &prm, long col, long &a, long &b)
{
    a = col * long(prm.k) - long(prm.held);
    b = a + long(prm.k);
    a = a < 0 ? 0 : a;
    b = b > prm.frames ? prm.frames : b;
}

// the accumulator of (pair, j) over frames [a, b), independent loads first
__device__ __forceinline__ Acc framesAcc(const PowerParams &prm, long a, long b, uint32_t pair, uint32_t j)
{
    const size_t perFrame = size_t(prm.out.C) * prm.out.SP;
    const uint32_t *row = reinterpret_cast<const uint32_t *>(prm.mapped) + size_t(pair) * prm.out.SP + j;
    Acc acc;
    for (long f = a; f < b; f += kOvUnroll) {
        uint32_t bits[kOvUnroll];
#pragma unroll
        for (int u = 0; u < kOvUnroll; ++u) bits[u] = f + u < b ? row[size_t(f + u) * perFrame] : 0xffffffffu;
#pragma unroll
        for (int u = 0; u < kOvUnroll; ++u) accFrame(acc, bits[u]);
    }
    // the last batch was filled up with NaNs, which moved nothing but their count
    const long n = b > a ? b - a : 0;
    acc.nans -= uint32_t((kOvUnroll - n % kOvUnroll) % kOvUnroll);
    return acc;
}

// what a (column, j) does with its accumulators: the carry into column 0, then a closed column's outputs or the open one's carry
template <typename AccOf>
__device__ __forceinline__ void emitColumn(const PowerParams &prm, long col, uint32_t j, AccOf accOf)
{
    const auto withCarry = [&](uint32_t pair) {
        Acc acc = accOf(pair);
        if (col == 0 && prm.held) accFold(acc, wordsRecord(loadWords(prm.carryIn + size_t(pair) * prm.out.SP + j)));
        return acc;
    };
    if (col < prm.closed) { emitClosed(prm.out, col, j, withCarry); return; }
    for (uint32_t pair = 0; pair < prm.out.C; ++pair) storeRecord(prm.carryOut + size_t(pair) * prm.out.SP + j, accRecord(withCarry(pair)));
}

__global__ void __launch_bounds__(kOvThreads)
overviewPowerColumnsKernel(const PowerParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t j = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (j >= prm.out.SP) return;
    long a, b;
    columnFrames(prm, col, a, b);
    emitColumn(prm, col, j, [&](uint32_t pair) { return framesAcc(prm, a, b, pair, j); });
}

// slice blockIdx.y of every column's frames (an empty slice -- more slices than frames -- leaves an empty record)
__global__ void __launch_bounds__(kOvThreads)
overviewPowerSliceKernel(const PowerParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t j = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (j >= prm.out.SP) return;
    long a, b;
    columnFrames(prm, col, a, b);
    const long n = b > a ? b - a : 0, per = (n + long(prm.slices) - 1) / long(prm.slices);
    const long sa = a + long(blockIdx.y) * per, sb = sa + per < b ? sa + per : b;
    for (uint32_t pair = 0; pair < prm.out.C; ++pair)
        storeRecord(prm.partial + ((size_t(blockIdx.y) * size_t(prm.columns) + size_t(col)) * prm.out.C + pair) * prm.out.SP + j,
                    accRecord(framesAcc(prm, sa, sb, pair, j)));
}

__global__ void __launch_bounds__(kOvThreads)
overviewPowerEmitKernel(const PowerParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t j = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (j >= prm.out.SP) return;
    const size_t perSlice = size_t(prm.columns) * prm.out.C * prm.out.SP;
    emitColumn(prm, col, j, [&](uint32_t pair) {
        return foldRecords(prm.partial + (size_t(col) * prm.out.C + pair) * prm.out.SP + j, perSlice, long(prm.slices));
    });
}

// ---- the view of kept records (sgz.h, "The power overview") --------------------------------------------------------------------------------
// records [n][pairs][sides][P] as any power call writes them; output column b is the fold of source columns ceil(b m / cols) <= j < ceil((b + 1)
// m / cols) of the range, m = x1 - x0 -- the boundary rule of the view of kept peaks, and a fold of folds, hence the bytes of the direct call
// wherever the boundaries coincide.
struct PowerViewParams {
    const Record *src;                   // [m][C][sides][P]: the range's first source column
    long m, cols;
    uint32_t blocks, slices;
    Record *partial;                     // [slices][cols][C][sides][P]
    PowerOut out;
};

// source columns [a, b) of output column `col`, relative to the range (m < 2^31 and col <= cols <= m: the products fit)
__device__ __forceinline__ void viewColumns(const PowerViewParams &prm, long col, long &a, long &b)
{
    a = (col * prm.m + prm.cols - 1) / prm.cols;
    b = ((col + 1) * prm.m + prm.cols - 1) / prm.cols;
}

__device__ __forceinline__ Acc viewAcc(const PowerViewParams &prm, long a, long b, uint32_t pair, uint32_t j)
{
    const size_t perColumn = size_t(prm.out.C) * prm.out.SP;
    return foldRecords(prm.src + size_t(a) * perColumn + size_t(pair) * prm.out.SP + j, perColumn, b > a ? b - a : 0);
}

__global__ void __launch_bounds__(kOvThreads)
overviewPowerViewKernel(const PowerViewParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t j = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (j >= prm.out.SP) return;
    long a, b;
    viewColumns(prm, col, a, b);
    emitClosed(prm.out, col, j, [&](uint32_t pair) { return viewAcc(prm, a, b, pair, j); });
}

// slice blockIdx.y of every output column's source columns (an empty slice leaves an empty record)
__global__ void __launch_bounds__(kOvThreads)
overviewPowerViewSliceKernel(const PowerViewParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t j = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (j >= prm.out.SP) return;
    long a, b;
    viewColumns(prm, col, a, b);
    const long per = (b - a + long(prm.slices) - 1) / long(prm.slices);
    const long sa = a + long(blockIdx.y) * per, sb = sa + per < b ? sa + per : b;
    for (uint32_t pair = 0; pair < prm.out.C; ++pair)
        storeRecord(prm.partial + ((size_t(blockIdx.y) * size_t(prm.cols) + size_t(col)) * prm.out.C + pair) * prm.out.SP + j,
                    accRecord(viewAcc(prm, sa, sb, pair, j)));
}

__global__ void __launch_bounds__(kOvThreads)
overviewPowerViewEmitKernel(const PowerViewParams prm)
{
    const long col = long(blockIdx.x / prm.blocks);
    const uint32_t j = (blockIdx.x % prm.blocks) * kOvThreads + threadIdx.x;
    if (j >= prm.out.SP) return;
    const size_t perSlice = size_t(prm.cols) * prm.out.C * prm.out.SP;
    emitClosed(prm.out, col, j, [&](uint32_t pair) {
        return foldRecords(prm.partial + (size_t(col) * prm.out.C + pair) * prm.out.SP + j, perSlice, long(prm.slices));
    });
}

constexpr size_t kRecordFloats = sizeof(Record) / sizeof(float);     // plan scratch is counted in floats (ensureCap)

PowerOut powerOut(const Plan &p, uint8_t *d_rgba, Record *d_power, float *d_levels)
{
    PowerOut o{};
    o.C = p.C; o.P = p.P; o.SP = uint32_t(p.sides) * p.P;
    o.rgba = reinterpret_cast<uchar4 *>(d_rgba); o.power = d_power; o.levels = d_levels;
    o.slope = p.d_slope; o.colourTables = p.d_colourTables; o.sc = p.scalars;
    return o;
}

sgz_status uploaded(Plan &p)                                         // the kernels read the plan's slope map and colour tables
{
    if (p.uploaded) return SGZ_OK;
    std::string err;
    const sgz_status st = uploadPlan(p, err);
    return st == SGZ_OK ? st : fail(st, err);
}

// host: the accumulator of sgz_overview_power_fold, with counts wide enough to see them pass 2^32 - 1
struct HostAcc { u128 sum = 0; uint64_t count = 0, nans = 0; uint32_t hi = 0u, lo = 0xffffffffu; };
uint32_t hostBits(float v) { uint32_t bits; std::memcpy(&bits, &v, sizeof bits); return bits; }
float hostFloat(uint32_t bits) { float v; std::memcpy(&v, &bits, sizeof v); return v; }

}  // namespace

namespace sgz {

// sgz_stage_overview_power behind its argument checks (the plan's tables are uploaded).  d_mapped [frames][C][sides][P] float.
sgz_status runOverviewPowerColumns(Plan &p, const float *d_mapped, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                   sgz_overview_power_record *d_carry, uint8_t *d_rgba, sgz_overview_power_record *d_power, float *d_levels,
                                   hipStream_t stream)
{
    const uint64_t t = uint64_t(held) + frames;
    const uint64_t closed = t / k + ((flush && t % k) ? 1u : 0u);
    const bool open = !flush && t % k != 0;
    const uint64_t columns = closed + (open ? 1u : 0u);
    if (frames == 0 && !(flush && held)) return SGZ_OK;          // nothing arrives and no column to flush
    const uint32_t sp = uint32_t(p.sides) * p.P;
    const uint32_t blocks = (sp + kOvThreads - 1) / kOvThreads;
    if (columns == 0 || blocks == 0) return SGZ_OK;
    if (columns > 0x7fffffffull / blocks || frames > size_t(0x7fffffffffffffffll)) return fail(SGZ_EINVAL, "too many columns for one launch");
    PowerParams prm{};
    prm.mapped = d_mapped;
    prm.frames = long(frames); prm.columns = long(columns); prm.closed = long(closed);
    prm.k = k; prm.held = held; prm.blocks = blocks;
    prm.carryIn = d_carry; prm.carryOut = d_carry;
    prm.out = powerOut(p, d_rgba, d_power, d_levels);
    if (held && open && columns > 1) {
        // column 0's threads read the carry while the open column's threads write it: they read a snapshot
        const size_t carryN = size_t(p.C) * sp;
        if (sgz_status st = ensureCap(&p.ov[kOvPower].d_carryCopy, &p.ov[kOvPower].carryCopyCap, carryN * kRecordFloats); st != SGZ_OK) return st;
        SGZ_HIP(hipMemcpyAsync(p.ov[kOvPower].d_carryCopy, d_carry, carryN * sizeof(Record), hipMemcpyDeviceToDevice, stream));
        prm.carryIn = reinterpret_cast<const Record *>(p.ov[kOvPower].d_carryCopy);
    }
    prm.slices = slices ? slices : overviewAutoSlices(long(columns), blocks, k, frames, numCUs());
    const dim3 grid(unsigned(columns * blocks));
    if (prm.slices <= 1) {
        hipLaunchKernelGGL(overviewPowerColumnsKernel, grid, dim3(kOvThreads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
        return SGZ_OK;
    }
    if (sgz_status st = ensureCap(&p.ov[kOvPower].d_partial, &p.ov[kOvPower].partialCap, size_t(prm.slices) * size_t(columns) * p.C * sp * kRecordFloats); st != SGZ_OK) return st;
    prm.partial = reinterpret_cast<Record *>(p.ov[kOvPower].d_partial);
    hipLaunchKernelGGL(overviewPowerSliceKernel, dim3(grid.x, prm.slices), dim3(kOvThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(overviewPowerEmitKernel, grid, dim3(kOvThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

// sgz_stage_overview_power_view behind its argument checks (the plan's tables are uploaded).  d_src [m][C][sides][P]: the range's first source column.
sgz_status runOverviewPowerView(Plan &p, const sgz_overview_power_record *d_src, size_t m, size_t cols, uint32_t slices, uint8_t *d_rgba,
                                sgz_overview_power_record *d_powerOut, float *d_levels, hipStream_t stream)
{
    const uint32_t sp = uint32_t(p.sides) * p.P;
    const uint32_t blocks = (sp + kOvThreads - 1) / kOvThreads;
    if (cols == 0 || blocks == 0) return SGZ_OK;
    if (cols > 0x7fffffffull / blocks) return fail(SGZ_EINVAL, "too many columns for one launch");
    PowerViewParams prm{};
    prm.src = d_src; prm.m = long(m); prm.cols = long(cols); prm.blocks = blocks;
    prm.out = powerOut(p, d_rgba, d_powerOut, d_levels);
    const uint32_t most = uint32_t((m + cols - 1) / cols);       // source columns of the longest output column
    // the rule of the view of kept peaks (overview.hip runOverviewView)
    prm.slices = slices ? slices : std::min(overviewAutoSlices(long(cols), blocks, most, m, 2 * numCUs()), std::max(1u, most / uint32_t(kOvUnroll)));
    const dim3 grid(unsigned(cols * blocks));
    if (prm.slices <= 1) {
        hipLaunchKernelGGL(overviewPowerViewKernel, grid, dim3(kOvThreads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
        return SGZ_OK;
    }
    if (sgz_status st = ensureCap(&p.ov[kOvPower].d_partial, &p.ov[kOvPower].partialCap, size_t(prm.slices) * cols * p.C * sp * kRecordFloats); st != SGZ_OK) return st;
    prm.partial = reinterpret_cast<Record *>(p.ov[kOvPower].d_partial);
    hipLaunchKernelGGL(overviewPowerViewSliceKernel, dim3(grid.x, prm.slices), dim3(kOvThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(overviewPowerViewEmitKernel, grid, dim3(kOvThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
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
    const uint64_t t = uint64_t(held) + frames;
    if (!d_carry && (held || (!flush && t % k))) return fail(SGZ_EINVAL, "sgz_stage_overview_power: d_carry is read (held > 0) or written (frames stay open)");
    if (frames == 0 && !(flush && held)) return SGZ_OK;
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
    if (!in || !out) return fail(SGZ_EINVAL, "sgz_overview_power_fold: null argument");
    if (width == 0) return fail(SGZ_EINVAL, "sgz_overview_power_fold: width >= 1 records per column");
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
                    acc.sum += (u128(r.sum[1]) << 64) | u128(r.sum[0]);
                    acc.count += r.count; acc.nans += r.nans;
                    acc.hi = std::max(acc.hi, orderKey(hostBits(r.hi)));
                    acc.lo = std::min(acc.lo, orderKeyMin(hostBits(r.lo)));
                }
                if (acc.count > 0xffffffffull || acc.nans > 0xffffffffull)
                    return fail(SGZ_EINVAL, "sgz_overview_power_fold: a folded column counts more than 2^32 - 1 frames");
                if (pass == 0) continue;
                Record &o = out[b * width + i];
                o.sum[0] = uint64_t(acc.sum); o.sum[1] = uint64_t(acc.sum >> 64);
                o.count = uint32_t(acc.count); o.nans = uint32_t(acc.nans);
                o.lo = hostFloat(keyBitsMin(acc.lo)); o.hi = hostFloat(keyBits(acc.hi));
            }
        }
    return SGZ_OK;
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
