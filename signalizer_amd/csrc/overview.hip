// overview.hip -- the overview image: k frames of line results per image column, reduced and coloured on the device (sgz.h, "The overview
// render").  gfx950 only.  The reference has no counterpart: renderColourSpectrum draws one column per audio frame
// (Source/Spectrum/SpectrumRendering.cpp:696-721); the colouring is its own (decay_body.hpp blendColour / toRgba8, called, not copied).
//   V[c][p][i] = the greatest of L[f][p][0][i].x over the column's frames (graph 0, first component: the value K_B colours from), under a
//   total order -- NaNs take no part, the others compare by the key bits ^ (sign ? 0xFFFFFFFF : 0x80000000) as unsigned, i.e. IEEE order
//   with -0 below +0 -- so that any split of the frames (slices, calls, slabs) gives the same bits.  A group of NaNs alone yields 0x7FC00000.
// The kernels keep KEYS: key 0 is "no value yet" (it is the key of a NaN pattern and of nothing else: -inf's key is 0x007FFFFF), a maximum
// of keys is associative and commutative, and a key turns back into the value's own bits.
//   overviewColumnsKernel   one thread per (column, pixel): pairs outermost (the blend order), the column's frames inside, 8 loads in
//                           flight before the compares; then the carry, the colour, one uchar4 store.
//   overviewSliceKernel     few columns of many frames: slice s of a column's frames -> partial keys [slices][columns][pairs][P] in plan
//   overviewEmitKernel      scratch; then the fold over the slices and the carry, the colour, the store -- a launch of its own behind it on
//                           the stream (no hand-off between workgroups inside a launch).
// The view of kept peaks (overviewViewKernel, overviewViewSliceKernel, overviewViewEmitKernel; further down) is the same reduction on V itself.
// From overview_kinds.hpp: the step of a call, the column / view / slice bounds, a thread's cell, the frames' batched fold, and the launch
// front of both forms (refusal, carry snapshot, slice choice, launches).  The kernel bodies, over keys, are this file's own (why: that header).
// Nothing is waited for; scratch grows on demand (only growth synchronises); everything runs on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "runtime.hpp"
#include "decay_body.hpp"
#include "order_key.hpp"       // orderKey / keyBits

#pragma clang fp contract(off)

#include "overview_kinds.hpp"   // behind the pragma: its templates are parsed without contraction

using namespace sgz;

namespace {

constexpr int kOvThreads = 256;

struct OverviewParams {
    const float2 *lines;                 // [frames][C][G][P]
    long frames;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t k, held, C, P;
    uint32_t blocks;                     // workgroups per column = ceil(P / 256)
    uint32_t slices;
    const float *carryIn;                // [C][P]: V of column 0's `held` earlier frames (read iff held > 0)
    float *carryOut;                     // [C][P]: V of the open column
    uchar4 *rgba;                        // [closed][P] or null
    float *peaks;                        // [closed][C][P] or null
    uint32_t *partial;                   // [slices][columns][C][P] keys
    const float *colourTables;
    DeviceScalars sc;
};

// the peak hold's part in the frames' fold (overview_kinds.hpp, foldFrames): the accumulator is the greatest key; a NaN's key is 0, so the
// fill of the last batch moves nothing
struct PeakKey {
    using Acc = uint32_t;
    static __device__ __forceinline__ void accFrame(Acc &run, uint32_t bits) { run = max(run, orderKey(bits)); }
    static __device__ __forceinline__ void accUnfill(Acc &, uint32_t) {}
};

// the greatest key of (pair, pixel) over frames [a, b): graph 0's row of every frame
__device__ __forceinline__ uint32_t framesKey(const OverviewParams &prm, long a, long b, uint32_t pair, uint32_t pixel)
{
    return foldFrames<PeakKey>(linesRow(prm.lines, prm.C, prm.P, pair, pixel), a, b);
}

// the greatest of a (column, pair, pixel)'s partial keys, `perSlice` apart, independent loads first
__device__ __forceinline__ uint32_t slicesKey(const uint32_t *q, size_t perSlice, uint32_t slices)
{
    uint32_t run = 0u;
    for (uint32_t s = 0; s < slices; s += kOvUnroll) {
        uint32_t key[kOvUnroll];
#pragma unroll
        for (int j = 0; j < kOvUnroll; ++j) key[j] = s + j < slices ? q[size_t(s + j) * perSlice] : 0u;
#pragma unroll
        for (int j = 0; j < kOvUnroll; ++j) run = max(run, key[j]);
    }
    return run;
}

// what a (column, pixel) does with its keys: the carry into column 0, then V to the peaks and the colour blend in pair order (a closed
// column) or to the carry (the open one)
template <typename KeyOf>
__device__ __forceinline__ void emitColumn(const OverviewParams &prm, long col, uint32_t pixel, KeyOf keyOf)
{
    const bool closed = col < prm.closed;
    float cb[3] = {0.f, 0.f, 0.f};
    for (uint32_t pair = 0; pair < prm.C; ++pair) {
        uint32_t key = keyOf(pair);
        if (col == 0 && prm.held) key = max(key, orderKey(__float_as_uint(prm.carryIn[size_t(pair) * prm.P + pixel])));
        const float v = __uint_as_float(keyBits(key));
        if (!closed) { prm.carryOut[size_t(pair) * prm.P + pixel] = v; continue; }
        if (prm.peaks) prm.peaks[(size_t(col) * prm.C + pair) * prm.P + pixel] = v;
        if (prm.rgba) blendColour(cb, v, prm.colourTables + size_t(pair) * NC * 3, prm.sc);
    }
    if (closed && prm.rgba) prm.rgba[size_t(col) * prm.P + pixel] = toRgba8(cb);
}

__global__ void __launch_bounds__(kOvThreads)
overviewColumnsKernel(const OverviewParams prm)
{
    long col;
    uint32_t pixel;
    threadCell<kOvThreads>(prm, col, pixel);
    if (pixel >= prm.P) return;
    long a, b;
    columnFrames(prm, col, a, b);
    emitColumn(prm, col, pixel, [&](uint32_t pair) { return framesKey(prm, a, b, pair, pixel); });
}

// slice blockIdx.y of every column's frames (an empty slice -- more slices than frames -- leaves key 0)
__global__ void __launch_bounds__(kOvThreads)
overviewSliceKernel(const OverviewParams prm)
{
    long col;
    uint32_t pixel;
    threadCell<kOvThreads>(prm, col, pixel);
    if (pixel >= prm.P) return;
    long a, b, sa, sb;
    columnFrames(prm, col, a, b);
    sliceRange(prm, a, b, b > a ? b - a : 0, sa, sb);
    for (uint32_t pair = 0; pair < prm.C; ++pair)
        prm.partial[((size_t(blockIdx.y) * size_t(prm.columns) + size_t(col)) * prm.C + pair) * prm.P + pixel] = framesKey(prm, sa, sb, pair, pixel);
}

__global__ void __launch_bounds__(kOvThreads)
overviewEmitKernel(const OverviewParams prm)
{
    long col;
    uint32_t pixel;
    threadCell<kOvThreads>(prm, col, pixel);
    if (pixel >= prm.P) return;
    const size_t perSlice = size_t(prm.columns) * prm.C * prm.P;
    emitColumn(prm, col, pixel, [&](uint32_t pair) {
        return slicesKey(prm.partial + (size_t(col) * prm.C + pair) * prm.P + pixel, perSlice, prm.slices);
    });
}

// ---- the view of kept peaks (sgz.h, "The view of kept peaks") -------------------------------------------------------------------------------
// V [n][pairs][P] as any overview call writes it; output column b is the greatest, under the same order, of source columns
// ceil(b m / cols) <= j < ceil((b + 1) m / cols) of the range, m = x1 - x0 -- a maximum of maxima, hence the bits of the direct render
// wherever the boundaries coincide.  The same three shapes as above, on [column][pair][P] floats instead of line results:
//   overviewViewKernel        one thread per (output column, pixel), pairs outermost, the column's source columns inside
//   overviewViewSliceKernel   few output columns over many source columns: slice s of every column -> partial keys in plan scratch
//   overviewViewEmitKernel    the fold over the slices, the colour, the store
struct ViewParams {
    const float *src;                    // [m][C][P]: the range's first source column
    long m, cols;
    uint32_t C, P, blocks, slices;
    uchar4 *rgba;                        // [cols][P] or null
    float *peaks;                        // [cols][C][P] or null
    uint32_t *partial;                   // [slices][cols][C][P] keys
    const float *colourTables;
    DeviceScalars sc;
};

// the greatest key of (pair, pixel) over source columns [a, b), independent loads first
__device__ __forceinline__ uint32_t viewKey(const ViewParams &prm, long a, long b, uint32_t pair, uint32_t pixel)
{
    const size_t perColumn = size_t(prm.C) * prm.P;
    const float *row = prm.src + size_t(pair) * prm.P + pixel;
    uint32_t run = 0u;
    for (long j = a; j < b; j += kOvUnroll) {
        uint32_t bits[kOvUnroll];
#pragma unroll
        for (int u = 0; u < kOvUnroll; ++u) bits[u] = j + u < b ? __float_as_uint(row[size_t(j + u) * perColumn]) : 0xffffffffu;
#pragma unroll
        for (int u = 0; u < kOvUnroll; ++u) run = max(run, orderKey(bits[u]));
    }
    return run;
}

template <typename KeyOf>
__device__ __forceinline__ void emitViewColumn(const ViewParams &prm, long col, uint32_t pixel, KeyOf keyOf)
{
    float cb[3] = {0.f, 0.f, 0.f};
    for (uint32_t pair = 0; pair < prm.C; ++pair) {
        const float v = __uint_as_float(keyBits(keyOf(pair)));
        if (prm.peaks) prm.peaks[(size_t(col) * prm.C + pair) * prm.P + pixel] = v;
        if (prm.rgba) blendColour(cb, v, prm.colourTables + size_t(pair) * NC * 3, prm.sc);
    }
    if (prm.rgba) prm.rgba[size_t(col) * prm.P + pixel] = toRgba8(cb);
}

__global__ void __launch_bounds__(kOvThreads)
overviewViewKernel(const ViewParams prm)
{
    long col;
    uint32_t pixel;
    threadCell<kOvThreads>(prm, col, pixel);
    if (pixel >= prm.P) return;
    long a, b;
    viewColumns(prm, col, a, b);
    emitViewColumn(prm, col, pixel, [&](uint32_t pair) { return viewKey(prm, a, b, pair, pixel); });
}

// slice blockIdx.y of every output column's source columns (an empty slice leaves key 0)
__global__ void __launch_bounds__(kOvThreads)
overviewViewSliceKernel(const ViewParams prm)
{
    long col;
    uint32_t pixel;
    threadCell<kOvThreads>(prm, col, pixel);
    if (pixel >= prm.P) return;
    long a, b, sa, sb;
    viewColumns(prm, col, a, b);
    sliceRange(prm, a, b, b - a, sa, sb);
    for (uint32_t pair = 0; pair < prm.C; ++pair)
        prm.partial[((size_t(blockIdx.y) * size_t(prm.cols) + size_t(col)) * prm.C + pair) * prm.P + pixel] = viewKey(prm, sa, sb, pair, pixel);
}

__global__ void __launch_bounds__(kOvThreads)
overviewViewEmitKernel(const ViewParams prm)
{
    long col;
    uint32_t pixel;
    threadCell<kOvThreads>(prm, col, pixel);
    if (pixel >= prm.P) return;
    const size_t perSlice = size_t(prm.cols) * prm.C * prm.P;
    emitViewColumn(prm, col, pixel, [&](uint32_t pair) {
        return slicesKey(prm.partial + (size_t(col) * prm.C + pair) * prm.P + pixel, perSlice, prm.slices);
    });
}

}  // namespace

namespace sgz {
// what every overview call refuses before anything else happens (message in g_lastError)
sgz_status checkOverviewStep(uint32_t k, uint64_t held, uint64_t frames)
{
    if (k == 0) return fail(SGZ_EINVAL, "overview: k >= 1 frames per column");
    if (held >= k) return fail(SGZ_EINVAL, "overview: held < k");
    if (held + frames < frames) return fail(SGZ_EINVAL, "overview: frame count");
    return SGZ_OK;
}

bool bytesOverlap(const void *a, size_t aBytes, const void *b, size_t bBytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a0 < b0 + bBytes && b0 < a0 + aBytes;
}

// The slices of a call that leaves the choice to the library: the smallest count <= min(64, k, frames) with columns x ceil(P / 256) x slices
// >= 2 workgroups per CU.
uint32_t overviewAutoSlices(long columns, uint32_t blocks, uint32_t k, size_t frames, int cus)
{
    const uint64_t unit = uint64_t(columns) * blocks, need = 2 * uint64_t(cus);
    if (unit >= need) return 1u;
    const uint64_t most = std::min<uint64_t>(std::min<uint64_t>(kOvMaxSlices, k), std::max<size_t>(frames, 1));
    return uint32_t(std::min<uint64_t>(most, (need + unit - 1) / unit));
}

// sgz_stage_overview behind its argument checks (the plan's tables are uploaded).  d_lines [frames][C][G][P] float2.
sgz_status runOverviewColumns(Plan &p, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices, float *d_carry,
                              uint8_t *d_rgba, float *d_peaks, hipStream_t stream)
{
    OverviewParams prm{};
    prm.lines = reinterpret_cast<const float2 *>(d_lines);
    prm.C = p.C; prm.P = p.P;
    prm.rgba = reinterpret_cast<uchar4 *>(d_rgba); prm.peaks = d_peaks;
    prm.colourTables = p.d_colourTables; prm.sc = p.scalars;
    return launchOverviewColumns(p, kOvPeaks, prm, frames, k, held, flush, slices, d_carry, p.P, kOvThreads,
                                 [&](uint64_t columns, uint32_t blocks) { return overviewAutoSlices(long(columns), blocks, k, frames, numCUs()); },
                                 overviewColumnsKernel, overviewSliceKernel, overviewEmitKernel, stream);
}

// what every view call refuses about its range (message in g_lastError); *cols = min(out_columns, x1 - x0)
sgz_status checkViewRange(uint64_t n, uint64_t x0, uint64_t x1, uint32_t outColumns, uint64_t *cols)
{
    if (n >= (uint64_t(1) << 31)) return fail(SGZ_EINVAL, "overview view: fewer than 2^31 source columns");
    if (x0 >= x1 || x1 > n) return fail(SGZ_EINVAL, "overview view: x0 < x1 <= n");
    if (outColumns == 0) return fail(SGZ_EINVAL, "overview view: out_columns >= 1");
    *cols = std::min<uint64_t>(outColumns, x1 - x0);
    return SGZ_OK;
}

// sgz_stage_overview_view behind its argument checks (the plan's tables are uploaded).  d_src [m][C][P]: the range's first source column.
sgz_status runOverviewView(Plan &p, const float *d_src, size_t m, size_t cols, uint32_t slices, uint8_t *d_rgba, float *d_peaksOut, hipStream_t stream)
{
    ViewParams prm{};
    prm.src = d_src;
    prm.C = p.C; prm.P = p.P;
    prm.rgba = reinterpret_cast<uchar4 *>(d_rgba); prm.peaks = d_peaksOut;
    prm.colourTables = p.d_colourTables; prm.sc = p.scalars;
    return launchOverviewView(p, kOvPeaks, prm, m, cols, slices, p.P, kOvThreads, overviewViewKernel, overviewViewSliceKernel,
                              overviewViewEmitKernel, stream);
}
}  // namespace sgz

struct sgz_plan { Plan impl; };

extern "C" sgz_status sgz_overview_view_columns(uint64_t n, uint64_t x0, uint64_t x1, uint32_t out_columns, uint64_t *columns, uint64_t *bounds)
{
    if (!columns) return fail(SGZ_EINVAL, "sgz_overview_view_columns: result non-null");
    uint64_t cols = 0;
    if (sgz_status st = checkViewRange(n, x0, x1, out_columns, &cols); st != SGZ_OK) return st;
    *columns = cols;
    const uint64_t m = x1 - x0;
    if (bounds)
        for (uint64_t b = 0; b <= cols; ++b) bounds[b] = x0 + (b * m + cols - 1) / cols;
    return SGZ_OK;
}

extern "C" sgz_status sgz_stage_overview_view(sgz_plan *plan, const float *d_peaks, size_t n, size_t x0, size_t x1, uint32_t out_columns, uint32_t slices,
                                              uint8_t *d_rgba, float *d_peaks_out, void *stream)
{
    if (!plan || !d_peaks) return fail(SGZ_EINVAL, "null argument");
    uint64_t cols = 0;
    if (sgz_status st = checkViewRange(n, x0, x1, out_columns, &cols); st != SGZ_OK) return st;
    if (slices > kOvMaxSlices) return fail(SGZ_EINVAL, "sgz_stage_overview_view: slices 0 (automatic) or 1 .. 64");
    if (!d_rgba && !d_peaks_out) return fail(SGZ_EINVAL, "sgz_stage_overview_view: an image, the peaks or both");
    Plan &p = plan->impl;
    const size_t column = size_t(p.C) * p.P;                     // floats of a source column
    const float *src = d_peaks + x0 * column;
    const size_t srcBytes = (x1 - x0) * column * sizeof(float);
    if (bytesOverlap(src, srcBytes, d_rgba, size_t(cols) * p.P * 4) || bytesOverlap(src, srcBytes, d_peaks_out, size_t(cols) * column * sizeof(float)))
        return fail(SGZ_EINVAL, "sgz_stage_overview_view: an output overlaps the source columns it is made from");
    if (sgz_status st = uploaded(p); st != SGZ_OK) return st;
    return runOverviewView(p, src, x1 - x0, size_t(cols), slices, d_rgba, d_peaks_out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" sgz_status sgz_overview_step(uint32_t k, uint64_t held, uint64_t frames, int flush, uint64_t *columns, uint64_t *held_out)
{
    if (!columns || !held_out) return fail(SGZ_EINVAL, "sgz_overview_step: results non-null");
    if (sgz_status st = checkOverviewStep(k, held, frames); st != SGZ_OK) return st;
    *columns = overviewStepShape(k, held, frames, flush).closed;
    *held_out = flush ? 0u : (held + frames) % k;
    return SGZ_OK;
}

extern "C" sgz_status sgz_stage_overview(sgz_plan *plan, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                         float *d_carry, uint8_t *d_rgba, float *d_peaks, void *stream)
{
    if (!plan || !d_lines) return fail(SGZ_EINVAL, "null argument");
    if (sgz_status st = checkOverviewStep(k, held, frames); st != SGZ_OK) return st;
    if (slices > kOvMaxSlices) return fail(SGZ_EINVAL, "sgz_stage_overview: slices 0 (automatic) or 1 .. 64");
    if (!d_rgba && !d_peaks) return fail(SGZ_EINVAL, "sgz_stage_overview: an image, the peaks or both");
    const OverviewStep sh = overviewStepShape(k, held, frames, flush);
    if (!d_carry && (held || sh.open)) return fail(SGZ_EINVAL, "sgz_stage_overview: d_carry is read (held > 0) or written (frames stay open)");
    if (!sh.launch) return SGZ_OK;
    Plan &p = plan->impl;
    if (sgz_status st = uploaded(p); st != SGZ_OK) return st;
    return runOverviewColumns(p, d_lines, frames, k, held, flush, slices, d_carry, d_rgba, d_peaks, reinterpret_cast<hipStream_t>(stream));
}
