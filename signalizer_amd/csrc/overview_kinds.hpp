// overview_kinds.hpp -- what the overview kinds (peak hold, mean, power, cross, flux, percentile: overview*.hip) have in common, written once:
// the step of a call, the column / view / slice bounds and a thread's cell, the two batched folds and the six kernel bodies of the mean and
// the power overview, the launch front of the direct and the view form, the carry snapshot, and the frame of the host folds.  A kind's file
// holds what is its own: its record, its definition functions, its accumulator, its emitClosed, its named __global__ entry points.
// The peak hold takes the bounds and the launch front and keeps its kernel bodies: its accumulator is a key, plan scratch holds keys where
// the carry and the peaks hold values, and its folds select where the bodies here branch -- through the bodies its sliced form measured
// about 1 us slower.  The percentile kind's bodies (LDS tables, run transfers), cross and flux are their own too.
// A kind's kernel-argument structs keep their own types and layouts; the helpers here are templates on them and read the fields by name:
//   k, held, blocks, slices (uint32_t); frames, columns, closed, m, cols (long); carryIn, carryOut, partial, src, out
// Floating-point contraction: this header neither sets nor resets it.  Every overview*.hip includes it BEHIND its
// `#pragma clang fp contract(off)`, so every template instantiated there was parsed without contraction.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>

#include "runtime.hpp"
#include "decay_body.hpp"      // G: the graphs of a line result

namespace sgz {

constexpr int kOvUnroll = 8;             // frames (or slices, or source columns) whose loads are issued before the first update
constexpr uint32_t kOvMaxSlices = 64;
template <class Record> constexpr size_t kRecordFloats = sizeof(Record) / sizeof(float);        // plan scratch is counted in floats (ensureCap)

// ---- 1. the step of a call (host) ------------------------------------------------------------------------------------------------------------
// Column c of a call covers its frames [c k - held, (c + 1) k - held) clipped to [0, frames): column 0 is the rest of the carried column
// (held > 0), the last one may stay open and goes to the carry.  For arguments that passed checkOverviewStep
struct OverviewStep {
    uint64_t closed, columns;            // columns the call emits; those it touches
    bool open, launch;                   // a last column stays open; anything happens at all (false: nothing arrives and no column to flush)
};

static inline OverviewStep overviewStepShape(uint32_t k, uint64_t held, uint64_t frames, int flush)
{
    OverviewStep sh{};
    const uint64_t t = held + frames;
    sh.closed = t / k + ((flush && t % k) ? 1u : 0u);
    sh.open = !flush && t % k != 0;
    sh.columns = sh.closed + (sh.open ? 1u : 0u);
    sh.launch = !(frames == 0 && !(flush && held));
    return sh;
}

// ---- 2. the bounds (device) ------------------------------------------------------------------------------------------------------------------
// frames [a, b) of this call that belong to column `col`
template <class Params>
__device__ __forceinline__ void columnFrames(const Params &prm, long col, long &a, long &b)
{
    a = col * long(prm.k) - long(prm.held);
    b = a + long(prm.k);
    a = a < 0 ? 0 : a;
    b = b > prm.frames ? prm.frames : b;
}

// source columns [a, b) of output column `col` of a view, relative to the range (m < 2^31 and col <= cols <= m: the products fit)
template <class ViewParams>
__device__ __forceinline__ void viewColumns(const ViewParams &prm, long col, long &a, long &b)
{
    a = (col * prm.m + prm.cols - 1) / prm.cols;
    b = ((col + 1) * prm.m + prm.cols - 1) / prm.cols;
}

// slice blockIdx.y's part [sa, sb) of [a, b), n = its length (a column without frames of this call has b < a: n is the caller's)
template <class Params>
__device__ __forceinline__ void sliceRange(const Params &prm, long a, long b, long n, long &sa, long &sb)
{
    const long per = (n + long(prm.slices) - 1) / long(prm.slices);
    sa = a + long(blockIdx.y) * per;
    sb = sa + per < b ? sa + per : b;
}

// the column of workgroup blockIdx.x and the first of its kThreads cells; a thread's own cell
template <int kThreads, class Params>
__device__ __forceinline__ void blockCells(const Params &prm, long &col, uint32_t &first)
{
    col = long(blockIdx.x / prm.blocks);
    first = (blockIdx.x % prm.blocks) * kThreads;
}
template <int kThreads, class Params>
__device__ __forceinline__ void threadCell(const Params &prm, long &col, uint32_t &cell)
{
    blockCells<kThreads>(prm, col, cell);
    cell += threadIdx.x;
}

// ---- 3. the batched folds (device) -----------------------------------------------------------------------------------------------------------
// A kind K names: Record, Acc (value-initialised to "nothing yet"), Words (a record as loaded), Params, ViewParams (each with `out`: the
// pairs C and what every emitting kernel writes), kThreads, and
//   cells(out)                       the values of one (column, pair): P, or sides * P
//   row(prm, pair, cell)             the cell's values over the call's frames: .bits(f) is frame f's
//   accFrame(acc, bits)              one value (a NaN moves nothing but its count)
//   accUnfill(acc, n)                takes n NaNs out of the count again
//   accFold(acc, record)             a record, field-wise;   accRecord(acc) turns the accumulator into one
//   loadWords, wordsRecord, storeRecord     a record from and to memory
//   emitClosed(out, col, cell, accOf)       a closed column's outputs, accOf(pair) in pair order
// graph 0's first component of line results [frames][C][G][P] float2: the row of the peak hold and the mean overview
struct LinesRow {
    size_t perFrame;
    const float2 *first;
    __device__ __forceinline__ uint32_t bits(long f) const { return __float_as_uint(first[size_t(f) * perFrame].x); }
};
__device__ __forceinline__ LinesRow linesRow(const float2 *lines, uint32_t C, uint32_t P, uint32_t pair, uint32_t pixel)
{
    return LinesRow{size_t(C) * G * P, lines + size_t(pair) * G * P + pixel};
}

// the accumulator of a row over frames [a, b), independent loads first (of K: Acc, accFrame, accUnfill)
template <class K, class Row>
__device__ __forceinline__ typename K::Acc foldFrames(const Row &row, long a, long b)
{
    typename K::Acc acc{};
    for (long f = a; f < b; f += kOvUnroll) {
        uint32_t bits[kOvUnroll];
#pragma unroll
        for (int j = 0; j < kOvUnroll; ++j) bits[j] = f + j < b ? row.bits(f + j) : 0xffffffffu;
#pragma unroll
        for (int j = 0; j < kOvUnroll; ++j) K::accFrame(acc, bits[j]);
    }
    // the last batch was filled up with NaNs, which moved nothing but their count
    const long n = b > a ? b - a : 0;
    K::accUnfill(acc, uint32_t((kOvUnroll - n % kOvUnroll) % kOvUnroll));
    return acc;
}

// the fold of `n` records `stride` apart, independent loads first: the slices of an emit, the source columns of a view, the slices of a view emit
template <class K>
__device__ __forceinline__ typename K::Acc foldRecords(const typename K::Record *first, size_t stride, long n)
{
    typename K::Acc acc{};
    for (long j = 0; j < n; j += kOvUnroll) {
        typename K::Words x[kOvUnroll];
#pragma unroll
        for (int u = 0; u < kOvUnroll; ++u)
            if (j + u < n) x[u] = K::loadWords(first + size_t(j + u) * stride);
#pragma unroll
        for (int u = 0; u < kOvUnroll; ++u)
            if (j + u < n) K::accFold(acc, K::wordsRecord(x[u]));
    }
    return acc;
}

// ---- 4. the six kernel bodies (device) -------------------------------------------------------------------------------------------------------
// what a (column, cell) does with its accumulators: the carry into column 0, then a closed column's outputs or the open one's carry
template <class K, typename AccOf>
__device__ __forceinline__ void emitColumn(const typename K::Params &prm, long col, uint32_t cell, AccOf accOf)
{
    const uint32_t cells = K::cells(prm.out);
    const auto withCarry = [&](uint32_t pair) {
        typename K::Acc acc = accOf(pair);
        if (col == 0 && prm.held) K::accFold(acc, K::wordsRecord(K::loadWords(prm.carryIn + size_t(pair) * cells + cell)));
        return acc;
    };
    if (col < prm.closed) { K::emitClosed(prm.out, col, cell, withCarry); return; }
    for (uint32_t pair = 0; pair < prm.out.C; ++pair) K::storeRecord(prm.carryOut + size_t(pair) * cells + cell, K::accRecord(withCarry(pair)));
}

// one thread per (column, cell): pairs outermost (the blend order), the column's frames inside
template <class K>
__device__ __forceinline__ void overviewColumnsBody(const typename K::Params &prm)
{
    long col, a, b;
    uint32_t cell;
    threadCell<K::kThreads>(prm, col, cell);
    if (cell >= K::cells(prm.out)) return;
    columnFrames(prm, col, a, b);
    emitColumn<K>(prm, col, cell, [&](uint32_t pair) { return foldFrames<K>(K::row(prm, pair, cell), a, b); });
}

// slice blockIdx.y of every column's frames -> partial records [slices][columns][pairs][cells] (an empty slice -- more slices than frames --
// leaves an empty record)
template <class K>
__device__ __forceinline__ void overviewSliceBody(const typename K::Params &prm)
{
    long col, a, b, sa, sb;
    uint32_t cell;
    threadCell<K::kThreads>(prm, col, cell);
    const uint32_t cells = K::cells(prm.out);
    if (cell >= cells) return;
    columnFrames(prm, col, a, b);
    sliceRange(prm, a, b, b > a ? b - a : 0, sa, sb);
    for (uint32_t pair = 0; pair < prm.out.C; ++pair)
        K::storeRecord(prm.partial + ((size_t(blockIdx.y) * size_t(prm.columns) + size_t(col)) * prm.out.C + pair) * cells + cell,
                       K::accRecord(foldFrames<K>(K::row(prm, pair, cell), sa, sb)));
}

// the fold over the slices, then emitColumn
template <class K>
__device__ __forceinline__ void overviewEmitBody(const typename K::Params &prm)
{
    long col;
    uint32_t cell;
    threadCell<K::kThreads>(prm, col, cell);
    const uint32_t cells = K::cells(prm.out);
    if (cell >= cells) return;
    const size_t perSlice = size_t(prm.columns) * prm.out.C * cells;
    emitColumn<K>(prm, col, cell, [&](uint32_t pair) {
        return foldRecords<K>(prm.partial + (size_t(col) * prm.out.C + pair) * cells + cell, perSlice, long(prm.slices));
    });
}

// The view of kept records [n][pairs][cells] as any call of the kind writes them: output column b is the fold of source columns
// ceil(b m / cols) <= j < ceil((b + 1) m / cols) of the range, m = x1 - x0 -- a fold of folds, hence the bytes of the direct call wherever the
// boundaries coincide.  The same three shapes
template <class K>
__device__ __forceinline__ typename K::Acc viewAcc(const typename K::ViewParams &prm, long a, long b, uint32_t pair, uint32_t cell)
{
    const size_t perColumn = size_t(prm.out.C) * K::cells(prm.out);
    return foldRecords<K>(prm.src + size_t(a) * perColumn + size_t(pair) * K::cells(prm.out) + cell, perColumn, b > a ? b - a : 0);
}

template <class K>
__device__ __forceinline__ void overviewViewBody(const typename K::ViewParams &prm)
{
    long col, a, b;
    uint32_t cell;
    threadCell<K::kThreads>(prm, col, cell);
    if (cell >= K::cells(prm.out)) return;
    viewColumns(prm, col, a, b);
    K::emitClosed(prm.out, col, cell, [&](uint32_t pair) { return viewAcc<K>(prm, a, b, pair, cell); });
}

// slice blockIdx.y of every output column's source columns (an empty slice leaves an empty record)
template <class K>
__device__ __forceinline__ void overviewViewSliceBody(const typename K::ViewParams &prm)
{
    long col, a, b, sa, sb;
    uint32_t cell;
    threadCell<K::kThreads>(prm, col, cell);
    const uint32_t cells = K::cells(prm.out);
    if (cell >= cells) return;
    viewColumns(prm, col, a, b);
    sliceRange(prm, a, b, b - a, sa, sb);
    for (uint32_t pair = 0; pair < prm.out.C; ++pair)
        K::storeRecord(prm.partial + ((size_t(blockIdx.y) * size_t(prm.cols) + size_t(col)) * prm.out.C + pair) * cells + cell,
                       K::accRecord(viewAcc<K>(prm, sa, sb, pair, cell)));
}

template <class K>
__device__ __forceinline__ void overviewViewEmitBody(const typename K::ViewParams &prm)
{
    long col;
    uint32_t cell;
    threadCell<K::kThreads>(prm, col, cell);
    const uint32_t cells = K::cells(prm.out);
    if (cell >= cells) return;
    const size_t perSlice = size_t(prm.cols) * prm.out.C * cells;
    K::emitClosed(prm.out, col, cell, [&](uint32_t pair) {
        return foldRecords<K>(prm.partial + (size_t(col) * prm.out.C + pair) * cells + cell, perSlice, long(prm.slices));
    });
}

// ---- 5. the launch front (host) --------------------------------------------------------------------------------------------------------------
static inline sgz_status uploaded(Plan &p)                                  // the kernels read the plan's tables
{
    if (p.uploaded) return SGZ_OK;
    std::string err;
    const sgz_status st = uploadPlan(p, err);
    return st == SGZ_OK ? st : fail(st, err);
}

// Column 0 reads the carry while the open column writes it: where a call has both, column 0 reads a snapshot.  *carryIn: d_carry, or the copy
template <class Record>
sgz_status snapshotCarry(Plan &p, OverviewKind kind, const OverviewStep &sh, uint32_t held, const Record *d_carry, size_t records, hipStream_t stream,
                         const Record **carryIn)
{
    *carryIn = d_carry;
    if (!(held && sh.open && sh.columns > 1)) return SGZ_OK;
    OverviewScratch &ov = p.ov[kind];
    if (sgz_status st = ensureCap(&ov.d_carryCopy, &ov.carryCopyCap, records * kRecordFloats<Record>); st != SGZ_OK) return st;
    SGZ_HIP(hipMemcpyAsync(ov.d_carryCopy, d_carry, records * sizeof(Record), hipMemcpyDeviceToDevice, stream));
    *carryIn = reinterpret_cast<const Record *>(ov.d_carryCopy);
    return SGZ_OK;
}

// the one launch, or the slice launch and the emit launch behind it; prm.slices is chosen, `records` partial records a slice
template <class Params>
sgz_status launchOverviewForms(Plan &p, OverviewKind kind, Params &prm, uint64_t units, uint32_t blocks, int threads, size_t records,
                               void (*whole)(Params), void (*slice)(Params), void (*emit)(Params), hipStream_t stream)
{
    using Partial = std::remove_pointer_t<decltype(prm.partial)>;
    const dim3 grid(unsigned(units * blocks));
    if (prm.slices <= 1) {
        hipLaunchKernelGGL(whole, grid, dim3(threads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
        return SGZ_OK;
    }
    OverviewScratch &ov = p.ov[kind];
    if (sgz_status st = ensureCap(&ov.d_partial, &ov.partialCap, size_t(prm.slices) * records * kRecordFloats<Partial>); st != SGZ_OK) return st;
    prm.partial = reinterpret_cast<Partial *>(ov.d_partial);
    hipLaunchKernelGGL(slice, dim3(grid.x, prm.slices), dim3(threads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(emit, grid, dim3(threads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

// The direct form behind a stage call's argument checks.  prm: the kind's own fields are set; the step, the grid, the carry and the slices are
// set here.  cells: a column's records of one pair; autoSlices(columns, blocks): the kind's rule where the caller leaves the choice
template <class Params, class Record, class Rule>
sgz_status launchOverviewColumns(Plan &p, OverviewKind kind, Params &prm, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                 Record *d_carry, uint32_t cells, int threads, Rule autoSlices, void (*whole)(Params), void (*slice)(Params),
                                 void (*emit)(Params), hipStream_t stream)
{
    const OverviewStep sh = overviewStepShape(k, held, frames, flush);
    if (!sh.launch) return SGZ_OK;
    const uint32_t blocks = (cells + threads - 1) / threads;
    if (sh.columns == 0 || blocks == 0) return SGZ_OK;
    if (sh.columns > 0x7fffffffull / blocks || frames > size_t(0x7fffffffffffffffll)) return fail(SGZ_EINVAL, "too many columns for one launch");
    prm.frames = long(frames); prm.columns = long(sh.columns); prm.closed = long(sh.closed);
    prm.k = k; prm.held = held; prm.blocks = blocks;
    prm.carryOut = d_carry;
    if (sgz_status st = snapshotCarry<Record>(p, kind, sh, held, d_carry, size_t(p.C) * cells, stream, &prm.carryIn); st != SGZ_OK) return st;
    prm.slices = slices ? slices : autoSlices(sh.columns, blocks);
    return launchOverviewForms(p, kind, prm, sh.columns, blocks, threads, size_t(sh.columns) * p.C * cells, whole, slice, emit, stream);
}

// The view form: d_src [m][pairs][cells], the range's first source column -> cols <= m output columns.  prm: the kind's own fields are set
template <class ViewParams>
sgz_status launchOverviewView(Plan &p, OverviewKind kind, ViewParams &prm, size_t m, size_t cols, uint32_t slices, uint32_t cells, int threads,
                              void (*whole)(ViewParams), void (*slice)(ViewParams), void (*emit)(ViewParams), hipStream_t stream)
{
    const uint32_t blocks = (cells + threads - 1) / threads;
    if (cols == 0 || blocks == 0) return SGZ_OK;
    if (cols > 0x7fffffffull / blocks) return fail(SGZ_EINVAL, "too many columns for one launch");
    prm.m = long(m); prm.cols = long(cols); prm.blocks = blocks;
    const uint32_t most = uint32_t((m + cols - 1) / cols);       // source columns of the longest output column
    // the overview's rule at four workgroups per CU, and no slice shorter than one batch of kOvUnroll loads
    prm.slices = slices ? slices : std::min(overviewAutoSlices(long(cols), blocks, most, m, 2 * numCUs()), std::max(1u, most / uint32_t(kOvUnroll)));
    return launchOverviewForms(p, kind, prm, cols, blocks, threads, cols * p.C * cells, whole, slice, emit, stream);
}

// ---- 6. the host fold's frame ----------------------------------------------------------------------------------------------------------------
static inline uint32_t hostBits(float v) { uint32_t bits; std::memcpy(&bits, &v, sizeof bits); return bits; }
static inline float hostFloat(uint32_t bits) { float v; std::memcpy(&v, &bits, sizeof v); return v; }

// The frame of sgz_overview_<kind>_fold: out[b][i] = the fold of source columns [bound(b), bound(b + 1)) of record i of `width`.  Acc: the
// kind's accumulator with tallies wide enough to see them pass 2^32 - 1, value-initialised to nothing; add(acc, record); fits(acc) says whether
// the record's 32-bit tallies hold it; write(acc, record).  Two passes: nothing is written when any column overflows
struct FoldRefusals { const char *null, *width, *overflow; };
template <class Acc, class Record, class Add, class Fits, class Write>
sgz_status foldKeptColumns(const FoldRefusals &refusal, const Record *in, size_t n, size_t width, size_t x0, size_t x1, uint32_t outColumns,
                           Record *out, Add add, Fits fits, Write write)
{
    if (!in || !out) return fail(SGZ_EINVAL, refusal.null);
    if (width == 0) return fail(SGZ_EINVAL, refusal.width);
    uint64_t cols = 0;
    if (sgz_status st = checkViewRange(n, x0, x1, outColumns, &cols); st != SGZ_OK) return st;
    const uint64_t m = x1 - x0;
    for (int pass = 0; pass < 2; ++pass)
        for (uint64_t b = 0; b < cols; ++b) {
            const uint64_t ja = x0 + (b * m + cols - 1) / cols, jb = x0 + ((b + 1) * m + cols - 1) / cols;
            for (size_t i = 0; i < width; ++i) {
                Acc acc{};
                for (uint64_t j = ja; j < jb; ++j) add(acc, in[j * width + i]);
                if (!fits(acc)) return fail(SGZ_EINVAL, refusal.overflow);
                if (pass) write(acc, out[b * width + i]);
            }
        }
    return SGZ_OK;
}

}  // namespace sgz
