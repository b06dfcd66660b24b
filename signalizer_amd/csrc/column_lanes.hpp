// column_lanes.hpp -- what the eight column lanes (wave, level, true-peak, loudness, stereo-field, band, histogram, run: <lane>_columns.hip) have in common,
// written once: the shape of a call, the column / tile / slice bounds, the aligned split and the staging of a row, the two quantisers, the
// stage call from its argument checks to the lane's launches (stageColumns), the grid's fields of a kernel-argument struct (fillGrid), the
// launch front of the six plain lanes (launchPlainLane), the fold's frame, and the parts in which the loudness and the band lane are twins:
// their shared fields (fillTwin), their launch front (launchTwinLane), the history kernel and the column sums.  A lane's file holds what is
// its own: its record, its accumulators, its kernels' bodies, the fields only it has.  pcm.hip includes this for the lanes' entry points.
// A lane's kernel-argument struct keeps its own type and layout; the helpers here are templates on it and read the grid's fields by name:
//   planar, stride (size_t); n, columns, closed (long); m, held, perTile, slices (uint32_t)
// Floating-point contraction: this header neither sets nor resets it.  loudness_columns.hip and band_columns.hip include it BEHIND their
// `#pragma clang fp contract(off)`, so every template instantiated there was parsed without contraction; the other six files have no pragma,
// and nothing here has a multiply feeding an add in floating point.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "runtime.hpp"
#include "scope_ring.hpp"      // StreamScratch

namespace sgz {

// ---- 1. the shape of a call ---------------------------------------------------------------------------------------------------------------------
// Column c of a call covers its samples [c m - held, (c + 1) m - held) clipped to [0, n): column 0 is the rest of the carried column
// (held > 0), the last one may stay open and goes to the carry.
struct ColumnsShape {
    uint64_t columns, closed;            // columns the call touches; those it emits
    bool open, launch;                   // a last column stays open (it goes to the carry); anything is launched at all
    uint32_t slices;                     // 0: the tile form
    size_t scratchBytes;                 // leadBytes and the partial records of the sliced form
};

// The shape of a call whose arguments passed the stage call's checks.  cells: the records of a column (channels or pairs).  slices: 0 = the
// tile form, else the sliced form with that many (the caller's count, or for m > switchOver the overview's rule: the smallest count <=
// min(64, m, n) with columns x cells x slices >= 2 workgroups per CU); scratchBytes: leadBytes (the q planes of the loudness and band lanes,
// else 0) and behind them the partial records of the sliced form.  launch: false -- nothing arrives and nothing is flushed.
inline ColumnsShape columnsShape(uint32_t cells, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices, uint32_t switchOver,
                                 size_t recordBytes, size_t leadBytes)
{
    ColumnsShape sh{};
    const uint64_t t = uint64_t(held) + nsamples;
    sh.closed = t / m + ((flush && t % m) ? 1u : 0u);
    sh.open = !flush && t % m != 0;
    sh.columns = sh.closed + (sh.open ? 1u : 0u);
    sh.launch = sh.columns != 0 && !(nsamples == 0 && !(flush && held));
    if (!sh.launch || nsamples == 0) return sh;
    if (slices >= 2 || m > switchOver) sh.slices = slices ? slices : overviewAutoSlices(long(sh.columns), cells, m, nsamples, numCUs());
    sh.scratchBytes = leadBytes + size_t(sh.slices) * size_t(sh.columns) * cells * recordBytes;
    return sh;
}

// The lanes' two steps, what the stage calls and sgz_pcm_stream share: <lane>ColumnsShape is columnsShape with the lane's switch-over and
// record, run<Lane>Columns the stage call behind its argument checks, asynchronous on `stream`, with the carry in two places and scratch of
// sh.scratchBytes bytes (aligned to 16 for loudness and band).  Wave, level, field, histogram: carryIn is read by column 0 (held > 0), carryOut written
// by the open column -- the same memory only where the call has one column.  True-peak, loudness, band: carryIn is read (the history when
// `continued`, the open column when held > 0) and carryOut is written whole by every call with samples -- never the same memory then.  The
// loudness and band carries are <lane>CarryBytes(f) bytes per channel: the open column's record, the last W + L - 1 quantised samples, a
// zero word; firstIndex: the absolute index of the call's first sample (the segment phase).
ColumnsShape waveColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices);
sgz_status runWaveColumns(const ColumnsShape &sh, const float *d_planar, size_t channelStride, uint32_t channels, size_t nsamples, uint32_t m,
                          uint32_t held, const float *carryIn, float *carryOut, float *d_wave, void *scratch, hipStream_t stream);
ColumnsShape levelColumnsShape(uint32_t pairs, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices);
sgz_status runLevelColumns(const ColumnsShape &sh, const float *d_planar, size_t channelStride, uint32_t pairs, size_t nsamples, uint32_t m,
                           uint32_t held, const sgz_level_record *carryIn, sgz_level_record *carryOut, sgz_level_record *d_level, void *scratch,
                           hipStream_t stream);
ColumnsShape fieldColumnsShape(uint32_t pairs, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices);
sgz_status runFieldColumns(const ColumnsShape &sh, const float *d_planar, size_t channelStride, uint32_t pairs, size_t nsamples, uint32_t m,
                           uint32_t held, const sgz_field_record *carryIn, sgz_field_record *carryOut, sgz_field_record *d_field, void *scratch,
                           hipStream_t stream);
ColumnsShape truePeakColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices);
sgz_status runTruePeakColumns(const ColumnsShape &sh, const float *d_planar, size_t channelStride, uint32_t channels, size_t nsamples, uint32_t m,
                              uint32_t held, uint32_t continued, const sgz_truepeak_carry *carryIn, sgz_truepeak_carry *carryOut,
                              sgz_truepeak_record *d_peaks, void *scratch, hipStream_t stream);
size_t loudnessCarryBytes(const sgz_loudness_filter &f);
ColumnsShape loudnessColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices);
sgz_status runLoudnessColumns(const ColumnsShape &sh, const sgz_loudness_filter &f, const float *d_planar, size_t channelStride, uint32_t channels,
                              size_t nsamples, uint64_t firstIndex, uint32_t m, uint32_t held, uint32_t continued, const void *carryIn,
                              void *carryOut, sgz_loudness_record *d_out, void *scratch, hipStream_t stream);
size_t bandCarryBytes(const sgz_band_filter &f);
ColumnsShape bandColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices);
sgz_status runBandColumns(const ColumnsShape &sh, const sgz_band_filter &f, const float *d_planar, size_t channelStride, uint32_t channels,
                          size_t nsamples, uint64_t firstIndex, uint32_t m, uint32_t held, uint32_t continued, const void *carryIn, void *carryOut,
                          sgz_band_record *d_out, void *scratch, hipStream_t stream);
ColumnsShape histColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices);
sgz_status runHistColumns(const ColumnsShape &sh, const float *d_planar, size_t channelStride, uint32_t channels, size_t nsamples, uint32_t m,
                          uint32_t held, const sgz_hist_record *carryIn, sgz_hist_record *carryOut, sgz_hist_record *d_hist, void *scratch,
                          hipStream_t stream);
// the run lane: the true-peak lane's carry rule (a history of two samples: sgz_run_carry), and its thresholds, checked by runParamsCheck
sgz_status runParamsCheck(const sgz_run_params *p, const char *who);
ColumnsShape runColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices);
sgz_status runRunColumns(const ColumnsShape &sh, const sgz_run_params &p, const float *d_planar, size_t channelStride, uint32_t channels,
                         size_t nsamples, uint32_t m, uint32_t held, uint32_t continued, const sgz_run_carry *carryIn, sgz_run_carry *carryOut,
                         sgz_run_record *d_runs, void *scratch, hipStream_t stream);

// ---- 2. device helpers --------------------------------------------------------------------------------------------------------------------------
// samples [a, b) of this call that belong to column `col`
template <class Params>
__device__ __forceinline__ void columnSamples(const Params &prm, long col, long &a, long &b)
{
    a = col * long(prm.m) - long(prm.held);
    b = a + long(prm.m);
    a = a < 0 ? 0 : a;
    b = b > prm.n ? prm.n : b;
}

// the columns [c0, c1) of workgroup blockIdx.x's tile: perTile whole columns of the call (column 0 counts as one, whatever is left of it)
template <class Params>
__device__ __forceinline__ void tileColumns(const Params &prm, long &c0, long &c1)
{
    c0 = long(blockIdx.x) * long(prm.perTile);
    c1 = c0 + long(prm.perTile) < prm.columns ? c0 + long(prm.perTile) : prm.columns;
}

// ... and with them their samples [a, b) (b - a <= perTile * m).  (A kernel copies the four into constants of its own: with that spelling
// every lane's tile kernel compiles to the instructions it had with the bounds written out in its body)
struct TileBounds { long c0, c1, a, b; };
template <class Params>
__device__ __forceinline__ void tileBounds(const Params &prm, TileBounds &t)
{
    tileColumns(prm, t.c0, t.c1);
    t.a = t.c0 * long(prm.m) - long(prm.held);
    t.b = t.c1 * long(prm.m) - long(prm.held);
    t.a = t.a < 0 ? 0 : t.a;
    t.b = t.b > prm.n ? prm.n : t.b;
}

// slice s of a column's samples [a, b): [sa, sb), empty where there are more slices than samples
template <class Params>
__device__ __forceinline__ void sliceSamples(const Params &prm, long a, long b, uint32_t s, long &sa, long &sb)
{
    const long n = b > a ? b - a : 0, per = (n + long(prm.slices) - 1) / long(prm.slices);
    sa = a + long(s) * per < b ? a + long(s) * per : b;
    sb = sa + per < b ? sa + per : b;
}

// where the 16-byte part of `count` floats at g (4-byte aligned) begins and ends: [0, head) and [tail, count) are scalar, `vecs` chunks lie
// between.  Count: size_t, or uint32_t where a tile bounds it
template <class Count>
__device__ __forceinline__ void splitAligned(const float *g, Count count, uint32_t &head, Count &vecs, Count &tail)
{
    const uint32_t lead = uint32_t(reinterpret_cast<uintptr_t>(g) >> 2) & 3u;
    const uint32_t toBoundary = (4u - lead) & 3u;
    head = count < toBoundary ? uint32_t(count) : toBoundary;
    vecs = (count - head) >> 2;
    tail = head + 4 * vecs;
}

// where word i of a tile's row lies in LDS: four words of padding behind every 64, so that columns a multiple of 32 words apart start on
// different banks (16-byte chunks stay whole and aligned)
__device__ __forceinline__ uint32_t tileWord(uint32_t i) { return i + ((i >> 6) << 2); }

// The quantiser: v = (int32) clamp(rintf(x 2^23), -2^26, +2^26).  (x 2^23 is exact or overflows to an infinity, which the clamp takes -- the
// median of three: the clamp in one instruction; a denormal times 2^23 is below 2^-102 and rounds to 0, as does the 0 a flushing device
// makes of it.)  Two forms: a NaN as a mark no quantised sample equals (|v| <= 2^26), or as 0
constexpr int32_t kQuantNaN = std::numeric_limits<int32_t>::min();
__device__ __forceinline__ int32_t quantiseMarked(uint32_t bits)
{
    const float x = __uint_as_float(bits);
    const float r = __builtin_amdgcn_fmed3f(rintf(x * 0x1p23f), -0x1p26f, 0x1p26f);
    return x != x ? kQuantNaN : int32_t(r);
}
__device__ __forceinline__ int32_t quantiseSilent(float x)
{
    const float r = __builtin_amdgcn_fmed3f(rintf(x * 0x1p23f), -0x1p26f, 0x1p26f);
    return x != x ? 0 : int32_t(r);
}

// `count` (<= 4 Threads Unroll) floats at g, quantised (a NaN marked), into a row of a tile, `lead` words in: 16-byte chunks of memory are
// 16-byte chunks of LDS; a lane issues Unroll 16-byte loads before the first store.  Padded: the row's words lie at tileWord; plain: nothing
// strides the row
template <bool Padded, int Threads, int Unroll>
__device__ __forceinline__ void stageRow(const float *g, uint32_t count, uint32_t lead, int32_t *row)
{
    const auto at = [](uint32_t i) { return Padded ? tileWord(i) : i; };
    const uint32_t tid = threadIdx.x;
    uint32_t head;
    size_t vecs, tail;
    splitAligned(g, size_t(count), head, vecs, tail);
    if (tid < head) row[at(lead + tid)] = quantiseMarked(__float_as_uint(g[tid]));
    if (tid < count - uint32_t(tail)) row[at(lead + uint32_t(tail) + tid)] = quantiseMarked(__float_as_uint(g[tail + tid]));
    const uint4 *gv = reinterpret_cast<const uint4 *>(g + head);
    uint4 v[Unroll];
#pragma unroll
    for (int j = 0; j < Unroll; ++j)
        v[j] = tid + uint32_t(j) * Threads < vecs ? gv[tid + uint32_t(j) * Threads] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int j = 0; j < Unroll; ++j)                                        // (lead + head is a multiple of 4 wherever vecs > 0)
        if (tid + uint32_t(j) * Threads < vecs)
            // (the plain row's offsets are added to the pointer one by one and nothing is named in between: spelled so, both lanes' kernels
            // compile to the instructions they had with a staging function of their own)
            *reinterpret_cast<int4 *>(Padded ? row + tileWord(lead + head + 4u * (tid + uint32_t(j) * Threads))
                                             : row + lead + head + 4u * (tid + uint32_t(j) * Threads)) =
                make_int4(quantiseMarked(v[j].x), quantiseMarked(v[j].y), quantiseMarked(v[j].z), quantiseMarked(v[j].w));
}

inline uint32_t pow2AtLeast(uint32_t v)
{
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

inline uint32_t log2Of(uint32_t v)
{
    uint32_t l = 0;
    while ((1u << l) < v) ++l;
    return l;
}

// ---- 3. the host front ----------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kLaneMaxSlices = 64;

// What a stage call's messages and checks differ in
struct StageFront {
    const char *who;                     // the call: "sgz_stage_wave_columns"
    const char *cells;                   // what a column's records are per: "channels" or "pairs"
    uint32_t maxCells;
    const char *out;                     // the output argument's name
    uint32_t align;                      // of d_carry and the output, in bytes
    bool history;                        // the carry holds a filter's history too: `continued`, and every call with samples writes it whole
    uint32_t sampleBits;                 // nsamples <= 2^sampleBits (62: nothing but the stride is named)
};

// The argument checks in front of the shape.  filter: the status of the lane's own filter check, made by the caller (SGZ_OK where the lane has
// none): it is returned, its message standing, behind the check of d_planar alone.  continued, firstIndex: 0 where the call has none
inline sgz_status checkStageArgs(const StageFront &f, sgz_status filter, const void *d_planar, size_t channelStride, uint32_t cells, size_t nsamples,
                                 uint32_t m, uint32_t held, uint32_t continued, uint64_t firstIndex, uint32_t slices, const void *d_carry,
                                 const void *d_out)
{
    const auto no = [&f](const std::string &why) { return fail(SGZ_EINVAL, std::string(f.who) + ": " + why); };
    if (!d_planar) return no("null d_planar");
    if (filter != SGZ_OK) return filter;
    if (cells == 0 || cells > f.maxCells) return no("1 .. " + std::to_string(f.maxCells) + " " + f.cells);
    if (m == 0) return no("m >= 1 samples per column");
    if (held >= m) return no("held < m");
    if (f.history && !continued && held) return no("held > 0 needs continued != 0 (a stream that begins here has no open column)");
    if (channelStride < nsamples || nsamples > (size_t(1) << f.sampleBits))
        return no(std::string("channel_stride < nsamples") + (f.sampleBits < 62 ? ", or more than 2^" + std::to_string(f.sampleBits) + " samples" : ""));
    if (firstIndex > (uint64_t(1) << 62)) return no("first_index above 2^62");
    if (slices > kLaneMaxSlices) return no("slices 0 (automatic) or 1 .. 64");
    if ((reinterpret_cast<uintptr_t>(d_planar) & 3u) || (reinterpret_cast<uintptr_t>(d_carry) & (f.align - 1u)) || (reinterpret_cast<uintptr_t>(d_out) & (f.align - 1u)))
        return no(std::string("d_planar aligned to 4 bytes, d_carry and ") + f.out + " to " + std::to_string(f.align));
    return SGZ_OK;
}

// ... and behind it: the buffers the call's shape reads or writes are there
inline sgz_status checkStageBuffers(const StageFront &f, const ColumnsShape &sh, size_t nsamples, uint32_t held, uint32_t continued,
                                    const void *d_carry, const void *d_out)
{
    const auto no = [&f](const std::string &why) { return fail(SGZ_EINVAL, std::string(f.who) + ": " + why); };
    if (f.history) {
        if (!d_carry && (continued || nsamples)) return no("d_carry is read (continued) or written (nsamples > 0)");
    } else if (!d_carry && (held || sh.open)) {
        return no("d_carry is read (held > 0) or written (samples stay open)");
    }
    if (!d_out && sh.closed) return no(std::string(f.out) + " is written (a column closes)");
    return SGZ_OK;
}

// The stream-ordered memory of a stage call: the scratch of its shape, and the carry's snapshot.  The snapshot rule: a launch must not read
// the carry that another of its workgroups writes.  Without a history that is column 0 reading (held > 0) while an open column is stored, in a
// call of more than one column; with one, the halos, the history and column 0 read while the new carry is written whole, in every continued
// call with samples.  Those calls read a copy
struct StageScratch {
    StreamScratch scratch, snapshot;
    explicit StageScratch(hipStream_t s) : scratch(s), snapshot(s) {}
    // carryIn: d_carry, or its snapshot of carryBytes bytes
    sgz_status get(const StageFront &f, const ColumnsShape &sh, size_t nsamples, uint32_t held, uint32_t continued, const void *d_carry,
                   size_t carryBytes, const void **carryIn)
    {
        *carryIn = d_carry;
        if (f.history ? (continued && nsamples) : (held && sh.open && sh.columns > 1)) {
            SGZ_HIP(snapshot.get(carryBytes));
            SGZ_HIP(hipMemcpyAsync(snapshot.p, d_carry, carryBytes, hipMemcpyDeviceToDevice, snapshot.s));
            *carryIn = snapshot.p;
        }
        if (sh.scratchBytes) SGZ_HIP(scratch.get(sh.scratchBytes));
        return SGZ_OK;
    }
};

// a grid dimension fits one launch; lane: the lane's word ("true-peak"), what: "columns" or "samples"
inline sgz_status fitsOneLaunch(uint64_t count, const char *lane, const char *what)
{
    if (count > 0x7fffffffull) return fail(SGZ_EINVAL, std::string(lane) + " columns: too many " + what + " for one launch");
    return SGZ_OK;
}
// the emit launch: workgroups of `threads` over one lane per cell
inline uint64_t emitBlocks(uint64_t cells, int threads) { return (cells + uint64_t(threads) - 1) / uint64_t(threads); }

// the fields every lane's kernel-argument struct has under the same names
template <class Params>
void fillGrid(Params &prm, const ColumnsShape &sh, const float *d_planar, size_t channelStride, size_t nsamples, uint32_t m, uint32_t held)
{
    prm.planar = d_planar; prm.stride = channelStride; prm.n = long(nsamples);
    prm.columns = long(sh.columns); prm.closed = long(sh.closed);
    prm.m = m; prm.held = held; prm.slices = sh.slices;
}

// The launch front of the wave, level, field, true-peak, histogram and run lanes: the tile kernel alone -- setTile(prm) sets the tile form's
// own fields, perTile among them --, or the slice kernel (samples arrive) and behind it the emit kernel, `emitLanes` threads per (column,
// cell).  word: the lane's, for fitsOneLaunch
template <class Params, class SetTile>
sgz_status launchPlainLane(void (*tileKernel)(Params), void (*sliceKernel)(Params), void (*emitKernel)(Params), int threads, const char *word,
                           Params &prm, const ColumnsShape &sh, uint32_t cells, size_t nsamples, uint32_t emitLanes, SetTile setTile, hipStream_t stream)
{
    if (nsamples != 0 && sh.slices == 0) {
        setTile(prm);
        const uint64_t tiles = (sh.columns + prm.perTile - 1) / prm.perTile;
        if (sgz_status st = fitsOneLaunch(tiles, word, "columns"); st != SGZ_OK) return st;
        hipLaunchKernelGGL(tileKernel, dim3(unsigned(tiles), cells), dim3(threads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
        return SGZ_OK;
    }
    const uint64_t blocks = emitBlocks(sh.columns * cells * emitLanes, threads);
    if (sgz_status st = fitsOneLaunch(std::max(sh.columns, blocks), word, "columns"); st != SGZ_OK) return st;
    if (nsamples != 0) {
        hipLaunchKernelGGL(sliceKernel, dim3(unsigned(sh.columns), cells, sh.slices), dim3(threads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(emitKernel, dim3(unsigned(blocks)), dim3(threads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

// The body of every sgz_stage_<lane>_columns, in the order that decides which refusal wins: the argument checks (filter: checkStageArgs), the
// shape, the buffers, before() -- what must succeed before anything is launched: the twins' tap table --, then the stream-ordered memory and
// run(sh, carryIn, scratch, stream), the lane's run<Lane>Columns.  carryBytes: of the whole carry (used behind the checks alone)
inline sgz_status noStep() { return SGZ_OK; }
template <class Shape, class Before, class Run>
sgz_status stageColumns(const StageFront &front, sgz_status filter, const float *d_planar, size_t channelStride, uint32_t cells, size_t nsamples,
                        uint32_t m, uint32_t held, int flush, uint32_t continued, uint64_t firstIndex, uint32_t slices, const void *d_carry,
                        const void *d_out, void *stream, Shape shape, size_t carryBytes, Before before, Run run)
{
    if (sgz_status st = checkStageArgs(front, filter, d_planar, channelStride, cells, nsamples, m, held, continued, firstIndex, slices, d_carry, d_out); st != SGZ_OK) return st;
    const ColumnsShape sh = shape(cells, nsamples, m, held, flush, slices);
    if (sgz_status st = checkStageBuffers(front, sh, nsamples, held, continued, d_carry, d_out); st != SGZ_OK) return st;
    if (sgz_status st = before(); st != SGZ_OK) return st;
    if (!sh.launch) return SGZ_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    StageScratch mem(s);
    const void *carryIn = nullptr;
    if (sgz_status st = mem.get(front, sh, nsamples, held, continued, d_carry, carryBytes, &carryIn); st != SGZ_OK) return st;
    return run(sh, carryIn, mem.scratch.p, s);
}

// The frame of every sgz_<lane>_fold: out[b][c] = the fold of source columns [bound(b), bound(b + 1)) of cell c.  fits(first, count, stride)
// says whether the 32-bit tallies of records first[0], first[stride], .. hold their sum -- asked of every output first: a refusal writes
// nothing --, sum(first, count, stride) is the folded record.  tooMany: what the refusal's message says behind "2^32 - 1"
template <class Record, class Fits, class Sum>
sgz_status foldColumns(const char *who, const char *cellsWord, const char *tooMany, const Record *in, size_t n, uint32_t cells, size_t x0, size_t x1,
                       uint32_t outColumns, Record *out, Fits fits, Sum sum)
{
    if (!in || !out) return fail(SGZ_EINVAL, std::string(who) + ": null argument");
    if (cells == 0) return fail(SGZ_EINVAL, std::string(who) + ": " + cellsWord + " >= 1");
    uint64_t cols = 0;
    if (sgz_status st = checkViewRange(n, x0, x1, outColumns, &cols); st != SGZ_OK) return st;
    const uint64_t w = x1 - x0;
    auto bound = [&](uint64_t b) { return x0 + (b * w + cols - 1) / cols; };                   // (b w < 2^62: n < 2^31)
    for (uint64_t b = 0; b < cols; ++b)
        for (uint32_t c = 0; c < cells; ++c)
            if (!fits(in + bound(b) * cells + c, size_t(bound(b + 1) - bound(b)), size_t(cells)))
                return fail(SGZ_EINVAL, std::string(who) + ": a folded column counts more than 2^32 - 1" + tooMany);
    for (uint64_t b = 0; b < cols; ++b)
        for (uint32_t c = 0; c < cells; ++c) out[b * cells + c] = sum(in + bound(b) * cells + c, size_t(bound(b + 1) - bound(b)), size_t(cells));
    return SGZ_OK;
}

// ---- 4. the loudness and the band lane's twin parts ---------------------------------------------------------------------------------------------
// Both cut the sample axis into segments of L samples, start a segment from exact integer FIRs over the last W quantised samples and run an
// fp64 recurrence over it into q planes in scratch, then sum q^2 per column.  Shared: the filter's shape, the tap table on the device, the
// carry's layout [record | W + L - 1 samples of history | a zero word], the run tile's geometry, the history kernel and the column sums.
// Filter: sgz_loudness_filter or sgz_band_filter (W, L).  Params: the lane's kernel arguments -- beside the grid's fields planar, stride,
// channels, continued, hist, logL, lanesPer, carryIn, carryOut, carryBytes, group, out, partial, and `typedef <record> Record`.  Acc: a
// column's, a lane's or a slice's part of a record: value-initialised to nothing, takeSample(prm, ch, r), add(record), foldLane(o),
// store(record *)
constexpr int kTwinThreads = 256;
constexpr uint32_t kTwinTile = 4096;             // samples of a run tile (a segment longer than this is a tile of its own) and of a sum tile
constexpr uint32_t kTwinRun = 16;                // samples of a lane in the sum tile
constexpr uint32_t kTwinMaxW = 65536, kTwinMinL = 16;
constexpr uint32_t kTwinDeviceMaxW = 16384;      // the halo and a tile fit the 160 KiB of LDS up to here

template <class Filter>
bool filterShapeOk(const Filter &f)
{
    const auto pow2 = [](uint32_t v) { return v && !(v & (v - 1)); };
    return pow2(f.W) && pow2(f.L) && f.L >= kTwinMinL && f.L <= f.W && f.W <= kTwinMaxW;
}

template <class Filter>
sgz_status filterForDevice(const Filter *f, const char *who)
{
    if (!f) return fail(SGZ_EINVAL, std::string(who) + ": null filter");
    if (!filterShapeOk(*f)) return fail(SGZ_EINVAL, std::string(who) + ": W and L are powers of two, 16 <= L <= W <= 65536");
    if (f->W > kTwinDeviceMaxW) return fail(SGZ_EINVAL, std::string(who) + ": the device takes W <= 16384");
    return SGZ_OK;
}

// The table on the device: one per (device, filter), made at the filter's first use and kept.  build(f, planes) fills C[c][k] at
// planes[c * W + k] for `comps` components (a multiple of 4), false where the filter is refused; the device holds rows C[g][k][0..3] of 16
// bytes, g the components 4 g .. 4 g + 3.  The first use of a filter on a device uploads them (the one blocking step of the stage call)
template <class Filter>
sgz_status deviceTaps(const Filter &f, uint32_t comps, bool (*build)(const Filter &, int32_t *), const char *lane, const int4 **out)
{
    struct Entry { int dev; Filter f; int4 *d; };
    static std::mutex mutex;
    static std::vector<Entry> cache;
    int dev = 0;
    SGZ_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mutex);
    for (const Entry &t : cache)
        if (t.dev == dev && std::memcmp(&t.f, &f, sizeof f) == 0) { *out = t.d; return SGZ_OK; }
    std::vector<int32_t> planes(size_t(comps) * f.W), rows(size_t(comps) * f.W);
    if (!build(f, planes.data())) return fail(SGZ_EINVAL, std::string(lane) + ": the filter is refused (sgz_" + lane + "_taps)");
    for (uint32_t g = 0; g < comps / 4u; ++g)
        for (uint32_t k = 0; k < f.W; ++k)
            for (uint32_t q = 0; q < 4; ++q) rows[(size_t(g) * f.W + k) * 4 + q] = planes[size_t(g * 4 + q) * f.W + k];
    Entry t{dev, f, nullptr};
    SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&t.d), rows.size() * sizeof(int32_t)));
    if (const hipError_t e = hipMemcpy(t.d, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice); e != hipSuccess) {
        (void)hipFree(t.d);
        return hipFail(e, (std::string("hipMemcpy(") + lane + " taps)").c_str());
    }
    cache.push_back(t);
    *out = t.d;
    return SGZ_OK;
}

// a channel's carry (sgz::<lane>CarryBytes)
template <class Record, class Filter> size_t twinCarryBytes(const Filter &f) { return sizeof(Record) + size_t(f.W + f.L) * sizeof(int32_t); }

// the run tile: T = max(4096, L) samples; q rows of a call's samples; the LDS words of the halo and the tile, padding included
template <class Filter> uint32_t runTileOf(const Filter &f) { return f.L > kTwinTile ? f.L : kTwinTile; }
inline size_t qStrideOf(size_t nsamples) { return (nsamples + 3) & ~size_t(3); }
template <class Filter>
uint32_t runTileWords(const Filter &f)
{
    const uint32_t tile = runTileOf(f), lanesPer = uint32_t(kTwinThreads) / (tile / f.L);
    return ((f.W + tile) + ((f.W + tile) / f.L + 1) * lanesPer + 3u) & ~3u;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: remember what has been granted
template <auto Kernel>
sgz_status grantRunLds(size_t need)
{
    static size_t granted[64] = {};
    static std::mutex mutex;
    int dev = 0;
    SGZ_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mutex);
    if (dev >= 0 && dev < 64 && granted[dev] >= need) return SGZ_OK;
    SGZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(need)));
    if (dev >= 0 && dev < 64) granted[dev] = need;
    return SGZ_OK;
}

// a channel's carry: the open column's record, then the history (oldest first)
template <class Record>
__device__ __forceinline__ const Record *carryOpen(const uint8_t *carry, size_t bytes, uint32_t ch)
{
    return reinterpret_cast<const Record *>(carry + size_t(ch) * bytes);
}
template <class Record>
__device__ __forceinline__ const int32_t *carryHist(const uint8_t *carry, size_t bytes, uint32_t ch)
{
    return reinterpret_cast<const int32_t *>(carry + size_t(ch) * bytes + sizeof(Record));
}

// what the filter sees at sample r of the call, r >= -hist: the call's own sample, the carried history in front of it, zeros behind the call
template <class Params>
__device__ __forceinline__ int32_t filterInput(const Params &prm, uint32_t ch, long r)
{
    if (r >= prm.n) return 0;
    if (r >= 0) return quantiseSilent(prm.planar[size_t(ch) * prm.stride + size_t(r)]);
    return prm.continued ? carryHist<typename Params::Record>(prm.carryIn, prm.carryBytes, ch)[long(prm.hist) + r] : 0;
}

// LDS word of the run tile's sample index i (0 = the halo's first): a shift of lanesPer words per segment keeps the segments' lanes on
// different banks
template <class Params>
__device__ __forceinline__ uint32_t segmentWord(const Params &prm, uint32_t i) { return i + (i >> prm.logL) * prm.lanesPer; }

// the carry of a call with samples but for an open column's record: the history, the zero word behind it, an all-zero open column (an open
// column's record is stored by the sums' launch behind this one)
template <class Params>
__global__ void __launch_bounds__(kTwinThreads)
historyKernel(const Params prm)
{
    typedef typename Params::Record Record;
    const uint32_t t = blockIdx.x * kTwinThreads + threadIdx.x, ch = blockIdx.y;
    uint8_t *mine = prm.carryOut + size_t(ch) * prm.carryBytes;
    int32_t *hist = reinterpret_cast<int32_t *>(mine + sizeof(Record));
    if (t < prm.hist) hist[t] = filterInput(prm, ch, prm.n - long(prm.hist) + long(t));
    if (t == prm.hist) hist[t] = 0;
    if (t < sizeof(Record) / 4) reinterpret_cast<uint32_t *>(mine)[t] = 0u;
}

// the carry into column 0, then to the output (a closed column) or to the carry's open column
template <class Params, class Acc>
__device__ __forceinline__ void emitSums(const Params &prm, long col, uint32_t ch, Acc k)
{
    typedef typename Params::Record Record;
    if (col == 0 && prm.held) k.add(*carryOpen<Record>(prm.carryIn, prm.carryBytes, ch));
    k.store(col < prm.closed ? prm.out + size_t(col) * prm.channels + ch : reinterpret_cast<Record *>(prm.carryOut + size_t(ch) * prm.carryBytes));
}

// workgroup (tile of perTile whole columns, channel): groups of prm.group lanes per column, the lanes of a group stride over its samples
template <class Params, class Acc>
__global__ void __launch_bounds__(kTwinThreads)
sumTileKernel(const Params prm)
{
    const uint32_t tid = threadIdx.x, ch = blockIdx.y;
    long c0, c1;
    tileColumns(prm, c0, c1);
    const uint32_t G = prm.group, sub = tid & (G - 1u), grp = tid / G, groups = uint32_t(kTwinThreads) / G;
    const uint32_t cols = uint32_t(c1 - c0);
    for (uint32_t base = 0; base < cols; base += groups) {                  // (the same trips in every lane: the cross-lane steps see whole waves)
        const uint32_t lc = base + grp;
        const bool mine = lc < cols;
        Acc k{};
        if (mine) {
            long a, b;
            columnSamples(prm, c0 + long(lc), a, b);
            for (long r = a + long(sub); r < b; r += long(G)) k.takeSample(prm, ch, r);
        }
        for (uint32_t o = G >> 1; o > 0; o >>= 1) k.foldLane(int(o));
        if (mine && sub == 0) emitSums(prm, c0 + long(lc), ch, k);
    }
}

// slice blockIdx.z of column blockIdx.x's samples of channel blockIdx.y (an empty slice leaves the zero record)
template <class Params, class Acc>
__global__ void __launch_bounds__(kTwinThreads)
sumSliceKernel(const Params prm)
{
    __shared__ typename Params::Record waves[kTwinThreads / 64];
    const long col = long(blockIdx.x);
    const uint32_t ch = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
    long a, b, sa, sb;
    columnSamples(prm, col, a, b);
    sliceSamples(prm, a, b, s, sa, sb);
    Acc k{};
    for (long r = sa + long(tid); r < sb; r += long(kTwinThreads)) k.takeSample(prm, ch, r);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k.foldLane(o);
    if ((tid & 63u) == 0) k.store(&waves[tid >> 6]);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < kTwinThreads / 64; ++v) k.add(waves[v]);
        k.store(prm.partial + (size_t(s) * size_t(prm.columns) + size_t(col)) * prm.channels + ch);
    }
}

// one thread per (column, channel): the fold of the slices (none: a flush of the carry alone), the carry, the store
template <class Params, class Acc>
__global__ void __launch_bounds__(kTwinThreads)
sumEmitKernel(const Params prm)
{
    const size_t at = size_t(blockIdx.x) * kTwinThreads + threadIdx.x, perSlice = size_t(prm.columns) * prm.channels;
    if (at >= perSlice) return;
    const long col = long(at / prm.channels);
    const uint32_t ch = uint32_t(at % prm.channels);
    Acc k{};
    for (uint32_t s = 0; s < prm.slices; ++s) k.add(prm.partial[size_t(s) * perSlice + at]);
    emitSums(prm, col, ch, k);
}

// The fields the two lanes' kernel arguments share, beside the grid's.  scratch: `planes` q planes of [channels][qStride] words (one for
// loudness, three for band), the partial records behind them
template <class Params, class Filter>
void fillTwin(Params &prm, const Filter &f, uint32_t planes, uint32_t channels, size_t nsamples, uint64_t firstIndex, const void *carryIn, void *carryOut,
              typename Params::Record *d_out, void *scratch)
{
    prm.W = f.W; prm.L = f.L; prm.logL = log2Of(f.L); prm.hist = f.W + f.L - 1;
    prm.tile = runTileOf(f); prm.segs = prm.tile / f.L; prm.lanesPer = uint32_t(kTwinThreads) / prm.segs;
    prm.tileWords = runTileWords(f);
    prm.phase = uint32_t(firstIndex % f.L);
    prm.carryIn = static_cast<const uint8_t *>(carryIn); prm.carryOut = static_cast<uint8_t *>(carryOut);
    prm.carryBytes = twinCarryBytes<typename Params::Record>(f);
    prm.q = static_cast<int32_t *>(scratch); prm.qStride = qStrideOf(nsamples);
    prm.out = d_out;
    prm.partial = reinterpret_cast<typename Params::Record *>(static_cast<uint8_t *>(scratch) + size_t(planes) * prm.qStride * channels * sizeof(int32_t));
}

// The two lanes' launch front: RunKernel over the sample tiles (lds: its dynamic LDS; taps(f, &prm.taps): the lane's table on the device),
// the history, then the column sums in the tile form or in slices; a flush without samples is the emit kernel alone
template <auto RunKernel, class Acc, class Params, class Filter, class Taps>
sgz_status launchTwinLane(const char *word, Params &prm, const ColumnsShape &sh, const Filter &f, uint32_t channels, size_t nsamples, uint32_t m,
                          size_t lds, Taps taps, hipStream_t stream)
{
    const uint64_t blocks = emitBlocks(sh.columns * channels, kTwinThreads);
    if (sgz_status st = fitsOneLaunch(std::max(sh.columns, blocks), word, "columns"); st != SGZ_OK) return st;
    if (nsamples != 0) {
        if (sgz_status st = taps(f, &prm.taps); st != SGZ_OK) return st;
        const uint64_t tiles = (uint64_t(nsamples) + prm.phase + prm.tile - 1) / prm.tile;
        if (sgz_status st = fitsOneLaunch(tiles, word, "samples"); st != SGZ_OK) return st;
        if (sgz_status st = grantRunLds<RunKernel>(lds); st != SGZ_OK) return st;
        hipLaunchKernelGGL(RunKernel, dim3(unsigned(tiles), channels), dim3(kTwinThreads), lds, stream, prm);
        SGZ_HIP(hipGetLastError());
        hipLaunchKernelGGL(historyKernel<Params>, dim3((prm.hist + 1 + kTwinThreads - 1) / kTwinThreads, channels), dim3(kTwinThreads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
        if (sh.slices == 0) {
            prm.perTile = kTwinTile / m;
            prm.group = std::min(pow2AtLeast((m + kTwinRun - 1) / kTwinRun), 64u);
            const uint64_t sumTiles = (sh.columns + prm.perTile - 1) / prm.perTile;
            hipLaunchKernelGGL((sumTileKernel<Params, Acc>), dim3(unsigned(sumTiles), channels), dim3(kTwinThreads), 0, stream, prm);
            SGZ_HIP(hipGetLastError());
            return SGZ_OK;
        }
        hipLaunchKernelGGL((sumSliceKernel<Params, Acc>), dim3(unsigned(sh.columns), channels, sh.slices), dim3(kTwinThreads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((sumEmitKernel<Params, Acc>), dim3(unsigned(blocks)), dim3(kTwinThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

}  // namespace sgz
