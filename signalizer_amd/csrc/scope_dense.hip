// scope_dense.hip -- the Oscilloscope's per-column min / max vertex stream (sgz_scope_dense_*).  gfx950 only.
//
// Below one pixel per sample drawWavePlot draws its sample-space Linear list (OscilloscopeRendering.cpp:575-578, :707-741): one vertex
// per sample, whatever the window.  A compute-only GPU hands every vertex over PCIe to the GPU that rasterises them onto a couple of
// thousand pixel columns.  The kernels here reduce that list V[0 .. n) on the device: for each of `cols` = min(columns, n) equal slices
// (column b = the indices  ceil(b n / cols) <= i < ceil((b + 1) n / cols)) the vertex with the smallest y and the vertex with the
// largest y, in stream order -- 2 cols vertices, a subsequence of V, bit for bit.  The reference has no counterpart.
//
// The rule (include/sgz.h): lo(b) = the lowest index whose y equals the column's minimum over its non-NaN y under IEEE `<` (-0 and +0
// tie; ties go to the lowest index), hi(b) likewise for the maximum, both the column's first index when every y is NaN.  As a reduction:
// (value, index) pairs ordered by value, then by index, with (+inf, kNone) / (-inf, kNone) as the identities -- a NaN never wins a
// compare, a real +-inf beats the identity by its index.  Associative and commutative, so any tree gives the same bytes.
//
// Two forms, chosen by the longest column's length  ceil(n / cols):
//   <= kLongColumn (1024 samples)  scopeDenseWaveKernel: a wave per column, four columns per workgroup; the lanes stride the column
//      (coalesced 256-byte reads), six cross-lane (value, index) steps, lanes 0 and 1 emit a vertex each.
//   >  kLongColumn                 scopeDenseChunkKernel: the column in chunks of kChunk (2048) samples, a 256-thread workgroup each
//      (eight loads per thread, all in flight), partial (min, idx, max, idx) records to scratch the caller owns; then
//      scopeDenseFoldKernel, a workgroup per column, folds the column's records and emits.
// Samples are read once (twice for Mid / Side: two planes); the colour ring is read for the two winners only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "runtime.hpp"
#include "fft_common.hpp"      // ldsBarrier
#include "scope_ring.hpp"

#pragma clang fp contract(off)

using namespace sgz;

namespace {

constexpr uint32_t kLongColumn = 1024;        // the switch-over: columns longer than this take the chunked form
constexpr uint32_t kChunk = 2048;             // samples per workgroup of the chunked form
constexpr uint32_t kNone = 0xffffffffu;       // "no sample yet" (every index is < 2^31)

struct DenseArgs {
    const float *ringA, *ringB;               // the evaluator's planes (+ blockIdx.y * ringStride: the stage call's channels)
    size_t ringStride;
    const uint32_t *d_cursor;                 // the ring's write cursor in device memory; nullptr: a ring in time order (cursor 0)
    const uint32_t *colRing;                  // per-sample colours beside ringA (nullptr: `key`)
    void *out;                                // float3 [2 cols] (XY: float2 [channels][2 cols])
    uint32_t *rgba;                           // RGBA8 [2 cols] or nullptr
    uint32_t evalMode, len, cap, key;
    uint32_t n, cols;
    long start0;                              // vertex i reads logical sample start0 + i (= -bufferOffset + i)
};

struct Extrema {
    float lo, hi;
    uint32_t loAt, hiAt;
    __device__ __forceinline__ void take(float v, uint32_t i)
    {
        if (v < lo || (v == lo && i < loAt)) { lo = v; loAt = i; }
        if (v > hi || (v == hi && i < hiAt)) { hi = v; hiAt = i; }
    }
};
__device__ __forceinline__ Extrema noExtrema() { return Extrema{__builtin_inff(), -__builtin_inff(), kNone, kNone}; }

__device__ __forceinline__ uint32_t columnStart(uint32_t b, uint32_t n, uint32_t cols)
{
    return uint32_t((uint64_t(b) * n + (cols - 1)) / cols);      // ceil(b n / cols)
}

// every lane ends with the fold of all 64
__device__ __forceinline__ Extrema waveFold(Extrema e)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float lo = __shfl_xor(e.lo, o), hi = __shfl_xor(e.hi, o);
        const uint32_t loAt = __shfl_xor(e.loAt, o), hiAt = __shfl_xor(e.hiAt, o);
        if (lo < e.lo || (lo == e.lo && loAt < e.loAt)) { e.lo = lo; e.loAt = loAt; }
        if (hi > e.hi || (hi == e.hi && hiAt < e.hiAt)) { e.hi = hi; e.hiAt = hiAt; }
    }
    return e;
}

// a 256-thread workgroup's fold: valid in thread 0
__device__ __forceinline__ Extrema blockFold(Extrema e, float4 *lds /*[4]*/)
{
    e = waveFold(e);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = make_float4(e.lo, __uint_as_float(e.loAt), e.hi, __uint_as_float(e.hiAt));
    ldsBarrier();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float4 r = lds[w];
            const uint32_t loAt = __float_as_uint(r.y), hiAt = __float_as_uint(r.w);
            if (r.x < e.lo || (r.x == e.lo && loAt < e.loAt)) { e.lo = r.x; e.loAt = loAt; }
            if (r.z > e.hi || (r.z == e.hi && hiAt < e.hiAt)) { e.hi = r.z; e.hiAt = hiAt; }
        }
    }
    return e;
}

// samples first, first + step, .. < last of the strip, the evaluator fixed at compile time (no branch per sample); UNROLL loads in flight
template <uint32_t MODE, int UNROLL>
__device__ __forceinline__ Extrema scanStrided(const float *a, const float *b, const DenseArgs &g, uint32_t cursor, uint32_t first,
                                               uint32_t last, uint32_t step)
{
    Extrema e = noExtrema();
    if (first >= last) return e;
    RingWalk w(g.start0 + long(first), step, cursor, g.cap, g.len);
    uint32_t i = first;
    while (i < last) {
        float v[UNROLL];
#pragma unroll
        for (int k = 0; k < UNROLL; ++k) {
            const bool in = i + uint32_t(k) * step < last;
            v[k] = in ? evalSample(a, b, MODE, w.phys) : __builtin_nanf("");     // (a NaN never wins)
            w.next();
        }
#pragma unroll
        for (int k = 0; k < UNROLL; ++k) e.take(v[k], i + uint32_t(k) * step);
        i += uint32_t(UNROLL) * step;
    }
    return e;
}

template <int UNROLL>
__device__ __forceinline__ Extrema scanEvaluator(const float *a, const float *b, const DenseArgs &g, uint32_t cursor, uint32_t first,
                                                 uint32_t last, uint32_t step)
{
    if (g.evalMode == 1u) return scanStrided<1u, UNROLL>(a, b, g, cursor, first, last, step);
    if (g.evalMode == 2u) return scanStrided<2u, UNROLL>(a, b, g, cursor, first, last, step);
    return scanStrided<0u, UNROLL>(a, b, g, cursor, first, last, step);
}

// vertex k (0, 1) of column b: V[min(lo, hi)], V[max(lo, hi)], copied as scopeWaveLinearKernel writes them
template <bool XY>
__device__ __forceinline__ void emitVertex(const DenseArgs &g, const float *a, const float *b, uint32_t cursor, uint32_t column,
                                           uint32_t first, const Extrema &e, uint32_t k)
{
    const uint32_t lo = e.loAt == kNone ? first : e.loAt, hi = e.hiAt == kNone ? first : e.hiAt;     // kNone: every y is NaN
    const uint32_t at = k ? max(lo, hi) : min(lo, hi);
    const uint32_t idx = ringPhys(g.start0 + long(at), cursor, g.cap, g.len);
    const float y = evalSample(a, b, g.evalMode, idx);
    const size_t o = 2 * size_t(column) + size_t(k);
    if constexpr (XY) {
        reinterpret_cast<float2 *>(g.out)[size_t(blockIdx.y) * 2 * g.cols + o] = make_float2(float(at), y);
    } else {
        reinterpret_cast<float3 *>(g.out)[o] = make_float3(float(at), y, 0.f);
        if (g.rgba) g.rgba[o] = g.colRing ? g.colRing[idx] : g.key;
    }
}

// Short columns: a wave per column, four columns per workgroup
template <bool XY>
__global__ void __launch_bounds__(256) scopeDenseWaveKernel(const DenseArgs g)
{
    const uint32_t lane = threadIdx.x & 63u, column = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (column >= g.cols) return;                                  // (whole waves; no barrier in this kernel)
    const float *a = g.ringA + size_t(blockIdx.y) * g.ringStride, *b = g.ringB + size_t(blockIdx.y) * g.ringStride;
    const uint32_t cursor = g.d_cursor ? *g.d_cursor : 0u;
    const uint32_t first = columnStart(column, g.n, g.cols), last = columnStart(column + 1, g.n, g.cols);
    const Extrema e = waveFold(scanEvaluator<4>(a, b, g, cursor, first + lane, last, 64u));
    if (lane < 2) emitVertex<XY>(g, a, b, cursor, column, first, e, lane);       // (every lane holds the fold: one vertex each)
}

// Long columns, pass 1: workgroup (column, chunk) -> one partial record  part[channel][column][chunk]
__global__ void __launch_bounds__(256) scopeDenseChunkKernel(const DenseArgs g, uint32_t chunksPerColumn, float4 *part)
{
    __shared__ float4 lds[4];
    const uint32_t column = blockIdx.x / chunksPerColumn, chunk = blockIdx.x - column * chunksPerColumn;
    const float *a = g.ringA + size_t(blockIdx.y) * g.ringStride, *b = g.ringB + size_t(blockIdx.y) * g.ringStride;
    const uint32_t cursor = g.d_cursor ? *g.d_cursor : 0u;
    const uint32_t first = columnStart(column, g.n, g.cols), last = columnStart(column + 1, g.n, g.cols);
    // (a column one sample shorter than the longest may leave its last chunk empty: that record is the identity)
    const uint64_t from = uint64_t(first) + uint64_t(chunk) * kChunk;
    const uint32_t lo = from < last ? uint32_t(from) : last, hi = from + kChunk < last ? uint32_t(from + kChunk) : last;
    const Extrema e = blockFold(scanEvaluator<int(kChunk / 256)>(a, b, g, cursor, lo + threadIdx.x, hi, 256u), lds);
    if (threadIdx.x == 0)
        part[size_t(blockIdx.y) * gridDim.x + blockIdx.x] = make_float4(e.lo, __uint_as_float(e.loAt), e.hi, __uint_as_float(e.hiAt));
}

// Long columns, pass 2: a workgroup per column folds its records and emits
template <bool XY>
__global__ void __launch_bounds__(256) scopeDenseFoldKernel(const DenseArgs g, uint32_t chunksPerColumn, const float4 *part)
{
    __shared__ float4 lds[4];
    const uint32_t column = blockIdx.x;
    const float4 *mine = part + (size_t(blockIdx.y) * g.cols + column) * chunksPerColumn;
    Extrema e = noExtrema();
    for (uint32_t c = threadIdx.x; c < chunksPerColumn; c += 256u) {
        const float4 r = mine[c];
        const uint32_t loAt = __float_as_uint(r.y), hiAt = __float_as_uint(r.w);
        if (r.x < e.lo || (r.x == e.lo && loAt < e.loAt)) { e.lo = r.x; e.loAt = loAt; }
        if (r.z > e.hi || (r.z == e.hi && hiAt < e.hiAt)) { e.hi = r.z; e.hiAt = hiAt; }
    }
    e = blockFold(e, lds);
    if (threadIdx.x == 0) {
        const float *a = g.ringA + size_t(blockIdx.y) * g.ringStride, *b = g.ringB + size_t(blockIdx.y) * g.ringStride;
        const uint32_t cursor = g.d_cursor ? *g.d_cursor : 0u, first = columnStart(column, g.n, g.cols);
        emitVertex<XY>(g, a, b, cursor, column, first, e, 0u);
        emitVertex<XY>(g, a, b, cursor, column, first, e, 1u);
    }
}

uint32_t longestColumn(size_t n, uint32_t cols) { return uint32_t((n + cols - 1) / cols); }
uint32_t chunksPerColumn(size_t n, uint32_t cols) { return (longestColumn(n, cols) + kChunk - 1) / kChunk; }

template <bool XY>
hipError_t launchDense(const DenseArgs &g, uint32_t channels, void *scratch, hipStream_t stream)
{
    if (longestColumn(g.n, g.cols) <= kLongColumn) {
        hipLaunchKernelGGL(scopeDenseWaveKernel<XY>, dim3((g.cols + 3) / 4, channels), dim3(256), 0, stream, g);
        return hipGetLastError();
    }
    const uint32_t per = chunksPerColumn(g.n, g.cols);
    hipLaunchKernelGGL(scopeDenseChunkKernel, dim3(g.cols * per, channels), dim3(256), 0, stream, g, per, static_cast<float4 *>(scratch));
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(scopeDenseFoldKernel<XY>, dim3(g.cols, channels), dim3(256), 0, stream, g, per, static_cast<const float4 *>(scratch));
    return hipGetLastError();
}

}  // namespace

namespace sgz {

// bytes of partial records one strip of n samples in `columns` columns needs (0: the short form, no scratch)
size_t scopeDenseScratchBytes(size_t n, uint32_t columns)
{
    const uint32_t cols = uint32_t(std::min<size_t>(columns, n));
    if (cols == 0 || longestColumn(n, cols) <= kLongColumn) return 0;
    return size_t(cols) * chunksPerColumn(n, cols) * sizeof(float4);
}

// One evaluator's dense strip of the handle's front ring into DEVICE buffers (d_xyz float3 [2 cols], d_rgba RGBA8 [2 cols] or nullptr).
// ringA / ringB / colRing / size / cap / d_cursor as launchScopeVertices (scope_vector.hip); n, start0: the frame's Linear strip
// (scopeLinearExtent); scratch: scopeDenseScratchBytes(n, columns) bytes.  *points = 2 cols.
hipError_t launchScopeDense(const float *ringA, const float *ringB, uint32_t evalMode, uint32_t size, uint32_t cap, const uint32_t *d_cursor,
                            size_t n, long start0, uint32_t columns, uint32_t key, const uint32_t *colRing, float *d_xyz, uint32_t *d_rgba,
                            void *scratch, size_t *points, hipStream_t stream)
{
    if (n == 0 || n >= (size_t(1) << 31) || columns == 0 || size == 0 || cap < size) return hipErrorInvalidValue;
    DenseArgs g{};
    g.ringA = ringA; g.ringB = ringB; g.ringStride = 0; g.d_cursor = d_cursor; g.colRing = colRing;
    g.out = d_xyz; g.rgba = d_rgba;
    g.evalMode = evalMode; g.len = size; g.cap = cap; g.key = key;
    g.n = uint32_t(n); g.cols = uint32_t(std::min<size_t>(columns, n));
    g.start0 = start0;
    *points = 2 * size_t(g.cols);
    return launchDense<false>(g, 1, scratch, stream);
}

}  // namespace sgz

extern "C" {

sgz_status sgz_scope_dense_device(const float *d_ring, size_t len, size_t stride, uint32_t channels, size_t n, uint32_t columns,
                                  float *d_xy, void *stream)
{
    if (!d_ring || !d_xy || len == 0 || len >= (size_t(1) << 31) || channels == 0 || channels > 65535u || n == 0 || n >= (size_t(1) << 31)
        || columns == 0)
        return fail(SGZ_EINVAL, "bad scope arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DenseArgs g{};
    g.ringA = g.ringB = d_ring; g.ringStride = stride;
    g.out = d_xy;
    g.len = g.cap = uint32_t(len);
    g.n = uint32_t(n); g.cols = uint32_t(std::min<size_t>(columns, n));
    g.start0 = -long(n);                                   // the newest n samples: vertex i reads ring[(len - n + i) mod len]
    StreamScratch scr(s);
    if (const size_t bytes = scopeDenseScratchBytes(n, columns) * channels; bytes) SGZ_HIP(scr.get(bytes));
    SGZ_HIP(launchDense<true>(g, channels, scr.p, s));
    return SGZ_OK;
}

}  // extern "C"
