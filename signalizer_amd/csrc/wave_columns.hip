// wave_columns.hip -- the waveform lane's reduction: a minimum and a maximum per column of m samples and channel of a linear planar stream,
// with a carried open column (sgz.h, "The waveform lane").  gfx950 only.  The reference has no counterpart: it draws a live ring, never a file.
// What the column lanes share -- the shape of a call, the column, tile and slice bounds, the aligned split of a row, the stage call's front --
// is column_lanes.hpp; this file is what the lane does with a sample.
//   Wv[c][d] = (lo, hi): the least and the greatest of the column's non-NaN samples under the overview's total order (order_key.hpp) --
//   each the sample's own bits; a column of NaNs alone gives 0x7FC00000 twice.  Least and greatest are associative and commutative, so
//   any cut of the stream (calls with a carry) or of a column (lanes, slices) gives the same bits.
// The kernels keep KEY PAIRS (minimum key, maximum key), identities (0xFFFFFFFF, 0).
//   m <= kWvSwitch (1024)   waveTileKernel: one workgroup per (channel, tile), so no column straddles two workgroups.  The tile goes to LDS
//                           once, raw bits, at the same offset within 16 bytes as in memory, four words of padding behind every 64.  Then
//                           groups of G lanes (a power of two near m / 16: a lane per column up to m = 16, a wave per column from m = 513)
//                           take a column each: the lanes stride the column in LDS, log2 G cross-lane steps, the group's first lane folds
//                           the carry (column 0) and stores the pair -- or the carry (the open column).
//                           (Measured, DESIGN.md section 8: with G near m / 4 the cross-lane steps, which go through the LDS pipe, cost
//                           a third of the rate at m = 64; a wave per column straight from memory at m >= 256 was slower than the tile.)
//   else, or slices >= 2    waveSliceKernel: workgroup (column, channel, slice) scans its part of the column from memory (16-byte loads
//                           where the address allows, 4 in flight per lane) -> partial pairs [slices][columns][channels] in scratch;
//                           waveEmitKernel, a launch of its own behind it, folds the slices and the carry and stores (no hand-off
//                           between workgroups inside a launch).  A flush without samples is the emit kernel alone, on the carry.
// Every sample is read from memory once.  Nothing is waited for.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "column_lanes.hpp"
#include "order_key.hpp"

using namespace sgz;

namespace {

constexpr int kWvThreads = 256;
constexpr uint32_t kWvTile = 4096;              // samples of a tile (16 KiB of LDS)
constexpr uint32_t kWvSwitch = 1024;            // the switch-over: columns longer than this take the sliced form
constexpr uint32_t kWvMaxChannels = 64;
constexpr int kWvUnroll = 4;                    // 16-byte loads a lane issues before the first compare
constexpr uint32_t kWvTileWords = kWvTile + 4 + 4 * ((kWvTile + 4) / 64 + 1);      // the lead, and four words of padding per 64 (tileWord)
static_assert(kWvTile == 4u * kWvThreads * kWvUnroll, "a lane moves kWvUnroll 16-byte chunks of a tile");
static_assert(kWvSwitch <= kWvTile, "a short column fits a tile");

struct WaveParams {
    const float *planar;                 // [channels][stride]
    size_t stride;
    long n;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t m, held, channels;
    uint32_t perTile;                    // columns of a tile = kWvTile / m
    uint32_t group;                      // lanes per column in the tile form
    uint32_t slices;
    const float2 *carryIn;               // [channels]: (lo, hi) of column 0's `held` earlier samples (read iff held > 0)
    float2 *carryOut;                    // [channels]: (lo, hi) of the open column
    float2 *wave;                        // [closed][channels]
    uint2 *partial;                      // [slices][columns][channels] key pairs
};

struct KeyPair {
    uint32_t lo, hi;
    __device__ __forceinline__ void take(uint32_t bits)
    {
        lo = min(lo, orderKeyMin(bits));
        hi = max(hi, orderKey(bits));
    }
    __device__ __forceinline__ void fold(uint32_t l, uint32_t h)
    {
        lo = min(lo, l);
        hi = max(hi, h);
    }
};
__device__ __forceinline__ KeyPair noKeys() { return KeyPair{0xffffffffu, 0u}; }

// what a (column, channel) does with its keys: the carry into column 0, then the pair to the output (a closed column) or to the carry
__device__ __forceinline__ void emitColumn(const WaveParams &prm, long col, uint32_t d, KeyPair k)
{
    if (col == 0 && prm.held) {
        const float2 c = prm.carryIn[d];
        k.fold(orderKeyMin(__float_as_uint(c.x)), orderKey(__float_as_uint(c.y)));
    }
    const float2 v = make_float2(__uint_as_float(keyBitsMin(k.lo)), __uint_as_float(keyBits(k.hi)));
    if (col < prm.closed) prm.wave[size_t(col) * prm.channels + d] = v;
    else prm.carryOut[d] = v;
}

// the tile through LDS, then groups of prm.group lanes per column
__global__ void __launch_bounds__(kWvThreads)
waveTileKernel(const WaveParams prm)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[kWvTileWords];
    const uint32_t tid = threadIdx.x, d = blockIdx.y;
    TileBounds t;
    tileBounds(prm, t);
    const long c0 = t.c0, c1 = t.c1, a = t.a, b = t.b;
    const uint32_t count = uint32_t(b - a);                                 // <= perTile * m <= kWvTile
    const float *g = prm.planar + size_t(d) * prm.stride + size_t(a);
    // the tile sits in LDS `lead` words in: 16-byte chunks of memory are 16-byte chunks of LDS
    const uint32_t lead = uint32_t(reinterpret_cast<uintptr_t>(g) >> 2) & 3u;
    uint32_t head;
    size_t vecs, tail;
    splitAligned(g, size_t(count), head, vecs, tail);
    if (tid < head) tile[tileWord(lead + tid)] = __float_as_uint(g[tid]);
    if (tid < count - uint32_t(tail)) tile[tileWord(lead + uint32_t(tail) + tid)] = __float_as_uint(g[tail + tid]);
    const uint4 *gv = reinterpret_cast<const uint4 *>(g + head);
    uint4 v[kWvUnroll];
#pragma unroll
    for (int j = 0; j < kWvUnroll; ++j)
        v[j] = tid + uint32_t(j) * kWvThreads < vecs ? gv[tid + uint32_t(j) * kWvThreads] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int j = 0; j < kWvUnroll; ++j)                                     // (lead + head is a multiple of 4 wherever vecs > 0)
        if (tid + uint32_t(j) * kWvThreads < vecs) *reinterpret_cast<uint4 *>(tile + tileWord(lead + head + 4u * (tid + uint32_t(j) * kWvThreads))) = v[j];
    __syncthreads();
    const uint32_t G = prm.group, sub = tid & (G - 1u), grp = tid / G, groups = uint32_t(kWvThreads) / G;
    const uint32_t cols = uint32_t(c1 - c0);
    for (uint32_t base = 0; base < cols; base += groups) {                  // (the same trips in every lane: the cross-lane steps see whole waves)
        const uint32_t lc = base + grp;
        const bool mine = lc < cols;
        KeyPair k = noKeys();
        if (mine) {
            long ca, cb;
            columnSamples(prm, c0 + long(lc), ca, cb);
            const uint32_t end = lead + uint32_t(cb - a);
#pragma unroll 4
            for (uint32_t i = lead + uint32_t(ca - a) + sub; i < end; i += G) k.take(tile[tileWord(i)]);
        }
        for (uint32_t o = G >> 1; o > 0; o >>= 1) k.fold(__shfl_xor(k.lo, int(o)), __shfl_xor(k.hi, int(o)));
        if (mine && sub == 0) emitColumn(prm, c0 + long(lc), d, k);
    }
}

// this lane's share of the key pair of row[a, b), `lanes` lanes side by side: 16-byte loads between the first and the last 16-byte boundary,
// kWvUnroll of them in flight, up to three scalar loads on either side
__device__ __forceinline__ KeyPair scanLanes(const float *row, long a, long b, uint32_t lane, uint32_t lanes)
{
    KeyPair k = noKeys();
    if (b <= a) return k;
    const float *g = row + a;
    const size_t count = size_t(b - a);
    uint32_t head;
    size_t vecs, tail;
    splitAligned(g, count, head, vecs, tail);
    if (lane < head) k.take(__float_as_uint(g[lane]));
    if (lane < count - tail) k.take(__float_as_uint(g[tail + lane]));
    const uint4 *gv = reinterpret_cast<const uint4 *>(g + head);
    for (size_t i = lane; i < vecs; i += size_t(lanes) * kWvUnroll) {
        uint4 v[kWvUnroll];
#pragma unroll
        for (int j = 0; j < kWvUnroll; ++j) {
            const size_t at = i + size_t(j) * lanes;
            v[j] = at < vecs ? gv[at] : make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);      // (a NaN takes no part)
        }
#pragma unroll
        for (int j = 0; j < kWvUnroll; ++j) { k.take(v[j].x); k.take(v[j].y); k.take(v[j].z); k.take(v[j].w); }
    }
    return k;
}

// every lane ends with the fold of all 64
__device__ __forceinline__ KeyPair waveFold(KeyPair k)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k.fold(__shfl_xor(k.lo, o), __shfl_xor(k.hi, o));
    return k;
}

// the key pair of row[a, b), the workgroup's lanes side by side; valid in thread 0
__device__ __forceinline__ KeyPair scanSamples(const float *row, long a, long b, uint2 *lds /*[4]*/)
{
    const uint32_t tid = threadIdx.x;
    KeyPair k = waveFold(scanLanes(row, a, b, tid, uint32_t(kWvThreads)));
    if ((tid & 63u) == 0) lds[tid >> 6] = make_uint2(k.lo, k.hi);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWvThreads / 64; ++w) k.fold(lds[w].x, lds[w].y);
    }
    return k;
}

// slice blockIdx.z of column blockIdx.x's samples of channel blockIdx.y (an empty slice -- more slices than samples -- leaves the identities)
__global__ void __launch_bounds__(kWvThreads)
waveSliceKernel(const WaveParams prm)
{
    __shared__ uint2 lds[kWvThreads / 64];
    const long col = long(blockIdx.x);
    const uint32_t d = blockIdx.y, s = blockIdx.z;
    long a, b, sa, sb;
    columnSamples(prm, col, a, b);
    sliceSamples(prm, a, b, s, sa, sb);
    const KeyPair k = scanSamples(prm.planar + size_t(d) * prm.stride, sa, sb, lds);
    if (threadIdx.x == 0) prm.partial[(size_t(s) * size_t(prm.columns) + size_t(col)) * prm.channels + d] = make_uint2(k.lo, k.hi);
}

// one thread per (column, channel): the fold over the slices (none: a flush of the carry alone), the carry, the store
__global__ void __launch_bounds__(kWvThreads)
waveEmitKernel(const WaveParams prm)
{
    const size_t at = size_t(blockIdx.x) * kWvThreads + threadIdx.x, perSlice = size_t(prm.columns) * prm.channels;
    if (at >= perSlice) return;
    const uint2 *q = prm.partial + at;
    KeyPair k = noKeys();
    for (uint32_t s = 0; s < prm.slices; s += 8) {
        uint2 p[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] = s + j < prm.slices ? q[size_t(s + j) * perSlice] : make_uint2(0xffffffffu, 0u);
#pragma unroll
        for (int j = 0; j < 8; ++j) k.fold(p[j].x, p[j].y);
    }
    emitColumn(prm, long(at / prm.channels), uint32_t(at % prm.channels), k);
}

}  // namespace

namespace sgz {

ColumnsShape waveColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices)
{
    return columnsShape(channels, nsamples, m, held, flush, slices, kWvSwitch, sizeof(uint2), 0);
}

sgz_status runWaveColumns(const ColumnsShape &sh, const float *d_planar, size_t channelStride, uint32_t channels, size_t nsamples, uint32_t m,
                          uint32_t held, const float *carryIn, float *carryOut, float *d_wave, void *scratch, hipStream_t stream)
{
    if (!sh.launch) return SGZ_OK;
    WaveParams prm{};
    fillGrid(prm, sh, d_planar, channelStride, nsamples, m, held);
    prm.channels = channels;
    prm.carryIn = reinterpret_cast<const float2 *>(carryIn); prm.carryOut = reinterpret_cast<float2 *>(carryOut);
    prm.wave = reinterpret_cast<float2 *>(d_wave); prm.partial = static_cast<uint2 *>(scratch);
    return launchPlainLane(waveTileKernel, waveSliceKernel, waveEmitKernel, kWvThreads, "wave", prm, sh, channels, nsamples, 1, [m](WaveParams &p) {
        p.perTile = kWvTile / m;
        p.group = pow2AtLeast((m + 15u) / 16u);                   // (1 .. 64: sixteen samples a lane, or as near as a power of two gets)
    }, stream);
}

}  // namespace sgz

extern "C" {

void sgz_wave_columns_limits(uint32_t *switch_over, uint32_t *tile_samples)
{
    if (switch_over) *switch_over = kWvSwitch;
    if (tile_samples) *tile_samples = kWvTile;
}

sgz_status sgz_stage_wave_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, uint32_t m, uint32_t held,
                                  int flush, uint32_t slices, float *d_carry, float *d_wave, void *stream)
{
    const StageFront front{"sgz_stage_wave_columns", "channels", kWvMaxChannels, "d_wave", 8, false, 62};
    return stageColumns(front, SGZ_OK, d_planar, channel_stride, channels, nsamples, m, held, flush, 0, 0, slices, d_carry, d_wave, stream, waveColumnsShape,
                        size_t(channels) * sizeof(float2), noStep, [&](const ColumnsShape &sh, const void *carryIn, void *scratch, hipStream_t s) {
                            return runWaveColumns(sh, d_planar, channel_stride, channels, nsamples, m, held, static_cast<const float *>(carryIn), d_carry, d_wave, scratch, s);
                        });
}

}  // extern "C"
