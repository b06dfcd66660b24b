// loudness_columns.hip -- the loudness lane's reduction: one sgz_loudness_record (the sum of the squared K-weighted samples, the count) per
// column of m samples and channel of a linear planar stream, with a carried open column and a carried sample history (sgz.h, "The loudness
// lane"); and the lane's host helpers: the filter of a sample rate, the tap table, the fold of kept records, the readout of a run of columns
// and the gated integrated loudness.  gfx950 only.  The reference has no counterpart: its meters are live one-pole filters.
//   v = (int32) clamp(rintf(x 2^23), -2^26, +2^26), a NaN is v = 0 and is not counted.  The sample axis is cut into segments of L samples on
//   an absolute grid.  The state of the two biquads at a segment's start is an exact integer FIR over the last W quantised samples (taps at
//   2^32, a 64-bit sum, any order), converted to fp64 once; from there the fp64 recurrence runs over the segment's L samples in one fixed
//   order with no contraction (the pragma below, for host and device alike).  q = rint(z) clamped to 32 bits, the record sums q^2 in 128
//   bits: every output depends on nothing but the samples, so any cut of the stream (calls with a carry) or of a column gives the same bytes.
// Three steps, each a launch of its own behind the other (no hand-off between workgroups inside a launch):
//   loudnessRunKernel       one workgroup per (tile of T = max(4096, L) samples on the segment grid, channel).  The tile goes to LDS quantised,
//                           behind a W-sample halo: the call's samples before the tile, the carried history before those, zeros at the stream's
//                           start.  Segment-start dot products: the 256 lanes are T / L segments x P lanes; a lane walks taps k = sub, sub + P,
//                           .. and reads one sample and one 16-byte row of the table C[k][0..3] for all four state components (32 x 32 -> 64-bit
//                           multiply-adds); the P partial sums of a (segment, component) are folded with integer adds by wave shuffles (through LDS where
//                           P > 64).  Which wave runs the segments rotates with the workgroup.  LDS index
//                           i lies at word i + (i / L) P, so that the lanes of different segments fall on different banks.  Then one lane per
//                           segment runs its L sequential steps out of LDS and leaves q where v was; the workgroup stores the tile's q in rows
//                           to stream-ordered scratch [channels][n].  A segment that began before the call is re-run from its start out of the
//                           history; its earlier samples are not stored, so they are not counted again.
//   loudnessHistoryKernel   the new carry but for an open column: the last W + L - 1 quantised samples of (the old history, the call).
//   the column sums         of q^2 and of the non-NaN samples, in the level lane's structure: m <= kLdSwitch (1024) loudnessSumTileKernel, a
//                           workgroup per (tile of 4096 / m whole columns, channel), groups of lanes per column; longer columns or slices >= 2
//                           loudnessSumSliceKernel into partial records [slices][columns][channels] + loudnessEmitKernel.  A flush without
//                           samples is the emit kernel alone, on the carry.
// Built: the integer form of the dot products (v_mad_i64_i32).  An fp64 form would need every tap split in two to stay exact (32-bit taps times
// 27-bit samples over W terms pass 2^53), twice the multiply-adds of the form that is exact as it stands.  The sums are a pass of their own over
// q in scratch, not fused into the run: columns and segments do not align, a lane of the run owns a segment, and the pass costs one read of q.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

#include "runtime.hpp"
#include "scope_ring.hpp"      // StreamScratch

// The definition's step is one IEEE operation per *, + and -: nothing in this file may be contracted into an FMA, on the host (the tap table)
// or on the device (the segment runs).  hipcc contracts by default.
#pragma clang fp contract(off)

using namespace sgz;

namespace {

constexpr int kLdThreads = 256;
constexpr uint32_t kLdTile = 4096;               // samples of a run tile (a segment longer than this is a tile of its own) and of a sum tile
constexpr uint32_t kLdSwitch = 1024;             // the switch-over of the column sums: longer columns take the sliced form
constexpr uint32_t kLdMaxSlices = 64, kLdMaxChannels = 64;
constexpr uint32_t kLdMaxW = 65536, kLdMinL = 16;
constexpr uint32_t kLdDeviceMaxW = 16384;        // the halo and a tile fit the 160 KiB of LDS up to here
constexpr uint32_t kLdBatch = 8;                 // loads a lane of the run kernel issues before it uses the first
constexpr uint32_t kLdRun = 16;                  // samples of a lane in the sum tile
constexpr double kLdTapScale = 4294967296.0;     // S = 32
constexpr uint64_t kLdTapSumBound = uint64_t(1) << 36;     // 2^26 sum |C| < 2^62
static_assert(sizeof(sgz_loudness_record) == 32 && sizeof(sgz_loudness_filter) == 88, "sgz.h documents 32 and 88 bytes");

// ---- the definition's step and the tap table (host) -----------------------------------------------------------------------------------------
struct LdState { double s1, s2, t1, t2; };
struct LdCoef { double b0[3], a0[2], b1[3], a1[2]; };

__host__ __device__ __forceinline__ double ldStep(const LdCoef &f, LdState &st, double x)
{
    // (every operation on its own: see the pragma above)
    const double y = f.b0[0] * x + st.s1;
    st.s1 = (f.b0[1] * x - f.a0[0] * y) + st.s2;
    st.s2 = f.b0[2] * x - f.a0[1] * y;
    const double z = f.b1[0] * y + st.t1;
    st.t1 = (f.b1[1] * y - f.a1[0] * z) + st.t2;
    st.t2 = f.b1[2] * y - f.a1[1] * z;
    return z;
}

LdCoef coefOf(const sgz_loudness_filter &f)
{
    LdCoef c;
    for (int i = 0; i < 3; ++i) { c.b0[i] = f.b[0][i]; c.b1[i] = f.b[1][i]; }
    for (int i = 0; i < 2; ++i) { c.a0[i] = f.a[0][i]; c.a1[i] = f.a[1][i]; }
    return c;
}

bool pow2(uint32_t v) { return v && !(v & (v - 1)); }

bool shapeOk(const sgz_loudness_filter &f) { return pow2(f.W) && pow2(f.L) && f.L >= kLdMinL && f.L <= f.W && f.W <= kLdMaxW; }

// C[c][k] at taps[c * W + k]; false where the filter is refused
bool buildTaps(const sgz_loudness_filter &f, int32_t *taps)
{
    if (!shapeOk(f)) return false;
    const LdCoef c = coefOf(f);
    LdState st{0.0, 0.0, 0.0, 0.0};
    uint64_t sum[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < f.W; ++k) {
        (void)ldStep(c, st, k == 0 ? 1.0 : 0.0);
        const double h[4] = {st.s1, st.s2, st.t1, st.t2};
        for (int q = 0; q < 4; ++q) {
            const double t = std::nearbyint(kLdTapScale * h[q]);          // (round to nearest even: the default mode; the scale is exact)
            if (!(t >= -2147483648.0 && t <= 2147483647.0)) return false;  // (a NaN fails too)
            const int32_t v = int32_t(t);
            taps[size_t(q) * f.W + k] = v;
            sum[q] += uint64_t(v < 0 ? -int64_t(v) : int64_t(v));
        }
    }
    return std::max(std::max(sum[0], sum[1]), std::max(sum[2], sum[3])) < kLdTapSumBound;
}

// ---- the table on the device: one per (device, filter), made at the filter's first use and kept ----------------------------------------------
struct DeviceTaps { int dev; sgz_loudness_filter f; int4 *d; };
std::mutex g_tapsMutex;
std::vector<DeviceTaps> g_taps;

// rows C[k][0..3] of 16 bytes; the first use of a filter on a device uploads them (the one blocking step of the stage call)
sgz_status deviceTaps(const sgz_loudness_filter &f, const int4 **out)
{
    int dev = 0;
    SGZ_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_tapsMutex);
    for (const DeviceTaps &t : g_taps)
        if (t.dev == dev && std::memcmp(&t.f, &f, sizeof f) == 0) { *out = t.d; return SGZ_OK; }
    std::vector<int32_t> planes(size_t(4) * f.W), rows(size_t(4) * f.W);
    if (!buildTaps(f, planes.data())) return fail(SGZ_EINVAL, "loudness: the filter is refused (sgz_loudness_taps)");
    for (uint32_t k = 0; k < f.W; ++k)
        for (int q = 0; q < 4; ++q) rows[size_t(k) * 4 + q] = planes[size_t(q) * f.W + k];
    DeviceTaps t{dev, f, nullptr};
    SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&t.d), rows.size() * sizeof(int32_t)));
    if (const hipError_t e = hipMemcpy(t.d, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice); e != hipSuccess) {
        (void)hipFree(t.d);
        return hipFail(e, "hipMemcpy(loudness taps)");
    }
    g_taps.push_back(t);
    *out = t.d;
    return SGZ_OK;
}

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------------
struct LoudnessParams {
    const float *planar;                 // [channels][stride]
    size_t stride;
    long n;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t m, held, channels;
    uint32_t continued;                  // the history in carryIn holds the samples before this call (else zeros)
    uint32_t W, L, logL, hist;           // hist = W + L - 1
    uint32_t tileWords;                  // LDS words of the halo and the tile, padding included
    uint32_t tile, segs, lanesPer;       // the run tile: T samples = segs segments, lanesPer = 256 / segs lanes per segment in the dot products
    uint32_t phase;                      // first_index % L: the call's first sample within its segment
    uint32_t perTile, group, slices;     // the column sums, as the true-peak lane's
    LdCoef coef;
    const int4 *taps;                    // [W]: C[k][0..3]
    const uint8_t *carryIn;              // [channels][carryBytes]: the open column, then the history (oldest first), then a zero word
    uint8_t *carryOut;
    size_t carryBytes;
    int32_t *q;                          // [channels][qStride]: q of the call's samples
    size_t qStride;
    sgz_loudness_record *out;            // [closed][channels]
    sgz_loudness_record *partial;        // [slices][columns][channels]
};

__device__ __forceinline__ const sgz_loudness_record *carryOpen(const uint8_t *carry, size_t bytes, uint32_t ch)
{
    return reinterpret_cast<const sgz_loudness_record *>(carry + size_t(ch) * bytes);
}
__device__ __forceinline__ const int32_t *carryHist(const uint8_t *carry, size_t bytes, uint32_t ch)
{
    return reinterpret_cast<const int32_t *>(carry + size_t(ch) * bytes + sizeof(sgz_loudness_record));
}

// the quantiser, 0 for a NaN (x 2^23 is exact or overflows to an infinity, which the clamp takes)
__device__ __forceinline__ int32_t quantise(float x)
{
    const float r = __builtin_amdgcn_fmed3f(rintf(x * 0x1p23f), -0x1p26f, 0x1p26f);
    return x != x ? 0 : int32_t(r);
}

// what the filter sees at sample r of the call, r >= -hist: the call's own sample, the carried history in front of it, zeros behind the call
__device__ __forceinline__ int32_t filterInput(const LoudnessParams &prm, uint32_t ch, long r)
{
    if (r >= prm.n) return 0;
    if (r >= 0) return quantise(prm.planar[size_t(ch) * prm.stride + size_t(r)]);
    return prm.continued ? carryHist(prm.carryIn, prm.carryBytes, ch)[long(prm.hist) + r] : 0;
}

// LDS word of the tile's sample index i (0 = the halo's first): a shift of lanesPer words per segment keeps the segments' lanes on different banks
__device__ __forceinline__ uint32_t ldWord(const LoudnessParams &prm, uint32_t i) { return i + (i >> prm.logL) * prm.lanesPer; }

__global__ void __launch_bounds__(kLdThreads)
loudnessRunKernel(const LoudnessParams prm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    // [segs][4] the segments' start states, the tile, and -- only where a segment's lanes are more than a wave -- [256][4] partial dot products
    double *start = reinterpret_cast<double *>(ldsRaw);
    int32_t *tile = reinterpret_cast<int32_t *>(ldsRaw + size_t(prm.segs) * 4 * 8);
    long long *part = reinterpret_cast<long long *>(ldsRaw + size_t(prm.segs) * 4 * 8 + size_t(prm.tileWords) * 4);
    const uint32_t tid = threadIdx.x, ch = blockIdx.y;
    const long r0 = long(blockIdx.x) * long(prm.tile) - long(prm.phase);               // the tile's first sample, on the segment grid (>= -(L - 1))
    // 1. the halo and the tile, quantised
    const uint32_t words = prm.W + prm.tile;
    for (uint32_t base = tid; base < words; base += kLdBatch * kLdThreads) {             // (kLdBatch loads of a lane in flight together)
        int32_t v[kLdBatch];
#pragma unroll
        for (uint32_t j = 0; j < kLdBatch; ++j) {
            const uint32_t i = base + j * kLdThreads;
            v[j] = i < words ? filterInput(prm, ch, r0 - long(prm.W) + long(i)) : 0;
        }
#pragma unroll
        for (uint32_t j = 0; j < kLdBatch; ++j) {
            const uint32_t i = base + j * kLdThreads;
            if (i < words) tile[ldWord(prm, i)] = v[j];
        }
    }
    __syncthreads();
    // 2. the dot products: lane (seg, sub) takes taps sub, sub + lanesPer, .. of its segment, all four components from one sample
    const uint32_t seg = tid / prm.lanesPer, sub = tid % prm.lanesPer;
    const bool live = r0 + long(seg) * long(prm.L) < prm.n;                             // (a segment behind the call's last sample is not run)
    long long acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    if (live) {
        const uint32_t before = prm.W + seg * prm.L - 1u;                               // the sample in front of the segment's first
        // (a lane's taps, W / lanesPer of them, are a power of two >= 16: kLdBatch at a time, their loads in flight together)
        for (uint32_t k = sub; k < prm.W; k += kLdBatch * prm.lanesPer) {
            int4 c[kLdBatch];
            int32_t v[kLdBatch];
#pragma unroll
            for (uint32_t j = 0; j < kLdBatch; ++j) {
                c[j] = prm.taps[k + j * prm.lanesPer];
                v[j] = tile[ldWord(prm, before - (k + j * prm.lanesPer))];
            }
#pragma unroll
            for (uint32_t j = 0; j < kLdBatch; ++j) {
                acc0 += (long long)c[j].x * v[j]; acc1 += (long long)c[j].y * v[j];
                acc2 += (long long)c[j].z * v[j]; acc3 += (long long)c[j].w * v[j];
            }
        }
    }
    // the fold of a segment's lanes, integer adds in any order; then one rounding to nearest even and an exact scale
    if (prm.lanesPer <= 64u) {                                                          // (inside a wave: every lane takes the same trips)
        for (uint32_t o = prm.lanesPer >> 1; o > 0; o >>= 1) {
            acc0 += __shfl_xor(acc0, int(o)); acc1 += __shfl_xor(acc1, int(o)); acc2 += __shfl_xor(acc2, int(o)); acc3 += __shfl_xor(acc3, int(o));
        }
        if (sub == 0) {
            start[seg * 4 + 0] = double(acc0) * 0x1p-32; start[seg * 4 + 1] = double(acc1) * 0x1p-32;
            start[seg * 4 + 2] = double(acc2) * 0x1p-32; start[seg * 4 + 3] = double(acc3) * 0x1p-32;
        }
    } else {                                                                            // (a segment of 2048 samples or more: its lanes are 2 or 4 waves)
        part[tid * 4 + 0] = acc0; part[tid * 4 + 1] = acc1; part[tid * 4 + 2] = acc2; part[tid * 4 + 3] = acc3;
        __syncthreads();
        for (uint32_t e = tid; e < prm.segs * 4u; e += kLdThreads) {
            const uint32_t s = e >> 2, c = e & 3u;
            long long sum = 0;
            for (uint32_t j = 0; j < prm.lanesPer; ++j) sum += part[(s * prm.lanesPer + j) * 4 + c];
            start[e] = double(sum) * 0x1p-32;
        }
    }
    __syncthreads();
    // 3. the runs: one lane per segment, L steps in the definition's order; q takes v's place
    // (up to 64 segments are one wave's work, and a workgroup's wave w always lands on SIMD w of its CU: which wave runs rotates with the
    // workgroup, or the runs of every workgroup of a CU would queue on one SIMD)
    const uint32_t runner = prm.segs <= 64u ? (tid + uint32_t(kLdThreads) - ((blockIdx.x + blockIdx.y) & 3u) * 64u) & uint32_t(kLdThreads - 1) : tid;
    if (runner < prm.segs && r0 + long(runner) * long(prm.L) < prm.n) {
        LdState st{start[runner * 4 + 0], start[runner * 4 + 1], start[runner * 4 + 2], start[runner * 4 + 3]};
        const LdCoef f = prm.coef;
        const uint32_t first = prm.W + runner * prm.L;
        const long left = prm.n - (r0 + long(runner) * long(prm.L));
        const uint32_t steps = left < long(prm.L) ? uint32_t(left) : prm.L;
        int32_t *mine = tile + ldWord(prm, first);                                       // (a segment's words are consecutive: j < L)
        for (uint32_t j = 0; j < steps; ++j) {
            int32_t *at = mine + j;
            const double z = ldStep(f, st, double(*at));
            const double r = __builtin_fmin(__builtin_fmax(__builtin_rint(z), -2147483647.0), 2147483647.0);
            *at = int32_t(r);
        }
    }
    __syncthreads();
    // 4. the tile's q of the call's own samples, in rows
    int32_t *q = prm.q + size_t(ch) * prm.qStride;
    for (uint32_t i = tid; i < prm.tile; i += kLdThreads) {
        const long r = r0 + long(i);
        if (r >= 0 && r < prm.n) q[r] = tile[ldWord(prm, prm.W + i)];
    }
}

// the carry of a call with samples but for an open column's record: the history, the zero word behind it, an all-zero open column (an open
// column's record is stored by the sums' launch behind this one)
__global__ void __launch_bounds__(kLdThreads)
loudnessHistoryKernel(const LoudnessParams prm)
{
    const uint32_t t = blockIdx.x * kLdThreads + threadIdx.x, ch = blockIdx.y;
    uint8_t *mine = prm.carryOut + size_t(ch) * prm.carryBytes;
    int32_t *hist = reinterpret_cast<int32_t *>(mine + sizeof(sgz_loudness_record));
    if (t < prm.hist) hist[t] = filterInput(prm, ch, prm.n - long(prm.hist) + long(t));
    if (t == prm.hist) hist[t] = 0;
    if (t < sizeof(sgz_loudness_record) / 4) reinterpret_cast<uint32_t *>(mine)[t] = 0u;
}

// a column's, a lane's or a slice's part of a record: 128-bit sum of q^2 and the count
struct LdAcc {
    uint64_t lo, hi;
    uint32_t count;
    __device__ __forceinline__ void addSquare(int32_t q)
    {
        const uint64_t s = uint64_t(int64_t(q) * int64_t(q));
        lo += s;
        hi += lo < s ? 1u : 0u;
    }
    __device__ __forceinline__ void add(uint64_t l, uint64_t h, uint32_t c)
    {
        lo += l;
        hi += h + (lo < l ? 1u : 0u);
        count += c;
    }
    __device__ __forceinline__ void add(const sgz_loudness_record &r) { add(r.sumsq[0], r.sumsq[1], r.count); }
    __device__ __forceinline__ void foldLane(int o)
    {
        add(__shfl_xor((unsigned long long)lo, o), __shfl_xor((unsigned long long)hi, o), __shfl_xor(count, o));
    }
    __device__ __forceinline__ void store(sgz_loudness_record *to) const
    {
        sgz_loudness_record r;
        r.sumsq[0] = lo; r.sumsq[1] = hi; r.count = count; r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
        *to = r;
    }
};

// samples [a, b) of this call that belong to column `col`
__device__ __forceinline__ void columnSamples(const LoudnessParams &prm, long col, long &a, long &b)
{
    a = col * long(prm.m) - long(prm.held);
    b = a + long(prm.m);
    a = a < 0 ? 0 : a;
    b = b > prm.n ? prm.n : b;
}

__device__ __forceinline__ void takeSample(const LoudnessParams &prm, uint32_t ch, long r, LdAcc &k)
{
    k.addSquare(prm.q[size_t(ch) * prm.qStride + size_t(r)]);
    const float x = prm.planar[size_t(ch) * prm.stride + size_t(r)];
    k.count += x != x ? 0u : 1u;
}

// the carry into column 0, then to the output (a closed column) or to the carry's open column
__device__ __forceinline__ void emitColumn(const LoudnessParams &prm, long col, uint32_t ch, LdAcc k)
{
    if (col == 0 && prm.held) k.add(*carryOpen(prm.carryIn, prm.carryBytes, ch));
    k.store(col < prm.closed ? prm.out + size_t(col) * prm.channels + ch
                             : reinterpret_cast<sgz_loudness_record *>(prm.carryOut + size_t(ch) * prm.carryBytes));
}

// workgroup (tile of perTile whole columns, channel): groups of prm.group lanes per column, the lanes of a group stride over its samples
__global__ void __launch_bounds__(kLdThreads)
loudnessSumTileKernel(const LoudnessParams prm)
{
    const uint32_t tid = threadIdx.x, ch = blockIdx.y;
    const long c0 = long(blockIdx.x) * long(prm.perTile);
    const long c1 = c0 + long(prm.perTile) < prm.columns ? c0 + long(prm.perTile) : prm.columns;
    const uint32_t G = prm.group, sub = tid & (G - 1u), grp = tid / G, groups = uint32_t(kLdThreads) / G;
    const uint32_t cols = uint32_t(c1 - c0);
    for (uint32_t base = 0; base < cols; base += groups) {                  // (the same trips in every lane: the cross-lane steps see whole waves)
        const uint32_t lc = base + grp;
        const bool mine = lc < cols;
        LdAcc k{0, 0, 0};
        if (mine) {
            long a, b;
            columnSamples(prm, c0 + long(lc), a, b);
            for (long r = a + long(sub); r < b; r += long(G)) takeSample(prm, ch, r, k);
        }
        for (uint32_t o = G >> 1; o > 0; o >>= 1) k.foldLane(int(o));
        if (mine && sub == 0) emitColumn(prm, c0 + long(lc), ch, k);
    }
}

// slice blockIdx.z of column blockIdx.x's samples of channel blockIdx.y (an empty slice leaves the zero record)
__global__ void __launch_bounds__(kLdThreads)
loudnessSumSliceKernel(const LoudnessParams prm)
{
    __shared__ sgz_loudness_record waves[kLdThreads / 64];
    const long col = long(blockIdx.x);
    const uint32_t ch = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
    long a, b;
    columnSamples(prm, col, a, b);
    const long n = b > a ? b - a : 0, per = (n + long(prm.slices) - 1) / long(prm.slices);
    const long sa = a + long(s) * per < b ? a + long(s) * per : b, sb = sa + per < b ? sa + per : b;
    LdAcc k{0, 0, 0};
    for (long r = sa + long(tid); r < sb; r += long(kLdThreads)) takeSample(prm, ch, r, k);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k.foldLane(o);
    if ((tid & 63u) == 0) k.store(&waves[tid >> 6]);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < kLdThreads / 64; ++v) k.add(waves[v]);
        k.store(prm.partial + (size_t(s) * size_t(prm.columns) + size_t(col)) * prm.channels + ch);
    }
}

// one thread per (column, channel): the fold of the slices (none: a flush of the carry alone), the carry, the store
__global__ void __launch_bounds__(kLdThreads)
loudnessEmitKernel(const LoudnessParams prm)
{
    const size_t at = size_t(blockIdx.x) * kLdThreads + threadIdx.x, perSlice = size_t(prm.columns) * prm.channels;
    if (at >= perSlice) return;
    const long col = long(at / prm.channels);
    const uint32_t ch = uint32_t(at % prm.channels);
    LdAcc k{0, 0, 0};
    for (uint32_t s = 0; s < prm.slices; ++s) k.add(prm.partial[size_t(s) * perSlice + at]);
    emitColumn(prm, col, ch, k);
}

uint32_t pow2AtLeast(uint32_t v)
{
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

uint32_t log2Of(uint32_t v)
{
    uint32_t l = 0;
    while ((1u << l) < v) ++l;
    return l;
}

uint32_t runTileOf(const sgz_loudness_filter &f) { return std::max(kLdTile, f.L); }
size_t qStrideOf(size_t nsamples) { return (nsamples + 3) & ~size_t(3); }

uint32_t runTileWords(const sgz_loudness_filter &f)
{
    const uint32_t tile = runTileOf(f), lanesPer = uint32_t(kLdThreads) / (tile / f.L);
    return ((f.W + tile) + ((f.W + tile) / f.L + 1) * lanesPer + 3u) & ~3u;
}

size_t runLdsBytes(const sgz_loudness_filter &f)
{
    const uint32_t tile = runTileOf(f), segs = tile / f.L, lanesPer = uint32_t(kLdThreads) / segs;
    return size_t(segs) * 32 + size_t(runTileWords(f)) * 4 + (lanesPer > 64u ? size_t(kLdThreads) * 32 : 0);
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: remember what has been granted
sgz_status grantRunLds(size_t need)
{
    static size_t granted[64] = {};
    static std::mutex mutex;
    int dev = 0;
    SGZ_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mutex);
    if (dev >= 0 && dev < 64 && granted[dev] >= need) return SGZ_OK;
    SGZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(loudnessRunKernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(need)));
    if (dev >= 0 && dev < 64) granted[dev] = need;
    return SGZ_OK;
}

sgz_status filterForDevice(const sgz_loudness_filter *f, const char *who)
{
    if (!f) return fail(SGZ_EINVAL, std::string(who) + ": null filter");
    if (!shapeOk(*f)) return fail(SGZ_EINVAL, std::string(who) + ": W and L are powers of two, 16 <= L <= W <= 65536");
    if (f->W > kLdDeviceMaxW) return fail(SGZ_EINVAL, std::string(who) + ": the device takes W <= 16384");
    return SGZ_OK;
}

}  // namespace

namespace sgz {

size_t loudnessCarryBytes(const sgz_loudness_filter &f) { return sizeof(sgz_loudness_record) + size_t(f.W + f.L) * sizeof(int32_t); }

// The shape of a call whose arguments passed sgz_stage_loudness_columns' checks, as truePeakColumnsShape; scratchBytes: q [channels][n rounded
// up to 4] and behind it the partial records of the sliced form.
LoudnessColumnsShape loudnessColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices)
{
    LoudnessColumnsShape sh{};
    const uint64_t t = uint64_t(held) + nsamples;
    sh.closed = t / m + ((flush && t % m) ? 1u : 0u);
    sh.open = !flush && t % m != 0;
    sh.columns = sh.closed + (sh.open ? 1u : 0u);
    sh.launch = sh.columns != 0 && !(nsamples == 0 && !(flush && held));
    if (!sh.launch || nsamples == 0) return sh;
    if (slices >= 2 || m > kLdSwitch) sh.slices = slices ? slices : overviewAutoSlices(long(sh.columns), channels, m, nsamples, numCUs());
    sh.scratchBytes = qStrideOf(nsamples) * channels * sizeof(int32_t) + size_t(sh.slices) * size_t(sh.columns) * channels * sizeof(sgz_loudness_record);
    return sh;
}

// sgz_stage_loudness_columns behind its argument checks, with the carry in two places: carryIn is read (the history when `continued`, the open
// column when held > 0), carryOut is written whole by every call with samples -- never the same memory then.  scratch: sh.scratchBytes bytes,
// aligned to 16.
sgz_status runLoudnessColumns(const LoudnessColumnsShape &sh, const sgz_loudness_filter &f, const float *d_planar, size_t channelStride,
                              uint32_t channels, size_t nsamples, uint64_t firstIndex, uint32_t m, uint32_t held, uint32_t continued,
                              const void *carryIn, void *carryOut, sgz_loudness_record *d_out, void *scratch, hipStream_t stream)
{
    if (!sh.launch) return SGZ_OK;
    LoudnessParams prm{};
    prm.planar = d_planar; prm.stride = channelStride; prm.n = long(nsamples);
    prm.columns = long(sh.columns); prm.closed = long(sh.closed);
    prm.m = m; prm.held = held; prm.channels = channels; prm.continued = continued; prm.slices = sh.slices;
    prm.W = f.W; prm.L = f.L; prm.logL = log2Of(f.L); prm.hist = f.W + f.L - 1;
    prm.tile = runTileOf(f); prm.segs = prm.tile / f.L; prm.lanesPer = uint32_t(kLdThreads) / prm.segs;
    prm.tileWords = runTileWords(f);
    prm.phase = uint32_t(firstIndex % f.L);
    prm.coef = coefOf(f);
    prm.carryIn = static_cast<const uint8_t *>(carryIn); prm.carryOut = static_cast<uint8_t *>(carryOut);
    prm.carryBytes = loudnessCarryBytes(f);
    prm.q = static_cast<int32_t *>(scratch); prm.qStride = qStrideOf(nsamples);
    prm.out = d_out;
    prm.partial = reinterpret_cast<sgz_loudness_record *>(static_cast<uint8_t *>(scratch) + prm.qStride * channels * sizeof(int32_t));
    const uint64_t cells = sh.columns * channels;
    if (sh.columns > 0x7fffffffull || (cells + kLdThreads - 1) / kLdThreads > 0x7fffffffull) return fail(SGZ_EINVAL, "loudness columns: too many columns for one launch");
    if (nsamples != 0) {
        if (sgz_status st = deviceTaps(f, &prm.taps); st != SGZ_OK) return st;
        const uint64_t tiles = (uint64_t(nsamples) + prm.phase + prm.tile - 1) / prm.tile;
        if (tiles > 0x7fffffffull) return fail(SGZ_EINVAL, "loudness columns: too many samples for one launch");
        const size_t lds = runLdsBytes(f);
        if (sgz_status st = grantRunLds(lds); st != SGZ_OK) return st;
        hipLaunchKernelGGL(loudnessRunKernel, dim3(unsigned(tiles), channels), dim3(kLdThreads), lds, stream, prm);
        SGZ_HIP(hipGetLastError());
        hipLaunchKernelGGL(loudnessHistoryKernel, dim3((prm.hist + 1 + kLdThreads - 1) / kLdThreads, channels), dim3(kLdThreads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
        if (sh.slices == 0) {
            prm.perTile = kLdTile / m;
            prm.group = std::min(pow2AtLeast((m + kLdRun - 1) / kLdRun), 64u);
            const uint64_t sumTiles = (sh.columns + prm.perTile - 1) / prm.perTile;
            hipLaunchKernelGGL(loudnessSumTileKernel, dim3(unsigned(sumTiles), channels), dim3(kLdThreads), 0, stream, prm);
            SGZ_HIP(hipGetLastError());
            return SGZ_OK;
        }
        hipLaunchKernelGGL(loudnessSumSliceKernel, dim3(unsigned(sh.columns), channels, sh.slices), dim3(kLdThreads), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(loudnessEmitKernel, dim3(unsigned((cells + kLdThreads - 1) / kLdThreads)), dim3(kLdThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

}  // namespace sgz

extern "C" {

sgz_status sgz_loudness_columns_limits(const sgz_loudness_filter *filter, uint32_t channels, uint32_t *switch_over, uint32_t *tile_samples,
                                       size_t *carry_bytes)
{
    if (sgz_status st = filterForDevice(filter, "sgz_loudness_columns_limits"); st != SGZ_OK) return st;
    if (channels == 0 || channels > kLdMaxChannels) return fail(SGZ_EINVAL, "sgz_loudness_columns_limits: 1 .. 64 channels");
    if (switch_over) *switch_over = kLdSwitch;
    if (tile_samples) *tile_samples = runTileOf(*filter);
    if (carry_bytes) *carry_bytes = loudnessCarryBytes(*filter) * channels;
    return SGZ_OK;
}

sgz_status sgz_stage_loudness_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, const sgz_loudness_filter *filter,
                                      uint64_t first_index, uint32_t m, uint32_t held, int flush, uint32_t continued, uint32_t slices, void *d_carry,
                                      sgz_loudness_record *d_records, void *stream)
{
    if (!d_planar) return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: null d_planar");
    if (sgz_status st = filterForDevice(filter, "sgz_stage_loudness_columns"); st != SGZ_OK) return st;
    if (channels == 0 || channels > kLdMaxChannels) return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: 1 .. 64 channels");
    if (m == 0) return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: m >= 1 samples per column");
    if (held >= m) return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: held < m");
    if (!continued && held) return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: held > 0 needs continued != 0 (a stream that begins here has no open column)");
    if (channel_stride < nsamples || nsamples > (size_t(1) << 40)) return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: channel_stride < nsamples, or more than 2^40 samples");
    if (first_index > (uint64_t(1) << 62)) return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: first_index above 2^62");
    if (slices > kLdMaxSlices) return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: slices 0 (automatic) or 1 .. 64");
    if ((reinterpret_cast<uintptr_t>(d_planar) & 3u) || (reinterpret_cast<uintptr_t>(d_carry) & 15u) || (reinterpret_cast<uintptr_t>(d_records) & 15u))
        return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: d_planar aligned to 4 bytes, d_carry and d_records to 16");
    const LoudnessColumnsShape sh = loudnessColumnsShape(channels, nsamples, m, held, flush, slices);
    if (!d_carry && (continued || nsamples)) return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: d_carry is read (continued) or written (nsamples > 0)");
    if (!d_records && sh.closed) return fail(SGZ_EINVAL, "sgz_stage_loudness_columns: d_records is written (a column closes)");
    if (nsamples) {                                                  // (the table before anything is launched: a refused filter writes nothing)
        const int4 *taps = nullptr;
        if (sgz_status st = deviceTaps(*filter, &taps); st != SGZ_OK) return st;
    }
    if (!sh.launch) return SGZ_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    StreamScratch scratch(s), snapshot(s);
    const void *carryIn = d_carry;
    const size_t carryBytes = loudnessCarryBytes(*filter) * channels;
    if (continued && nsamples) {
        // the halos, the history and column 0 read the carry while other workgroups write the new one: they read a snapshot
        SGZ_HIP(snapshot.get(carryBytes));
        SGZ_HIP(hipMemcpyAsync(snapshot.p, d_carry, carryBytes, hipMemcpyDeviceToDevice, s));
        carryIn = snapshot.p;
    }
    if (sh.scratchBytes) SGZ_HIP(scratch.get(sh.scratchBytes));
    return runLoudnessColumns(sh, *filter, d_planar, channel_stride, channels, nsamples, first_index, m, held, continued, carryIn, d_carry, d_records,
                              scratch.p, s);
}

// ---- host arithmetic ---------------------------------------------------------------------------------------------------------------------------
sgz_status sgz_loudness_filter_for_rate(double rate, sgz_loudness_filter *f)
{
    if (!f) return fail(SGZ_EINVAL, "sgz_loudness_filter_for_rate: null argument");
    if (!(rate >= 200.0 && rate <= 819200.0)) return fail(SGZ_EINVAL, "sgz_loudness_filter_for_rate: 200 <= rate <= 819200 (W = 16 .. 65536)");
    sgz_loudness_filter r{};
    if (rate == 48000.0) {                                          // ITU-R BS.1770-4, tables 1 and 2, as printed
        r.b[0][0] = 1.53512485958697; r.b[0][1] = -2.69169618940638; r.b[0][2] = 1.19839281085285;
        r.a[0][0] = -1.69065929318241; r.a[0][1] = 0.73248077421585;
        r.b[1][0] = 1.0; r.b[1][1] = -2.0; r.b[1][2] = 1.0;
        r.a[1][0] = -1.99004745483398; r.a[1][1] = 0.99007225036621;
    } else {                                                        // the bilinear transform of the analogue prototype those tables came from
        const double pi = 3.14159265358979323846;
        {
            const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
            const double K = std::tan(pi * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
            const double a0 = 1.0 + K / Q + K * K;
            r.b[0][0] = (Vh + Vb * K / Q + K * K) / a0; r.b[0][1] = 2.0 * (K * K - Vh) / a0; r.b[0][2] = (Vh - Vb * K / Q + K * K) / a0;
            r.a[0][0] = 2.0 * (K * K - 1.0) / a0; r.a[0][1] = (1.0 - K / Q + K * K) / a0;
        }
        {
            const double f0 = 38.13547087602444, Q = 0.5003270373238773;
            const double K = std::tan(pi * f0 / rate), a0 = 1.0 + K / Q + K * K;
            r.b[1][0] = 1.0; r.b[1][1] = -2.0; r.b[1][2] = 1.0;
            r.a[1][0] = 2.0 * (K * K - 1.0) / a0; r.a[1][1] = (1.0 - K / Q + K * K) / a0;
        }
    }
    r.W = std::max(pow2AtLeast(uint32_t(std::ceil(0.08 * rate))), 16u * kLdMinL);
    r.L = r.W / 16;
    *f = r;
    return SGZ_OK;
}

sgz_status sgz_loudness_taps(const sgz_loudness_filter *f, int32_t *taps)
{
    if (!f || !taps) return fail(SGZ_EINVAL, "sgz_loudness_taps: null argument");
    if (!shapeOk(*f)) return fail(SGZ_EINVAL, "sgz_loudness_taps: W and L are powers of two, 16 <= L <= W <= 65536");
    std::vector<int32_t> t(size_t(4) * f->W);                       // (a refusal writes nothing)
    if (!buildTaps(*f, t.data())) return fail(SGZ_EINVAL, "sgz_loudness_taps: a tap outside int32, or 2^26 sum |C| >= 2^62");
    std::memcpy(taps, t.data(), t.size() * sizeof(int32_t));
    return SGZ_OK;
}

sgz_status sgz_loudness_fold(const sgz_loudness_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns,
                             sgz_loudness_record *out)
{
    if (!in || !out) return fail(SGZ_EINVAL, "sgz_loudness_fold: null argument");
    if (channels == 0) return fail(SGZ_EINVAL, "sgz_loudness_fold: channels >= 1");
    uint64_t cols = 0;
    if (sgz_status st = checkViewRange(n, x0, x1, out_columns, &cols); st != SGZ_OK) return st;
    const uint64_t w = x1 - x0;
    auto bound = [&](uint64_t b) { return x0 + (b * w + cols - 1) / cols; };                   // (b w < 2^62: n < 2^31)
    // the counts first: a refusal writes nothing
    for (uint64_t b = 0; b < cols; ++b)
        for (uint32_t c = 0; c < channels; ++c) {
            uint64_t count = 0;
            for (uint64_t j = bound(b); j < bound(b + 1); ++j) count += in[j * channels + c].count;
            if (count > 0xffffffffull) return fail(SGZ_EINVAL, "sgz_loudness_fold: a folded column counts more than 2^32 - 1");
        }
    for (uint64_t b = 0; b < cols; ++b)
        for (uint32_t c = 0; c < channels; ++c) {
            unsigned __int128 sum = 0;
            uint32_t count = 0;
            for (uint64_t j = bound(b); j < bound(b + 1); ++j) {
                const sgz_loudness_record &v = in[j * channels + c];
                sum += (static_cast<unsigned __int128>(v.sumsq[1]) << 64) | v.sumsq[0];
                count += v.count;
            }
            sgz_loudness_record r{};
            r.sumsq[0] = uint64_t(sum); r.sumsq[1] = uint64_t(sum >> 64); r.count = count;
            out[b * channels + c] = r;
        }
    return SGZ_OK;
}

}  // extern "C"

namespace {

// sum over channels of G_c times the mean square (1.0 = full scale squared) of `ncols` columns read together
double weightedMeanSquare(const sgz_loudness_record *recs, size_t ncols, uint32_t channels, const double *weights)
{
    double z = 0.0;
    for (uint32_t c = 0; c < channels; ++c) {
        unsigned __int128 sum = 0;
        uint64_t count = 0;
        for (size_t j = 0; j < ncols; ++j) {
            const sgz_loudness_record &v = recs[j * channels + c];
            sum += (static_cast<unsigned __int128>(v.sumsq[1]) << 64) | v.sumsq[0];
            count += v.count;
        }
        if (count) z += (weights ? weights[c] : 1.0) * (double(sum) / double(count) * 0x1p-46);
    }
    return z;
}

double lufsOf(double z) { return z > 0.0 ? -0.691 + 10.0 * std::log10(z) : -std::numeric_limits<double>::infinity(); }

}  // namespace

extern "C" {

sgz_status sgz_loudness_readout(const sgz_loudness_record *recs, size_t ncols, uint32_t channels, const double *weights, double *lufs, double *mean_square)
{
    if (!recs) return fail(SGZ_EINVAL, "sgz_loudness_readout: null argument");
    if (channels == 0 || ncols == 0) return fail(SGZ_EINVAL, "sgz_loudness_readout: channels >= 1 and ncols >= 1");
    const double z = weightedMeanSquare(recs, ncols, channels, weights);
    if (mean_square) *mean_square = z;
    if (lufs) *lufs = lufsOf(z);
    return SGZ_OK;
}

sgz_status sgz_loudness_integrated(const sgz_loudness_record *recs, size_t n, uint32_t channels, const double *weights, double *lufs)
{
    if (!recs || !lufs) return fail(SGZ_EINVAL, "sgz_loudness_integrated: null argument");
    if (channels == 0) return fail(SGZ_EINVAL, "sgz_loudness_integrated: channels >= 1");
    const double none = -std::numeric_limits<double>::infinity();
    *lufs = none;
    if (n < 4) return SGZ_OK;
    std::vector<double> z(n - 3);
    for (size_t i = 0; i + 4 <= n; ++i) z[i] = weightedMeanSquare(recs + i * channels, 4, channels, weights);
    double sum = 0.0;
    size_t passed = 0;
    for (double v : z)
        if (lufsOf(v) > -70.0) { sum += v; ++passed; }
    if (!passed) return SGZ_OK;
    const double gate = lufsOf(sum / double(passed)) - 10.0;
    sum = 0.0; passed = 0;
    for (double v : z)
        if (lufsOf(v) > -70.0 && lufsOf(v) > gate) { sum += v; ++passed; }
    if (passed) *lufs = lufsOf(sum / double(passed));
    return SGZ_OK;
}

}  // extern "C"
