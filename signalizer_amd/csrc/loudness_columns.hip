// loudness_columns.hip -- the loudness lane's reduction: one sgz_loudness_record (the sum of the squared K-weighted samples, the count) per
// column of m samples and channel of a linear planar stream, with a carried open column and a carried sample history (sgz.h, "The loudness
// lane"); and the lane's host helpers: the filter of a sample rate, the tap table, the fold of kept records, the readout of a run of columns
// and the gated integrated loudness.  gfx950 only.  The reference has no counterpart: its meters are live one-pole filters.
// What the column lanes share is column_lanes.hpp, and so is what this lane shares with the band lane alone (section 4 there: the tap table on
// the device, the carry's layout and history kernel, the run tile's geometry, the column sums); this file is the K-weighting's step, its
// tap table, the run kernel and the record's readouts.
//   v = the quantiser's (quantiseSilent): a NaN is v = 0 and is not counted.  The sample axis is cut into segments of L samples on
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
//   historyKernel           the new carry but for an open column: the last W + L - 1 quantised samples of (the old history, the call).
//   the column sums         of q^2 and of the non-NaN samples (LdAcc): m <= kLdSwitch (1024) sumTileKernel, longer columns or slices >= 2
//                           sumSliceKernel + sumEmitKernel.  A flush without samples is the emit kernel alone, on the carry.
// Built: the integer form of the dot products (v_mad_i64_i32).  An fp64 form would need every tap split in two to stay exact (32-bit taps times
// 27-bit samples over W terms pass 2^53), twice the multiply-adds of the form that is exact as it stands.  The sums are a pass of their own over
// q in scratch, not fused into the run: columns and segments do not align, a lane of the run owns a segment, and the pass costs one read of q.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "runtime.hpp"

// The definition's step is one IEEE operation per *, + and -: nothing in this file may be contracted into an FMA, on the host (the tap table)
// or on the device (the segment runs).  hipcc contracts by default.
#pragma clang fp contract(off)

#include "column_lanes.hpp"    // (behind the pragma: what is instantiated from it here is not contracted either)

using namespace sgz;

namespace {

constexpr int kLdThreads = kTwinThreads;
constexpr uint32_t kLdSwitch = 1024;             // the switch-over of the column sums: longer columns take the sliced form
constexpr uint32_t kLdMaxChannels = 64;
constexpr uint32_t kLdBatch = 8;                 // loads a lane of the run kernel issues before it uses the first
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

// C[c][k] at taps[c * W + k]; false where the filter is refused
bool buildTaps(const sgz_loudness_filter &f, int32_t *taps)
{
    if (!filterShapeOk(f)) return false;
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

sgz_status tapsOnDevice(const sgz_loudness_filter &f, const int4 **out) { return deviceTaps(f, 4, buildTaps, "loudness", out); }

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------------
struct LoudnessParams {
    typedef sgz_loudness_record Record;
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
    uint32_t perTile, group, slices;     // the column sums (column_lanes.hpp sumTileKernel)
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
            if (i < words) tile[segmentWord(prm, i)] = v[j];
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
                v[j] = tile[segmentWord(prm, before - (k + j * prm.lanesPer))];
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
        int32_t *mine = tile + segmentWord(prm, first);                                       // (a segment's words are consecutive: j < L)
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
        if (r >= 0 && r < prm.n) q[r] = tile[segmentWord(prm, prm.W + i)];
    }
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
    __device__ __forceinline__ void takeSample(const LoudnessParams &prm, uint32_t ch, long r)
    {
        addSquare(prm.q[size_t(ch) * prm.qStride + size_t(r)]);
        const float x = prm.planar[size_t(ch) * prm.stride + size_t(r)];
        count += x != x ? 0u : 1u;
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

size_t runLdsBytes(const sgz_loudness_filter &f)
{
    const uint32_t tile = runTileOf(f), segs = tile / f.L, lanesPer = uint32_t(kLdThreads) / segs;
    return size_t(segs) * 32 + size_t(runTileWords(f)) * 4 + (lanesPer > 64u ? size_t(kLdThreads) * 32 : 0);
}

}  // namespace

namespace sgz {

size_t loudnessCarryBytes(const sgz_loudness_filter &f) { return twinCarryBytes<sgz_loudness_record>(f); }

ColumnsShape loudnessColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices)
{
    return columnsShape(channels, nsamples, m, held, flush, slices, kLdSwitch, sizeof(sgz_loudness_record), qStrideOf(nsamples) * channels * sizeof(int32_t));
}

sgz_status runLoudnessColumns(const ColumnsShape &sh, const sgz_loudness_filter &f, const float *d_planar, size_t channelStride,
                              uint32_t channels, size_t nsamples, uint64_t firstIndex, uint32_t m, uint32_t held, uint32_t continued,
                              const void *carryIn, void *carryOut, sgz_loudness_record *d_out, void *scratch, hipStream_t stream)
{
    if (!sh.launch) return SGZ_OK;
    LoudnessParams prm{};
    fillGrid(prm, sh, d_planar, channelStride, nsamples, m, held);
    prm.channels = channels; prm.continued = continued;
    fillTwin(prm, f, 1, channels, nsamples, firstIndex, carryIn, carryOut, d_out, scratch);
    prm.coef = coefOf(f);
    return launchTwinLane<loudnessRunKernel, LdAcc>("loudness", prm, sh, f, channels, nsamples, m, runLdsBytes(f), tapsOnDevice, stream);
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
    const StageFront front{"sgz_stage_loudness_columns", "channels", kLdMaxChannels, "d_records", 16, true, 40};
    // (the filter's check stands behind d_planar's: checkStageArgs.  The carry's size is read behind that check alone)
    return stageColumns(front, filterForDevice(filter, front.who), d_planar, channel_stride, channels, nsamples, m, held, flush, continued, first_index, slices, d_carry,
                        d_records, stream, loudnessColumnsShape, filter ? loudnessCarryBytes(*filter) * channels : 0,
                        [&] {                                        // (the table before anything is launched: a refused filter writes nothing)
                            const int4 *taps = nullptr;
                            return nsamples ? tapsOnDevice(*filter, &taps) : SGZ_OK;
                        },
                        [&](const ColumnsShape &sh, const void *carryIn, void *scratch, hipStream_t s) {
                            return runLoudnessColumns(sh, *filter, d_planar, channel_stride, channels, nsamples, first_index, m, held, continued, carryIn, d_carry, d_records, scratch, s);
                        });
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
    r.W = std::max(pow2AtLeast(uint32_t(std::ceil(0.08 * rate))), 16u * kTwinMinL);
    r.L = r.W / 16;
    *f = r;
    return SGZ_OK;
}

sgz_status sgz_loudness_taps(const sgz_loudness_filter *f, int32_t *taps)
{
    if (!f || !taps) return fail(SGZ_EINVAL, "sgz_loudness_taps: null argument");
    if (!filterShapeOk(*f)) return fail(SGZ_EINVAL, "sgz_loudness_taps: W and L are powers of two, 16 <= L <= W <= 65536");
    std::vector<int32_t> t(size_t(4) * f->W);                       // (a refusal writes nothing)
    if (!buildTaps(*f, t.data())) return fail(SGZ_EINVAL, "sgz_loudness_taps: a tap outside int32, or 2^26 sum |C| >= 2^62");
    std::memcpy(taps, t.data(), t.size() * sizeof(int32_t));
    return SGZ_OK;
}

sgz_status sgz_loudness_fold(const sgz_loudness_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns,
                             sgz_loudness_record *out)
{
    return foldColumns(
        "sgz_loudness_fold", "channels", "", in, n, channels, x0, x1, out_columns, out,
        [](const sgz_loudness_record *v, size_t count, size_t stride) {
            uint64_t tally = 0;
            for (size_t j = 0; j < count; ++j) tally += v[j * stride].count;
            return tally <= 0xffffffffull;
        },
        [](const sgz_loudness_record *v, size_t count, size_t stride) {
            unsigned __int128 sum = 0;
            sgz_loudness_record r{};
            for (size_t j = 0; j < count; ++j) {
                sum += (static_cast<unsigned __int128>(v[j * stride].sumsq[1]) << 64) | v[j * stride].sumsq[0];
                r.count += v[j * stride].count;
            }
            r.sumsq[0] = uint64_t(sum); r.sumsq[1] = uint64_t(sum >> 64);
            return r;
        });
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
