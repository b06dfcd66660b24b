// band_columns.hip -- the band lane's reduction: one sgz_band_record (the sums of the squared low, mid and high band samples, the count) per
// column of m samples and channel of a linear planar stream, with a carried open column and a carried sample history (sgz.h, "The band
// lane"); and the lane's host helpers: the Oscilloscope's crossover of a sample rate, the tap table, the fold of kept records, the readout of
// a run of columns and the colours the Oscilloscope draws them with.  gfx950 only.  The reference's counterpart is live
// (StreamState::audioProcessing; scope_stream.hip scopeIngestKernel phase F); this is the same network per column of a file.
// What the column lanes share is column_lanes.hpp, and so is what this lane shares with the loudness lane alone (section 4 there: the tap
// table on the device, the carry's layout and history kernel, the run tile's geometry, the column sums); this file is the crossover tree, its
// tap table, the run kernel and the record's readouts.
//   v = the quantiser's (quantiseSilent): a NaN is v = 0 and is not counted.  The sample axis is cut into segments of L samples on an absolute grid.  The 16 state components of the crossover tree at
//   a segment's start are exact integer FIRs over the last W quantised samples (taps at 2^30, 64-bit sums, any order), converted to fp64
//   once; from there the fp64 recurrence of the eight sections runs over the segment's L samples in one fixed order with no contraction (the
//   pragma below, for host and device alike).  q_b = rint(z_b) clamped to 32 bits for the three bands, the record sums q_b^2 in 128 bits.
// Three steps, each a launch of its own behind the other (no hand-off between workgroups inside a launch):
//   bandRunKernel       one workgroup per (tile of T = max(4096, L) samples on the segment grid, channel).  The tile goes to LDS quantised,
//                       behind a W-sample halo.  Segment-start dot products: the 256 lanes are T / L segments x P
//                       lanes; the 16 components are taken four at a time (one 16-byte row C[g][k][0..3] and one sample per four
//                       multiply-adds), a lane walks taps k = sub, sub + P, ..; the P partial sums are folded by wave shuffles (through LDS
//                       where P > 64).  The runs: the tree is three independent chains -- lp1a lp1b (low); hp1a hp1b lp2a lp2b (mid); hp1a
//                       hp1b hp2a hp2b (high) -- and a lane runs one chain of one segment; the two copies of hp1a hp1b perform the same
//                       operations on the same values, so `rest` is the same bits in both.  A chain's state lives in LDS between rounds of
//                       kBdStage / segments steps: a round leaves its q in three staging planes, which the workgroup then stores in rows to
//                       stream-ordered scratch [3][channels][n].  A segment that began before the call is re-run from its start out of the
//                       history; its earlier samples are not stored.
//   historyKernel       the new carry but for an open column: the last W + L - 1 quantised samples of (the old history, the call).
//   the column sums     of the three q^2 and of the non-NaN samples in one pass over the planes (BdAcc): m <= kBdSwitch (1024)
//                       sumTileKernel; longer columns or slices >= 2 sumSliceKernel + sumEmitKernel.  A flush without samples is the emit
//                       kernel alone, on the carry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "runtime.hpp"

// The definition's step is one IEEE operation per *, + and -: nothing in this file may be contracted into an FMA, on the host (the tap table,
// the colours) or on the device (the segment runs).  hipcc contracts by default.
#pragma clang fp contract(off)

#include "column_lanes.hpp"    // (behind the pragma: what is instantiated from it here is not contracted either)

using namespace sgz;

namespace {

constexpr int kBdThreads = kTwinThreads;
constexpr uint32_t kBdSwitch = 1024;             // the switch-over of the column sums: longer columns take the sliced form
constexpr uint32_t kBdStage = 1024;              // samples of a tile that one round of the runs leaves in the staging planes
constexpr uint32_t kBdMaxChannels = 64;
constexpr uint32_t kBdBatch = 8;                 // loads a lane of the run kernel issues before it uses the first
constexpr uint32_t kBdComps = 16, kBdChainWords = 20;      // state components; doubles of a segment's three chains in LDS (4 + 8 + 8)
constexpr double kBdTapScale = 1073741824.0;     // S = 30
constexpr uint64_t kBdTapSumBound = uint64_t(1) << 36;     // 2^26 sum |C| < 2^62
static_assert(sizeof(sgz_band_record) == 64 && sizeof(sgz_band_filter) == 168, "sgz.h documents 64 and 168 bytes");

// ---- the definition's step and the tap table (host) -----------------------------------------------------------------------------------------
struct BdCoef { double c[4][5]; };               // {b0, b1, b2, a1, a2} of lp1, hp1, lp2, hp2

// one section, transposed direct form II (every operation on its own: see the pragma above)
__host__ __device__ __forceinline__ double bdSection(const double *c, double &z0, double &z1, double x)
{
    const double y = c[0] * x + z0;
    z0 = (c[1] * x - c[3] * y) + z1;
    z1 = c[2] * x - c[4] * y;
    return y;
}

// the tree on the definition's 16 components; bands = {low, mid, high}
void bdTree(const BdCoef &f, double *z, double x, double *bands)
{
    const double low = bdSection(f.c[0], z[2], z[3], bdSection(f.c[0], z[0], z[1], x));
    const double rest = bdSection(f.c[1], z[6], z[7], bdSection(f.c[1], z[4], z[5], x));
    bands[0] = low;
    bands[1] = bdSection(f.c[2], z[10], z[11], bdSection(f.c[2], z[8], z[9], rest));
    bands[2] = bdSection(f.c[3], z[14], z[15], bdSection(f.c[3], z[12], z[13], rest));
}

BdCoef coefOf(const sgz_band_filter &f)
{
    BdCoef c;
    for (int s = 0; s < 4; ++s)
        for (int i = 0; i < 5; ++i) c.c[s][i] = f.c[s][i];
    return c;
}

// C[c][k] at taps[c * W + k]; false where the filter is refused
bool buildTaps(const sgz_band_filter &f, int32_t *taps)
{
    if (!filterShapeOk(f)) return false;
    const BdCoef c = coefOf(f);
    double z[kBdComps] = {}, bands[3];
    uint64_t sum[kBdComps] = {};
    for (uint32_t k = 0; k < f.W; ++k) {
        bdTree(c, z, k == 0 ? 1.0 : 0.0, bands);
        for (uint32_t q = 0; q < kBdComps; ++q) {
            const double t = std::nearbyint(kBdTapScale * z[q]);           // (round to nearest even: the default mode; the scale is exact)
            if (!(t >= -2147483648.0 && t <= 2147483647.0)) return false;  // (a NaN fails too)
            const int32_t v = int32_t(t);
            taps[size_t(q) * f.W + k] = v;
            sum[q] += uint64_t(v < 0 ? -int64_t(v) : int64_t(v));
        }
    }
    return *std::max_element(sum, sum + kBdComps) < kBdTapSumBound;
}

sgz_status tapsOnDevice(const sgz_band_filter &f, const int4 **out) { return deviceTaps(f, kBdComps, buildTaps, "band", out); }

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------------
struct BandParams {
    typedef sgz_band_record Record;
    const float *planar;                 // [channels][stride]
    size_t stride;
    long n;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t m, held, channels;
    uint32_t continued;                  // the history in carryIn holds the samples before this call (else zeros)
    uint32_t W, L, logL, hist;           // hist = W + L - 1
    uint32_t tileWords;                  // LDS words of the halo and the tile, padding included
    uint32_t tile, segs, logSegs, lanesPer;  // the run tile: T samples = segs segments, lanesPer = 256 / segs lanes per segment in the dot products
    uint32_t stage, perRound, logRound, rounds;  // a round: perRound = stage / segs steps of every segment; rounds = L / perRound
    uint32_t phase;                      // first_index % L: the call's first sample within its segment
    uint32_t perTile, group, slices;     // the column sums (column_lanes.hpp sumTileKernel)
    BdCoef coef;
    const int4 *taps;                    // [4][W]: C[g][k][0..3]
    const uint8_t *carryIn;              // [channels][carryBytes]: the open column, then the history (oldest first), then a zero word
    uint8_t *carryOut;
    size_t carryBytes;
    int32_t *q;                          // [3][channels][qStride]: q of the call's samples, low, mid, high
    size_t qStride;
    sgz_band_record *out;                // [closed][channels]
    sgz_band_record *partial;            // [slices][columns][channels]
};

// component c of segment seg's start state into the chains' words: [0..3] lp1a lp1b; [4..11] hp1a hp1b lp2a lp2b; [12..19] hp1a hp1b hp2a hp2b
__device__ __forceinline__ void putStart(double *chains, uint32_t seg, uint32_t c, double v)
{
    double *s = chains + size_t(seg) * kBdChainWords;
    if (c < 4u) s[c] = v;
    else if (c < 8u) { s[c] = v; s[c + 8u] = v; }
    else if (c < 12u) s[c] = v;
    else s[c + 4u] = v;
}

__global__ void __launch_bounds__(kBdThreads)
bandRunKernel(const BandParams prm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    // [segs][20] the chains' states, the tile, and one block that is first -- only where a segment's lanes are more than a wave -- [256][4]
    // partial dot products and then the three staging planes [3][stage + segs]
    double *chains = reinterpret_cast<double *>(ldsRaw);
    int32_t *tile = reinterpret_cast<int32_t *>(ldsRaw + size_t(prm.segs) * kBdChainWords * 8);
    unsigned char *shared = ldsRaw + size_t(prm.segs) * kBdChainWords * 8 + size_t(prm.tileWords) * 4;
    long long *part = reinterpret_cast<long long *>(shared);
    int32_t *staged = reinterpret_cast<int32_t *>(shared);
    const uint32_t tid = threadIdx.x, ch = blockIdx.y;
    const long r0 = long(blockIdx.x) * long(prm.tile) - long(prm.phase);               // the tile's first sample, on the segment grid (>= -(L - 1))
    // 1. the halo and the tile, quantised
    const uint32_t words = prm.W + prm.tile;
    for (uint32_t base = tid; base < words; base += kBdBatch * kBdThreads) {             // (kBdBatch loads of a lane in flight together)
        int32_t v[kBdBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBdBatch; ++j) {
            const uint32_t i = base + j * kBdThreads;
            v[j] = i < words ? filterInput(prm, ch, r0 - long(prm.W) + long(i)) : 0;
        }
#pragma unroll
        for (uint32_t j = 0; j < kBdBatch; ++j) {
            const uint32_t i = base + j * kBdThreads;
            if (i < words) tile[segmentWord(prm, i)] = v[j];
        }
    }
    __syncthreads();
    // 2. the dot products, four components at a time: lane (seg, sub) takes taps sub, sub + lanesPer, .. of its segment
    const uint32_t seg = tid / prm.lanesPer, sub = tid % prm.lanesPer;
    const bool live = r0 + long(seg) * long(prm.L) < prm.n;                             // (a segment behind the call's last sample is not run)
    const uint32_t before = prm.W + seg * prm.L - 1u;                                   // the sample in front of the segment's first
    for (uint32_t g = 0; g < 4u; ++g) {
        const int4 *taps = prm.taps + size_t(g) * prm.W;
        long long acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
        if (live) {
            // (a lane's taps, W / lanesPer of them, are a power of two >= 16: kBdBatch at a time, their loads in flight together)
            for (uint32_t k = sub; k < prm.W; k += kBdBatch * prm.lanesPer) {
                int4 c[kBdBatch];
                int32_t v[kBdBatch];
#pragma unroll
                for (uint32_t j = 0; j < kBdBatch; ++j) {
                    c[j] = taps[k + j * prm.lanesPer];
                    v[j] = tile[segmentWord(prm, before - (k + j * prm.lanesPer))];
                }
#pragma unroll
                for (uint32_t j = 0; j < kBdBatch; ++j) {
                    acc0 += (long long)c[j].x * v[j]; acc1 += (long long)c[j].y * v[j];
                    acc2 += (long long)c[j].z * v[j]; acc3 += (long long)c[j].w * v[j];
                }
            }
        }
        // the fold of a segment's lanes, integer adds in any order; then one rounding to nearest even and an exact scale
        if (prm.lanesPer <= 64u) {                                                      // (inside a wave: every lane takes the same trips)
            for (uint32_t o = prm.lanesPer >> 1; o > 0; o >>= 1) {
                acc0 += __shfl_xor(acc0, int(o)); acc1 += __shfl_xor(acc1, int(o)); acc2 += __shfl_xor(acc2, int(o)); acc3 += __shfl_xor(acc3, int(o));
            }
            if (sub == 0) {
                putStart(chains, seg, g * 4u + 0u, double(acc0) * 0x1p-30); putStart(chains, seg, g * 4u + 1u, double(acc1) * 0x1p-30);
                putStart(chains, seg, g * 4u + 2u, double(acc2) * 0x1p-30); putStart(chains, seg, g * 4u + 3u, double(acc3) * 0x1p-30);
            }
        } else {                                                                        // (a segment of 2048 samples or more: its lanes are 2 or 4 waves)
            part[tid * 4 + 0] = acc0; part[tid * 4 + 1] = acc1; part[tid * 4 + 2] = acc2; part[tid * 4 + 3] = acc3;
            __syncthreads();
            for (uint32_t e = tid; e < prm.segs * 4u; e += kBdThreads) {
                const uint32_t s = e >> 2, c = e & 3u;
                long long sum = 0;
                for (uint32_t j = 0; j < prm.lanesPer; ++j) sum += part[(s * prm.lanesPer + j) * 4 + c];
                putStart(chains, s, g * 4u + c, double(sum) * 0x1p-30);
            }
            __syncthreads();                                                            // (the next four components, then the staging planes, reuse `part`)
        }
    }
    __syncthreads();
    // 3. the runs, in rounds of perRound steps: job (chain, segment) loads its chain's state, runs the steps in the definition's order, leaves
    // q in its staging plane and the state where it was; then the workgroup stores the round's q of the call's own samples in rows
    // (a workgroup's wave w always lands on SIMD w of its CU: which waves take the first jobs rotates with the workgroup)
    const uint32_t jobs = 3u * prm.segs, plane = prm.stage + prm.segs;                  // (a staging plane: one pad word per segment against bank conflicts)
    const uint32_t firstJob = (tid + uint32_t(kBdThreads) - ((blockIdx.x + blockIdx.y) & 3u) * 64u) & uint32_t(kBdThreads - 1);
    const size_t qPlane = size_t(prm.channels) * prm.qStride;
    int32_t *q = prm.q + size_t(ch) * prm.qStride;
    for (uint32_t rd = 0; rd < prm.rounds; ++rd) {
        for (uint32_t job = firstJob; job < jobs; job += kBdThreads) {
            const uint32_t chain = job >> prm.logSegs, s = job & (prm.segs - 1u);
            const long left = prm.n - (r0 + long(s) * long(prm.L));
            const uint32_t steps = left <= 0 ? 0u : left < long(prm.L) ? uint32_t(left) : prm.L;
            const uint32_t j0 = rd * prm.perRound, j1 = j0 + prm.perRound < steps ? j0 + prm.perRound : steps;
            if (j0 >= j1) continue;
            double a[5], b[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                a[i] = chain == 0u ? prm.coef.c[0][i] : prm.coef.c[1][i];
                b[i] = chain == 1u ? prm.coef.c[2][i] : prm.coef.c[3][i];
            }
            double *st = chains + size_t(s) * kBdChainWords + (chain == 0u ? 0u : chain == 1u ? 4u : 12u);
            double z0 = st[0], z1 = st[1], z2 = st[2], z3 = st[3], z4 = 0.0, z5 = 0.0, z6 = 0.0, z7 = 0.0;
            if (chain) { z4 = st[4]; z5 = st[5]; z6 = st[6]; z7 = st[7]; }
            const int32_t *in = tile + segmentWord(prm, prm.W + s * prm.L);                   // (a segment's words are consecutive: j < L)
            int32_t *to = staged + chain * plane + s * (prm.perRound + 1u);
            for (uint32_t j = j0; j < j1; ++j) {
                double y = bdSection(a, z2, z3, bdSection(a, z0, z1, double(in[j])));
                if (chain) y = bdSection(b, z6, z7, bdSection(b, z4, z5, y));
                to[j - j0] = int32_t(__builtin_fmin(__builtin_fmax(__builtin_rint(y), -2147483647.0), 2147483647.0));
            }
            st[0] = z0; st[1] = z1; st[2] = z2; st[3] = z3;
            if (chain) { st[4] = z4; st[5] = z5; st[6] = z6; st[7] = z7; }
        }
        __syncthreads();
        for (uint32_t e = tid; e < prm.stage; e += kBdThreads) {
            const uint32_t s = e >> prm.logRound, j = e & (prm.perRound - 1u);
            const long r = r0 + long(s) * long(prm.L) + long(rd * prm.perRound + j);
            if (r >= 0 && r < prm.n) {
#pragma unroll
                for (uint32_t b = 0; b < 3u; ++b) q[size_t(b) * qPlane + size_t(r)] = staged[b * plane + e + s];
            }
        }
        __syncthreads();
    }
}

// a column's, a lane's or a slice's part of a record: three 128-bit sums of q^2 and the count
struct BdAcc {
    uint64_t lo[3], hi[3];
    uint32_t count;
    __device__ __forceinline__ void addSquare(int b, int32_t q)
    {
        const uint64_t s = uint64_t(int64_t(q) * int64_t(q));
        lo[b] += s;
        hi[b] += lo[b] < s ? 1u : 0u;
    }
    __device__ __forceinline__ void takeSample(const BandParams &prm, uint32_t ch, long r)
    {
        const size_t plane = size_t(prm.channels) * prm.qStride, at = size_t(ch) * prm.qStride + size_t(r);
        addSquare(0, prm.q[at]);
        addSquare(1, prm.q[plane + at]);
        addSquare(2, prm.q[2 * plane + at]);
        const float x = prm.planar[size_t(ch) * prm.stride + size_t(r)];
        count += x != x ? 0u : 1u;
    }
    __device__ __forceinline__ void add(int b, uint64_t l, uint64_t h)
    {
        lo[b] += l;
        hi[b] += h + (lo[b] < l ? 1u : 0u);
    }
    __device__ __forceinline__ void add(const sgz_band_record &r)
    {
#pragma unroll
        for (int b = 0; b < 3; ++b) add(b, r.sumsq[b][0], r.sumsq[b][1]);
        count += r.count;
    }
    __device__ __forceinline__ void foldLane(int o)
    {
#pragma unroll
        for (int b = 0; b < 3; ++b) add(b, __shfl_xor((unsigned long long)lo[b], o), __shfl_xor((unsigned long long)hi[b], o));
        count += __shfl_xor(count, o);
    }
    __device__ __forceinline__ void store(sgz_band_record *to) const
    {
        sgz_band_record r;
#pragma unroll
        for (int b = 0; b < 3; ++b) { r.sumsq[b][0] = lo[b]; r.sumsq[b][1] = hi[b]; }
        r.count = count; r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
        *to = r;
    }
};

// the chains' states, the halo and the tile, and the block the partial dot products and the staging planes share (at most 143 KiB of the
// 160: W = 16384 with L = 16 or L = 16384)
size_t runLdsBytes(const sgz_band_filter &f)
{
    const uint32_t tile = runTileOf(f), segs = tile / f.L, lanesPer = uint32_t(kBdThreads) / segs;
    const size_t staged = size_t(3) * (kBdStage + segs) * 4, part = lanesPer > 64u ? size_t(kBdThreads) * 32 : 0;
    return size_t(segs) * kBdChainWords * 8 + size_t(runTileWords(f)) * 4 + std::max(staged, part);
}

}  // namespace

namespace sgz {

size_t bandCarryBytes(const sgz_band_filter &f) { return twinCarryBytes<sgz_band_record>(f); }

ColumnsShape bandColumnsShape(uint32_t channels, size_t nsamples, uint32_t m, uint32_t held, int flush, uint32_t slices)
{
    return columnsShape(channels, nsamples, m, held, flush, slices, kBdSwitch, sizeof(sgz_band_record), size_t(3) * qStrideOf(nsamples) * channels * sizeof(int32_t));
}

sgz_status runBandColumns(const ColumnsShape &sh, const sgz_band_filter &f, const float *d_planar, size_t channelStride, uint32_t channels,
                          size_t nsamples, uint64_t firstIndex, uint32_t m, uint32_t held, uint32_t continued, const void *carryIn, void *carryOut,
                          sgz_band_record *d_out, void *scratch, hipStream_t stream)
{
    if (!sh.launch) return SGZ_OK;
    BandParams prm{};
    fillGrid(prm, sh, d_planar, channelStride, nsamples, m, held);
    prm.channels = channels; prm.continued = continued;
    fillTwin(prm, f, 3, channels, nsamples, firstIndex, carryIn, carryOut, d_out, scratch);
    prm.logSegs = log2Of(prm.segs);
    prm.stage = kBdStage; prm.perRound = kBdStage / prm.segs; prm.logRound = log2Of(prm.perRound); prm.rounds = f.L / prm.perRound;
    prm.coef = coefOf(f);
    return launchTwinLane<bandRunKernel, BdAcc>("band", prm, sh, f, channels, nsamples, m, runLdsBytes(f), tapsOnDevice, stream);
}

}  // namespace sgz

extern "C" {

sgz_status sgz_band_columns_limits(const sgz_band_filter *filter, uint32_t channels, uint32_t *switch_over, uint32_t *tile_samples, size_t *carry_bytes)
{
    if (sgz_status st = filterForDevice(filter, "sgz_band_columns_limits"); st != SGZ_OK) return st;
    if (channels == 0 || channels > kBdMaxChannels) return fail(SGZ_EINVAL, "sgz_band_columns_limits: 1 .. 64 channels");
    if (switch_over) *switch_over = kBdSwitch;
    if (tile_samples) *tile_samples = runTileOf(*filter);
    if (carry_bytes) *carry_bytes = bandCarryBytes(*filter) * channels;
    return SGZ_OK;
}

sgz_status sgz_stage_band_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, const sgz_band_filter *filter,
                                  uint64_t first_index, uint32_t m, uint32_t held, int flush, uint32_t continued, uint32_t slices, void *d_carry,
                                  sgz_band_record *d_records, void *stream)
{
    const StageFront front{"sgz_stage_band_columns", "channels", kBdMaxChannels, "d_records", 16, true, 40};
    // (the filter's check stands behind d_planar's: checkStageArgs.  The carry's size is read behind that check alone)
    return stageColumns(front, filterForDevice(filter, front.who), d_planar, channel_stride, channels, nsamples, m, held, flush, continued, first_index, slices, d_carry,
                        d_records, stream, bandColumnsShape, filter ? bandCarryBytes(*filter) * channels : 0,
                        [&] {                                        // (the table before anything is launched: a refused filter writes nothing)
                            const int4 *taps = nullptr;
                            return nsamples ? tapsOnDevice(*filter, &taps) : SGZ_OK;
                        },
                        [&](const ColumnsShape &sh, const void *carryIn, void *scratch, hipStream_t s) {
                            return runBandColumns(sh, *filter, d_planar, channel_stride, channels, nsamples, first_index, m, held, continued, carryIn, d_carry, d_records, scratch, s);
                        });
}

// ---- host arithmetic ---------------------------------------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

// the Oscilloscope's second-order Butterworth section at the normalised frequency fn (cycles per sample), each coefficient rounded to float
// as the live scope holds it
void butterworthSection(double fn, bool highpass, double *c)
{
    const double w0 = 6.283185307179586476925286766559 * fn;
    const double cw = std::cos(w0), alpha = std::sin(w0) / (2.0 * 0.70710678118654752440);
    const double a0 = 1 + alpha;
    const double b0 = highpass ? (1 + cw) / 2 : (1 - cw) / 2, b1 = highpass ? -(1 + cw) : 1 - cw;
    c[0] = double(float(b0 / a0)); c[1] = double(float(b1 / a0)); c[2] = double(float(b0 / a0));
    c[3] = double(float(-2 * cw / a0)); c[4] = double(float((1 - alpha) / a0));
}

unsigned __int128 sumOf(const sgz_band_record &v, int b) { return (static_cast<unsigned __int128>(v.sumsq[b][1]) << 64) | v.sumsq[b][0]; }

// the mean squares (1.0 = full scale squared) of the three bands of `ncols` columns of one channel read together
void bandMeanSquares(const sgz_band_record *recs, size_t ncols, uint32_t channels, uint32_t channel, double *ms)
{
    unsigned __int128 sum[3] = {0, 0, 0};
    uint64_t count = 0;
    for (size_t j = 0; j < ncols; ++j) {
        const sgz_band_record &v = recs[j * channels + channel];
        for (int b = 0; b < 3; ++b) sum[b] += sumOf(v, b);
        count += v.count;
    }
    for (int b = 0; b < 3; ++b) ms[b] = count ? double(sum[b]) / double(count) * 0x1p-46 : 0.0;
}

// static_cast<uint8_t>(float) as the live scope's build performs it: truncation, 0 out of range and for a NaN
uint8_t toU8(float v) { return (!(v > -1.0f) || !(v < 256.0f)) ? uint8_t(0) : uint8_t(v); }
uint8_t lerpU8(uint8_t a, uint8_t b, float t) { return toU8(float(a) + (float(b) - float(a)) * t); }

}  // namespace

extern "C" {

sgz_status sgz_band_filter_for_rate(double rate, double low_hz, double high_hz, sgz_band_filter *f)
{
    if (!f) return fail(SGZ_EINVAL, "sgz_band_filter_for_rate: null argument");
    if (!(rate > 0.0) || !std::isfinite(rate)) return fail(SGZ_EINVAL, "sgz_band_filter_for_rate: rate > 0");
    if (!(low_hz > 0.0) || !(high_hz > low_hz) || !(high_hz < rate / 2)) return fail(SGZ_EINVAL, "sgz_band_filter_for_rate: 0 < low_hz < high_hz < rate / 2");
    const double need = std::ceil(6.0 * rate / low_hz);
    if (!(need <= double(kTwinMaxW))) return fail(SGZ_EINVAL, "sgz_band_filter_for_rate: 6 rate / low_hz above 65536 samples of memory");
    sgz_band_filter r{};
    const double f1 = double(float(low_hz / rate)), f2 = double(float(high_hz / rate));
    butterworthSection(f1, false, r.c[0]); butterworthSection(f1, true, r.c[1]);
    butterworthSection(f2, false, r.c[2]); butterworthSection(f2, true, r.c[3]);
    r.W = std::max(pow2AtLeast(uint32_t(need)), 16u * kTwinMinL);
    r.L = r.W / 16;
    *f = r;
    return SGZ_OK;
}

sgz_status sgz_band_taps(const sgz_band_filter *f, int32_t *taps)
{
    if (!f || !taps) return fail(SGZ_EINVAL, "sgz_band_taps: null argument");
    if (!filterShapeOk(*f)) return fail(SGZ_EINVAL, "sgz_band_taps: W and L are powers of two, 16 <= L <= W <= 65536");
    std::vector<int32_t> t(size_t(kBdComps) * f->W);                // (a refusal writes nothing)
    if (!buildTaps(*f, t.data())) return fail(SGZ_EINVAL, "sgz_band_taps: a tap outside int32, or 2^26 sum |C| >= 2^62");
    std::memcpy(taps, t.data(), t.size() * sizeof(int32_t));
    return SGZ_OK;
}

sgz_status sgz_band_fold(const sgz_band_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns, sgz_band_record *out)
{
    return foldColumns(
        "sgz_band_fold", "channels", "", in, n, channels, x0, x1, out_columns, out,
        [](const sgz_band_record *v, size_t count, size_t stride) {
            uint64_t tally = 0;
            for (size_t j = 0; j < count; ++j) tally += v[j * stride].count;
            return tally <= 0xffffffffull;
        },
        [](const sgz_band_record *v, size_t count, size_t stride) {
            unsigned __int128 sum[3] = {0, 0, 0};
            sgz_band_record r{};
            for (size_t j = 0; j < count; ++j) {
                for (int k = 0; k < 3; ++k) sum[k] += sumOf(v[j * stride], k);
                r.count += v[j * stride].count;
            }
            for (int k = 0; k < 3; ++k) { r.sumsq[k][0] = uint64_t(sum[k]); r.sumsq[k][1] = uint64_t(sum[k] >> 64); }
            return r;
        });
}

sgz_status sgz_band_readout(const sgz_band_record *recs, size_t ncols, uint32_t channels, uint32_t channel, double *mean_square, double *db)
{
    if (!recs) return fail(SGZ_EINVAL, "sgz_band_readout: null argument");
    if (channels == 0 || ncols == 0 || channel >= channels) return fail(SGZ_EINVAL, "sgz_band_readout: channels >= 1, ncols >= 1 and channel < channels");
    double ms[3];
    bandMeanSquares(recs, ncols, channels, channel, ms);
    for (int b = 0; b < 3; ++b) {
        if (mean_square) mean_square[b] = ms[b];
        if (db) db[b] = ms[b] > 0.0 ? 10.0 * std::log10(ms[b]) : -std::numeric_limits<double>::infinity();
    }
    return SGZ_OK;
}

sgz_status sgz_band_colours(const sgz_band_record *recs, size_t ncols, uint32_t channels, uint32_t channel, const float band_colours[3][3],
                            const uint8_t key_rgba8[4], double frequency_colouring_blend, uint8_t *out_rgba8)
{
    if (!recs || !band_colours || !key_rgba8 || !out_rgba8) return fail(SGZ_EINVAL, "sgz_band_colours: null argument");
    if (channels == 0 || channel >= channels) return fail(SGZ_EINVAL, "sgz_band_colours: channels >= 1 and channel < channels");
    const float blend = 1 - float(frequency_colouring_blend);       // what the live scope hands to accumulateColour
    for (size_t j = 0; j < ncols; ++j) {
        double ms[3];
        bandMeanSquares(recs + j * channels, 1, channels, channel, ms);
        const float state[3] = {float(ms[0]), float(ms[1]), float(ms[2])};
        // accumulateColour (OscilloscopeDSP.inl:472-497) in its order; a silent column is 255 / 0 * 0, a NaN, which the conversion makes 0
        float red = 0, green = 0, blue = 0;
        for (int i = 0; i < 3; ++i) {
            red += state[i] * band_colours[i][0];
            green += state[i] * band_colours[i][1];
            blue += state[i] * band_colours[i][2];
        }
        const float invMax = 255.0f / std::fmax(red, std::fmax(blue, green));
        const uint8_t ret[4] = {toU8(red * invMax), toU8(green * invMax), toU8(blue * invMax), 255};
        for (int k = 0; k < 4; ++k) out_rgba8[j * 4 + k] = lerpU8(ret[k], key_rgba8[k], blend);
    }
    return SGZ_OK;
}

}  // extern "C"
