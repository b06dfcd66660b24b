// overview_cross.hip -- the cross overview: band power, coherence and phase per column (sgz.h, "The cross overview").  gfx950 only.
// The fourth reduction over the overview's columns, of the complex bins B [frames][pairs][N + 1] float2 that K_A writes on an SGZ_CH_PHASE plan
// (sgz_stage_bins: csf[k] = L[k], csf[N - k] = R[k]) -- the one place where both channels' complex bins exist.  Per admitted bin 1 <= k <= N/2 - 2
// of a frame the four fp64 values |L|^2, |R|^2, Re and Im of L conj R are scaled by 2^(62 - 2n), clamped, rounded once and summed as 128-bit
// integers per (column, pair, band); a bin with a non-finite float is left out and counted.  Integers only, so every field folds associatively
// and commutatively and any split of the frames (slices, calls, slabs, feeds) or of a band (tiles, finer bands) gives the same bytes.
//   overviewCrossTileKernel   a workgroup owns (column, pair, a tile of 256 consecutive bins, a slice of the column's frames).  A lane keeps its
//                             bin's four 128-bit sums and two counts in registers over the frames: loads first (the ascending L run and the
//                             descending R run are both whole contiguous rows), then products, scaling, conversion and the adds -- no cross-lane
//                             work in the loop.  At the end the tile's bins go to its bands: 32-bit limbs added into 64-bit LDS slots without
//                             return, a wave that lies inside one band folded by shuffles first (hist_columns.hip's way for its contended
//                             case), and one record per (slice, column, pair, piece) to plan scratch -- a piece is a (tile, band) that meet.
//   overviewCrossEmitKernel   one thread per (column, pair, band): the fold of the band's pieces over its tiles and the slices, the carry into
//                             column 0, and the record to the output or, for the open column, to the carry.  A launch of its own behind the
//                             first on the stream: no hand-off between workgroups inside a launch, no global atomics.
// The band table is the plan's (sgz_plan_set_cross_edges): host-built tables name every bin's band, every tile's bands and every band's tiles.
// Empty bands take no slot: the tables count the non-empty ones, so that a tile's 256 bins meet at most 256 of them.
// Nothing is waited for; scratch grows on demand (only growth synchronises); everything runs on the caller's stream.
// From overview_kinds.hpp: the step of a call, the column and slice bounds, the carry snapshot.  The launches and the host fold (band edges) are
// this file's own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "runtime.hpp"

#pragma clang fp contract(off)

#include "overview_kinds.hpp"   // behind the pragma: its templates are parsed without contraction

using namespace sgz;

namespace {

using Record = sgz_overview_cross_record;
typedef unsigned __int128 u128;
typedef __int128 i128;

constexpr int kTile = 256;               // bins of a tile and threads of a workgroup
constexpr int kUnroll = 4;               // frames whose loads are issued before the first product
constexpr uint32_t kNoBand = 0xffffffffu;
constexpr int kSlotWords = 18;           // 4 sums x 4 limbs, count, skipped
constexpr double kQMost = 9223372036854774784.0;        // 2^63 - 2^10, the largest double below 2^63
constexpr double kTwo64 = 18446744073709551616.0;

// ---- the definition, for the host and the device -------------------------------------------------------------------------------------------
__host__ __device__ inline bool finiteBits(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

__host__ __device__ inline int64_t crossRound(double x, double s)
{
    return int64_t(rint(fmin(fmax(x * s, -kQMost), kQMost)));
}

// the four q of one bin of one frame; the products are exact (48 significant bits), each sum rounds once, the scaling is exact
__host__ __device__ inline void crossQuantise(float lr, float li, float rr, float ri, double s, int64_t q[4])
{
    const double Lr = lr, Li = li, Rr = rr, Ri = ri;
    const double ll0 = Lr * Lr, ll1 = Li * Li, rr0 = Rr * Rr, rr1 = Ri * Ri;
    const double re0 = Lr * Rr, re1 = Li * Ri, im0 = Li * Rr, im1 = Lr * Ri;
    q[0] = crossRound(ll0 + ll1, s);
    q[1] = crossRound(rr0 + rr1, s);
    q[2] = crossRound(re0 + re1, s);
    q[3] = crossRound(im0 - im1, s);
}

inline double crossScale(uint32_t N)
{
    int n = 0;
    while ((uint32_t(1) << n) < N) ++n;
    return std::ldexp(1.0, 62 - 2 * n);
}

// ---- the accumulator ---------------------------------------------------------------------------------------------------------------------
struct Acc {
    u128 sum[4] = {0, 0, 0, 0};          // ll, rr, re, im; the signed ones modulo 2^128
    uint64_t count = 0, skipped = 0;
};

__device__ __forceinline__ void accBin(Acc &a, float2 L, float2 R, double s)
{
    const bool ok = finiteBits(__float_as_uint(L.x)) && finiteBits(__float_as_uint(L.y)) && finiteBits(__float_as_uint(R.x)) && finiteBits(__float_as_uint(R.y));
    // a bin left out takes the same instructions on zeros
    int64_t q[4];
    crossQuantise(ok ? L.x : 0.f, ok ? L.y : 0.f, ok ? R.x : 0.f, ok ? R.y : 0.f, s, q);
#pragma unroll
    for (int i = 0; i < 4; ++i) a.sum[i] += u128(i128(q[i]));
    a.count += ok ? 1u : 0u;
    a.skipped += ok ? 0u : 1u;
}

__device__ __forceinline__ void accFold(Acc &a, const Record &r)
{
    a.sum[0] += (u128(r.ll[1]) << 64) | u128(r.ll[0]);
    a.sum[1] += (u128(r.rr[1]) << 64) | u128(r.rr[0]);
    a.sum[2] += (u128(r.re[1]) << 64) | u128(r.re[0]);
    a.sum[3] += (u128(r.im[1]) << 64) | u128(r.im[0]);
    a.count += r.count;
    a.skipped += r.skipped;
}

__host__ __device__ inline Record accRecord(const u128 sum[4], uint64_t count, uint64_t skipped)
{
    Record r;
    r.ll[0] = uint64_t(sum[0]); r.ll[1] = uint64_t(sum[0] >> 64);
    r.rr[0] = uint64_t(sum[1]); r.rr[1] = uint64_t(sum[1] >> 64);
    r.re[0] = uint64_t(sum[2]); r.re[1] = uint64_t(sum[2] >> 64);
    r.im[0] = uint64_t(sum[3]); r.im[1] = uint64_t(sum[3] >> 64);
    r.count = count; r.skipped = skipped;
    return r;
}

// a record as five 16-byte words
__device__ __forceinline__ Record loadRecord(const Record *p)
{
    const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(p);
    const ulonglong2 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4];
    Record r;
    r.ll[0] = a.x; r.ll[1] = a.y; r.rr[0] = b.x; r.rr[1] = b.y; r.re[0] = c.x; r.re[1] = c.y; r.im[0] = d.x; r.im[1] = d.y;
    r.count = e.x; r.skipped = e.y;
    return r;
}
__device__ __forceinline__ void storeRecord(Record *p, const Record &r)
{
    ulonglong2 *q = reinterpret_cast<ulonglong2 *>(p);
    q[0] = make_ulonglong2(r.ll[0], r.ll[1]); q[1] = make_ulonglong2(r.rr[0], r.rr[1]); q[2] = make_ulonglong2(r.re[0], r.re[1]);
    q[3] = make_ulonglong2(r.im[0], r.im[1]); q[4] = make_ulonglong2(r.count, r.skipped);
}

// ---- the kernels ---------------------------------------------------------------------------------------------------------------------------
struct CrossParams {
    const float2 *bins;                  // [frames][C][N + 1]
    long frames;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t k, held, slices, C, N, B, tiles, pieces;
    double scale;
    // the plan's tables (CrossTables below)
    const uint32_t *binRank;             // [N/2]: the rank of bin k's band among the non-empty bands, or kNoBand
    const uint32_t *tileRankLo, *tileRanks, *tilePieceBase;         // [tiles]: the least rank a tile meets, how many, and its first piece
    const uint32_t *bandRank, *bandTileLo, *bandTiles;              // [B]: a band's rank (kNoBand: empty), its first tile and how many it spans
    const Record *carryIn;               // [C][B]: the records of column 0's `held` earlier frames (read iff held > 0)
    Record *carryOut;                    // [C][B]: the records of the open column
    Record *partial;                     // [slices][columns][C][pieces]
    Record *out;                         // [columns][C][B]
};

__device__ __forceinline__ uint64_t waveSum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ void __launch_bounds__(kTile)
overviewCrossTileKernel(const CrossParams prm)
{
    __shared__ unsigned long long slots[kTile * kSlotWords];
    const uint32_t tile = blockIdx.x % prm.tiles;
    const uint32_t pair = (blockIdx.x / prm.tiles) % prm.C;
    const long col = long(blockIdx.x / (prm.tiles * prm.C));
    const uint32_t nRanks = prm.tileRanks[tile];
    if (nRanks == 0) return;                                      // no bin of this tile lies in a band (uniform over the workgroup)
    const uint32_t bin = 1u + tile * kTile + threadIdx.x;
    const bool admitted = bin + 2u <= prm.N / 2u;
    const uint32_t rank = admitted ? prm.binRank[bin] : kNoBand;
    for (uint32_t i = threadIdx.x; i < nRanks * kSlotWords; i += kTile) slots[i] = 0ull;

    long a, b, sa, sb;
    columnFrames(prm, col, a, b);
    sliceRange(prm, a, b, b > a ? b - a : 0, sa, sb);
    Acc acc;
    if (rank != kNoBand) {
        const size_t perFrame = size_t(prm.C) * (size_t(prm.N) + 1);
        const float2 *rowL = prm.bins + size_t(pair) * (size_t(prm.N) + 1) + bin;
        const float2 *rowR = prm.bins + size_t(pair) * (size_t(prm.N) + 1) + (prm.N - bin);
        for (long f = sa; f < sb; f += kUnroll) {
            float2 L[kUnroll], R[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (f + u < sb) { L[u] = rowL[size_t(f + u) * perFrame]; R[u] = rowR[size_t(f + u) * perFrame]; }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (f + u < sb) accBin(acc, L[u], R[u], prm.scale);
        }
    }
    __syncthreads();                                              // the slots are zero

    // the lane's 18 words: the sums as 32-bit limbs, which add in 64-bit slots without a carry between them
    uint64_t w[kSlotWords];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int l = 0; l < 4; ++l) w[i * 4 + l] = uint64_t(uint32_t(acc.sum[i] >> (32 * l)));
    w[16] = acc.count; w[17] = acc.skipped;
    const uint32_t first = __shfl(rank, 0, 64);
    if (__all(rank == first)) {
        // the wave lies inside one band (or outside every band): one lane adds the wave's sums
        if (first != kNoBand) {
#pragma unroll
            for (int i = 0; i < kSlotWords; ++i) w[i] = waveSum(w[i]);
            if ((threadIdx.x & 63u) == 0u) {
                unsigned long long *slot = slots + size_t(first - prm.tileRankLo[tile]) * kSlotWords;
#pragma unroll
                for (int i = 0; i < kSlotWords; ++i) atomicAdd(slot + i, (unsigned long long)w[i]);
            }
        }
    } else if (rank != kNoBand) {
        unsigned long long *slot = slots + size_t(rank - prm.tileRankLo[tile]) * kSlotWords;
#pragma unroll
        for (int i = 0; i < kSlotWords; ++i) atomicAdd(slot + i, (unsigned long long)w[i]);
    }
    __syncthreads();

    if (threadIdx.x < nRanks) {
        const unsigned long long *slot = slots + size_t(threadIdx.x) * kSlotWords;
        u128 sum[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sum[i] = 0;
#pragma unroll
            for (int l = 0; l < 4; ++l) sum[i] += u128(slot[i * 4 + l]) << (32 * l);   // (bits past 2^128 fall off: the sums are modulo 2^128)
        }
        const size_t at = ((size_t(blockIdx.y) * size_t(prm.columns) + size_t(col)) * prm.C + pair) * prm.pieces + prm.tilePieceBase[tile] + threadIdx.x;
        storeRecord(prm.partial + at, accRecord(sum, slot[16], slot[17]));
    }
}

__global__ void __launch_bounds__(kTile)
overviewCrossEmitKernel(const CrossParams prm)
{
    const size_t idx = size_t(blockIdx.x) * kTile + threadIdx.x;
    const size_t perColumn = size_t(prm.C) * prm.B;
    if (idx >= size_t(prm.columns) * perColumn) return;
    const long col = long(idx / perColumn);
    const uint32_t pair = uint32_t((idx % perColumn) / prm.B), band = uint32_t(idx % prm.B);
    Acc acc;
    const uint32_t rank = prm.bandRank[band];
    if (rank != kNoBand && prm.frames > 0) {
        const uint32_t t0 = prm.bandTileLo[band], nt = prm.bandTiles[band];
        const size_t perSlice = size_t(prm.columns) * prm.C * prm.pieces;
        const Record *base = prm.partial + (size_t(col) * prm.C + pair) * prm.pieces;
        for (uint32_t s = 0; s < prm.slices; ++s)
            for (uint32_t t = t0; t < t0 + nt; ++t)
                accFold(acc, loadRecord(base + size_t(s) * perSlice + prm.tilePieceBase[t] + (rank - prm.tileRankLo[t])));
    }
    if (col == 0 && prm.held) accFold(acc, loadRecord(prm.carryIn + size_t(pair) * prm.B + band));
    const Record r = accRecord(acc.sum, acc.count, acc.skipped);
    if (col < prm.closed) storeRecord(prm.out + idx, r);
    else storeRecord(prm.carryOut + size_t(pair) * prm.B + band, r);
}

// ---- the plan's band table -----------------------------------------------------------------------------------------------------------------
// one device block of uint32: binRank [N/2] | tileRankLo, tileRanks, tilePieceBase [tiles] each | bandRank, bandTileLo, bandTiles [B] each
struct CrossTables {
    std::vector<uint32_t> words;
    uint32_t tiles = 0, pieces = 0;
};

CrossTables buildTables(uint32_t N, const uint32_t *edges, uint32_t B)
{
    CrossTables t;
    const uint32_t half = N / 2, admitted = half - 2;                // bins 1 .. N/2 - 2
    t.tiles = (admitted + kTile - 1) / kTile;
    t.words.assign(size_t(half) + 3 * size_t(t.tiles) + 3 * size_t(B), 0u);
    uint32_t *binRank = t.words.data(), *tileRankLo = binRank + half, *tileRanks = tileRankLo + t.tiles, *tilePieceBase = tileRanks + t.tiles;
    uint32_t *bandRank = tilePieceBase + t.tiles, *bandTileLo = bandRank + B, *bandTiles = bandTileLo + B;
    std::fill(binRank, binRank + half, kNoBand);
    uint32_t rank = 0;
    for (uint32_t b = 0; b < B; ++b) {
        if (edges[b] == edges[b + 1]) { bandRank[b] = kNoBand; continue; }
        bandRank[b] = rank;
        for (uint32_t k = edges[b]; k < edges[b + 1]; ++k) binRank[k] = rank;
        bandTileLo[b] = (edges[b] - 1) / kTile;
        bandTiles[b] = (edges[b + 1] - 2) / kTile - bandTileLo[b] + 1;
        ++rank;
    }
    for (uint32_t tile = 0; tile < t.tiles; ++tile) {
        uint32_t lo = kNoBand, hi = 0;
        for (uint32_t k = 1 + tile * kTile; k < 1 + (tile + 1) * kTile && k <= admitted; ++k)
            if (binRank[k] != kNoBand) { lo = std::min(lo, binRank[k]); hi = std::max(hi, binRank[k]); }
        tileRankLo[tile] = lo == kNoBand ? 0u : lo;
        tileRanks[tile] = lo == kNoBand ? 0u : hi - lo + 1;
        tilePieceBase[tile] = t.pieces;
        t.pieces += tileRanks[tile];
    }
    return t;
}

sgz_status checkEdges(uint32_t N, const uint32_t *edges, uint32_t B, const char *who)
{
    if (!edges) return fail(SGZ_EINVAL, std::string(who) + ": null edges");
    if (B < 1 || B > 4096) return fail(SGZ_EINVAL, std::string(who) + ": 1 .. 4096 bands");
    if (edges[0] < 1 || edges[B] > N / 2 - 1) return fail(SGZ_EINVAL, std::string(who) + ": 1 <= edges[0] and edges[bands] <= N/2 - 1");
    for (uint32_t b = 0; b < B; ++b)
        if (edges[b] > edges[b + 1]) return fail(SGZ_EINVAL, std::string(who) + ": the edges do not descend");
    return SGZ_OK;
}

// S -> double as the power overview does: hi 2^64 + lo; a signed sum through its magnitude
double unsignedDouble(u128 s) { return double(uint64_t(s >> 64)) * kTwo64 + double(uint64_t(s)); }
double signedDouble(u128 s)
{
    const bool neg = (s >> 127) != 0;
    const double m = unsignedDouble(neg ? u128(0) - s : s);
    return neg ? -m : m;
}
u128 word128(const uint64_t w[2]) { return (u128(w[1]) << 64) | u128(w[0]); }

}  // namespace

namespace sgz {

sgz_status crossOverviewSupported(const Plan &p)
{
    if (p.cfg.algorithm == SGZ_ALGO_RSNT) return fail(SGZ_EUNSUPPORTED, "the cross overview reduces transform bins: RSNT plans are not supported");
    if (p.cfg.channel_mode != SGZ_CH_PHASE) return fail(SGZ_EUNSUPPORTED, "the cross overview reduces the complex bins of both channels: only SGZ_CH_PHASE plans keep them");
    if (p.N < 8 || (p.N & (p.N - 1)) != 0) return fail(SGZ_EUNSUPPORTED, "the cross overview: N = 2^n >= 8");
    return SGZ_OK;
}

// sgz_stage_overview_cross behind its argument checks.  d_bins [frames][C][N + 1] float2.
sgz_status runOverviewCrossColumns(Plan &p, const float *d_bins, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                   sgz_overview_cross_record *d_carry, sgz_overview_cross_record *d_cross, hipStream_t stream)
{
    const OverviewStep sh = overviewStepShape(k, held, frames, flush);
    const uint64_t columns = sh.columns;
    if (!sh.launch || columns == 0) return SGZ_OK;
    const uint32_t B = p.crossBands, tiles = p.crossTiles;
    const uint64_t units = columns * p.C * tiles, records = columns * p.C * B;
    if (units > 0x7fffffffull || records > 0x7fffffffull * kTile || frames > size_t(0x7fffffffffffffffll))
        return fail(SGZ_EINVAL, "too many columns for one launch");
    CrossParams prm{};
    prm.bins = reinterpret_cast<const float2 *>(d_bins);
    prm.frames = long(frames); prm.columns = long(columns); prm.closed = long(sh.closed);
    prm.k = k; prm.held = held; prm.C = p.C; prm.N = p.N; prm.B = B; prm.tiles = tiles; prm.pieces = p.crossPieces;
    prm.scale = crossScale(p.N);
    const uint32_t half = p.N / 2;
    prm.binRank = p.d_crossTables; prm.tileRankLo = prm.binRank + half; prm.tileRanks = prm.tileRankLo + tiles; prm.tilePieceBase = prm.tileRanks + tiles;
    prm.bandRank = prm.tilePieceBase + tiles; prm.bandTileLo = prm.bandRank + B; prm.bandTiles = prm.bandTileLo + B;
    prm.carryOut = d_carry; prm.out = d_cross;
    if (sgz_status st = snapshotCarry<Record>(p, kOvCross, sh, held, d_carry, size_t(p.C) * B, stream, &prm.carryIn); st != SGZ_OK) return st;
    prm.slices = slices ? slices : overviewAutoSlices(long(columns), std::max(1u, p.C * tiles), k, frames, numCUs());
    if (frames > 0 && prm.pieces > 0) {
        if (sgz_status st = ensureCap(&p.ov[kOvCross].d_partial, &p.ov[kOvCross].partialCap, size_t(prm.slices) * size_t(columns) * p.C * prm.pieces * kRecordFloats<Record>); st != SGZ_OK) return st;
        prm.partial = reinterpret_cast<Record *>(p.ov[kOvCross].d_partial);
        hipLaunchKernelGGL(overviewCrossTileKernel, dim3(unsigned(units), prm.slices), dim3(kTile), 0, stream, prm);
        SGZ_HIP(hipGetLastError());
    } else {
        prm.frames = 0;                                           // the emit launch reads no piece
    }
    hipLaunchKernelGGL(overviewCrossEmitKernel, dim3(unsigned((records + kTile - 1) / kTile)), dim3(kTile), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

}  // namespace sgz

struct sgz_plan { Plan impl; };

extern "C" sgz_status sgz_plan_set_cross_edges(sgz_plan *plan, const uint32_t *edges, uint32_t bands)
{
    if (!plan) return fail(SGZ_EINVAL, "null argument");
    Plan &p = plan->impl;
    if (sgz_status st = crossOverviewSupported(p); st != SGZ_OK) return st;
    if (sgz_status st = checkEdges(p.N, edges, bands, "sgz_plan_set_cross_edges"); st != SGZ_OK) return st;
    const CrossTables t = buildTables(p.N, edges, bands);
    uint32_t *d_new = nullptr;
    SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&d_new), t.words.size() * sizeof(uint32_t)));
    if (hipError_t e = hipMemcpy(d_new, t.words.data(), t.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice); e != hipSuccess) {
        (void)hipFree(d_new);
        return hipFail(e, "hipMemcpy (cross band tables)");
    }
    if (p.d_crossTables) (void)hipFree(p.d_crossTables);          // (waits for the launches that read it)
    p.d_crossTables = d_new;
    p.crossEdges.assign(edges, edges + bands + 1);
    p.crossBands = bands; p.crossTiles = t.tiles; p.crossPieces = t.pieces;
    return SGZ_OK;
}

extern "C" sgz_status sgz_stage_overview_cross(sgz_plan *plan, const float *d_bins, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                               sgz_overview_cross_record *d_carry, sgz_overview_cross_record *d_cross, void *stream)
{
    if (!plan || !d_bins) return fail(SGZ_EINVAL, "null argument");
    if (sgz_status st = crossOverviewSupported(plan->impl); st != SGZ_OK) return st;
    if (sgz_status st = checkOverviewStep(k, held, frames); st != SGZ_OK) return st;
    if (slices > kOvMaxSlices) return fail(SGZ_EINVAL, "sgz_stage_overview_cross: slices 0 (automatic) or 1 .. 64");
    if (!plan->impl.crossBands) return fail(SGZ_EINVAL, "sgz_stage_overview_cross: the plan has no band table (sgz_plan_set_cross_edges)");
    const OverviewStep sh = overviewStepShape(k, held, frames, flush);
    if (!d_cross && sh.closed && sh.launch) return fail(SGZ_EINVAL, "sgz_stage_overview_cross: d_cross is written (a column closes)");
    if (!d_carry && (held || sh.open)) return fail(SGZ_EINVAL, "sgz_stage_overview_cross: d_carry is read (held > 0) or written (frames stay open)");
    if (!sh.launch) return SGZ_OK;
    return runOverviewCrossColumns(plan->impl, d_bins, frames, k, held, flush, slices, d_carry, d_cross, reinterpret_cast<hipStream_t>(stream));
}

// ---- the host helpers (no GPU) ----------------------------------------------------------------------------------------------------------------
extern "C" sgz_status sgz_overview_cross_quantise(uint32_t n, const float *lr, const float *li, const float *rr, const float *ri, size_t count,
                                                  int64_t *q, uint8_t *skipped)
{
    if ((!lr || !li || !rr || !ri || !q || !skipped) && count) return fail(SGZ_EINVAL, "sgz_overview_cross_quantise: null argument");
    if (n < 3 || n > 30) return fail(SGZ_EINVAL, "sgz_overview_cross_quantise: N = 2^n, 3 <= n <= 30");
    const double s = std::ldexp(1.0, 62 - 2 * int(n));
    for (size_t i = 0; i < count; ++i) {
        uint32_t bits[4];
        std::memcpy(bits + 0, lr + i, 4); std::memcpy(bits + 1, li + i, 4); std::memcpy(bits + 2, rr + i, 4); std::memcpy(bits + 3, ri + i, 4);
        const bool ok = finiteBits(bits[0]) && finiteBits(bits[1]) && finiteBits(bits[2]) && finiteBits(bits[3]);
        skipped[i] = ok ? 0u : 1u;
        if (ok) crossQuantise(lr[i], li[i], rr[i], ri[i], s, q + 4 * i);
        else q[4 * i] = q[4 * i + 1] = q[4 * i + 2] = q[4 * i + 3] = 0;                 // (a bin left out has no q)
    }
    return SGZ_OK;
}

extern "C" sgz_status sgz_overview_cross_fold(const sgz_overview_cross_record *in, size_t n, size_t pairs, const uint32_t *edges, uint32_t bands,
                                              size_t x0, size_t x1, uint32_t out_columns, const uint32_t *coarse_edges, uint32_t coarse_bands,
                                              sgz_overview_cross_record *out)
{
    if (!in || !out) return fail(SGZ_EINVAL, "sgz_overview_cross_fold: null argument");
    if (pairs == 0 || bands == 0) return fail(SGZ_EINVAL, "sgz_overview_cross_fold: pairs >= 1 and bands >= 1 records per column");
    uint64_t cols = 0;
    if (sgz_status st = checkViewRange(n, x0, x1, out_columns, &cols); st != SGZ_OK) return st;
    // the fine bands [lo[c], hi[c]) of every output band
    std::vector<uint32_t> lo, hi;
    if (coarse_edges) {
        if (!edges) return fail(SGZ_EINVAL, "sgz_overview_cross_fold: a fold over bands needs the fine edges");
        if (coarse_bands == 0) return fail(SGZ_EINVAL, "sgz_overview_cross_fold: coarse_bands >= 1");
        for (uint32_t b = 0; b < bands; ++b)
            if (edges[b] > edges[b + 1]) return fail(SGZ_EINVAL, "sgz_overview_cross_fold: the edges do not descend");
        for (uint32_t c = 0; c <= coarse_bands; ++c) {
            if (c && coarse_edges[c - 1] > coarse_edges[c]) return fail(SGZ_EINVAL, "sgz_overview_cross_fold: the coarse edges do not descend");
            if (!std::binary_search(edges, edges + bands + 1, coarse_edges[c]))
                return fail(SGZ_EINVAL, "sgz_overview_cross_fold: every coarse edge must be a fine edge");
        }
        for (uint32_t c = 0; c < coarse_bands; ++c) {
            // the non-empty fine bands inside [coarse_edges[c], coarse_edges[c + 1]): from the last fine edge equal to the lower coarse edge
            // to the first equal to the upper one
            const uint32_t a = uint32_t(std::upper_bound(edges, edges + bands + 1, coarse_edges[c]) - edges) - 1;
            const uint32_t b = uint32_t(std::lower_bound(edges, edges + bands + 1, coarse_edges[c + 1]) - edges);
            lo.push_back(a); hi.push_back(std::max(a, b));
        }
    } else {
        for (uint32_t b = 0; b < bands; ++b) { lo.push_back(b); hi.push_back(b + 1); }
    }
    const size_t outBands = lo.size();
    const uint64_t m = x1 - x0;
    // two passes: nothing is written when any count overflows
    for (int pass = 0; pass < 2; ++pass)
        for (uint64_t c = 0; c < cols; ++c) {
            const uint64_t ja = x0 + (c * m + cols - 1) / cols, jb = x0 + ((c + 1) * m + cols - 1) / cols;
            for (size_t pair = 0; pair < pairs; ++pair)
                for (size_t ob = 0; ob < outBands; ++ob) {
                    u128 sum[4] = {0, 0, 0, 0}, count = 0, skipped = 0;
                    for (uint64_t j = ja; j < jb; ++j)
                        for (uint32_t b = lo[ob]; b < hi[ob]; ++b) {
                            if (coarse_edges && edges[b] == edges[b + 1]) continue;         // (an empty fine band holds no bin)
                            const Record &r = in[(j * pairs + pair) * bands + b];
                            sum[0] += word128(r.ll); sum[1] += word128(r.rr); sum[2] += word128(r.re); sum[3] += word128(r.im);
                            count += r.count; skipped += r.skipped;
                        }
                    if ((count >> 64) != 0 || (skipped >> 64) != 0)
                        return fail(SGZ_EINVAL, "sgz_overview_cross_fold: a folded record counts more than 2^64 - 1 bin-frames");
                    if (pass) out[(c * pairs + pair) * outBands + ob] = accRecord(sum, uint64_t(count), uint64_t(skipped));
                }
        }
    return SGZ_OK;
}

extern "C" sgz_status sgz_overview_cross_readout(const sgz_overview_cross_record *in, size_t count, sgz_overview_cross_reading *out)
{
    if ((!in || !out) && count) return fail(SGZ_EINVAL, "sgz_overview_cross_readout: null argument");
    const double nan = std::nan("");
    for (size_t i = 0; i < count; ++i) {
        const Record &r = in[i];
        sgz_overview_cross_reading &o = out[i];
        if (r.count == 0) { o.ll = o.rr = o.mid = o.side = o.re = o.im = o.coherence = o.phase = o.correlation = nan; continue; }
        const u128 sll = word128(r.ll), srr = word128(r.rr), sre = word128(r.re), sim = word128(r.im);
        const double A = unsignedDouble(sll), B = unsignedDouble(srr), C = signedDouble(sre), D = signedDouble(sim);
        const double cnt = double(r.count);
        constexpr double k60 = 8.6736173798840355e-19, k62 = 2.1684043449710089e-19;       // 2^-60, 2^-62
        o.ll = A / cnt * k60; o.rr = B / cnt * k60; o.re = C / cnt * k60; o.im = D / cnt * k60;
        const u128 mid = sll + srr + (sre << 1), side = sll + srr - (sre << 1);           // exact in 128 bits
        o.mid = ((mid >> 127) ? 0.0 : unsignedDouble(mid)) / cnt * k62;
        o.side = ((side >> 127) ? 0.0 : unsignedDouble(side)) / cnt * k62;
        const double ab = A * B;
        o.phase = std::atan2(D, C);
        if (ab == 0.0) { o.coherence = o.correlation = nan; continue; }
        o.coherence = std::fmin(1.0, (C * C + D * D) / ab);
        o.correlation = C / std::sqrt(ab);
    }
    return SGZ_OK;
}

extern "C" sgz_status sgz_overview_cross_unit(const sgz_plan *plan, double *unit)
{
    if (!plan || !unit) return fail(SGZ_EINVAL, "null argument");
    const Plan &p = plan->impl;
    const double v = double(p.scalars.invSize) * double(p.N) / 2.0;
    *unit = v * v;
    return SGZ_OK;
}

extern "C" sgz_status sgz_cross_edges_octave(double sample_rate, uint32_t N, uint32_t bands_per_octave, double f_lo, double f_hi, uint32_t *edges,
                                             uint32_t capacity, uint32_t *bands, double *centres)
{
    if (!edges || !bands) return fail(SGZ_EINVAL, "sgz_cross_edges_octave: null argument");
    if (!(sample_rate > 0.0) || N < 8 || (N & (N - 1)) != 0) return fail(SGZ_EINVAL, "sgz_cross_edges_octave: sample_rate > 0 and N = 2^n >= 8");
    if (bands_per_octave < 1 || bands_per_octave > 48) return fail(SGZ_EINVAL, "sgz_cross_edges_octave: 1 .. 48 bands per octave");
    if (!(f_lo > 0.0) || !(f_hi >= f_lo) || !std::isfinite(f_hi)) return fail(SGZ_EINVAL, "sgz_cross_edges_octave: 0 < f_lo <= f_hi");
    const double b = double(bands_per_octave);
    const double down = std::exp2(-1.0 / (2.0 * b)), up = std::exp2(1.0 / (2.0 * b));
    const long j0 = long(std::floor(b * std::log2(f_lo / 1000.0))) - 2, j1 = long(std::ceil(b * std::log2(f_hi / 1000.0))) + 2;
    const double most = double(N / 2 - 1);
    const auto edge = [&](double f, double factor) { return uint32_t(std::fmin(std::fmax(std::ceil(f * factor * double(N) / sample_rate), 1.0), most)); };
    uint32_t count = 0;
    double last = 0.0;
    for (long j = j0; j <= j1; ++j) {
        const double f = 1000.0 * std::exp2(double(j) / b);
        if (!(f_lo <= f && f <= f_hi)) continue;
        if (count + 2 > capacity) return fail(SGZ_EINVAL, "sgz_cross_edges_octave: capacity below bands + 1 edges");
        if (count >= 4096) return fail(SGZ_EINVAL, "sgz_cross_edges_octave: more than 4096 bands");
        edges[count] = edge(f, down);
        if (centres) centres[count] = f;
        last = f;
        ++count;
    }
    if (count == 0) return fail(SGZ_EINVAL, "sgz_cross_edges_octave: no centre 1000 * 2^(j / b) lies in [f_lo, f_hi]");
    edges[count] = edge(last, up);
    *bands = count;
    return SGZ_OK;
}
