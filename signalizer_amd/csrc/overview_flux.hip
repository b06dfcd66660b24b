// overview_flux.hip -- the flux overview: onset strength, centroid and spread of k frames per column (sgz.h, "The flux overview").  gfx950 only.
// The first reduction ALONG the frequency axis, and the first that compares a frame with the frame before it, of the mapped magnitudes M
// [frames][pairs][sides][P] that K_A leaves in HBM:
//   a(x) = rint(min(|x| 2^30, 2^34)), a NaN 0 and its frame marked; per frame and row (pair, side)  A = sum a_i, M1 = sum i a_i, M2 = sum i^2 a_i,
//   F = sum max(0, a_i(f) - a_i(f - 1)) (0 without a predecessor); per (column, row) one 88-byte record of the 128-bit sums of A, M1, M2 and F over
//   the column's frames, the greatest F with the first frame that attains it, the frames and the marked frames.  Integers and an order's extreme, so
//   every field folds associatively and commutatively and any split of the frames (runs, slices, calls, slabs, feeds) gives the same bytes.
// A workgroup of 256 threads owns a run of consecutive frames of one row.  Thread t owns the pixels [4 (256 c + t), + 4) of every pass c, so a pixel's
// previous a never leaves its thread: in registers for P <= 2048 (MODE = passes), and for larger P as the frame's raw bits in the thread's own words
// of a 48 KiB LDS row (P <= 12288) or, beyond that, fetched again from the previous row, which the L2 still holds (MODE 0).  Only a run's first
// frame costs a second fetch from HBM: the frame in front of it, or d_prev for frame 0 of the call.  Loads are 16 bytes wide where a row starts on a
// 16-byte boundary.  Per frame one cross-lane reduction of F (wave shuffles, then four LDS slots, one barrier; the slots alternate with the frame's
// parity); the three moment sums stay per thread as unsigned __int128 and reduce where a column ends.  No floating-point sum, no atomics, no
// hand-off between workgroups inside a launch.  Three shapes, as the siblings':
//   overviewFluxColumnsKernel   a run of G whole columns per workgroup; thread 0 folds the carry into column 0 and writes every record.
//   overviewFluxSliceKernel     few columns of many frames: slice s of a column's frames -> partial records [slices][columns][rows] in plan scratch;
//   overviewFluxEmitKernel      behind it on the stream, one thread per (column, row): the fold over the slices and the carry.
// Nothing is waited for; scratch grows on demand (only growth synchronises); everything runs on the caller's stream.
// From overview_kinds.hpp: the step of a call, the column bounds, the carry snapshot and the host fold's frame.  The launches and the slice
// range (its start is clamped) are this file's own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "runtime.hpp"

#pragma clang fp contract(off)

#include "overview_kinds.hpp"   // behind the pragma: its templates are parsed without contraction

using namespace sgz;

static_assert(sizeof(sgz_overview_flux_record) == 88 && alignof(sgz_overview_flux_record) == 8, "sgz_overview_flux_record: 88 bytes, 8-aligned");
static_assert(offsetof(sgz_overview_flux_record, amp) == 0 && offsetof(sgz_overview_flux_record, mom1) == 16 && offsetof(sgz_overview_flux_record, mom2) == 32 &&
              offsetof(sgz_overview_flux_record, flux) == 48 && offsetof(sgz_overview_flux_record, flux_max) == 64 &&
              offsetof(sgz_overview_flux_record, flux_at) == 72 && offsetof(sgz_overview_flux_record, count) == 80 &&
              offsetof(sgz_overview_flux_record, nans) == 84, "sgz_overview_flux_record: the layout sgz.h documents");

namespace {

using Record = sgz_overview_flux_record;
typedef unsigned __int128 u128;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kPass = 4u * kThreads;            // pixels of one pass: 16 bytes per thread
constexpr uint32_t kRegPasses = 2;                   // P <= 2048: the previous a in registers
constexpr uint32_t kLdsPixels = 12288;               // P <= 12288: the previous frame's bits in LDS (48 KiB)
constexpr uint32_t kRunFrames = 32;                  // a run of whole columns has at most this many frames (one column when k is above it)
constexpr uint64_t kWantGroups = 512;                // ... and is shortened while the launch would have fewer workgroups than this
constexpr uint32_t kSliceFrames = 8;                 // an automatic slice keeps at least this many frames: each slice pays one halo fetch
constexpr double kQuantum = 1073741824.0;            // 2^30 steps per unit of amplitude
constexpr double kQMost = 17179869184.0;             // 2^34: the clamp, at |x| = 16
constexpr double kTwo64 = 18446744073709551616.0;
constexpr double kAmpScale = 9.3132257461547852e-10; // 2^-30

// ---- the definition, for the host and the device -------------------------------------------------------------------------------------------
// a of a non-NaN value: the product is exact (24 significant bits), +inf stays +inf and clamps; rint goes to even; the result is an integer
// below 2^35 and converts exactly.  A NaN handed in takes the same instructions (fmin drops it for the clamp); the caller masks it to 0
__host__ __device__ inline uint64_t fluxQuantise(float x)
{
    return uint64_t(rint(fmin(fabs(double(x)) * kQuantum, kQMost)));
}

// a 128-bit sum as a double: the first term is exact, the conversion of the low word and the addition round to nearest even
inline double wide(const uint64_t w[2]) { return double(w[1]) * kTwo64 + double(w[0]); }

// ---- the accumulator of one (column, row) ---------------------------------------------------------------------------------------------------
struct Acc {
    u128 amp = 0, m1 = 0, m2 = 0, flux = 0;
    uint64_t fmax = 0, fat = ~0ull;      // the greatest F and the first frame that attains it; no frame yet: 0 and UINT64_MAX
    uint32_t count = 0, nans = 0;
};

__host__ __device__ inline void accPeak(Acc &a, uint64_t F, uint64_t at)
{
    if (F > a.fmax || (F == a.fmax && at < a.fat)) { a.fmax = F; a.fat = at; }
}

__host__ __device__ inline u128 wide128(const uint64_t w[2]) { return (u128(w[1]) << 64) | u128(w[0]); }

__device__ __forceinline__ void accFold(Acc &a, const Record &r)
{
    a.amp += wide128(r.amp); a.m1 += wide128(r.mom1); a.m2 += wide128(r.mom2); a.flux += wide128(r.flux);
    accPeak(a, r.flux_max, r.flux_at);
    a.count += r.count; a.nans += r.nans;
}

__host__ __device__ inline void accRecord(const Acc &a, Record &r)
{
    r.amp[0] = uint64_t(a.amp); r.amp[1] = uint64_t(a.amp >> 64);
    r.mom1[0] = uint64_t(a.m1); r.mom1[1] = uint64_t(a.m1 >> 64);
    r.mom2[0] = uint64_t(a.m2); r.mom2[1] = uint64_t(a.m2 >> 64);
    r.flux[0] = uint64_t(a.flux); r.flux[1] = uint64_t(a.flux >> 64);
    r.flux_max = a.fmax; r.flux_at = a.fat;
    r.count = a.count; r.nans = a.nans;
}

struct FluxParams {
    const uint32_t *mapped;              // [frames][R][P], the floats' bits
    long frames;
    long columns, closed;                // columns this call touches; the first `closed` of them are emitted, a last open one goes to carryOut
    uint32_t k, held, P, R;              // R = pairs * sides rows per frame
    uint32_t G, slices;                  // columns of a run (columns kernel); slices of a column (slice and emit kernels)
    uint64_t firstFrame;                 // the absolute index of frame 0 of the call
    const uint32_t *prevIn;              // [R][P]: the frame before frame 0, or null: frame 0 has no predecessor
    uint32_t *prevOut;                   // [R][P]: receives the call's last frame, or null
    const Record *carryIn;               // [R]: the record of column 0's `held` earlier frames (read iff held > 0)
    Record *carryOut;                    // [R]: the record of the open column
    Record *partial;                     // [slices][columns][R]
    Record *flux;                        // [columns][R]
};

// what becomes of a (column, row)'s accumulator: the carry into column 0, then a closed column's record or the open one's carry
__device__ __forceinline__ void emitColumn(const FluxParams &prm, long col, uint32_t r, Acc acc)
{
    if (col == 0 && prm.held) accFold(acc, prm.carryIn[r]);
    Record rec;
    accRecord(acc, rec);
    if (col < prm.closed) prm.flux[size_t(col) * prm.R + r] = rec;
    else prm.carryOut[r] = rec;
}

// ---- one thread's four pixels ----------------------------------------------------------------------------------------------------------------
struct Quad { uint32_t w[4]; };

// pixels [base, base + 4) of a row of P (global, or the LDS row through a flat pointer); past the row's end 0, whose a is 0.  wide16: the row
// starts on a 16-byte boundary
__device__ __forceinline__ Quad loadQuad(const uint32_t *row, uint32_t base, uint32_t P, bool wide16)
{
    Quad q;
    if (wide16 && base + 4u <= P) {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + base);
        q.w[0] = v.x; q.w[1] = v.y; q.w[2] = v.z; q.w[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) q.w[j] = base + j < P ? row[base + j] : 0u;
    }
    return q;
}

__device__ __forceinline__ void storeQuad(uint32_t *row, uint32_t base, uint32_t P, const Quad &q)
{
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if (base + j < P) row[base + j] = q.w[j];
}

__device__ __forceinline__ bool isWide16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// a of the four, a NaN 0 and reported
__device__ __forceinline__ bool quantiseQuad(const Quad &q, uint64_t a[4])
{
    bool nan = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float x = __uint_as_float(q.w[j]);
        const bool n = x != x;
        nan |= n;
        a[j] = n ? 0ull : fluxQuantise(x);
    }
    return nan;
}

struct Moments { u128 amp = 0, m1 = 0, m2 = 0; };

// the four pixels at `base` into the thread's sums: with S = sum a_j, w1 = sum j a_j, w2 = sum j^2 a_j (j = 0 .. 3)
//   sum (base + j) a_j = base S + w1 < 2^57;   sum (base + j)^2 a_j = base^2 S + 2 base w1 + w2, the first product in 128 bits
// and the rectified difference against the previous a, which the new one replaces
__device__ __forceinline__ void accQuad(Moments &m, uint64_t &F, uint32_t base, const uint64_t a[4], uint64_t prev[4])
{
    const uint64_t S = a[0] + a[1] + a[2] + a[3];
    const uint64_t w1 = a[1] + 2u * a[2] + 3u * a[3], w2 = a[1] + 4u * a[2] + 9u * a[3];
    const uint64_t b = base;
    m.amp += S;
    m.m1 += b * S + w1;
    m.m2 += u128(b * b) * S + u128(2u * b * w1) + w2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        F += a[j] > prev[j] ? a[j] - prev[j] : 0ull;
        prev[j] = a[j];
    }
}

// ---- the cross-lane reductions ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t shuffleXor(uint64_t v, int o) { return __shfl_xor((unsigned long long)v, o); }
__device__ __forceinline__ uint64_t waveSum(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shuffleXor(v, o);
    return v;
}
__device__ __forceinline__ u128 waveSum(u128 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (u128(shuffleXor(uint64_t(v >> 64), o)) << 64) | u128(shuffleXor(uint64_t(v), o));
    return v;
}

struct Shared {
    uint64_t F[2][kWaves];               // a frame's F per wave, by the frame's parity
    uint32_t nan[2][kWaves];
    uint64_t mom[kWaves][6];             // a column's moment sums per wave
};

// the frame's F and mark, over the workgroup, into thread 0's accumulator.  One barrier: the slots of the frame after next are written behind the
// next frame's barrier, which thread 0 reaches after it has read these
__device__ __forceinline__ void frameReduce(Shared &sh, long f, uint64_t F, bool nan, Acc &acc, uint64_t at)
{
    const uint32_t wave = threadIdx.x >> 6, par = uint32_t(f) & 1u;
    F = waveSum(F);
    const bool any = __ballot(nan) != 0ull;
    if ((threadIdx.x & 63u) == 0) { sh.F[par][wave] = F; sh.nan[par][wave] = any ? 1u : 0u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t total = 0; uint32_t marked = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) { total += sh.F[par][w]; marked |= sh.nan[par][w]; }
        acc.flux += total;
        accPeak(acc, total, at);
        acc.count += 1u; acc.nans += marked;
    }
}

// the moment sums of the frames since the last call, over the workgroup, into thread 0's accumulator; every thread's sums start over.  At least one
// frameReduce lies between two calls: its barrier keeps the next call's writes behind thread 0's reads
__device__ __forceinline__ void momentsReduce(Shared &sh, Moments &m, Acc &acc)
{
    const uint32_t wave = threadIdx.x >> 6;
    const u128 amp = waveSum(m.amp), m1 = waveSum(m.m1), m2 = waveSum(m.m2);
    if ((threadIdx.x & 63u) == 0) {
        sh.mom[wave][0] = uint64_t(amp); sh.mom[wave][1] = uint64_t(amp >> 64);
        sh.mom[wave][2] = uint64_t(m1); sh.mom[wave][3] = uint64_t(m1 >> 64);
        sh.mom[wave][4] = uint64_t(m2); sh.mom[wave][5] = uint64_t(m2 >> 64);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            acc.amp += wide128(&sh.mom[w][0]); acc.m1 += wide128(&sh.mom[w][2]); acc.m2 += wide128(&sh.mom[w][4]);
        }
    }
    m = Moments{};
}

// ---- the walk over a run's frames ------------------------------------------------------------------------------------------------------------
// frames [fa, fb) of row r (fa < fb), all threads of the workgroup.  SLICED: the frames are one slice's and thread 0 returns their accumulator in
// `acc`; otherwise they are whole columns from column `col` on (the call's first and last may be shorter), emitted where each ends.
// MODE 1, 2: that many passes, the previous a in registers.  MODE 0: any P, the previous frame as bits behind `prevRow`
template <int MODE, bool SLICED>
__device__ __forceinline__ void walkFrames(const FluxParams &prm, Shared &sh, uint32_t *ldsRow, uint32_t r, long fa, long fb, long col, Acc &acc)
{
    const uint32_t P = prm.P, t = threadIdx.x;
    const size_t perFrame = size_t(prm.R) * P;
    const uint32_t *row = prm.mapped + size_t(r) * P;                  // frame 0's row
    const uint32_t *halo = fa > 0 ? row + size_t(fa - 1) * perFrame : (prm.prevIn ? prm.prevIn + size_t(r) * P : nullptr);
    uint32_t *last = prm.prevOut ? prm.prevOut + size_t(r) * P : nullptr;
    Moments m;
    long colEnd = 0, unused = 0;
    if (!SLICED) columnFrames(prm, col, unused, colEnd);

    if constexpr (MODE > 0) {
        uint64_t prev[MODE][4];
        Quad next[MODE];
#pragma unroll
        for (int c = 0; c < MODE; ++c) {
            const uint32_t base = (uint32_t(c) * kThreads + t) * 4u;
            Quad h{};
            if (halo) h = loadQuad(halo, base, P, isWide16(halo));
            (void)quantiseQuad(h, prev[c]);                            // (the zeros of a missing predecessor: a = 0, and its F is dropped below)
            next[c] = loadQuad(row + size_t(fa) * perFrame, base, P, isWide16(row + size_t(fa) * perFrame));
        }
        for (long f = fa; f < fb; ++f) {
            Quad cur[MODE];
#pragma unroll
            for (int c = 0; c < MODE; ++c) cur[c] = next[c];
            if (f + 1 < fb) {                                          // the next frame's loads are in flight across this frame's reduction
                const uint32_t *nrow = row + size_t(f + 1) * perFrame;
#pragma unroll
                for (int c = 0; c < MODE; ++c) next[c] = loadQuad(nrow, (uint32_t(c) * kThreads + t) * 4u, P, isWide16(nrow));
            }
            uint64_t F = 0;
            bool nan = false;
#pragma unroll
            for (int c = 0; c < MODE; ++c) {
                const uint32_t base = (uint32_t(c) * kThreads + t) * 4u;
                uint64_t a[4];
                nan |= quantiseQuad(cur[c], a);
                accQuad(m, F, base, a, prev[c]);
                if (last && f + 1 == prm.frames) storeQuad(last, base, P, cur[c]);
            }
            if (f == fa && !halo) F = 0;
            frameReduce(sh, f, F, nan, acc, prm.firstFrame + uint64_t(f));
            if (!SLICED && f + 1 == colEnd) {
                momentsReduce(sh, m, acc);
                if (t == 0) { emitColumn(prm, col, r, acc); acc = Acc{}; }
                ++col;
                columnFrames(prm, col, unused, colEnd);
            }
        }
    } else {
        const bool inLds = P <= kLdsPixels;
        const uint32_t *prevRow = halo;
        for (long f = fa; f < fb; ++f) {
            const uint32_t *crow = row + size_t(f) * perFrame;
            const bool curWide = isWide16(crow), prevWide = prevRow && isWide16(prevRow);
            uint64_t F = 0;
            bool nan = false;
            for (uint32_t base = t * 4u; base < P; base += kPass) {
                const Quad cur = loadQuad(crow, base, P, curWide);
                Quad before{};
                if (prevRow) before = loadQuad(prevRow, base, P, prevWide);
                uint64_t a[4], prev[4];
                (void)quantiseQuad(before, prev);
                nan |= quantiseQuad(cur, a);
                accQuad(m, F, base, a, prev);
                if (inLds) *reinterpret_cast<uint4 *>(ldsRow + base) = make_uint4(cur.w[0], cur.w[1], cur.w[2], cur.w[3]);   // this thread's own words
                if (last && f + 1 == prm.frames) storeQuad(last, base, P, cur);
            }
            if (!prevRow) F = 0;
            prevRow = inLds ? ldsRow : crow;
            frameReduce(sh, f, F, nan, acc, prm.firstFrame + uint64_t(f));
            if (!SLICED && f + 1 == colEnd) {
                momentsReduce(sh, m, acc);
                if (t == 0) { emitColumn(prm, col, r, acc); acc = Acc{}; }
                ++col;
                columnFrames(prm, col, unused, colEnd);
            }
        }
    }
    if (SLICED) momentsReduce(sh, m, acc);
}

template <int MODE>
__global__ void __launch_bounds__(kThreads)
overviewFluxColumnsKernel(const FluxParams prm)
{
    __shared__ Shared sh;
    __shared__ __attribute__((aligned(16))) uint32_t ldsRow[MODE == 0 ? kLdsPixels : 4];
    const uint32_t r = blockIdx.x % prm.R;
    const long col = long(blockIdx.x / prm.R) * long(prm.G);
    const long colStop = col + long(prm.G) < prm.columns ? col + long(prm.G) : prm.columns;
    long fa, fb, unused;
    columnFrames(prm, col, fa, unused);
    columnFrames(prm, colStop - 1, unused, fb);
    Acc acc;
    if (fa >= fb) {                                                    // no frame arrives: the flush of the carried column
        if (threadIdx.x == 0) emitColumn(prm, col, r, acc);
        return;
    }
    walkFrames<MODE, false>(prm, sh, ldsRow, r, fa, fb, col, acc);
}

// slice blockIdx.y of every column's frames (an empty slice -- more slices than frames -- leaves an empty record)
template <int MODE>
__global__ void __launch_bounds__(kThreads)
overviewFluxSliceKernel(const FluxParams prm)
{
    __shared__ Shared sh;
    __shared__ __attribute__((aligned(16))) uint32_t ldsRow[MODE == 0 ? kLdsPixels : 4];
    const uint32_t r = blockIdx.x % prm.R;
    const long col = long(blockIdx.x / prm.R);
    long a, b;
    columnFrames(prm, col, a, b);
    const long n = b > a ? b - a : 0, per = (n + long(prm.slices) - 1) / long(prm.slices);
    const long sa = a + long(blockIdx.y) * per < b ? a + long(blockIdx.y) * per : b, sb = sa + per < b ? sa + per : b;
    Acc acc;
    if (sa < sb) walkFrames<MODE, true>(prm, sh, ldsRow, r, sa, sb, col, acc);
    if (threadIdx.x == 0) accRecord(acc, prm.partial[(size_t(blockIdx.y) * size_t(prm.columns) + size_t(col)) * prm.R + r]);
}

// one thread per (column, row): the fold over the slices, the carry, the record
__global__ void __launch_bounds__(kThreads)
overviewFluxEmitKernel(const FluxParams prm)
{
    const size_t j = size_t(blockIdx.x) * kThreads + threadIdx.x;
    if (j >= size_t(prm.columns) * prm.R) return;
    Acc acc;
    for (uint32_t s = 0; s < prm.slices; ++s) accFold(acc, prm.partial[size_t(s) * size_t(prm.columns) * prm.R + j]);
    emitColumn(prm, long(j / prm.R), uint32_t(j % prm.R), acc);
}

void launchColumns(uint32_t P, dim3 grid, hipStream_t stream, const FluxParams &prm)
{
    if (P <= kPass) hipLaunchKernelGGL(overviewFluxColumnsKernel<1>, grid, dim3(kThreads), 0, stream, prm);
    else if (P <= kRegPasses * kPass) hipLaunchKernelGGL(overviewFluxColumnsKernel<2>, grid, dim3(kThreads), 0, stream, prm);
    else hipLaunchKernelGGL(overviewFluxColumnsKernel<0>, grid, dim3(kThreads), 0, stream, prm);
}

void launchSlices(uint32_t P, dim3 grid, hipStream_t stream, const FluxParams &prm)
{
    if (P <= kPass) hipLaunchKernelGGL(overviewFluxSliceKernel<1>, grid, dim3(kThreads), 0, stream, prm);
    else if (P <= kRegPasses * kPass) hipLaunchKernelGGL(overviewFluxSliceKernel<2>, grid, dim3(kThreads), 0, stream, prm);
    else hipLaunchKernelGGL(overviewFluxSliceKernel<0>, grid, dim3(kThreads), 0, stream, prm);
}

// host: the accumulator of sgz_overview_flux_fold, with counts wide enough to see them pass 2^32 - 1
struct HostAcc { Acc acc; uint64_t count = 0, nans = 0; };

}  // namespace

namespace sgz {

// sgz_stage_overview_flux behind its argument checks.  d_mapped [frames][R][P] float.  d_prev [R][P] or null: read iff prevValid (the frame before
// frame 0), written with the call's last frame when frames > 0
sgz_status runOverviewFluxColumns(Plan &p, const float *d_mapped, size_t frames, uint32_t k, uint32_t held, int flush, uint64_t firstFrame, uint32_t slices,
                                  float *d_prev, bool prevValid, sgz_overview_flux_record *d_carry, sgz_overview_flux_record *d_flux, hipStream_t stream)
{
    const OverviewStep sh = overviewStepShape(k, held, frames, flush);
    const uint64_t columns = sh.columns;
    if (!sh.launch) return SGZ_OK;
    const uint32_t R = p.C * uint32_t(p.sides);
    if (columns == 0 || R == 0) return SGZ_OK;
    if (columns > 0x7fffffffull / R || frames > size_t(0x7fffffffffffffffll)) return fail(SGZ_EINVAL, "too many columns for one launch");
    FluxParams prm{};
    prm.mapped = reinterpret_cast<const uint32_t *>(d_mapped);
    prm.frames = long(frames); prm.columns = long(columns); prm.closed = long(sh.closed);
    prm.k = k; prm.held = held; prm.P = p.P; prm.R = R;
    prm.firstFrame = firstFrame;
    prm.prevIn = prevValid ? reinterpret_cast<const uint32_t *>(d_prev) : nullptr;
    prm.prevOut = frames ? reinterpret_cast<uint32_t *>(d_prev) : nullptr;
    prm.carryOut = d_carry; prm.flux = d_flux;
    // a slice pays a halo fetch, so there are none by default unless each keeps kSliceFrames frames
    prm.slices = slices ? slices : std::max(1u, overviewAutoSlices(long(columns), R, k / kSliceFrames, frames, int(kWantGroups / 2)));
    // runs of whole columns: kRunFrames frames at the most, fewer while that leaves fewer than kWantGroups workgroups
    prm.G = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(kRunFrames / k, columns * R / kWantGroups)));
    const uint64_t groups = (columns + prm.G - 1) / prm.G;
    if (sgz_status st = snapshotCarry<Record>(p, kOvFlux, sh, held, d_carry, R, stream, &prm.carryIn); st != SGZ_OK) return st;
    if (prm.prevIn && prm.prevOut && (prm.slices > 1 || groups > 1)) {
        // the same snapshot for the previous frame, where frame 0's workgroup is not the last frame's (in one workgroup a pixel is read and written by one thread)
        if (sgz_status st = ensureCap(&p.d_ovfPrevCopy, &p.ovfPrevCopyCap, size_t(R) * p.P); st != SGZ_OK) return st;
        SGZ_HIP(hipMemcpyAsync(p.d_ovfPrevCopy, d_prev, size_t(R) * p.P * sizeof(float), hipMemcpyDeviceToDevice, stream));
        prm.prevIn = reinterpret_cast<const uint32_t *>(p.d_ovfPrevCopy);
    }
    if (prm.slices <= 1) {
        launchColumns(p.P, dim3(unsigned(groups * R)), stream, prm);
        SGZ_HIP(hipGetLastError());
        return SGZ_OK;
    }
    if (sgz_status st = ensureCap(&p.ov[kOvFlux].d_partial, &p.ov[kOvFlux].partialCap, size_t(prm.slices) * size_t(columns) * R * kRecordFloats<Record>); st != SGZ_OK) return st;
    prm.partial = reinterpret_cast<Record *>(p.ov[kOvFlux].d_partial);
    launchSlices(p.P, dim3(unsigned(columns * R), prm.slices), stream, prm);
    SGZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(overviewFluxEmitKernel, dim3(unsigned((columns * R + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

}  // namespace sgz

struct sgz_plan { Plan impl; };

extern "C" sgz_status sgz_stage_overview_flux(sgz_plan *plan, const float *d_mapped, size_t frames, uint32_t k, uint32_t held, int flush, uint64_t first_frame,
                                              uint32_t slices, float *d_prev, sgz_overview_flux_record *d_carry, sgz_overview_flux_record *d_flux, void *stream)
{
    if (!plan || !d_mapped) return fail(SGZ_EINVAL, "null argument");
    if (sgz_status st = checkOverviewStep(k, held, frames); st != SGZ_OK) return st;
    if (slices > kOvMaxSlices) return fail(SGZ_EINVAL, "sgz_stage_overview_flux: slices 0 (automatic) or 1 .. 64");
    const OverviewStep sh = overviewStepShape(k, held, frames, flush);
    if (!d_flux && sh.closed) return fail(SGZ_EINVAL, "sgz_stage_overview_flux: d_flux receives the columns that close");
    if (!d_carry && (held || sh.open)) return fail(SGZ_EINVAL, "sgz_stage_overview_flux: d_carry is read (held > 0) or written (frames stay open)");
    if ((reinterpret_cast<uintptr_t>(d_mapped) & 3u) || (reinterpret_cast<uintptr_t>(d_prev) & 3u) || (reinterpret_cast<uintptr_t>(d_carry) & 7u) ||
        (reinterpret_cast<uintptr_t>(d_flux) & 7u))
        return fail(SGZ_EINVAL, "sgz_stage_overview_flux: d_mapped and d_prev aligned to 4 bytes, d_carry and d_flux to 8");
    if (!sh.launch) return SGZ_OK;
    return runOverviewFluxColumns(plan->impl, d_mapped, frames, k, held, flush, first_frame, slices, d_prev, d_prev != nullptr, d_carry, d_flux,
                                  reinterpret_cast<hipStream_t>(stream));
}

// ---- the host helpers (no GPU) ----------------------------------------------------------------------------------------------------------------
extern "C" sgz_status sgz_overview_flux_quantise(const float *x, size_t n, uint64_t *a)
{
    if ((!x || !a) && n) return fail(SGZ_EINVAL, "sgz_overview_flux_quantise: null argument");
    for (size_t i = 0; i < n; ++i) a[i] = x[i] != x[i] ? 0u : fluxQuantise(x[i]);
    return SGZ_OK;
}

extern "C" sgz_status sgz_overview_flux_fold(const sgz_overview_flux_record *in, size_t n, size_t width, size_t x0, size_t x1, uint32_t out_columns,
                                             sgz_overview_flux_record *out)
{
    return foldKeptColumns<HostAcc>(
        {"sgz_overview_flux_fold: null argument", "sgz_overview_flux_fold: width >= 1 records per column",
         "sgz_overview_flux_fold: a folded column counts more than 2^32 - 1 frames"},
        in, n, width, x0, x1, out_columns, out,
        [](HostAcc &h, const Record &r) {
            h.acc.amp += wide128(r.amp); h.acc.m1 += wide128(r.mom1); h.acc.m2 += wide128(r.mom2); h.acc.flux += wide128(r.flux);
            accPeak(h.acc, r.flux_max, r.flux_at);
            h.count += r.count; h.nans += r.nans;
        },
        [](const HostAcc &h) { return h.count <= 0xffffffffull && h.nans <= 0xffffffffull; },
        [](const HostAcc &h, Record &o) {
            Acc acc = h.acc;
            acc.count = uint32_t(h.count); acc.nans = uint32_t(h.nans);
            accRecord(acc, o);
        });
}

extern "C" sgz_status sgz_overview_flux_readout(const sgz_overview_flux_record *in, size_t count, uint32_t pixels, double *mean_amplitude, double *centroid,
                                                double *spread, double *mean_flux, double *relative_flux)
{
    if (!in && count) return fail(SGZ_EINVAL, "sgz_overview_flux_readout: null records");
    if (!mean_amplitude && !centroid && !spread && !mean_flux && !relative_flux)
        return fail(SGZ_EINVAL, "sgz_overview_flux_readout: the mean amplitudes, the centroids, the spreads, the mean fluxes, the relative fluxes or any of them");
    if (mean_amplitude && pixels == 0) return fail(SGZ_EINVAL, "sgz_overview_flux_readout: the mean amplitude is per pixel: pixels >= 1");
    const double none = std::nan("");
    for (size_t i = 0; i < count; ++i) {
        const Record &r = in[i];
        const double amp = wide(r.amp), frames = double(r.count);
        const bool some = (r.amp[0] | r.amp[1]) != 0 && r.count != 0;
        if (mean_amplitude) mean_amplitude[i] = r.count ? amp / (frames * double(pixels)) * kAmpScale : none;
        const double c = some ? wide(r.mom1) / amp : none;
        if (centroid) centroid[i] = c;
        if (spread) {
            double v = none;
            if (some) { const double second = wide(r.mom2) / amp, square = c * c; v = std::sqrt(std::fmax(0.0, second - square)); }
            spread[i] = v;
        }
        if (mean_flux) mean_flux[i] = r.count ? wide(r.flux) / frames * kAmpScale : none;
        if (relative_flux) relative_flux[i] = some ? wide(r.flux) / amp : none;
    }
    return SGZ_OK;
}

extern "C" sgz_status sgz_overview_flux_hz(const sgz_plan *plan, const double *pixel, size_t n, double *hz)
{
    if (!plan || ((!pixel || !hz) && n)) return fail(SGZ_EINVAL, "sgz_overview_flux_hz: null argument");
    const std::vector<float> &f = plan->impl.mapped;
    const size_t P = f.size();
    if (P == 0) return fail(SGZ_EINVAL, "sgz_overview_flux_hz: the plan has no axis");
    for (size_t j = 0; j < n; ++j) {
        const double x = pixel[j];
        if (x != x) { hz[j] = x; continue; }
        if (P == 1 || x <= 0.0) { hz[j] = double(f[0]); continue; }
        if (x >= double(P - 1)) { hz[j] = double(f[P - 1]); continue; }
        const size_t i = size_t(x);                                    // floor: 0 <= x < P - 1
        const double frac = x - double(i), lo = double(f[i]), step = double(f[i + 1]) - lo;
        hz[j] = lo + frac * step;
    }
    return SGZ_OK;
}
