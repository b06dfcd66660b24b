// scope_stream.hip -- the Oscilloscope's real-time handle (sgz_scope_*): the whole audio-thread state machine lives in HBM and
// runs as ONE kernel launch per audio block, so sgz_scope_push only stages the block and enqueues -- no device -> host round trip
// for the trigger list, no host copy of the rings.  gfx950 only.
//
// Replaces, per onStreamAudio callback (Source/Oscilloscope/Oscilloscope.h:293 -> StreamState::audioEntryPoint,
// OscilloscopeDSP.inl:401-424):
//   TriggeringProcessor::update                          StreamPreprocessing.h:55-76
//   preAnalyseAudio -> ZeroCrossingProcessor::process    OscilloscopeDSP.inl:311-399, StreamPreprocessing.h:315-349
//   TriggeringProcessor::processMutating                 StreamPreprocessing.h:79-206  (trigger -> window selection)
//   ChannelData::swapBuffers                             ChannelData.h:147-161         (back -> front ring)
//   StreamState::audioProcessing: RMS envelope + writes  OscilloscopeDSP.inl:520-585, :676-697
// and on the render thread: Oscilloscope::runPeakFilter (OscilloscopeDSP.inl:713-886, every OscChannels mode) and drawWavePlot's
// Linear and Lanczos branches (OscilloscopeRendering.cpp:551-649, :707-741, :790-891) -> (x, y, z) + RGBA8 per vertex.
//
// Layout in HBM.  front: [channels][size] rings, size = ceil(window + 1) (ChannelData::resizeAudioStorage), one write cursor for
// all channels -- exactly the memory the reference's CLIFOStream proxy views expose (begin() / cursorPosition()), so memory-order
// semantics (runPeakFilter's dropped tail) carry over.  back: [channels][backCap] indexed by ABSOLUTE sample number mod backCap
// (backCap = power of two >= size): "cursor - bufferedSamples" of the reference is absolute index  written - bufferedSamples.
// A swap's source range may straddle the history and the block being ingested; the copy reads either.
//
// The block kernel (one 1024-thread workgroup -- a block is a few thousand samples):
//   A  trigger detection as two prefix-max scans + ordered compaction (the automaton's closed form, scope_vector.hip K10) into
//      the device-resident peaks queue;
//   B  thread 0 replays update() + processMutating's integer automaton (same uint64 / double conversions as the reference) and
//      emits the list of swaps (source sample, length) and the extent of the last audioProcessing call;
//   C  all threads execute the swaps in order into the front rings;
//   D  the block is appended to the back rings;
//   E  RMS envelope: one lane per recurrence, sequential fp32 (rounding order is the reference's).
//   F  (colour_by_frequency) the per-sample colours of audioProcessing (:445-647) for the whole block, before C so that swaps can
//      take them along: F1/F2 the 3-band Linkwitz-Riley tree as two passes of cascaded biquads (one lane per channel and branch,
//      sequential in time), F3 the twelve band-energy smoothers of a channel pair (left / right / mid / side x 3 bands, one lane
//      each), F4 accumulateColour for every (sample, signal) in parallel.  Colour rings sit beside the audio rings (colourData /
//      auxColourData, ChannelData.h:58-66) and move with them (swapBuffers, ChannelData.h:155-159).
//
// Spectral triggering (sgz_scope_analyse -> scopeSpectralKernel, OscilloscopeDSP.inl:62-308): audio goes straight into the front ring
// like TriggeringMode::None; once per rendered frame one workgroup transforms the newest 8192 samples in LDS (fp64), picks the
// fundamental, runs the median of 8 and the Goertzel phase, and leaves cycleSamples / sampleOffset for the vertex kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>

#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "rt_common.hpp"
#include "scope_ring.hpp"

#pragma clang fp contract(off)

using namespace sgz;

namespace sgz {
// scope_vector.hip: Lanczos / linear vertex kernels on a ring whose cursor lives in device memory
bool launchScopeLanczosPair(const sgz_scope_view &view, uint32_t triggerMode, uint32_t interpolation, const float *const ringA[2],
                            const float *const ringB[2], const uint32_t evalMode[2], uint32_t size, uint32_t cap, const uint32_t *d_cursor,
                            double cycleSamples, double sampleOffset, long long transport, const uint32_t key[2], const uint32_t *const colRing[2],
                            float *const d_xyz[2], uint32_t *const d_rgba[2], size_t capacity, size_t *points, hipStream_t stream, hipError_t *err);
hipError_t launchScopeVertices(const sgz_scope_view &view, uint32_t triggerMode, uint32_t interpolation, const float *ringA,
                               const float *ringB, uint32_t evalMode, uint32_t size, uint32_t cap, const uint32_t *d_cursor,
                               double cycleSamples, double sampleOffset, long long transport, uint32_t rgba, const uint32_t *colRing, float *d_xyz,
                               uint32_t *d_rgba, size_t capacity, size_t *points, hipStream_t stream);
size_t scopeVertexCount(const sgz_scope_view &view, uint32_t interpolation, uint32_t triggerMode, double cycleSamples);
// scope_dense.hip: the per-column min / max reduction of the Linear strip
size_t scopeDenseScratchBytes(size_t n, uint32_t columns);
hipError_t launchScopeDense(const float *ringA, const float *ringB, uint32_t evalMode, uint32_t size, uint32_t cap, const uint32_t *d_cursor,
                            size_t n, long start0, uint32_t columns, uint32_t key, const uint32_t *colRing, float *d_xyz, uint32_t *d_rgba,
                            void *scratch, size_t *points, hipStream_t stream);
}

namespace {

constexpr uint32_t kPeakCap = 1u << 16;       // pending triggers (std::queue<std::uint64_t> peaks)
constexpr uint32_t kMaxSwaps = kPeakCap + 8;  // one swap pops one trigger
constexpr uint32_t kMaxCh = 64;

struct Swap { unsigned long long src; unsigned int len; unsigned int pad; };

struct ScopeDev {
    // TriggeringProcessor (StreamPreprocessing.h:210-226)
    double threshold, windowSize, state, hysteresis;
    int windowChanged, isPeakHold, isWorkingOnPeak, pad0;
    unsigned long long crossOrigin, oldPeak, currentPeak, bufferedSamples, frontOrigin, steadyClock;
    unsigned long long playhead;              // ctx.getPlayhead().getSteadyClock(): samples delivered so far
    unsigned int qHead, qCount;               // peaks queue (ring of kPeakCap)
    // rings
    unsigned long long written;               // samples ever appended to the back rings
    unsigned int frontCursor, pad1;
    // envelope
    float envelope[kMaxCh];                   // filterStates.channels[c].envelope
    double envelopeGain;                      // StreamState::envelopeGain
    double autoGain;                          // state.autoGain after runPeakFilter
    unsigned long long swaps, droppedPeaks;
};

// frequency colouring state: filterStates.channels[c].{network, smoothFilters, auxSmoothFilter} (ChannelData.h:68-80)
struct ColourDev {
    float z[kMaxCh][8][2];                    // biquad states: lp1 a, b; hp1 a, b; lp2 a, b; hp2 a, b (transposed direct form II)
    float smooth[kMaxCh][3], aux[kMaxCh][3];
};
struct ColourParams {
    ColourDev *st;
    float lp1[5], hp1[5], lp2[5], hp2[5];     // b0 b1 b2 a1 a2 (Crossover::Coefficients::design, UNVERIFIED vs cpl: see oracle/scope_spectral.c)
    float pole, blend;                        // channelData.smoothFilterPole; 1 - frequencyColouringBlend
    float band[3][3];                         // low / mid / high colour
    float *bands;                             // scratch [channels][4][maxBlock]: low, mid, high, rest
    float *sm;                                // scratch [channels / 2 * 12][maxBlock]: smoothed band energies
    uint32_t *block;                          // [2 channels][maxBlock] colours of the block: colourData planes, then auxColourData
    uint32_t *front, *back;                   // [2 channels][size] / [2 channels][backCap]
    uint32_t maxBlock;
    uint32_t keys[kMaxCh];                    // defaultKey per channel, RGBA8
};

struct PeakParams {           // Oscilloscope::runPeakFilter (scopePeakBody below)
    ScopeDev *st;
    const float *front; uint32_t size, channels, mode, lanes;
    double coeff;
    uint32_t len;       // Spectral: the reference's ring of the moment (the newest len samples, taken as memory order); else 0
};

struct IngestParams {
    ScopeDev *st;
    unsigned long long *peaks;                // [kPeakCap]
    Swap *swapList;                           // [kMaxSwaps]
    BatchArgs in;                             // the staged blocks and sgz_scope_set_mix's routing (rt_common.hpp)
    float *front; uint32_t size;              // [channels][size]
    float *back; uint32_t backCap;            // [channels][backCap], power of two
    uint32_t triggerMode, oscMode, envMode;
    uint32_t trigSeparate, trigPair;
    float envelopeCoeff;
    uint32_t colours;                         // colour_by_frequency
    uint32_t doPeak; PeakParams peak;         // the render thread's peak filter behind the batch's last block (sgz_scope_peak_filter found a batch waiting: one launch)
};

// A lane that walks a block sequentially (a recurrence) must not wait a memory round trip per sample: the samples come in batches of
// 16 independent loads, the next batch in flight while the current one is consumed.  load(i) -> float, step(i, v).
template <typename Load, typename Step>
__device__ __forceinline__ void walkSequential(uint32_t n, Load load, Step step)
{
    constexpr uint32_t B = 16;
    const uint32_t full = n & ~(B - 1);                      // whole batches: straight-line code, no per-sample predicate
    if (full) {
        float cur[B], nxt[B];
#pragma unroll
        for (uint32_t j = 0; j < B; ++j) cur[j] = load(j);
        for (uint32_t i0 = 0; i0 < full; i0 += B) {
            const uint32_t in = i0 + B < full ? i0 + B : i0;  // (the last batch reloads itself: uniform code)
#pragma unroll
            for (uint32_t j = 0; j < B; ++j) nxt[j] = load(in + j);
#pragma unroll
            for (uint32_t j = 0; j < B; ++j) step(i0 + j, cur[j]);
#pragma unroll
            for (uint32_t j = 0; j < B; ++j) cur[j] = nxt[j];
        }
    }
    for (uint32_t i = full; i < n; ++i) step(i, load(i));     // < 16 samples
}

__device__ __forceinline__ float biquadStep(const float *c, float &z0, float &z1, float x)
{
    const float y = c[0] * x + z0;
    z0 = (c[1] * x - c[3] * y) + z1;
    z1 = c[2] * x - c[4] * y;
    return y;
}
// static_cast<uint8_t>(float) as the x86 build behaves (see oracle/scope_spectral.c to_u8)
__device__ __forceinline__ uint32_t toU8(float v) { return (!(v > -1.0f) || !(v < 256.0f)) ? 0u : uint32_t(int(v)) & 255u; }
// accumulateColour (OscilloscopeDSP.inl:472-497) + PixelType::lerp(key, blend)
__device__ __forceinline__ uint32_t accumulateColour(const float st[3], const float band[3][3], uint32_t key, float blend)
{
    float red = 0.f, green = 0.f, blue = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        red += st[i] * band[i][0];
        green += st[i] * band[i][1];
        blue += st[i] * band[i][2];
    }
    const float invMax = 255.0f / fmaxf(red, fmaxf(blue, green));
    const uint32_t ret[4] = {toU8(red * invMax), toU8(green * invMax), toU8(blue * invMax), 255u};
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float a = float(ret[k]), b = float((key >> (8 * k)) & 255u);
        out |= toU8(a + (b - a) * blend) << (8 * k);
    }
    return out;
}

// two exclusive prefix-max scans at once on 32-bit values (the zero-crossing phase's "last arm" / "last threshold crossing": sample
// indices of one block and small negative sentinels) -- one pass of shuffles, one pair of barriers.  (As two 64-bit scans they were
// 3.7 us of the phase's 6.6: every 64-bit shuffle is two permutes, every scan two barriers of sixteen waves.)
__device__ __forceinline__ void blockExclusiveMax2(int va, int initA, int vb, int initB, int *lds /*[32]*/, int &inA, int &inB, int &totA, int &totB)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    int ia = va, ib = vb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ua = __shfl_up(ia, o), ub = __shfl_up(ib, o);
        if (lane >= o) { ia = ua > ia ? ua : ia; ib = ub > ib ? ub : ib; }
    }
    if (lane == 63) { lds[wave] = ia; lds[16 + wave] = ib; }
    __syncthreads();
    int baseA = initA, baseB = initB, ta = initA, tb = initB;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int pa = lds[w], pb = lds[16 + w];
        if (w < wave) { baseA = pa > baseA ? pa : baseA; baseB = pb > baseB ? pb : baseB; }
        if (w < waves) { ta = pa > ta ? pa : ta; tb = pb > tb ? pb : tb; }
    }
    int prevA = __shfl_up(ia, 1), prevB = __shfl_up(ib, 1);
    if (lane == 0) { prevA = INT_MIN; prevB = INT_MIN; }
    __syncthreads();
    totA = ta; totB = tb;
    inA = prevA > baseA ? prevA : baseA;
    inB = prevB > baseB ? prevB : baseB;
}
__device__ __forceinline__ unsigned int blockExclusiveSum(unsigned int v, unsigned int *lds, unsigned int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    unsigned int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned int base = 0, tot = 0;
    for (int w = 0; w < waves; ++w) { if (w < wave) base += lds[w]; tot += lds[w]; }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// inclusive prefix sum over the workgroup (all threads call it); lds: 16 words of T
template <typename T>
__device__ __forceinline__ T blockInclusiveSum(T v, T *lds, T *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (int w = 0; w < waves; ++w) { if (w < wave) base += lds[w]; tot += lds[w]; }
    __syncthreads();
    *total = tot;
    return base + inc;
}

__device__ __forceinline__ double trigSample(uint32_t mode, const float *a, const float *b, uint32_t i)
{
    if (mode == SGZ_OSC_MID) return double(0.5f * (a[i] + b[i]));          // OscilloscopeDSP.inl:371-376
    if (mode == SGZ_OSC_SIDE) return double(0.5f * (a[i] - b[i]));         // :377-382
    return double(a[i]);
}

// The detectors' source in a block of n samples: the planes (a, b) trigSample reads and the mode it reads them in (MidSide triggers
// on the Mid of its pair)
__device__ __forceinline__ uint32_t triggerPlanes(const IngestParams &prm, const float *blk, uint32_t n, const float *&a, const float *&b)
{
    uint32_t mode = prm.oscMode, pair = prm.trigPair;
    if (mode == SGZ_OSC_MIDSIDE) { mode = SGZ_OSC_MID; pair = prm.trigSeparate & ~1u; }             // :340-352
    if (mode == SGZ_OSC_RIGHT) a = b = blk + size_t(pair + 1) * n;
    else if (mode == SGZ_OSC_LEFT) a = b = blk + size_t(pair) * n;
    else if (mode == SGZ_OSC_SEPARATE) a = b = blk + size_t(prm.trigSeparate) * n;
    else { a = blk + size_t(pair) * n; b = a + n; }
    return mode;
}

__device__ __forceinline__ unsigned long long minU64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

#ifdef SGZ_DEBUG
__device__ unsigned long long g_ingestClk[8];
#define ICLK(k) do { if (threadIdx.x == 0) g_ingestClk[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define ICLK(k) do { } while (0)
#endif

constexpr unsigned int kStage = 64;             // triggers / swaps of a callback staged in LDS
constexpr unsigned int kFlat = 1024;            // swaps of a callback the one-pass copy takes (one per thread; more: one after the other)

// The planes that move together through the rings: the audio channels, or (colour_by_frequency) the colour planes
template <typename T>
struct Planes {
    const T *block; uint32_t pitch;             // the callback's samples: plane c at block + c * pitch
    T *back, *front;                            // [count][backCap], [count][size]
    uint32_t count;
};

// sample `abs` (absolute index: the block from written0 on, the back ring before it) of every plane -> slot d of the front ring
template <typename T>
__device__ __forceinline__ void copyToFront(const Planes<T> &p, unsigned long long abs, unsigned long long written0, uint32_t d, uint32_t size,
                                            uint32_t backCap)
{
    const bool fromBlock = abs >= written0;
    const uint32_t bi = uint32_t(abs - written0), ri = uint32_t(abs & (backCap - 1));
    for (uint32_t c = 0; c < p.count; ++c)
        p.front[size_t(c) * size + d] = fromBlock ? p.block[size_t(c) * p.pitch + bi] : p.back[size_t(c) * backCap + ri];
}

// the block (its newest backCap samples) -> the back ring, at absolute index mod backCap
template <typename T>
__device__ __forceinline__ void copyToBack(const Planes<T> &p, uint32_t n, unsigned long long written0, uint32_t backCap)
{
    const uint32_t keep = n > backCap ? backCap : n, first = n - keep;
    for (uint32_t e = threadIdx.x; e < keep * p.count; e += blockDim.x) {
        const uint32_t c = e / keep, i = first + (e - c * keep);
        p.back[size_t(c) * backCap + uint32_t((written0 + i) & (backCap - 1))] = p.block[size_t(c) * p.pitch + i];
    }
}

// What a swap of len samples leaves in the front ring when `later` more samples follow it in the same block: the ring holds `size`
// samples, so only the last `size` of a longer run are written, and of those the first ones that the later swaps overwrite are dead.
// Returns the count m of surviving samples; they start at sample `first` of the swap.  (A noisy signal fires a dozen triggers per
// block, each swap copies a window's worth, and only the last one or two are still there when the block is done -- the others just
// move the cursor.)
__device__ __forceinline__ uint32_t survivingRange(uint32_t len, unsigned long long later, uint32_t size, uint32_t &first)
{
    const uint32_t skip = len > size ? len - size : 0u;
    const uint32_t m0 = len - skip;
    const unsigned long long room = later >= size ? 0ull : size - later;       // newest samples of this swap that stay visible
    const uint32_t dead = m0 > room ? uint32_t(m0 - room) : 0u;
    first = skip + dead;
    return m0 - dead;
}

// ---- update(), StreamPreprocessing.h:55-76 (thread 0; the queue edits must precede phase A's appends)
__device__ __forceinline__ void updatePhase(ScopeDev *st, const unsigned long long *peaks, unsigned long long playhead)
{
    st->steadyClock = playhead;
    if (st->windowChanged) {
        st->windowChanged = 0;
        if (st->isWorkingOnPeak && st->qCount) { st->qHead = (st->qHead + 1) % kPeakCap; st->qCount--; }
        while (st->qCount && peaks[st->qHead] < playhead) { st->qHead = (st->qHead + 1) % kPeakCap; st->qCount--; }
        st->bufferedSamples = st->currentPeak = st->oldPeak = 0;
        st->frontOrigin = playhead;
        st->isWorkingOnPeak = 0;
    }
}

// ---- A': PeakHoldProcessor over the block (StreamPreprocessing.h:270-313): an envelope follower whose every step depends on the
// last one's branch -- one lane walks the block (a few microseconds per 512 samples; the triggers it finds are rare)
__device__ __forceinline__ void peakHoldPhase(const IngestParams &prm, ScopeDev *st, const float *blk, uint32_t n, unsigned long long playhead)
{
    const float *a, *b;
    const uint32_t mode = triggerPlanes(prm, blk, n, a, b);
    double state = st->state;
    const double thr2 = st->threshold * st->threshold, hysteresis = st->hysteresis;
    int holding = st->isPeakHold;
    unsigned int qc = st->qCount;
    const unsigned int q0 = st->qHead;
    unsigned long long dropped = 0;
    for (uint32_t i = 0; i < n; ++i) {
        double sample = trigSample(mode, a, b, i);
        sample *= sample;
        const double delta = sample - state;
        if (delta < 0) {
            state *= 0.9999;
            state = fmax(thr2, state);
            if (holding) {
                if (qc < kPeakCap) { prm.peaks[(q0 + qc) % kPeakCap] = playhead + (unsigned long long)i - 1ull; ++qc; }
                else ++dropped;
                holding = 0;
            }
        } else {
            if (delta > hysteresis * state) holding = 1;
            state = sample;
        }
    }
    st->state = state; st->isPeakHold = holding; st->qCount = qc; st->droppedPeaks += dropped;
}

// ---- A: ZeroCrossingProcessor (executeSamplingWindows, OscilloscopeDSP.inl:311-385) over the n samples of a run of blocks, the
// whole workgroup: each thread walks a segment three times -- last arm / last threshold crossing (two prefix-max scans give every
// segment the state in front of it), triggers counted (a prefix sum gives each its slot in the queue), triggers written.
//   arm_i = (s_i > 0 && s_{i-1} < 0);  fire_i <=> s_i > threshold && lastArm(i) > lastThr(i-1)
// (virtual indices: an arm inherited from before the run sits at -1, "no arm" at -3, "no threshold crossing yet" at -2).
// load(i, b) -> double: sample i of the run; b is the accessor's cursor (the block sample i is in), kept per thread as it walks forward.
// blockFires null: one callback -- triggers beyond the queue's room are not written and count as dropped.  Otherwise the whole
// batch, all or nothing: per-block counts go to blockFires, and if the queue cannot take every trigger nothing is written and
// false is returned (the queue's count is then left to the callbacks).  Ends in a barrier-free section: the caller syncs.
template <typename Load>
__device__ __forceinline__ bool zeroCrossings(uint32_t n, Load load, ScopeDev *st, unsigned long long *peaks, unsigned long long playhead,
                                              unsigned int *blockFires, int *sScan2, unsigned int *sSum)
{
    const int tid = threadIdx.x, T = blockDim.x;
    const double threshold = st->threshold, prevState = st->state;
    const int armedIn = st->isPeakHold;
    const unsigned long long originIn = st->crossOrigin;
    const uint32_t seg = (n + T - 1) / T;
    const uint32_t i0 = min(n, uint32_t(tid) * seg), i1 = min(n, i0 + seg);
    uint32_t bStart = 0;                                                   // the block of sample i0 - 1 (or of i0)
    const double before = i0 > 0 ? load(i0 - 1, bStart) : prevState;      // sample i0 - 1
    auto walk = [&, i0, i1](auto step) {                                   // step(i, s_i, arm_i, b)
        uint32_t b = bStart;
        double prev = before;
        for (uint32_t i = i0; i < i1; ++i) {
            const double s = load(i, b);
            step(i, s, s > 0 && prev < 0, b);
            prev = s;
        }
    };
    int segArm = INT_MIN, segThr = INT_MIN;                               // (sample indices < 2^31; "nothing yet" below every sentinel)
    walk([&](uint32_t i, double s, bool arm, uint32_t) { if (arm) segArm = int(i); if (s > threshold) segThr = int(i); });
    int totArm, totThr, inArm, inThr;
    blockExclusiveMax2(segArm, armedIn ? -1 : -3, segThr, -2, sScan2, inArm, inThr, totArm, totThr);
    auto triggers = [&](auto fire) {                                       // fire(lastArm, b) for each trigger of the segment
        int la = inArm, lt = inThr;
        walk([&](uint32_t i, double s, bool arm, uint32_t b) {
            if (arm) la = int(i);
            if (s > threshold) { if (la > lt) fire(la, b); lt = int(i); }
        });
    };
    unsigned int fires = 0;
    triggers([&](int, uint32_t b) { ++fires; if (blockFires) atomicAdd(&blockFires[b], 1u); });
    unsigned int totalFires;
    unsigned int pos = blockExclusiveSum(fires, sSum, &totalFires);
    const unsigned int q0 = st->qHead, qc0 = st->qCount;
    if (blockFires && qc0 + totalFires > kPeakCap) return false;          // (uniform)
    triggers([&](int la, uint32_t) {
        if (qc0 + pos < kPeakCap) peaks[(q0 + qc0 + pos) % kPeakCap] = (la == -1) ? originIn : playhead + (unsigned long long)la;
        ++pos;
    });
    __syncthreads();
    if (tid == 0) {
        if (!blockFires) {
            const unsigned int room = kPeakCap - qc0;
            st->qCount = qc0 + (totalFires < room ? totalFires : room);
            if (totalFires > room) st->droppedPeaks += totalFires - room;
        }
        st->isPeakHold = totArm > totThr ? 1 : 0;
        if (totArm >= 0) st->crossOrigin = playhead + (unsigned long long)totArm;
        uint32_t b = 0;
        st->state = n ? load(n - 1, b) : prevState;
    }
    return true;
}

// What phase B hands on to C and E: the callback's swap count and the extent of its last audioProcessing call
struct SwapPlan { unsigned int numSwaps, lastStart, lastLen; };

// ---- B: processMutating's automaton (StreamPreprocessing.h:79-206) over a callback of n samples -> the swap list: the first kStage
// swaps in sSwaps, the rest in swapList.  Wave 0, every lane the same scalar walk (lane 0 stores); the 64-trigger rounds use all of
// them.  The head of the trigger queue is staged in sPeaks: the automaton walks without memory round trips (a block holds a handful
// of triggers).
__device__ __forceinline__ void processMutating(const IngestParams &prm, ScopeDev *st, uint32_t n, const unsigned long long *sPeaks,
                                                Swap *sSwaps, SwapPlan &plan)
{
    const unsigned int lane = threadIdx.x;
    const bool lane0 = lane == 0;
    const unsigned int qHeadIn = st->qHead;
    auto peakAt = [&](unsigned int q) {
        const unsigned int k = (q + kPeakCap - qHeadIn) % kPeakCap;
        return k < kStage ? sPeaks[k] : prm.peaks[q];
    };
    auto storeSwap = [&](unsigned int k, unsigned long long src, unsigned int len) {     // swap k of the callback, if the list has room
        if (k < kMaxSwaps) {
            const Swap sw{src, len};
            if (k < kStage) sSwaps[k] = sw; else prm.swapList[k] = sw;   // (two stores: a selected reference is a flat one)
        }
    };
    unsigned int numSwaps = 0, lastStart = 0, lastLen = n;
    const unsigned long long written0 = st->written;
    unsigned long long bufferedSamples = st->bufferedSamples, frontOrigin = st->frontOrigin, steadyClock = st->steadyClock;
    unsigned long long oldPeak = st->oldPeak, currentPeak = st->currentPeak;
    unsigned int qHead = st->qHead, qCount = st->qCount;
    int isWorkingOnPeak = st->isWorkingOnPeak;
    unsigned int swapsDone = 0;
    unsigned long long numSamples = n, consumed = 0;
    if (frontOrigin + bufferedSamples < steadyClock) { frontOrigin = steadyClock; bufferedSamples = 0; }   // :81-85
    const double ceilingSize = ceil(st->windowSize);
    const double halfSize = ceilingSize / 2;
    const unsigned long long bufferedCap = (unsigned long long)(ceilingSize + 1);                      // :101
    // (for an integer d >= 0:  double(d) < halfSize  <=>  d < ceil(halfSize))
    const unsigned long long halfCeil = (unsigned long long)ceil(halfSize);
    auto processIntoBackBuffer = [&](unsigned long long samples) {                                     // :90-105
        lastStart = (unsigned int)consumed; lastLen = (unsigned int)samples;
        consumed += samples;
        numSamples -= samples;
        const unsigned long long oldSamples = bufferedSamples;
        steadyClock += samples;
        bufferedSamples += samples;
        bufferedSamples = minU64(bufferedSamples, bufferedCap);
        frontOrigin += (oldSamples + samples) - bufferedSamples;
    };
    auto pickUpNextPeak = [&]() {                                                                      // :120-141
        const unsigned long long nextPeak = peakAt(qHead);
        isWorkingOnPeak = 1;
        if (nextPeak >= steadyClock) {
            const unsigned long long deltaToPeak = nextPeak - steadyClock;
            processIntoBackBuffer(minU64(numSamples, (unsigned long long)(double(deltaToPeak) + halfSize)));
        }
        currentPeak = nextPeak;
    };
    // swapBuffers(cappedSize, -bufferedSamples): source = the oldest buffered sample onwards; the trigger is done (:191-205).  Both
    // callers hold a queued trigger and cappedSize <= bufferedSamples.
    auto swapBuffers = [&](unsigned long long cappedSize) {
        if (lane0) storeSwap(numSwaps, (written0 + consumed) - bufferedSamples, (unsigned int)cappedSize);
        if (numSwaps < kMaxSwaps) ++numSwaps;
        bufferedSamples -= cappedSize;
        frontOrigin += cappedSize;
        oldPeak = currentPeak;
        isWorkingOnPeak = 0;
        qHead = (qHead + 1) % kPeakCap; qCount--;
        ++swapsDone;
    };
    if (ceilingSize == 0 && qCount) qCount = 0;                                                        // :107-110
    // The walk below is the reference's, branch for branch.  In front of it, the same walk for the case a running stream is
    // in at almost every trigger -- the next trigger lies inside the current window (less than half a window after the last
    // one): what the general body computes then is  missing = peak - oldPeak, neededPreSamples = 0, take what is missing
    // from the callback, swap min(buffered, missing + 1) samples  (every
    // double in :147-190 is an integer plus, at most, the half of an odd window: the casts truncate it away on both sides of
    // the one subtraction that matters).  Some forty triggers per callback at cfg3: 8.9 us of a 16 us callback in the general body, 6.3 us here (a lone lane issues an
    // instruction every ~8 cycles; the same in 32-bit arithmetic relative to the callback's start, or with the queue's head read
    // one trigger ahead, measured no faster).  Anything else -- a trigger outside the window -- leaves the state exactly as
    // the general body expects it at that point and falls through to it.
    while (numSamples != 0) {
        // ---- a ROUND: up to 64 queued triggers at once, one per lane.  For a trigger that is fetched with the running clock
        // already past it (no samples swallowed at the fetch, :128), inside the window and in order, the walk does
        //     taken = max(missing - buffered, 0) samples from the callback;  swap min(max(buffered, missing), missing + 1);
        //     buffered <- max(buffered - (missing + 1), 0)
        // -- maps that compose by addition: buffered in front of trigger l is max(buffered_0 - sum_{i<l}(missing_i + 1), 0),
        // so every trigger's numbers are prefix sums.  The round takes the longest run of such triggers that the callback's
        // samples cover (the first one fetched at or after the running clock, out of order, outside the window, or short of
        // samples ends it) and leaves the walk's state behind it; the scalar iteration below handles whatever comes next.
        if (!isWorkingOnPeak && qCount >= 4u && halfCeil <= (1ull << 24) && bufferedSamples <= bufferedCap && bufferedSamples < (1ull << 30) &&
            numSamples < (1ull << 30) && steadyClock < (1ull << 51)) {
            const unsigned long long base = steadyClock;
            auto fits = [&](unsigned long long v) { const long long r = (long long)(v - base); return r > -(1ll << 30) && r < (1ll << 30); };
            if (fits(oldPeak)) {
                const unsigned int cnt = qCount < 64u ? qCount : 64u;
                const unsigned int buf0 = (unsigned int)bufferedSamples, ns0 = (unsigned int)numSamples, hc = (unsigned int)halfCeil;
                auto scan = [&](unsigned int v) {                         // inclusive prefix sum over the wave
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const unsigned int u = __shfl_up(v, o); if (lane >= (unsigned int)o) v += u; }
                    return v;
                };
                const unsigned long long pk = lane < cnt ? peakAt((qHead + lane) % kPeakCap) : 0ull;
                bool ok = lane < cnt && fits(pk);
                const int p = ok ? int((long long)(pk - base)) : 0;
                int prev = __shfl_up(p, 1);
                if (lane == 0) prev = int((long long)(oldPeak - base));
                ok = ok && p >= prev;
                const unsigned int d = ok ? (unsigned int)(p - prev) : 0u;
                ok = ok && d < hc;
                const unsigned int a = ok ? d + 1u : 0u;
                const unsigned int S = scan(a), Sprev = S - a;
                const unsigned int bufL = buf0 > Sprev ? buf0 - Sprev : 0u;
                const unsigned int tp = ok && d > bufL ? d - bufL : 0u;
                const unsigned int Cc = scan(tp), Cprev = Cc - tp;
                const bool swallow = ok && p >= 0 && (unsigned int)p >= Cprev;       // fetched at or after the running clock (base + Cprev)
                const bool stop = !ok || swallow || Cc > ns0 || Cprev >= ns0;
                const unsigned long long stops = __ballot(stop);
                const unsigned int m = stops ? (unsigned int)__builtin_ctzll(stops) : 64u;   // triggers 0 .. m-1 complete
                if (m > 0) {
                    const unsigned int bufTake = bufL > d ? bufL : d, capped = bufTake < d + 1u ? bufTake : d + 1u;
                    const unsigned int capSum = scan(lane < m ? capped : 0u);
                    if (lane < m) storeSwap(numSwaps + lane, written0 + consumed + Cc - bufTake, capped);
                    const unsigned long long took = __ballot(lane < m && tp > 0u);
                    if (took) {
                        const int hl = 63 - __builtin_clzll(took);
                        lastStart = (unsigned int)consumed + __shfl(Cprev, hl);
                        lastLen = __shfl(tp, hl);
                    }
                    const unsigned int Sm = __shfl(S, int(m) - 1), Cm = __shfl(Cc, int(m) - 1), capM = __shfl(capSum, int(m) - 1);
                    const int pm = __shfl(p, int(m) - 1);
                    bufferedSamples = buf0 > Sm ? buf0 - Sm : 0u;
                    numSamples -= Cm; consumed += Cm; steadyClock += Cm;
                    frontOrigin += capM;
                    oldPeak = currentPeak = base + (unsigned long long)(long long)pm;
                    qHead = (qHead + m) % kPeakCap; qCount -= m;
                    swapsDone += m;
                    numSwaps = numSwaps + m < kMaxSwaps ? numSwaps + m : kMaxSwaps;
                    continue;
                }
            }
        }
        bool fastDone = false;
        if (qCount) do {
            if (!isWorkingOnPeak) pickUpNextPeak();
            if (currentPeak < oldPeak) break;                                // (the general body: the difference wraps, "outside the window")
            const unsigned long long d = currentPeak - oldPeak;
            if (d >= halfCeil || oldPeak >= (1ull << 51)) break;
            // inside the window: windowEnd = oldPeak + (u64)halfSize, peakWindowEnd = currentPeak + (u64)halfSize,
            // missingBufferSamples = d, neededPreSamples = 0
            if (bufferedSamples < d) {                                       // :176-182: the samples still missing come out of this callback
                const unsigned long long numRemaining = d - bufferedSamples;
                const unsigned long long toProcess = minU64(numSamples, numRemaining);
                if (toProcess > 0) processIntoBackBuffer(toProcess);
                if (numRemaining != toProcess) { fastDone = true; break; }   // not ready: the callback is used up, the trigger stays open
            }
            swapBuffers(minU64(bufferedSamples, d + 1ull));
            fastDone = true;
        } while (false);
        if (fastDone) continue;
        if (!qCount) { processIntoBackBuffer(numSamples); break; }
        else if (!isWorkingOnPeak) pickUpNextPeak();
        unsigned long long windowEnd;
        bool isPeakOutsideOfWindow = false, readyForBufferSwap = false;
        if (double(currentPeak - oldPeak) < halfSize) windowEnd = (unsigned long long)(double(oldPeak) + halfSize);   // :147-150
        else { isPeakOutsideOfWindow = true; windowEnd = frontOrigin + bufferedSamples; }
        const unsigned long long peakWindowEnd =
            (unsigned long long)(double((isPeakOutsideOfWindow ? 1ull : 0ull) + currentPeak) + halfSize);       // :158
        unsigned long long toProcess = 0;
        const unsigned long long missingBufferSamples = peakWindowEnd - minU64(peakWindowEnd, windowEnd);
        const unsigned long long neededPreSamples =
            minU64((unsigned long long)halfSize, (unsigned long long)(fmax(double(currentPeak - oldPeak), halfSize) - halfSize));
        if (isPeakOutsideOfWindow) {
            toProcess = minU64(numSamples, missingBufferSamples);
            if (toProcess > 0) processIntoBackBuffer(toProcess);
            readyForBufferSwap = missingBufferSamples == toProcess;
        } else if (bufferedSamples >= missingBufferSamples) readyForBufferSwap = true;
        else {
            const unsigned long long numRemaining = missingBufferSamples - bufferedSamples;
            toProcess = minU64(numSamples, numRemaining);
            if (toProcess > 0) processIntoBackBuffer(toProcess);
            readyForBufferSwap = numRemaining == toProcess;
        }
        if (readyForBufferSwap) {
            const double amount = (isPeakOutsideOfWindow ? halfSize : double(missingBufferSamples)) + double(neededPreSamples);
            swapBuffers(minU64(bufferedSamples, (unsigned long long)ceil(amount + 1)));
        }
    }
    if (lane0) {
        st->swaps += swapsDone;                            // (once: a read-modify-write of global memory inside the walk is a round trip per trigger)
        st->bufferedSamples = bufferedSamples; st->frontOrigin = frontOrigin; st->steadyClock = steadyClock;
        st->oldPeak = oldPeak; st->currentPeak = currentPeak; st->qHead = qHead; st->qCount = qCount;
        st->isWorkingOnPeak = isWorkingOnPeak;
        plan.numSwaps = numSwaps; plan.lastStart = lastStart; plan.lastLen = lastLen;
    }
}

// ---- F: per-sample colours of the block (audioProcessing :445-517, :588-647) -> col.block.  Every sample passes through
// audioProcessing exactly once and in order, whatever the split into calls, so the filters run over the block as a whole.
__device__ __forceinline__ void colourPhase(const ColourParams &col, const float *blk, uint32_t n, uint32_t C)
{
    const int tid = threadIdx.x, T = blockDim.x;
    // The three filter stages hand their per-sample outputs on through LDS, a tile of the callback at a time (samples in, band
    // signals, smoothed energies: 11 floats per channel and sample; a stereo tile is 416 samples).  Through the HBM scratch every
    // sixteen samples of every stage waited for a memory round trip of its own: 64 us per stage, 193 us of a 206 us callback.
    constexpr uint32_t kFFloats = 9216;
    __shared__ float sF[kFFloats];
    const uint32_t MB = col.maxBlock;
    ColourDev *cs = col.st;
    uint32_t tile = kFFloats / (11u * C);
    tile = tile >= 16u ? (tile & ~15u) : (tile ? tile : 1u);
    if (tile > 512u) tile = 512u;
    float *sX = sF, *sB = sX + size_t(C) * tile, *sS = sB + size_t(4 * C) * tile;       // [C][tile], [4 C][tile], [6 C][tile]
    // the lanes' filter states stay in registers from tile to tile
    const bool r12 = uint32_t(tid) < 2 * C, r3 = uint32_t(tid) < 6 * C;
    const uint32_t fc = uint32_t(tid) >> 1, fhp = uint32_t(tid) & 1u;
    float k1[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, k2[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f, c0 = 0.f, c1 = 0.f, d0 = 0.f, d1 = 0.f, y = 0.f;
    float *stp = nullptr;
    const uint32_t pair3 = uint32_t(tid) / 12u, r = uint32_t(tid) % 12u, sig3 = r / 3u, band3 = r % 3u;
    if (r12) {
        const float *ka = fhp ? col.hp1 : col.lp1, *kb = fhp ? col.hp2 : col.lp2;
        for (int j = 0; j < 5; ++j) { k1[j] = ka[j]; k2[j] = kb[j]; }
        float (*z1)[2] = cs->z[fc] + (fhp ? 2 : 0), (*z2)[2] = cs->z[fc] + (fhp ? 6 : 4);
        a0 = z1[0][0]; a1 = z1[0][1]; b0 = z1[1][0]; b1 = z1[1][1];
        c0 = z2[0][0]; c1 = z2[0][1]; d0 = z2[1][0]; d1 = z2[1][1];
    }
    if (r3) {
        stp = sig3 == 0 ? &cs->smooth[2 * pair3][band3] : sig3 == 1 ? &cs->smooth[2 * pair3 + 1][band3]
            : sig3 == 2 ? &cs->aux[2 * pair3][band3] : &cs->aux[2 * pair3 + 1][band3];
        y = *stp;
    }
    const float pole = col.pole;
    for (uint32_t t0 = 0; t0 < n; t0 += tile) {
        const uint32_t m = min(tile, n - t0);
        for (uint32_t e = tid; e < C * m; e += T) { const uint32_t c = e / m, i = e - c * m; sX[size_t(c) * tile + i] = blk[size_t(c) * n + t0 + i]; }
        __syncthreads();
        if (r12) {                                                     // F1: low = LP4_f1(x), rest = HP4_f1(x)
            const float *x = sX + size_t(fc) * tile;
            float *out = sB + (size_t(fc) * 4 + (fhp ? 3 : 0)) * tile;
            walkSequential(m, [&](uint32_t i) { return x[i]; },
                           [&](uint32_t i, float v) { out[i] = biquadStep(k1, b0, b1, biquadStep(k1, a0, a1, v)); });
        }
        __syncthreads();
        if (r12) {                                                     // F2: mid = LP4_f2(rest), high = HP4_f2(rest)
            const float *x = sB + (size_t(fc) * 4 + 3) * tile;
            float *out = sB + (size_t(fc) * 4 + (fhp ? 2 : 1)) * tile;
            walkSequential(m, [&](uint32_t i) { return x[i]; },
                           [&](uint32_t i, float v) { out[i] = biquadStep(k2, d0, d1, biquadStep(k2, c0, c1, v)); });
        }
        __syncthreads();
        if (r3) {                                                      // F3: filterStates (:460-468) of left, right, mid, side
            const float *l = sB + (size_t(2 * pair3) * 4 + band3) * tile, *rr = sB + (size_t(2 * pair3 + 1) * 4 + band3) * tile;
            float *out = sS + size_t(tid) * tile;
            // (which signal a lane smooths is a lane constant: both inputs are read and the lane's one picked by selects -- as a
            // branch inside the batched loads the four cases ran one after the other: 90 us of a 150 us callback)
            const bool isL = sig3 == 0, isR = sig3 == 1, isMid = sig3 == 2;
            walkSequential(m, [&](uint32_t i) { return l[i]; },
                           [&](uint32_t i, float lv) {
                               const float rv = rr[i];
                               const float sum = lv + rv, dif = lv - rv;
                               const float v = isL ? lv : (isR ? rv : (isMid ? sum : dif));
                               const float input = v * v;
                               y = input + pole * (y - input);
                               out[i] = y;
                           });
        }
        __syncthreads();
        for (uint32_t e = tid; e < 2 * C * m; e += T) {                // F4: accumulateColour per (signal, sample)
            const uint32_t q = e / m, i = e - q * m, pair = q >> 2, sig = q & 3u;
            const float *sp = sS + size_t(pair * 12 + sig * 3) * tile + i;
            const float stv[3] = {sp[0], sp[tile], sp[2 * size_t(tile)]};
            const uint32_t keyCh = 2 * pair + (sig & 1u);              // left / mid: the left key, right / side: the right key
            const uint32_t plane = (sig < 2 ? 0u : C) + keyCh;         // cwLeft, cwRight -> colourData; cwMid, cwSide -> auxColourData
            col.block[size_t(plane) * MB + t0 + i] = accumulateColour(stv, col.band, col.keys[keyCh], col.blend);
        }
        __syncthreads();
    }
    if (r12) {
        float (*z1)[2] = cs->z[fc] + (fhp ? 2 : 0), (*z2)[2] = cs->z[fc] + (fhp ? 6 : 4);
        z1[0][0] = a0; z1[0][1] = a1; z1[1][0] = b0; z1[1][1] = b1;
        z2[0][0] = c0; z2[0][1] = c1; z2[1][0] = d0; z2[1][1] = d1;
    }
    if (r3) *stp = y;
}

// ---- C: the ns swaps of phase B (hold: ZeroCrossing, EnvelopeHold) or the block itself (None / Spectral: audioProcessing straight
// into the front buffer), in order, into the front rings from ring slot cursor0 on; returns the cursor behind them.
// written0: the absolute index of the block's first sample.
__device__ __forceinline__ uint32_t frontPhase(const IngestParams &prm, const Planes<float> &audio, const Planes<uint32_t> &colour,
                                               bool hold, const Swap *swaps, uint32_t ns, uint32_t n, uint32_t cursor0, unsigned long long written0,
                                               unsigned int *sSum)
{
    const uint32_t size = prm.size, backCap = prm.backCap;
    const int tid = threadIdx.x, T = blockDim.x;
    auto copy = [&](unsigned long long abs, uint32_t d) {
        copyToFront(audio, abs, written0, d, size, backCap);
        if (prm.colours) copyToFront(colour, abs, written0, d, size, backCap);
    };
    auto swapAt = [&](uint32_t k) { return k < kStage ? swaps[k] : prm.swapList[k]; };
    if (hold && ns <= kFlat) {
        // The usual case -- a handful of swaps, all in LDS -- as ONE pass: no two swaps of a block write the same ring slot (what a later
        // swap would overwrite is dead and never written), and their sources are read-only here, so they need no order among
        // themselves.  Swap k's surviving range comes from prefix sums of the lengths (lane k of wave 0; one thread each past 64);
        // then every thread copies its share of the concatenation.  (One swap after the other with a barrier each cost a memory
        // round trip per swap: 8.9 us of a 25 us block at a dozen swaps, tools/ingest_clocks.py; now 1.9 us.)
        __shared__ unsigned long long sFlatSrc[kFlat];
        __shared__ uint32_t sFlatDst[kFlat], sFlatEnd[kFlat], sFlatTotal, sCursorEnd;
        // swap k's row of the tables; scan(v, total) -> inclusive prefix sum of v over the swaps
        auto tableRow = [&](uint32_t k, bool live, const Swap &sw, auto scanLen, auto scanM) {
            unsigned long long total;
            const unsigned long long inc = scanLen((unsigned long long)sw.len, total);
            uint32_t first, totalM;
            const uint32_t incM = scanM(survivingRange(sw.len, total - inc, size, first), totalM);
            if (live) {
                sFlatSrc[k] = sw.src + first;
                sFlatDst[k] = uint32_t((cursor0 + (inc - sw.len) + first) % size);
                sFlatEnd[k] = incM;
            }
            if (k == 0) { sFlatTotal = totalM; sCursorEnd = uint32_t((cursor0 + total) % size); }
        };
        const uint32_t k = uint32_t(tid);
        const bool live = k < ns;
        if (ns > kStage) {
            // more swaps than a wave has lanes (a 10 kHz tone at 48 kHz crosses zero 107 times per 512-sample callback): workgroup-wide
            // prefix sums, one swap per thread (the swaps beyond the staged ones are read back from HBM).  One after the other they cost
            // 0.65 us each: 74 us per callback at 107, 143 us at 213.
            __shared__ unsigned long long sScan64[16];
            // (read at a loop-variant index: at k alone the selected LDS-or-HBM address is hoisted out of the block loop, a flat
            // pointer per thread that the colour phase has no registers for)
            Swap sw = swapAt(live ? k : 0u);
            if (!live) sw = Swap{0ull, 0u, 0u};
            tableRow(k, live, sw,
                     [&](unsigned long long v, unsigned long long &t) { return blockInclusiveSum(v, sScan64, &t); },
                     [&](uint32_t v, uint32_t &t) { return blockInclusiveSum(v, sSum, &t); });
        } else if (tid < 64) {
            auto waveScan = [&](auto v, auto &total) {
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const auto u = __shfl_up(v, o); if (tid >= o) v += u; }
                total = __shfl(v, 63);
                return v;
            };
            tableRow(k, live, live ? swaps[k] : Swap{0ull, 0u, 0u}, waveScan, waveScan);
        }
        __syncthreads();
        const uint32_t M = sFlatTotal;
        for (uint32_t e = tid; e < M; e += T) {
            uint32_t lo = 0, hi = ns;                                    // the swap of element e: smallest k with sFlatEnd[k] > e
            while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if (sFlatEnd[mid - 1] > e) hi = mid; else lo = mid; }
            const uint32_t i = e - (lo ? sFlatEnd[lo - 1] : 0u);
            copy(sFlatSrc[lo] + i, (sFlatDst[lo] + i) % size);
        }
        const uint32_t cursor = sCursorEnd;
        __syncthreads();
        return cursor;
    }
    // one run after the other, each behind a barrier; `later`: the samples the runs after it append
    uint32_t cursor = cursor0;
    auto append = [&](unsigned long long src, uint32_t len, unsigned long long later) {
        uint32_t first;
        const uint32_t m = survivingRange(len, later, size, first);
        const uint32_t d0 = uint32_t((cursor + first) % size);
        for (uint32_t i = tid; i < m; i += T) copy(src + first + i, (d0 + i) % size);
        cursor = uint32_t((cursor + len) % size);
        __syncthreads();
    };
    if (!hold) { append(written0, n, 0ull); return cursor; }
    unsigned long long later = 0;                                        // suffix sums of the swap lengths: a thread-private walk from the back
    for (uint32_t k = 0; k < ns; ++k) later += swapAt(k).len;
    for (uint32_t k = 0; k < ns; ++k) {
        const Swap sw = swapAt(k);
        later -= sw.len;
        append(sw.src, sw.len, later);
    }
    return cursor;
}

// ---- E: RMS envelope (audioProcessing, OscilloscopeDSP.inl:520-585, :676-693); wave 0, lane c = recurrence c.  The callback's last
// audioProcessing call covers samples [lastStart, lastStart + lastLen).
// (the reference runs the recurrence in PeakDecay mode too and throws the result away, :506-585 against :676: only RMS stores it)
__device__ __forceinline__ void envelopePhase(const IngestParams &prm, ScopeDev *st, const float *blk, uint32_t n, uint32_t lastStart, uint32_t lastLen)
{
    const int tid = threadIdx.x;
    const uint32_t C = prm.in.channels;
    const bool active = tid < int(C);
    const float k = prm.envelopeCoeff;
    const uint32_t mode = prm.oscMode;
    // channels 0 / 1 are stored back (:690-691) and so run through every audioProcessing call of the block; the others restart
    // from their stored envelope in every call, so only the last call's samples matter for them
    const uint32_t from = tid < 2 ? 0u : lastStart, to = lastStart + lastLen;
    float y = active ? st->envelope[tid] : 0.f;
    const float *b0 = blk, *b1 = blk + n, *bc = blk + size_t(active ? tid : 0) * n;
    bool own = false;
    if (mode == SGZ_OSC_SEPARATE) {
        own = true;
        if (active) walkSequential(to - from, [&](uint32_t i) { return bc[from + i]; }, [&](uint32_t, float v) { const float s = v * v; y = s + k * (y - s); });
    } else if (mode == SGZ_OSC_MIDSIDE) {
        if (tid < 2) {
            own = true;
            // the mix itself is exact in either order of evaluation: (l +- r) once, squared, halved
            walkSequential(to, [&](uint32_t i) { return tid == 0 ? b0[i] + b1[i] : b0[i] - b1[i]; },
                           [&](uint32_t, float v) { const float s = 0.5f * (v * v); y = s + k * (y - s); });
        }
    } else if (tid == 0) {
        own = true;
        const float *src = mode == SGZ_OSC_RIGHT ? b1 : b0;
        // (one walk per mode: a branch inside the load would keep the batch of loads from being issued together)
        auto rms = [&](uint32_t, float v) { const float s = v * v; y = s + k * (y - s); };
        if (mode == SGZ_OSC_MID) walkSequential(to, [&](uint32_t i) { return 0.5f * (b0[i] + b1[i]); }, rms);
        else if (mode == SGZ_OSC_SIDE) walkSequential(to, [&](uint32_t i) { return 0.5f * (b0[i] - b1[i]); }, rms);
        else walkSequential(to, [&](uint32_t i) { return src[i]; }, rms);
    }
    // filterEnv[c] of the last call: copies of channel 0 (mono modes) / channel 1 (MidSide) where the channel has no recurrence
    const float y0 = __shfl(y, 0), y1 = __shfl(y, 1);
    const float fe = own ? y : (mode == SGZ_OSC_MIDSIDE ? y1 : y0);
    float start = active ? __builtin_sqrtf(fe) : 0.f;                  // RMS: gain and stored envelopes
    for (int o = 32; o > 0; o >>= 1) start = fmaxf(start, __shfl_xor(start, o));
    if (tid == 0) {
        st->envelopeGain = 1.0 / double(start);
        st->envelope[0] = y0;
        st->envelope[1] = (mode == SGZ_OSC_SEPARATE || mode == SGZ_OSC_MIDSIDE) ? y1 : y0;
    }
}

// (the colour parameters -- ~100 words with the per-channel keys -- come through a pointer: as a by-value argument they stayed live in
// scalar registers across the loop over the batch's blocks and pushed four vector registers into scratch)
__device__ void scopePeakBody(const PeakParams &prm);

__global__ void __launch_bounds__(1024) scopeIngestKernel(const IngestParams prm, const ColourParams *colp)
{
    const ColourParams &col = *colp;
    __shared__ int sScan2[32];
    __shared__ unsigned int sSum[16];
    // The stream state lives in LDS for the length of the kernel (one coalesced read, one write-back): the phases below touch its fields
    // some thirty times, mostly from one lane and each time behind the last (the kernels of the render thread read the copy in HBM,
    // between launches)
    __shared__ ScopeDev sState;
    const uint32_t C = prm.in.channels;
    const int tid = threadIdx.x, T = blockDim.x;
    static_assert(sizeof(ScopeDev) % 4 == 0, "copied as words");
    for (uint32_t w = tid; w < sizeof(ScopeDev) / 4; w += T) reinterpret_cast<uint32_t *>(&sState)[w] = reinterpret_cast<const uint32_t *>(prm.st)[w];
    __syncthreads();
    ScopeDev *st = &sState;
    __shared__ unsigned long long sPeaks[kStage];
    __shared__ Swap sSwaps[kStage];
    __shared__ SwapPlan sPlan;
    // One launch ingests every block that was waiting (sgz_scope_push only stages; whoever needs the state -- the render thread's calls, a
    // full batch, sgz_scope_flush -- submits): the blocks go through the reference's per-callback state machine ONE AFTER THE OTHER, with
    // their boundaries where the host put them (audioEntryPoint runs once per onStreamAudio: update(), the detector, processMutating's
    // window selection all see callback extents), the stream state staying in LDS in between.
    // (rt_common.hpp batchOpen's three steps, written out: through the function this kernel spilt 154 scalar registers instead of 142)
    // (the block table goes through LDS: a run-time subscript into the by-value argument struct would move the struct to scratch)
    __shared__ uint32_t sBlockOff[BatchRing::kMaxBlocks], sBlockLen[BatchRing::kMaxBlocks];
#pragma unroll
    for (uint32_t b = 0; b < BatchRing::kMaxBlocks; ++b)
        if (tid == int(b)) { sBlockOff[b] = prm.in.blockOff[b]; sBlockLen[b] = prm.in.blockLen[b]; }
    __syncthreads();
    batchFetch(prm.in.batchHost, const_cast<float *>(prm.in.batch), prm.in.batchFloats, tid, T);
    // sgz_scope_set_mix: the staged source rows -> the destination rows every phase below reads (and sBlockOff into them)
    __shared__ MixRoute sRoute;
    const float *batch = prm.in.batch;
    if (prm.in.route) {                                                    // (uniform)
        batchMix(prm.in.route, sRoute, prm.in.batch, prm.in.mixRows, prm.in.numSources, C, prm.in.numBlocks, sBlockOff, sBlockLen, tid, T);
        batch = prm.in.mixRows;
    }
    // ---- A for the WHOLE batch.  The zero-crossing detector (phase A) is a scan over the samples whose state (armed, last threshold
    // crossing, previous sample) does not depend on what processMutating does with the triggers, and a trigger's slot in the queue's
    // ring is head + count + (triggers before it) whatever has been popped meanwhile: so the detector runs ONCE over the
    // concatenation of the batch's blocks (three passes and two block-wide scans instead of that per block: 4 us per block saved),
    // writes every trigger where the per-callback walk would, and each block's processMutating then sees the queue grow by its own
    // block's triggers only (sFires).  Taken when no trigger can be dropped (count + all fires <= capacity: then no callback of the
    // sequential walk drops one either) and no window change is pending (update() edits the queue); otherwise block by block.
    __shared__ uint32_t sBlockStart[BatchRing::kMaxBlocks + 1];
    __shared__ unsigned int sFires[BatchRing::kMaxBlocks];
    __shared__ int sBatchedA;
    if (tid == 0) {
        uint32_t acc = 0;
        for (uint32_t b = 0; b < BatchRing::kMaxBlocks; ++b) { sBlockStart[b] = acc; acc += b < prm.in.numBlocks ? sBlockLen[b] : 0u; }
        sBlockStart[BatchRing::kMaxBlocks] = acc;
        sBatchedA = 0;
    }
    if (tid < int(BatchRing::kMaxBlocks)) sFires[tid] = 0;
    __syncthreads();
    if (prm.triggerMode == 4u && C >= 2 && prm.in.numBlocks > 1 && !st->windowChanged) {       // (uniform)
        auto sampleAt = [&](uint32_t i, uint32_t &b) -> double {           // sample i of the concatenation
            while (sBlockStart[b + 1] <= i) ++b;
            const float *a, *c;
            const uint32_t mode = triggerPlanes(prm, batch + sBlockOff[b], sBlockLen[b], a, c);
            return trigSample(mode, a, c, i - sBlockStart[b]);
        };
        if (zeroCrossings(sBlockStart[prm.in.numBlocks], sampleAt, st, prm.peaks, st->playhead, sFires, sScan2, sSum) && tid == 0) sBatchedA = 1;
        __syncthreads();
    }
    const bool batchedA = sBatchedA != 0;
    const bool hold = prm.triggerMode == 4u || prm.triggerMode == 3u;      // ZeroCrossing, EnvelopeHold: detector -> processMutating
    for (uint32_t blockIndex = 0; blockIndex < prm.in.numBlocks; ++blockIndex) {
        const float *const blk = batch + sBlockOff[blockIndex];
        const uint32_t n = sBlockLen[blockIndex];
        const unsigned long long playhead = st->playhead;
        ICLK(0);
        if (tid == 0) updatePhase(st, prm.peaks, playhead);
        __syncthreads();
        if (prm.triggerMode == 3u && C >= 2) {
            if (tid == 0) peakHoldPhase(prm, st, blk, n, playhead);
            __syncthreads();
        }
        if (batchedA) {                                                    // (found for the whole batch above: this callback's triggers become visible)
            if (tid == 0) st->qCount += sFires[blockIndex];
            __syncthreads();
        } else if (prm.triggerMode == 4u && C >= 2) {
            const float *a, *b;
            const uint32_t mode = triggerPlanes(prm, blk, n, a, b);
            zeroCrossings(n, [&](uint32_t i, uint32_t &) { return trigSample(mode, a, b, i); }, st, prm.peaks, playhead, nullptr, sScan2, sSum);
            __syncthreads();
        }
        ICLK(1);
        if (hold && tid < int(kStage) && uint32_t(tid) < st->qCount) sPeaks[tid] = prm.peaks[(st->qHead + uint32_t(tid)) % kPeakCap];
        __syncthreads();
        if (hold && tid < 64) processMutating(prm, st, n, sPeaks, sSwaps, sPlan);
        else if (tid == 0) sPlan = SwapPlan{0u, 0u, n};
        __syncthreads();
        ICLK(2);
        if (prm.colours) {
            colourPhase(col, blk, n, C);
            __syncthreads();
        }
        // (phase B has not touched the ring fields of the state: the block's rings start where the last block left them)
        const uint32_t cursor0 = st->frontCursor;
        const unsigned long long written0 = st->written;
        ICLK(3);
        const Planes<float> audio{blk, n, prm.back, prm.front, C};
        const Planes<uint32_t> colour{col.block, col.maxBlock, col.back, col.front, 2 * C};
        const uint32_t cursor = frontPhase(prm, audio, colour, hold, sSwaps, sPlan.numSwaps, n, cursor0, written0, sSum);
        ICLK(4);
        if (hold) {                                                        // ---- D: the block goes into the back rings
            copyToBack(audio, n, written0, prm.backCap);
            if (prm.colours) copyToBack(colour, n, written0, prm.backCap);
        }
        ICLK(5);
        if (prm.envMode == 1u && tid < 64) envelopePhase(prm, st, blk, n, sPlan.lastStart, sPlan.lastLen);
        __syncthreads();
        ICLK(6);
        if (tid == 0) {
            st->frontCursor = cursor;
            if (hold) st->written = written0 + n;
            st->playhead = playhead + n;
        }
        __syncthreads();
    }
    for (uint32_t w = tid; w < sizeof(ScopeDev) / 4; w += T) reinterpret_cast<uint32_t *>(prm.st)[w] = reinterpret_cast<const uint32_t *>(&sState)[w];
    ICLK(7);
    if (prm.doPeak) {                                            // (uniform) the rings and the state this launch wrote, as every lane sees them
        __threadfence();
        __syncthreads();
        scopePeakBody(prm.peak);
    }
}

// ---- Oscilloscope::runPeakFilter on the front rings (memory order, last size mod lanes slots dropped), every channel mode.
// A 1024-thread workgroup: scopePeakKernel, or the tail of scopeIngestKernel.
__device__ void scopePeakBody(const PeakParams &prm)
{
    __shared__ float sL[kMaxCh][16], sR[16];
    const uint32_t C = prm.channels, size = prm.size;
    const uint32_t mode = C == 1 ? uint32_t(SGZ_OSC_LEFT) : prm.mode;
    const uint32_t len = prm.len ? prm.len : size;
    const uint32_t stop = len - (len & (prm.lanes - 1));
    // memory index of slot i of the reference's ring: the ring itself, or (Spectral) the newest len samples of the larger ring
    const uint32_t first = prm.len ? (prm.st->frontCursor + size - len) % size : 0u;
    auto at = [&](uint32_t i) { uint32_t p = first + i; return p >= size ? p - size : p; };
    const int tid = threadIdx.x, wave = tid >> 6, waves = blockDim.x >> 6;
    auto blockMax = [&](float v, float *slot) {
        for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
        if ((tid & 63) == 0) slot[wave] = v;
    };
    const float *L = prm.front, *R = prm.front + (C > 1 ? size : 0);
    if (mode <= SGZ_OSC_SIDE) {
        float m = 0.f;
        for (uint32_t j = tid; j < stop; j += blockDim.x) {
            const uint32_t i = at(j);
            float v;
            if (mode == SGZ_OSC_LEFT) v = L[i];
            else if (mode == SGZ_OSC_RIGHT) v = R[i];
            else if (mode == SGZ_OSC_MID) v = (L[i] + R[i]) * 0.5f;
            else v = (L[i] - R[i]) * 0.5f;
            m = fmaxf(fabsf(v), m);
        }
        blockMax(m, sL[0]);
    } else if (mode == SGZ_OSC_SEPARATE) {
        for (uint32_t c = 0; c < C; ++c) {
            float m = 0.f;
            const float *x = prm.front + size_t(c) * size;
            for (uint32_t j = tid; j < stop; j += blockDim.x) m = fmaxf(fabsf(x[at(j)]), m);
            blockMax(m, sL[c]);
        }
    } else {
        float ml = 0.f, mr = 0.f;
        for (uint32_t j = tid; j < stop; j += blockDim.x) {
            const uint32_t i = at(j);
            const float a = L[i] + R[i], b = L[i] - R[i];
            ml = fmaxf(fabsf(a * 0.5f), ml);
            mr = fmaxf(fabsf(b * 0.5f), mr);
        }
        blockMax(ml, sL[0]);
        blockMax(mr, sR);
    }
    __syncthreads();
    if (tid != 0) return;
    ScopeDev *st = prm.st;
    auto fold = [&](const float *slot) { float r = 0.f; for (int w = 0; w < waves; ++w) r = fmaxf(r, slot[w]); return r; };
    const double coeff = prm.coeff;
    if (mode <= SGZ_OSC_SIDE) {
        const double highest = double(fold(sL[0]));
        st->envelope[0] = float(fmax(double(st->envelope[0]) * coeff, highest * highest));
        if (C > 1) st->envelope[1] = float(fmax(double(st->envelope[1]) * coeff, highest * highest));
        for (uint32_t c = 2; c < C; ++c) st->envelope[c] = st->envelope[1];
    } else if (mode == SGZ_OSC_SEPARATE) {
        float running = 0.f;                                // vLMax is not reset between channels (:827-838)
        for (uint32_t c = 0; c < C; ++c) {
            running = fmaxf(running, fold(sL[c]));
            st->envelope[c] = fmaxf(float(double(st->envelope[c]) * coeff), running * running);   // std::max<float>(...)
        }
    } else {
        const double hl = double(fold(sL[0])), hr = double(fold(sR));
        st->envelope[0] = float(fmax(double(st->envelope[0]) * coeff, hl * hl));
        st->envelope[1] = float(fmax(double(st->envelope[1]) * coeff, hr * hr));
        for (uint32_t c = 2; c < C; ++c) st->envelope[c] = st->envelope[1];
    }
    float start = __builtin_sqrtf(st->envelope[0]);
    for (uint32_t c = 0; c < C; ++c) start = fmaxf(start, __builtin_sqrtf(st->envelope[c]));
    st->autoGain = 1.0 / double(start);
}
__global__ void __launch_bounds__(1024) scopePeakKernel(const PeakParams prm) { scopePeakBody(prm); }


// ---- Spectral triggering: Oscilloscope::calculateFundamentalPeriod + calculateTriggeringOffset (OscilloscopeDSP.inl:62-308)
struct BinRec { unsigned long long index; double value, offset; };           // BinRecord, Oscilloscope.h
struct SpectralDev {
    BinRec median[8];                        // medianTriggerFilter[i].record (value-initialised)
    unsigned long long medianPos;
    BinRec record;                           // triggerState.record
    double fundamental, cycleSamples, sampleOffset, phase;
    unsigned long long ringSize;             // resizeAudioStorage's size (ChannelData.h:107-128): in = of the previous frame, out = of this one
    double effectiveWindow;                  // state.effectiveWindowSize of the frame (out)
};
struct SpectralParams {
    SpectralDev *st;
    const float *ringA, *ringB; uint32_t evalMode, cap;
    const uint32_t *d_cursor;
    double windowSize, sampleRate, threshold, hysteresis, phaseOffsetDeg, quarterSemitone;
    double customFrequency;                  // state.customTrigger ? state.customTriggerFrequency : 0
    const double2 *tw;                       // [4096] exp(-2 pi i k / 8192)
    double cycles;                           // SGZ_TIME_CYCLES: the window value (windowSize = cycles * the last frame's cycleSamples + 1); else 0
    unsigned long long firstRing;            // the ring of the frame before the first one, if not st->ringSize (SGZ_TIME_BEATS); else 0
    ScopeDev *trig;                          // Cycles / Beats: the TriggeringProcessor that setSettings gives the frame's window; else null
};

__device__ __forceinline__ double recOmega(const BinRec &r) { return double(r.index) + r.offset; }
__device__ __forceinline__ uint32_t brev13(uint32_t i) { return __brev(i) >> 19; }
__device__ __forceinline__ uint32_t logicalPhys(long rel, uint32_t cursor, uint32_t cap, uint32_t len)
{
    long q = rel % long(len);
    if (q < 0) q += long(len);
    return uint32_t((long(cursor) + long(cap - len) + q) % long(cap));
}
__device__ __forceinline__ double evalD(const float *a, const float *b, uint32_t mode, uint32_t idx)
{
    if (mode == 1u) return double(0.5f * (a[idx] + b[idx]));
    if (mode == 2u) return double(0.5f * (a[idx] - b[idx]));
    return double(a[idx]);
}

// libstdc++'s std::nth_element(v, v + 4, v + 8, by index) -- see oracle/scope_spectral.c for why the algorithm itself matters
__device__ inline bool recLess(const BinRec &a, const BinRec &b) { return a.index < b.index; }
__device__ inline void recSwap(BinRec &a, BinRec &b) { const BinRec t = a; a = b; b = t; }
__device__ void nthElementByIndex(BinRec *v, int n, int nth)
{
    int first = 0, last = n;
    int depth = 0;
    for (int k = n; k > 1; k >>= 1) ++depth;
    depth *= 2;
    while (last - first > 3) {
        if (depth == 0) {
            for (int i = first; i <= nth; ++i)
                for (int j = i + 1; j < last; ++j)
                    if (recLess(v[j], v[i])) recSwap(v[i], v[j]);
            return;
        }
        --depth;
        const int mid = first + (last - first) / 2;
        {   // __move_median_to_first(first, first + 1, mid, last - 1)
            const int r = first, a = first + 1, b = mid, c = last - 1;
            if (recLess(v[a], v[b])) {
                if (recLess(v[b], v[c])) recSwap(v[r], v[b]);
                else if (recLess(v[a], v[c])) recSwap(v[r], v[c]);
                else recSwap(v[r], v[a]);
            } else if (recLess(v[a], v[c])) recSwap(v[r], v[a]);
            else if (recLess(v[b], v[c])) recSwap(v[r], v[c]);
            else recSwap(v[r], v[b]);
        }
        int f = first + 1, l = last;                       // __unguarded_partition(first + 1, last, pivot = first)
        for (;;) {
            while (recLess(v[f], v[first])) ++f;
            --l;
            while (recLess(v[first], v[l])) --l;
            if (!(f < l)) break;
            recSwap(v[f], v[l]);
            ++f;
        }
        if (f <= nth) first = f;
        else last = f;
    }
    for (int i = first + 1; i < last; ++i) {               // __insertion_sort
        const BinRec val = v[i];
        if (recLess(val, v[first])) {
            for (int j = i; j > first; --j) v[j] = v[j - 1];
            v[first] = val;
        } else {
            int j = i;
            while (recLess(val, v[j - 1])) { v[j] = v[j - 1]; --j; }
            v[j] = val;
        }
    }
}

// One workgroup; dynamic LDS: re[8192], im[8192] doubles.  The transform is an in-place radix-2 DIF (bit-reversed output); natural bin
// k sits at position brev13(k).  Only bins 0 .. 4096 are read afterwards, i.e. position 1 and the even positions, so |X[i]| of bin i
// (1 <= i < 4096) is parked at re[brev13(i) + 1] -- the slot of bin i + 4096.
__global__ void __launch_bounds__(1024) scopeSpectralKernel(const SpectralParams prm)
{
    extern __shared__ double spectralLds[];
    double *re = spectralLds, *im = spectralLds + 8192;
    __shared__ double sRed[2][16];
    __shared__ double sRadians, sSampleDifference;
    __shared__ long sOffset2;
    const int tid = threadIdx.x;
    __shared__ double sWindow;
    SpectralDev *st = prm.st;
    const uint32_t cursor = *prm.d_cursor, cap = prm.cap, len = uint32_t(prm.firstRing ? prm.firstRing : st->ringSize);
    constexpr uint32_t N = 8192;
    // handleFlagUpdates' window step (Oscilloscope.cpp:293-307) for this frame -- Cycles: from the cycleSamples the last frame left,
    // read before anything below overwrites it (every thread takes the same fp64 value: no host round trip)
    if (tid == 0) {
        const double w = prm.cycles > 0 ? prm.cycles * st->cycleSamples + 1 : prm.windowSize;
        sWindow = w;
        if (prm.trig) {                                    // setSettings (StreamPreprocessing.h:46-53; a change still pending stays so)
            if (ceil(w) != ceil(prm.trig->windowSize)) prm.trig->windowChanged = 1;
            prm.trig->windowSize = w;
        }
    }
    __syncthreads();
    const double windowSize = sWindow;

    // what calculateFundamentalPeriod leaves behind and what calculateTriggeringOffset derives from it first (:256-270)
    auto settle = [&](const BinRec &rec, double fundamental) {
        st->record = rec;
        st->fundamental = fundamental;
        const double cycleSamples = prm.sampleRate / fundamental;
        st->cycleSamples = cycleSamples;
        const double tau = 6.283185307179586476925286766559;
        const double radians = tau * recOmega(rec) / double(N);
        const double offsetReal = fmax(double(N), windowSize + cycleSamples);
        const unsigned long long offset = (unsigned long long)ceil(offsetReal);
        sRadians = radians;
        sSampleDifference = double(offset) - (windowSize + cycleSamples);
        sOffset2 = long(offset);
    };
    if (prm.customFrequency > 0) {
        // state.customTrigger (:71-81): the user names the frequency -- no transform, no median filter; the Goertzel phase below runs on it
        if (tid == 0) {
            BinRec rec; rec.index = 0; rec.value = 1; rec.offset = prm.customFrequency / prm.sampleRate * double(N);
            settle(rec, prm.customFrequency);
        }
    } else {
    {   // transformBuffer[i] = eval.evaluateSampleInc() from -max(ceil(effectiveWindowSize), LookaheadSize) (:92-99)
        const long offset = long(fmax(ceil(windowSize), double(N)));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t i = uint32_t(tid) + 1024u * j;
            re[i] = evalD(prm.ringA, prm.ringB, prm.evalMode, logicalPhys(-offset + long(i), cursor, cap, len));
            im[i] = 0.0;
        }
    }
    __syncthreads();
    for (int s = 0; s < 13; ++s) {                         // DustFFT_fwdDa: forward DFT, fp64
        const uint32_t half = 4096u >> s;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t b = uint32_t(tid) + 1024u * j;
            const uint32_t pos = b & (half - 1), i0 = ((b >> (12 - s)) << (13 - s)) + pos, i1 = i0 + half;
            const double2 w = prm.tw[pos << s];
            const double ar = re[i0], ai = im[i0], br = re[i1], bi = im[i1];
            const double dr = ar - br, di = ai - bi;
            re[i0] = ar + br; im[i0] = ai + bi;
            re[i1] = dr * w.x - di * w.y; im[i1] = dr * w.y + di * w.x;
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = uint32_t(tid) + 1024u * j;
        if (i >= 1) { const uint32_t p = brev13(i); re[p + 1] = hypot(re[p], im[p]); }      // std::abs(complex<double>)
    }
    __syncthreads();

    if (tid < 64) {                                        // the candidate scan (:134-181), 64 bins at a time
        const int lane = tid;
        auto mag = [&](uint32_t i) { return re[brev13(i) + 1]; };
        auto quadDelta = [&](uint32_t w) -> double {       // :113-124
            const uint32_t p0 = brev13(w), p1 = brev13(w + 1), pm = brev13(w == 0 ? 1 : w - 1);
            const double dre = re[p0] * 2.0 - re[pm] - re[p1], dim = im[p0] * 2.0 - im[pm] - im[p1];
            if ((dre + dim) == 0) return 0.0;
            const double nre = re[pm] - re[p1], nim = im[pm] - im[p1];
            return (nre * dre + nim * dim) / (dre * dre + dim * dim);
        };
        const double invHysteresis = 1 - prm.hysteresis, quarterSemitone = prm.quarterSemitone;
        BinRec max;
        max.index = 1;
        max.value = fmax(prm.threshold * double(N) / 6.0, mag(1));
        max.offset = quadDelta(1);
        uint32_t start = 2;
        while (start < (N >> 1)) {
            const uint32_t i = start + uint32_t(lane);
            const bool cand = i < (N >> 1) && invHysteresis * mag(i) > max.value * 2;      // candidate must be vastly better
            const unsigned long long mask = __ballot(cand);
            if (!mask) { start += 64; continue; }
            const uint32_t k = start + uint32_t(__ffsll((long long)mask) - 1);
            BinRec current{k, mag(k), 0.0};
            if (recOmega(max) > 0) {
                current.offset = quadDelta(k);
                const double factor = recOmega(current) / recOmega(max);
                const double sensivity = current.value / max.value;
                if (invHysteresis * sensivity > 20) max = current;
                else if (fabs(1 - factor) < invHysteresis * quarterSemitone) max = current;
                else {
                    const double multipleDeviation = fabs(factor - floor(factor + 0.5));
                    if (invHysteresis * fabs(multipleDeviation) > quarterSemitone) max = current;
                }
            } else {
                max = current;
                max.offset = quadDelta(uint32_t(max.index));
            }
            start = k + 1;
        }
        if (lane == 0) {                                   // the median of 8 (:183-214)
            BinRec localMedian[8];
            for (int i = 0; i < 8; ++i) localMedian[i] = st->median[i];
            st->median[st->medianPos] = max;
            st->medianPos = (st->medianPos + 1) & 7ull;
            nthElementByIndex(localMedian, 8, 4);
            const BinRec oldMedianBin = localMedian[4];
            if (oldMedianBin.index != ~0ull && fabs(recOmega(max) - recOmega(oldMedianBin)) > 0.5) max = oldMedianBin;
            double fundamental = prm.sampleRate * recOmega(max) / double(N);
            settle(max, fmax(5.0, fundamental));
        }
    }
    }
    __syncthreads();
    {   // cpl::dsp::goertzel: z = s[N-1] - exp(-i w) s[N-2] = sum_n x[n] exp(i w (N - 1 - n)) (oracle/scope_spectral.c); evaluated as the
        // sum, all threads, fp64
        const double radians = sRadians;
        const long offset = sOffset2;
        double zr = 0, zi = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t n = uint32_t(tid) + 1024u * j;
            const double x = evalD(prm.ringA, prm.ringB, prm.evalMode, logicalPhys(-offset + long(n), cursor, cap, len));
            double sn, cs;
            sincos(radians * double(N - 1 - n), &sn, &cs);
            zr += x * cs; zi += x * sn;
        }
        for (int o = 32; o > 0; o >>= 1) { zr += __shfl_xor(zr, o); zi += __shfl_xor(zi, o); }
        if ((tid & 63) == 0) { sRed[0][tid >> 6] = zr; sRed[1][tid >> 6] = zi; }
    }
    __syncthreads();
    if (tid == 0) {
        double zr = 0, zi = 0;
        for (int w = 0; w < 16; ++w) { zr += sRed[0][w]; zi += sRed[1][w]; }
        const double tau = 6.283185307179586476925286766559;
        const double rotation = -sSampleDifference * sRadians;              // :272-278
        const double cr = cos(rotation), ci = -sin(rotation);
        const double wr = zr * cr - zi * ci, wi = zr * ci + zi * cr;
        double phase = tau - atan2(wi, wr);
        phase += st->record.offset * tau;
        phase -= 1.5707963267948966192313216916398;
        phase += tau * prm.phaseOffsetDeg / 360;
        phase = fmod(phase, tau);
        while (phase < 0) phase += tau;
        st->phase = phase;
        const double cycles = phase / tau;
        st->sampleOffset = cycles * prm.sampleRate / st->fundamental - 1;
        // resizeAudioStorage(Spectral) for this frame (ChannelData.h:113-117)
        const unsigned long long need = (unsigned long long)(0.5 + st->cycleSamples + ceil(windowSize));
        st->ringSize = need > N ? need : N;
        st->effectiveWindow = windowSize;
    }
}

}  // namespace

struct sgz_scope : BatchFront {                // (rt_common.hpp: stream, staging, routing, push lock, options)
    sgz_scope_config cfg{};
    ScopeDev *d_state = nullptr;
    unsigned long long *d_peaks = nullptr;
    Swap *d_swaps = nullptr;
    float *d_front = nullptr, *d_back = nullptr;
    uint32_t size = 0, backCap = 0;
    uint32_t trigSeparate = 0, trigPair = 0;
    float envelopeCoeff = 0.f;
    // frequency colouring (colour_by_frequency)
    ColourParams col{};
    ColourParams *d_col = nullptr;               // device copy of `col`, what the ingest kernel reads
    // Spectral triggering
    SpectralDev *d_spectral = nullptr;
    double2 *d_tw = nullptr;
    std::atomic<long long> transport{0};                 // cs.transportPosition (OscilloscopeDSP.inl:706): TriggeringMode::Window places the window by it
    std::atomic<double> tempo{0.0};                       // cs.bpm (OscilloscopeDSP.inl:707): SGZ_TIME_BEATS reads it at the frame boundary
    bool spectralFresh = false;                           // the Spectral state was reset and no frame has been analysed since
    sgz_trigger_state trig{};                             // triggerState as of the last sgz_scope_analyse (consumer thread)
    double effWindow = 0;                                 // state.effectiveWindowSize of the current frame (consumer thread)
    // vertex output (consumer side)
    float *d_xyz = nullptr; uint32_t *d_rgba = nullptr; size_t vertexCap = 0;
    void *h_out = nullptr; size_t hOutBytes = 0;          // pinned
    void *d_dense = nullptr; size_t denseBytes = 0;       // partial records of the dense stream's long columns (scope_dense.hip)
};

static void scopeFree(sgz_scope *s)
{
    if (!s) return;
    s->release([s] {
        for (void *p : {(void *)s->d_state, (void *)s->d_peaks, (void *)s->d_swaps, (void *)s->d_front, (void *)s->d_back, (void *)s->d_xyz,
                        (void *)s->d_rgba, (void *)s->col.st, (void *)s->col.bands, (void *)s->col.sm, (void *)s->col.block, (void *)s->col.front,
                        (void *)s->col.back, (void *)s->d_spectral, (void *)s->d_tw, (void *)s->d_col, s->d_dense})
            if (p) (void)hipFree(p);
        if (s->h_out) (void)hipHostFree(s->h_out);
    });
    delete s;
}

// handleFlagUpdates' window step, Oscilloscope.cpp:293-307 (the Cycles branch also runs in scopeSpectralKernel, the same fp64 expression)
static double timeWindow(uint32_t mode, double value, double sampleRate, double bpm, double cycleSamples)
{
    if (mode == SGZ_TIME_BEATS) return std::max(sampleRate * (60 / (std::max(10.0, bpm) * value)), 128.0);
    if (mode == SGZ_TIME_CYCLES) return value * cycleSamples + 1;
    return value;
}

// The largest effectiveWindowSize a configuration can reach, and (Spectral) the largest cycleSamples: what the rings are allocated for.
// Cycles: cycleSamples <= sampleRate / 5 (the fundamental's floor, calculateFundamentalPeriod) or sampleRate / custom frequency;
// Beats: the 10 BPM floor.  (The same operations as the per-frame values: a correctly rounded division and product are monotone.)
static double scopeMaxCycleSamples(const sgz_scope_config *c)
{
    return c->sample_rate / (c->custom_trigger ? std::min(5.0, c->custom_trigger_frequency) : 5.0);
}
static double scopeMaxWindow(const sgz_scope_config *c)
{
    if (c->time_mode == SGZ_TIME_CYCLES) return timeWindow(SGZ_TIME_CYCLES, c->window_size, c->sample_rate, 0.0, scopeMaxCycleSamples(c));
    if (c->time_mode == SGZ_TIME_BEATS) return timeWindow(SGZ_TIME_BEATS, c->window_size, c->sample_rate, 0.0, 0.0);
    return c->window_size;
}

static sgz_status scopeValidate(const sgz_scope_config *c)
{
    if (!(c->sample_rate >= 1) || !std::isfinite(c->sample_rate)) return fail(SGZ_EINVAL, "sample_rate");
    if (!std::isfinite(c->window_size) || c->window_size < 0 || c->window_size > double(1u << 26)) return fail(SGZ_EINVAL, "window_size");
    if (c->num_channels < 2 || (c->num_channels & 1) || c->num_channels > kMaxCh)
        return fail(SGZ_EINVAL, "num_channels must be even, 2..64 (OscilloscopeDSP.inl:318)");
    if (c->trigger_mode > SGZ_TRIG_ZERO_CROSSING) return fail(SGZ_EINVAL, "trigger_mode");
    if (c->trigger_mode == SGZ_TRIG_ENVELOPE_HOLD && (!(c->trigger_hysteresis >= 0) || !std::isfinite(c->trigger_hysteresis)))
        return fail(SGZ_EINVAL, "trigger_hysteresis");
    if (c->trigger_mode == SGZ_TRIG_SPECTRAL) {
        if (!(c->trigger_hysteresis >= 0) || !(c->trigger_hysteresis <= 1)) return fail(SGZ_EINVAL, "trigger_hysteresis outside 0..1");
        if (!std::isfinite(c->trigger_phase_offset)) return fail(SGZ_EINVAL, "trigger_phase_offset");
        if (c->custom_trigger && (!(c->custom_trigger_frequency > 0) || !(c->custom_trigger_frequency < c->sample_rate * 0.5)))
            return fail(SGZ_EINVAL, "custom_trigger_frequency must lie in (0, sample_rate / 2)");
        if (c->sample_rate / 5.0 + c->window_size > double(1u << 26)) return fail(SGZ_EINVAL, "ring too long");
    }
    if (c->colour_by_frequency) {
        if (!(c->frequency_colouring_blend >= 0) || !(c->frequency_colouring_blend <= 1)) return fail(SGZ_EINVAL, "frequency_colouring_blend");
        if (!(c->colour_smoothing_ms >= 0) || !std::isfinite(c->colour_smoothing_ms)) return fail(SGZ_EINVAL, "colour_smoothing_ms");
        if (!(c->sample_rate > 2 * 3000.0)) return fail(SGZ_EINVAL, "frequency colouring needs a sample rate above 6 kHz (crossovers at 300 / 3000 Hz)");
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) if (!std::isfinite(c->band_colours[i][j])) return fail(SGZ_EINVAL, "band_colours");
    }
    if (c->channel_mode > SGZ_OSC_MIDSIDE || c->envelope_mode > SGZ_ENV_PEAK_DECAY) return fail(SGZ_EINVAL, "enum value");
    if (c->interpolation > SGZ_SUBSAMPLE_LANCZOS) return fail(SGZ_EINVAL, "interpolation");
    if (!std::isfinite(c->trigger_threshold) || !std::isfinite(c->trigger_channel) || !(c->trigger_channel >= 1)) return fail(SGZ_EINVAL, "trigger");
    if (!std::isfinite(c->envelope_window) || c->envelope_window < 0) return fail(SGZ_EINVAL, "envelope_window");
    if (c->max_block > (1u << 17)) return fail(SGZ_EINVAL, "max_block above 131072 samples");
    if (c->time_mode > SGZ_TIME_BEATS) return fail(SGZ_EINVAL, "time_mode");
    if (c->time_mode != SGZ_TIME_TIME) {
        // checkAndInformInvalidCombinations (OscilloscopeRendering.cpp:244-259) draws nothing but its message for these
        if (c->time_mode == SGZ_TIME_CYCLES && c->trigger_mode != SGZ_TRIG_SPECTRAL)
            return fail(SGZ_EINVAL, "Invalid combination of time and triggering modes (Cycles needs the Spectral trigger)");
        if (!(c->window_size > 0)) return fail(SGZ_EINVAL, "window_size must be > 0 in the Cycles and Beats time modes");
        const double maxWindow = scopeMaxWindow(c);
        const double ring = c->trigger_mode == SGZ_TRIG_SPECTRAL ? scopeMaxCycleSamples(c) + maxWindow : maxWindow;
        if (!(ring <= double(1u << 26))) return fail(SGZ_EINVAL, "ring too long for the largest window of the time mode");
    }
    return SGZ_OK;
}

// (re)allocates everything for a configuration; the device state starts as make_unique<TriggeringProcessor>() leaves it (zeroes)
// followed by setSettings(mode, window, threshold, hysteresis) (Oscilloscope.cpp:310).
// retime (SGZ_TIME_BEATS, another trigger than Spectral: sgz_scope_analyse found the frame's window changed): the same with
// effectiveWindowSize = *retime and the rest of the configuration as it is -- the routing of sgz_scope_set_mix and the staging stay.
static sgz_status scopeSetup(sgz_scope *s, const sgz_scope_config *cfg, bool fresh, const double *retime = nullptr)
{
    sgz_status st = scopeValidate(cfg);
    if (st != SGZ_OK) return st;
    if (!s->stream) SGZ_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    SGZ_HIP(hipStreamSynchronize(s->stream));
    const uint32_t C = cfg->num_channels;
    const bool spectral = cfg->trigger_mode == SGZ_TRIG_SPECTRAL;
    // state.effectiveWindowSize (handleFlagUpdates' window step; Cycles: with the cycleSamples the Spectral state keeps, set below).
    // A configure that leaves the time mode and its value as they are keeps the frame's window: the next analyse moves it.
    const bool keepFrame = !fresh && !retime && cfg->time_mode != SGZ_TIME_TIME && cfg->time_mode == s->cfg.time_mode &&
                           cfg->window_size == s->cfg.window_size && cfg->sample_rate == s->cfg.sample_rate;
    double window = retime ? *retime : keepFrame ? s->effWindow
                  : timeWindow(cfg->time_mode, cfg->window_size, cfg->sample_rate, s->tempo.load(std::memory_order_relaxed), 0.0);
    // ChannelData::resizeAudioStorage (ChannelData.h:107-128).  Spectral: the largest ring the reference can ask for (5 Hz floor of the
    // fundamental); the reference's ring of the frame is cut out of it by the readers (sgz_trigger_state::ring_size).  Cycles / Beats:
    // for the largest window the time mode can reach, so that a new window never reallocates
    uint32_t size = uint32_t(std::ceil(window + 1));                                  // :121
    if (spectral && cfg->time_mode == SGZ_TIME_TIME)
        size = uint32_t(std::max<size_t>(size_t(0.5 + cfg->sample_rate / 5.0 + std::ceil(cfg->window_size)), 8192));
    else if (spectral)
        size = uint32_t(std::max<size_t>(size_t(0.5 + scopeMaxCycleSamples(cfg) + std::ceil(scopeMaxWindow(cfg))), 8192));
    uint32_t backCap = 1; while (backCap < size) backCap <<= 1;
    const uint32_t maxBlock = cfg->max_block ? cfg->max_block : 8192u;
    const bool colours = cfg->colour_by_frequency != 0;
    const bool realloc = fresh || C != s->cfg.num_channels || size != s->size || maxBlock != s->maxBlock ||
                         colours != (s->cfg.colour_by_frequency != 0);
    ScopeDev h{};
    if (!fresh) SGZ_HIP(hipMemcpy(&h, s->d_state, sizeof(h), hipMemcpyDeviceToHost));
    if (realloc) {
        for (void **p : {(void **)&s->d_front, (void **)&s->d_back}) if (*p) { (void)hipFree(*p); *p = nullptr; }
        SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_front), size_t(C) * size * sizeof(float)));
        SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_back), size_t(C) * backCap * sizeof(float)));
        SGZ_HIP(hipMemset(s->d_front, 0, size_t(C) * size * sizeof(float)));
        SGZ_HIP(hipMemset(s->d_back, 0, size_t(C) * backCap * sizeof(float)));
        if (!retime && (st = s->staging(C, cfg->sample_rate, maxBlock)) != SGZ_OK) return st;     // (s->maxBlock = maxBlock once the slots are there)
        if (!s->d_state) {
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_state), sizeof(ScopeDev)));
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_peaks), size_t(kPeakCap) * sizeof(unsigned long long)));
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_swaps), size_t(kMaxSwaps) * sizeof(Swap)));
        }
        h.frontCursor = 0; h.written = 0;
        for (void **p : {(void **)&s->col.st, (void **)&s->col.bands, (void **)&s->col.sm, (void **)&s->col.block, (void **)&s->col.front,
                         (void **)&s->col.back})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        if (colours) {
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->col.st), sizeof(ColourDev)));
            SGZ_HIP(hipMemset(s->col.st, 0, sizeof(ColourDev)));
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->col.bands), size_t(C) * 4 * maxBlock * sizeof(float)));
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->col.sm), size_t(C) * 6 * maxBlock * sizeof(float)));
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->col.block), size_t(C) * 2 * maxBlock * sizeof(uint32_t)));
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->col.front), size_t(C) * 2 * size * sizeof(uint32_t)));
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->col.back), size_t(C) * 2 * backCap * sizeof(uint32_t)));
            SGZ_HIP(hipMemset(s->col.front, 0, size_t(C) * 2 * size * sizeof(uint32_t)));
            SGZ_HIP(hipMemset(s->col.back, 0, size_t(C) * 2 * backCap * sizeof(uint32_t)));
        }
        s->col.maxBlock = maxBlock;
    }
    if (!retime) {
        if (s->batch.channels != C)           // a configure after sgz_scope_set_mix: the staging takes num_channels rows again
            if ((st = s->staging(C, cfg->sample_rate, s->maxBlock)) != SGZ_OK) return st;
        s->mix.reset(C);                      // the routing returns to the identity over num_channels
    }
    if (colours) {
        // tuneCrossOver(300, 3000, sampleRate), tuneColourSmoothing(ms, sampleRate) (ChannelData.h:163-171).  cpl's designs are not in the
        // reference tree: the 3-band Linkwitz-Riley tree and the one-pole design are the published ones (oracle/scope_spectral.c)
        auto butterworth = [](double fnorm, bool highpass, float *c) {
            const double w0 = 6.283185307179586476925286766559 * fnorm;
            const double cw = std::cos(w0), alpha = std::sin(w0) / (2.0 * 0.70710678118654752440);
            const double a0 = 1 + alpha;
            double b0, b1;
            if (highpass) { b0 = (1 + cw) / 2; b1 = -(1 + cw); }
            else { b0 = (1 - cw) / 2; b1 = 1 - cw; }
            c[0] = float(b0 / a0); c[1] = float(b1 / a0); c[2] = float(b0 / a0);
            c[3] = float(-2 * cw / a0); c[4] = float((1 - alpha) / a0);
        };
        const float f1 = float(300.0 / cfg->sample_rate), f2 = float(3000.0 / cfg->sample_rate);
        butterworth(double(f1), false, s->col.lp1); butterworth(double(f1), true, s->col.hp1);
        butterworth(double(f2), false, s->col.lp2); butterworth(double(f2), true, s->col.hp2);
        s->col.pole = float(std::exp(-1.0 / (cfg->colour_smoothing_ms / 1000.0 * cfg->sample_rate)));
        s->col.blend = 1 - cfg->frequency_colouring_blend;                               // OscilloscopeDSP.inl:515
        std::memcpy(s->col.band, cfg->band_colours, sizeof(s->col.band));
        for (uint32_t c = 0; c < C; ++c) std::memcpy(&s->col.keys[c], cfg->colours[c], 4);
    }
    if (cfg->trigger_mode == SGZ_TRIG_SPECTRAL) {
        if (!s->d_tw) {
            std::vector<double2> tw(4096);
            for (int k = 0; k < 4096; ++k) {
                const double a = -6.283185307179586476925286766559 * double(k) / 8192.0;
                tw[k] = make_double2(std::cos(a), std::sin(a));
            }
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_tw), sizeof(double2) * 4096));
            SGZ_HIP(hipMemcpy(s->d_tw, tw.data(), sizeof(double2) * 4096, hipMemcpyHostToDevice));
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_spectral), sizeof(SpectralDev)));
            SGZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(scopeSpectralKernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        2 * 8192 * int(sizeof(double))));
        }
        if (realloc || s->cfg.trigger_mode != SGZ_TRIG_SPECTRAL) {
            if (cfg->time_mode == SGZ_TIME_CYCLES) window = timeWindow(SGZ_TIME_CYCLES, cfg->window_size, cfg->sample_rate, 0.0, 0.0);
            SpectralDev sd{};                                                             // Oscilloscope(): medianPos(), value-initialised filter
            sd.ringSize = std::max<size_t>(size_t(0.5 + 0.0 + std::ceil(window)), 8192);
            sd.effectiveWindow = window;
            SGZ_HIP(hipMemcpy(s->d_spectral, &sd, sizeof(sd), hipMemcpyHostToDevice));
            s->trig = sgz_trigger_state{};
            s->trig.ring_size = sd.ringSize;
            s->spectralFresh = true;
        } else if (cfg->time_mode == SGZ_TIME_CYCLES && !keepFrame) {
            window = timeWindow(SGZ_TIME_CYCLES, cfg->window_size, cfg->sample_rate, 0.0, s->trig.cycle_samples);   // (the state kept)
        }
    } else {
        s->trig = sgz_trigger_state{};
        s->trig.ring_size = size;
        if (cfg->trigger_mode == SGZ_TRIG_ZERO_CROSSING || cfg->trigger_mode == SGZ_TRIG_ENVELOPE_HOLD)   // calculateTriggeringOffset :233-240
            s->trig.sample_offset = (window * 0.5 - double(int(window * 0.5))) - 1.5;
    }
    // TriggeringProcessor::setSettings, StreamPreprocessing.h:46-53.  Rings reallocated here (or by an earlier call that no block has
    // seen yet: the flag still pending) start over at written = 0, so update() must reset what processMutating has buffered -- the
    // reference's assignment would drop a pending flag on a second call with the same ceil, and the next swap would then address
    // bufferedSamples behind a ring that no longer holds them
    h.windowChanged = (std::ceil(window) != std::ceil(h.windowSize) || (!fresh && (realloc || h.windowChanged))) ? 1 : 0;
    h.windowSize = window;
    h.threshold = cfg->trigger_threshold;
    h.hysteresis = cfg->trigger_hysteresis;
    SGZ_HIP(hipMemcpy(s->d_state, &h, sizeof(h), hipMemcpyHostToDevice));
    s->size = size; s->backCap = backCap;
    // calculateTriggerIndices, OscilloscopeParameters.h:491-507
    const size_t idx = size_t(std::llround(cfg->trigger_channel - 1));
    s->trigSeparate = uint32_t(std::min<size_t>(C - 1, idx));
    s->trigPair = uint32_t(std::min<size_t>(C / 4, idx) * 2);
    s->envelopeCoeff = float(std::exp(-1.0 / (cfg->envelope_window * cfg->sample_rate)));   // OscilloscopeDSP.inl:448
    if (!s->d_col) SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_col), sizeof(ColourParams)));
    SGZ_HIP(hipStreamSynchronize(s->stream));                                               // (no ingest launch is reading the old copy)
    SGZ_HIP(hipMemcpy(s->d_col, &s->col, sizeof(ColourParams), hipMemcpyHostToDevice));
    s->cfg = *cfg;
    s->effWindow = window;
    return SGZ_OK;
}

extern "C" {

#ifdef SGZ_DEBUG
sgz_status sgz_debug_ingest_clocks(unsigned long long *out8)
{
    SGZ_HIP(hipDeviceSynchronize());
    SGZ_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_ingestClk), 8 * sizeof(unsigned long long)));
    return SGZ_OK;
}
#endif

sgz_status sgz_scope_create(const sgz_scope_config *cfg, sgz_scope **out)
{
    if (!cfg || !out) return fail(SGZ_EINVAL, "null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(SGZ_EHIP, "no HIP device visible (libsgz has no CPU fallback)");
    sgz_scope *s = new (std::nothrow) sgz_scope();
    if (!s) return fail(SGZ_ENOMEM, "out of memory");
    const sgz_status st = scopeSetup(s, cfg, true);
    if (st != SGZ_OK) { scopeFree(s); return st; }
    *out = s;
    return SGZ_OK;
}

void sgz_scope_destroy(sgz_scope *s) { scopeFree(s); }

static sgz_status scopeSync(sgz_scope *s);

sgz_status sgz_scope_configure(sgz_scope *s, const sgz_scope_config *cfg)
{
    if (!s || !cfg) return fail(SGZ_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    if (sgz_status sy = scopeSync(s); sy != SGZ_OK) return sy;            // the audio already taken goes through the old configuration
    return scopeSetup(s, cfg, false);
}

// the open batch -> GPU: one staged copy, one launch of the ingest kernel over its blocks (caller holds the batch flag; count > 0)
static sgz_status scopeSubmit(sgz_scope *s, const PeakParams *peak = nullptr)
{
    sgz_status st;
    const float *fetchFrom; uint32_t floats;
    const float *d_batch = s->batch.upload(s->stream, &st, &fetchFrom, &floats);
    if (!d_batch) return st;
    IngestParams prm{};
    s->fill(prm.in, d_batch, fetchFrom, floats, s->cfg.num_channels);
    prm.st = s->d_state; prm.peaks = s->d_peaks; prm.swapList = s->d_swaps;
    prm.front = s->d_front; prm.size = s->size; prm.back = s->d_back; prm.backCap = s->backCap;
    prm.triggerMode = s->cfg.trigger_mode; prm.oscMode = s->cfg.channel_mode; prm.envMode = s->cfg.envelope_mode;
    prm.trigSeparate = s->trigSeparate; prm.trigPair = s->trigPair; prm.envelopeCoeff = s->envelopeCoeff;
    prm.colours = s->cfg.colour_by_frequency ? 1u : 0u;
    if (peak) { prm.doPeak = 1u; prm.peak = *peak; }
    hipLaunchKernelGGL(scopeIngestKernel, dim3(1), dim3(1024), 0, s->stream, prm, s->d_col);
    SGZ_HIP(hipGetLastError());
    return s->batch.commit(s->stream);
}

static auto scopeSubmitter(sgz_scope *s) { return [s] { return scopeSubmit(s); }; }

// consumer side (flush on read): what waits in the host FIFO and in the open batch goes to the GPU in front of the caller's own work
static sgz_status scopeSync(sgz_scope *s) { return s->sync(scopeSubmitter(s)); }

sgz_status sgz_scope_push(sgz_scope *s, const float *const *planar, uint32_t num_channels, uint32_t nsamples)
{
    return s ? s->push(scopeSubmitter(s), planar, num_channels, nsamples, "scope") : fail(SGZ_EINVAL, "null argument");
}

sgz_status sgz_scope_set_mix(sgz_scope *s, uint32_t num_sources, const uint8_t *matrix)
{
    return s ? s->setMix(num_sources, s->cfg.num_channels, s->cfg.sample_rate, matrix, scopeSubmitter(s)) : fail(SGZ_EINVAL, "bad argument");
}

void *sgz_scope_stream(sgz_scope *s) { return s ? s->stream : nullptr; }

sgz_status sgz_scope_set_option(sgz_scope *s, uint32_t option, uint64_t value)
{
    return s ? s->setOption(option, value, "scope") : fail(SGZ_EINVAL, "null handle");
}

sgz_status sgz_scope_flush(sgz_scope *s) { return s ? s->flush(scopeSubmitter(s)) : fail(SGZ_EINVAL, "null handle"); }

sgz_status sgz_scope_peak_filter(sgz_scope *s, double delta_time, uint32_t lanes, double *auto_gain)
{
    if (!s || lanes == 0 || (lanes & (lanes - 1))) return fail(SGZ_EINVAL, "bad argument");
    // coeff = pow(exp(-lanes / (envelopeWindow * sampleRate)), numSamples * dt), OscilloscopeDSP.inl:745-747
    const bool spectral = s->cfg.trigger_mode == SGZ_TRIG_SPECTRAL;
    const uint32_t numSamples = spectral ? uint32_t(s->trig.ring_size) : s->size;          // audioData.getSize()
    const double power = double(numSamples) * delta_time;
    const double coeff = std::pow(std::exp(-double(lanes) / (s->cfg.envelope_window * s->cfg.sample_rate)), power);
    PeakParams prm{s->d_state, s->d_front, s->size, s->cfg.num_channels, s->cfg.channel_mode, lanes, coeff, spectral ? numSamples : 0u};
    // flush on read: the blocks that wait in the open batch come first -- and the filter rides on their launch (one workgroup either
    // way: a launch and the gap in front of it less per rendered frame)
    auto submit = scopeSubmitter(s);
    auto side = s->side(submit);
    s->batch.lock();
    const sgz_status tb = batchTakeBacklog(side, false);
    const bool fused = tb == SGZ_OK && s->batch.count != 0;
    const sgz_status sy = tb != SGZ_OK ? tb : fused ? scopeSubmit(s, &prm) : SGZ_OK;
    s->batch.unlock();
    if (sy != SGZ_OK) return sy;
    if (!fused) {
        hipLaunchKernelGGL(scopePeakKernel, dim3(1), dim3(1024), 0, s->stream, prm);
        SGZ_HIP(hipGetLastError());
    }
    if (auto_gain) {
        SGZ_HIP(hipMemcpyAsync(auto_gain, reinterpret_cast<const char *>(s->d_state) + offsetof(ScopeDev, autoGain), sizeof(double),
                               hipMemcpyDeviceToHost, s->stream));
        SGZ_HIP(hipStreamSynchronize(s->stream));
    }
    return SGZ_OK;
}

sgz_status sgz_scope_gains(sgz_scope *s, double *envelope_gain, float *envelopes)
{
    if (!s) return fail(SGZ_EINVAL, "null handle");
    if (sgz_status sy = scopeSync(s); sy != SGZ_OK) return sy;            // (flush on read: the blocks that wait in the open batch come first)
    ScopeDev h;
    SGZ_HIP(hipMemcpyAsync(&h, s->d_state, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    SGZ_HIP(hipStreamSynchronize(s->stream));
    if (envelope_gain) *envelope_gain = h.envelopeGain;
    if (envelopes) std::memcpy(envelopes, h.envelope, sizeof(float) * s->cfg.num_channels);
    return SGZ_OK;
}

sgz_status sgz_scope_front(sgz_scope *s, uint32_t channel, float *out, uint32_t *size, uint32_t *cursor)
{
    if (!s || channel >= s->cfg.num_channels) return fail(SGZ_EINVAL, "bad argument");
    if (sgz_status sy = scopeSync(s); sy != SGZ_OK) return sy;            // (flush on read: the blocks that wait in the open batch come first)
    ScopeDev h;
    if (out) SGZ_HIP(hipMemcpyAsync(out, s->d_front + size_t(channel) * s->size, size_t(s->size) * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    SGZ_HIP(hipMemcpyAsync(&h, s->d_state, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    SGZ_HIP(hipStreamSynchronize(s->stream));
    if (size) *size = s->size;
    if (cursor) *cursor = h.frontCursor;
    return SGZ_OK;
}

sgz_status sgz_scope_front_colours(sgz_scope *s, uint32_t channel, uint32_t aux, uint8_t *out)
{
    if (!s || !out || channel >= s->cfg.num_channels || aux > 1) return fail(SGZ_EINVAL, "bad argument");
    if (!s->cfg.colour_by_frequency) return fail(SGZ_EINVAL, "colour_by_frequency is off");
    if (sgz_status sy = scopeSync(s); sy != SGZ_OK) return sy;            // (flush on read: the blocks that wait in the open batch come first)
    const size_t plane = size_t(aux ? s->cfg.num_channels : 0u) + channel;
    SGZ_HIP(hipMemcpyAsync(out, s->col.front + plane * s->size, size_t(s->size) * 4, hipMemcpyDeviceToHost, s->stream));
    SGZ_HIP(hipStreamSynchronize(s->stream));
    return SGZ_OK;
}

#ifdef SGZ_DEBUG
// (debug builds: the spectral trigger's median ring, 8 x (index, value, offset) as doubles)
sgz_status sgz_scope_debug_median(sgz_scope *s, double out[24])
{
    SpectralDev h;
    SGZ_HIP(hipMemcpyAsync(&h, s->d_spectral, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    SGZ_HIP(hipStreamSynchronize(s->stream));
    for (int i = 0; i < 8; ++i) { out[3 * i] = double(h.median[i].index); out[3 * i + 1] = h.median[i].value; out[3 * i + 2] = h.median[i].offset; }
    return SGZ_OK;
}
#endif

sgz_status sgz_scope_debug_state(sgz_scope *s, uint64_t out[8])
{
    if (!s || !out) return fail(SGZ_EINVAL, "null argument");
    if (sgz_status sy = scopeSync(s); sy != SGZ_OK) return sy;            // (flush on read: the blocks that wait in the open batch come first)
    ScopeDev h;
    SGZ_HIP(hipMemcpyAsync(&h, s->d_state, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    SGZ_HIP(hipStreamSynchronize(s->stream));
    out[0] = h.frontOrigin; out[1] = h.bufferedSamples; out[2] = h.oldPeak; out[3] = h.currentPeak;
    out[4] = h.steadyClock; out[5] = h.qCount; out[6] = uint64_t(h.isWorkingOnPeak); out[7] = h.swaps;
    return SGZ_OK;
}

sgz_status sgz_scope_set_transport(sgz_scope *s, int64_t position_in_samples)
{
    if (!s) return fail(SGZ_EINVAL, "null handle");
    s->transport.store(position_in_samples, std::memory_order_relaxed);
    return SGZ_OK;
}

sgz_status sgz_scope_set_tempo(sgz_scope *s, double bpm)
{
    if (!s) return fail(SGZ_EINVAL, "null handle");
    s->tempo.store(bpm, std::memory_order_relaxed);
    return SGZ_OK;
}

double sgz_scope_effective_window(const sgz_scope *s) { return s ? s->effWindow : 0.0; }

double sgz_scope_time_window(uint32_t time_mode, double value, double sample_rate, double bpm, double cycle_samples)
{
    return timeWindow(time_mode, value, sample_rate, bpm, cycle_samples);
}

size_t sgz_scope_vertex_count(const sgz_scope *s, const sgz_scope_view *view)
{
    if (!s || !view || view->width < 2 || !(view->right > view->left)) return 0;
    sgz_scope_view v = *view;
    v.window_size = s->effWindow;
    return scopeVertexCount(v, s->cfg.interpolation, s->cfg.trigger_mode, s->trig.cycle_samples);
}

sgz_status sgz_scope_analyse(sgz_scope *s, uint32_t evaluator, uint32_t channel, sgz_trigger_state *out)
{
    if (!s) return fail(SGZ_EINVAL, "null handle");
    const bool spectral = s->cfg.trigger_mode == SGZ_TRIG_SPECTRAL;
    if (s->cfg.time_mode == SGZ_TIME_BEATS && !spectral) {
        // handleFlagUpdates at the frame boundary: a new tempo's window goes through setSettings and resizeAudioStorage as a
        // configure with that window would (the blocks taken so far through the old one; a push meanwhile is refused with SGZ_BUSY)
        const double window = timeWindow(SGZ_TIME_BEATS, s->cfg.window_size, s->cfg.sample_rate, s->tempo.load(std::memory_order_relaxed), 0.0);
        if (window != s->effWindow) {
            std::lock_guard<std::mutex> lk(s->mu);
            if (sgz_status sy = scopeSync(s); sy != SGZ_OK) return sy;
            if (sgz_status st = scopeSetup(s, &s->cfg, false, &window); st != SGZ_OK) return st;
        }
    }
    if (sgz_status sy = scopeSync(s); sy != SGZ_OK) return sy;            // (flush on read: the blocks that wait in the open batch come first)
    if (spectral) {
        const uint32_t C = s->cfg.num_channels;
        uint32_t chA, chB, evalMode;
        switch (evaluator) {
        case SGZ_OSC_LEFT: chA = chB = channel; evalMode = 0; break;
        case SGZ_OSC_RIGHT: chA = chB = channel + 1; evalMode = 0; break;
        case SGZ_OSC_MID: chA = channel; chB = channel + 1; evalMode = 1; break;
        case SGZ_OSC_SIDE: chA = channel; chB = channel + 1; evalMode = 2; break;
        default: return fail(SGZ_EINVAL, "evaluator: SGZ_OSC_LEFT / RIGHT / MID / SIDE");
        }
        if (chA >= C || chB >= C) return fail(SGZ_EINVAL, "channel out of range");
        SpectralParams prm{};
        prm.st = s->d_spectral;
        prm.ringA = s->d_front + size_t(chA) * s->size; prm.ringB = s->d_front + size_t(chB) * s->size;
        prm.evalMode = evalMode; prm.cap = s->size;
        prm.d_cursor = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(s->d_state) + offsetof(ScopeDev, frontCursor));
        // the frame's window: Cycles computes it inside the kernel from the cycleSamples it keeps, Beats from the tempo of the moment
        prm.windowSize = timeWindow(s->cfg.time_mode, s->cfg.window_size, s->cfg.sample_rate, s->tempo.load(std::memory_order_relaxed), 0.0);
        prm.cycles = s->cfg.time_mode == SGZ_TIME_CYCLES ? s->cfg.window_size : 0.0;
        // Beats: before the first frame the reference's ring is the one the first frame's window asks for (as a Time handle created
        // with that window has it), whatever the tempo was when the state was set up
        if (s->cfg.time_mode != SGZ_TIME_TIME) prm.trig = s->d_state;
        if (s->cfg.time_mode == SGZ_TIME_BEATS && s->spectralFresh)
            prm.firstRing = std::max<size_t>(size_t(0.5 + 0.0 + std::ceil(prm.windowSize)), 8192);
        prm.sampleRate = s->cfg.sample_rate;
        prm.threshold = s->cfg.trigger_threshold; prm.hysteresis = s->cfg.trigger_hysteresis;
        prm.customFrequency = s->cfg.custom_trigger ? s->cfg.custom_trigger_frequency : 0.0;
        prm.phaseOffsetDeg = s->cfg.trigger_phase_offset;
        prm.quarterSemitone = std::pow(2, 0.25 / 12.0) - 1;                                  // OscilloscopeDSP.inl:126
        prm.tw = s->d_tw;
        hipLaunchKernelGGL(scopeSpectralKernel, dim3(1), dim3(1024), 2 * 8192 * sizeof(double), s->stream, prm);
        SGZ_HIP(hipGetLastError());
        SpectralDev h;
        SGZ_HIP(hipMemcpyAsync(&h, s->d_spectral, sizeof(h), hipMemcpyDeviceToHost, s->stream));
        SGZ_HIP(hipStreamSynchronize(s->stream));
        s->trig.record_index = h.record.index; s->trig.record_value = h.record.value; s->trig.record_offset = h.record.offset;
        s->trig.fundamental = h.fundamental; s->trig.cycle_samples = h.cycleSamples; s->trig.sample_offset = h.sampleOffset;
        s->trig.phase = h.phase; s->trig.ring_size = h.ringSize;
        s->effWindow = h.effectiveWindow;
        s->spectralFresh = false;
    }
    if (out) *out = s->trig;
    return SGZ_OK;
}

// one evaluator's vertex stream into DEVICE buffers (the handle's own, or the caller's mapped VBO); *points = vertices written
// what an evaluator reads: SampleColourEvaluator<OscChannels::...>, SampleColourEvaluators.h: Left / Right one channel, Mid / Side 0.5 (l +- r)
struct StripSource { const float *ringA, *ringB; const uint32_t *colRing; uint32_t evalMode, key; };
static sgz_status scopeStripSource(sgz_scope *s, uint32_t evaluator, uint32_t channel, bool wantColours, StripSource *out)
{
    const uint32_t C = s->cfg.num_channels;
    uint32_t chA, chB, evalMode, colourCh;
    switch (evaluator) {
    case SGZ_OSC_LEFT: chA = chB = channel; evalMode = 0; colourCh = channel; break;
    case SGZ_OSC_RIGHT: chA = chB = channel + 1; evalMode = 0; colourCh = channel + 1; break;
    case SGZ_OSC_MID: chA = channel; chB = channel + 1; evalMode = 1; colourCh = channel; break;
    case SGZ_OSC_SIDE: chA = channel; chB = channel + 1; evalMode = 2; colourCh = channel + 1; break;
    default: return fail(SGZ_EINVAL, "evaluator: SGZ_OSC_LEFT / RIGHT / MID / SIDE");
    }
    if (chA >= C || chB >= C) return fail(SGZ_EINVAL, "channel out of range");
    uint32_t key;
    std::memcpy(&key, s->cfg.colours[colourCh], 4);                    // evaluator.getDefaultKey()
    // colourChannelsByFrequency: Left / Right read colourData of their channel, Mid / Side auxColourData (SampleColourEvaluators.h:64,183)
    const uint32_t *colRing = nullptr;
    if (s->cfg.colour_by_frequency && wantColours)
        colRing = s->col.front + size_t((evalMode == 0 ? 0u : C) + colourCh) * s->size;
    *out = StripSource{s->d_front + size_t(chA) * s->size, s->d_front + size_t(chB) * s->size, colRing, evalMode, key};
    return SGZ_OK;
}

static sgz_status scopeVerticesInto(sgz_scope *s, const sgz_scope_view *view, uint32_t evaluator, uint32_t channel, float *d_xyz,
                                    uint32_t *d_rgba, size_t capacity, size_t *points)
{
    if (sgz_status sy = scopeSync(s); sy != SGZ_OK) return sy;            // (flush on read: the blocks that wait in the open batch come first)
    StripSource src;
    if (sgz_status st = scopeStripSource(s, evaluator, channel, d_rgba != nullptr, &src); st != SGZ_OK) return st;
    sgz_scope_view v = *view;
    v.window_size = s->effWindow;                                     // state.effectiveWindowSize is the stream's (this frame's)
    SGZ_HIP(launchScopeVertices(v, s->cfg.trigger_mode, s->cfg.interpolation, src.ringA, src.ringB, src.evalMode, uint32_t(s->trig.ring_size), s->size,
                                reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(s->d_state) + offsetof(ScopeDev, frontCursor)),
                                s->trig.cycle_samples, s->trig.sample_offset, s->transport.load(std::memory_order_relaxed), src.key, src.colRing, d_xyz,
                                d_rgba, capacity, points, s->stream));
    return SGZ_OK;
}

// two strips of one view: Lanczos strips share their tap weights in ONE launch (scope_vector.hip scopeWaveLanczosKernel<2>); false: not Lanczos
static sgz_status scopeVerticesPairInto(sgz_scope *s, const sgz_scope_view *view, const uint32_t *evaluators, const uint32_t *channels,
                                        float *const d_xyz[2], uint32_t *const d_rgba[2], size_t capacity, size_t *points, bool *done)
{
    *done = false;
    if (sgz_status sy = scopeSync(s); sy != SGZ_OK) return sy;
    StripSource a, b;
    if (sgz_status st = scopeStripSource(s, evaluators[0], channels[0], d_rgba[0] != nullptr, &a); st != SGZ_OK) return st;
    if (sgz_status st = scopeStripSource(s, evaluators[1], channels[1], d_rgba[1] != nullptr, &b); st != SGZ_OK) return st;
    sgz_scope_view v = *view;
    v.window_size = s->effWindow;
    const float *ra[2] = {a.ringA, b.ringA}, *rb[2] = {a.ringB, b.ringB};
    const uint32_t em[2] = {a.evalMode, b.evalMode}, key[2] = {a.key, b.key};
    const uint32_t *cr[2] = {a.colRing, b.colRing};
    hipError_t e = hipSuccess;
    *done = launchScopeLanczosPair(v, s->cfg.trigger_mode, s->cfg.interpolation, ra, rb, em, uint32_t(s->trig.ring_size), s->size,
                                   reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(s->d_state) + offsetof(ScopeDev, frontCursor)),
                                   s->trig.cycle_samples, s->trig.sample_offset, s->transport.load(std::memory_order_relaxed), key, cr, d_xyz, d_rgba,
                                   capacity, points, s->stream, &e);
    if (*done) SGZ_HIP(e);
    return SGZ_OK;
}

// the handle's own vertex buffers (device + pinned bounce) hold `need` vertices
static sgz_status scopeReserveVertices(sgz_scope *s, size_t need)
{
    if (s->vertexCap < need) {
        if (s->d_xyz) (void)hipFree(s->d_xyz);
        if (s->d_rgba) (void)hipFree(s->d_rgba);
        if (s->h_out) (void)hipHostFree(s->h_out);
        s->d_xyz = nullptr; s->d_rgba = nullptr; s->h_out = nullptr; s->vertexCap = 0;
        SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_xyz), need * 3 * sizeof(float)));
        SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_rgba), need * sizeof(uint32_t)));
        SGZ_HIP(hipHostMalloc(&s->h_out, need * 16, hipHostMallocDefault));
        s->vertexCap = need;
    }
    return SGZ_OK;
}

sgz_status sgz_scope_vertices(sgz_scope *s, const sgz_scope_view *view, uint32_t evaluator, uint32_t channel, float *xyz, uint8_t *rgba,
                              uint32_t *count)
{
    if (!s || !view || !xyz || !count) return fail(SGZ_EINVAL, "null argument");
    if (view->width < 2 || !(view->right > view->left)) return fail(SGZ_EINVAL, "bad view");
    sgz_scope_view v = *view;
    v.window_size = s->effWindow;
    const size_t need = scopeVertexCount(v, s->cfg.interpolation, s->cfg.trigger_mode, s->trig.cycle_samples);
    if (need > *count) { *count = uint32_t(need); return fail(SGZ_EINVAL, "vertex buffer too small (count holds the required size)"); }
    if (sgz_status rs = scopeReserveVertices(s, need); rs != SGZ_OK) return rs;
    size_t points = 0;
    // pinned, device-mapped destinations: the vertex kernel writes them itself (2.4 MB per evaluator at cfg3: the DMA copy behind the
    // kernel was most of a rendered frame's GPU time)
    void *mx = mappedDevicePointer(xyz, s->stream), *mc = rgba ? mappedDevicePointer(rgba, s->stream) : nullptr;
    if (mx && (!rgba || mc)) {
        const sgz_status sd = scopeVerticesInto(s, view, evaluator, channel, static_cast<float *>(mx), static_cast<uint32_t *>(mc), need, &points);
        if (sd != SGZ_OK) return sd;
        SGZ_HIP(hipStreamSynchronize(s->stream));
        *count = uint32_t(points);
        return SGZ_OK;
    }
    const sgz_status st = scopeVerticesInto(s, view, evaluator, channel, s->d_xyz, rgba ? s->d_rgba : nullptr, need, &points);
    if (st != SGZ_OK) return st;
    if (sgz_status rb = readBack(xyz, s->d_xyz, points * 3 * sizeof(float), rgba, s->d_rgba, points * sizeof(uint32_t), s->h_out, s->stream);
        rb != SGZ_OK) return rb;
    *count = uint32_t(points);
    return SGZ_OK;
}

sgz_status sgz_scope_vertices_all(sgz_scope *s, const sgz_scope_view *view, uint32_t items, const uint32_t *evaluators, const uint32_t *channels,
                                  float *const *xyz, uint8_t *const *rgba, uint32_t *counts)
{
    if (!s || !view || !evaluators || !channels || !xyz || !counts) return fail(SGZ_EINVAL, "null argument");
    if (view->width < 2 || !(view->right > view->left)) return fail(SGZ_EINVAL, "bad view");
    sgz_scope_view v = *view;
    v.window_size = s->effWindow;
    const size_t need = scopeVertexCount(v, s->cfg.interpolation, s->cfg.trigger_mode, s->trig.cycle_samples);
    bool small = false, direct = true;
    for (uint32_t k = 0; k < items; ++k) {
        if (!xyz[k]) return fail(SGZ_EINVAL, "null argument");
        if (need > counts[k]) { counts[k] = uint32_t(need); small = true; }
        direct = direct && mappedDevicePointer(xyz[k], s->stream) && (!rgba || !rgba[k] || mappedDevicePointer(rgba[k], s->stream));
    }
    if (small) return fail(SGZ_EINVAL, "vertex buffer too small (counts hold the required size)");
    if (!direct) {                                            // a pageable buffer among them: item by item through the bounce buffer
        for (uint32_t k = 0; k < items; ++k) {
            const sgz_status st = sgz_scope_vertices(s, view, evaluators[k], channels[k], xyz[k], rgba ? rgba[k] : nullptr, &counts[k]);
            if (st != SGZ_OK) return st;
        }
        return SGZ_OK;
    }
    for (uint32_t k = 0; k < items; ++k) {
        size_t points = 0;
        if (k + 1 < items) {                                  // two strips at a time when they are Lanczos strips (shared tap weights, one launch)
            float *px[2] = {static_cast<float *>(mappedDevicePointer(xyz[k], s->stream)), static_cast<float *>(mappedDevicePointer(xyz[k + 1], s->stream))};
            uint32_t *pc[2] = {rgba && rgba[k] ? static_cast<uint32_t *>(mappedDevicePointer(rgba[k], s->stream)) : nullptr,
                               rgba && rgba[k + 1] ? static_cast<uint32_t *>(mappedDevicePointer(rgba[k + 1], s->stream)) : nullptr};
            bool done = false;
            const sgz_status sp = scopeVerticesPairInto(s, view, evaluators + k, channels + k, px, pc, need, &points, &done);
            if (sp != SGZ_OK) { (void)hipStreamSynchronize(s->stream); return sp; }
            if (done) { counts[k] = counts[k + 1] = uint32_t(points); ++k; continue; }
        }
        const sgz_status st = scopeVerticesInto(s, view, evaluators[k], channels[k], static_cast<float *>(mappedDevicePointer(xyz[k], s->stream)),
                                                rgba && rgba[k] ? static_cast<uint32_t *>(mappedDevicePointer(rgba[k], s->stream)) : nullptr, need, &points);
        if (st != SGZ_OK) { (void)hipStreamSynchronize(s->stream); return st; }
        counts[k] = uint32_t(points);
    }
    SGZ_HIP(hipStreamSynchronize(s->stream));
    return SGZ_OK;
}

sgz_status sgz_scope_vertices_device(sgz_scope *s, const sgz_scope_view *view, uint32_t evaluator, uint32_t channel, float *d_xyz,
                                     uint8_t *d_rgba, uint32_t *count)
{
    if (!s || !view || !d_xyz || !count) return fail(SGZ_EINVAL, "null argument");
    if (view->width < 2 || !(view->right > view->left)) return fail(SGZ_EINVAL, "bad view");
    if ((reinterpret_cast<uintptr_t>(d_xyz) & 3) || (reinterpret_cast<uintptr_t>(d_rgba) & 3)) return fail(SGZ_EINVAL, "4-byte aligned buffers");
    sgz_scope_view v = *view;
    v.window_size = s->effWindow;
    const size_t need = scopeVertexCount(v, s->cfg.interpolation, s->cfg.trigger_mode, s->trig.cycle_samples);
    if (need > *count) { *count = uint32_t(need); return fail(SGZ_EINVAL, "vertex buffer too small (count holds the required size)"); }
    size_t points = 0;
    const sgz_status st = scopeVerticesInto(s, view, evaluator, channel, d_xyz, reinterpret_cast<uint32_t *>(d_rgba), need, &points);
    if (st != SGZ_OK) return st;
    SGZ_HIP(hipStreamSynchronize(s->stream));                 // the vertices are in place when the call returns
    *count = uint32_t(points);
    return SGZ_OK;
}

// ---- the dense stream (scope_dense.hip): the frame's Linear strip reduced to a min and a max vertex per column
static LinearExtent scopeDenseExtent(const sgz_scope *s)
{
    return scopeLinearExtent(s->effWindow, s->cfg.trigger_mode, s->trig.cycle_samples, s->transport.load(std::memory_order_relaxed));
}

size_t sgz_scope_dense_vertex_count(const sgz_scope *s, uint32_t columns)
{
    if (!s || columns == 0) return 0;
    return 2 * std::min<size_t>(columns, scopeDenseExtent(s).n);
}

// what every dense call checks before it touches the handle; *need = 2 min(columns, n)
static sgz_status scopeDenseCheck(sgz_scope *s, uint32_t columns, uint32_t evaluator, uint32_t channel, size_t *need)
{
    if (columns == 0) return fail(SGZ_EINVAL, "columns == 0");
    StripSource src;
    if (sgz_status st = scopeStripSource(s, evaluator, channel, false, &src); st != SGZ_OK) return st;
    *need = sgz_scope_dense_vertex_count(s, columns);
    return SGZ_OK;
}

// one evaluator's dense strip into DEVICE buffers, enqueued behind the blocks that wait (flush on read); no wait
static sgz_status scopeDenseInto(sgz_scope *s, uint32_t columns, uint32_t evaluator, uint32_t channel, float *d_xyz, uint32_t *d_rgba,
                                 size_t *points)
{
    if (sgz_status sy = scopeSync(s); sy != SGZ_OK) return sy;
    StripSource src;
    if (sgz_status st = scopeStripSource(s, evaluator, channel, d_rgba != nullptr, &src); st != SGZ_OK) return st;
    const LinearExtent ext = scopeDenseExtent(s);
    // the long columns' partial records: the handle's own, in stream order behind the previous strip's
    if (const size_t bytes = scopeDenseScratchBytes(ext.n, columns); bytes > s->denseBytes) {
        if (s->d_dense) (void)hipFree(s->d_dense);
        s->d_dense = nullptr; s->denseBytes = 0;
        SGZ_HIP(hipMalloc(&s->d_dense, bytes));
        s->denseBytes = bytes;
    }
    SGZ_HIP(launchScopeDense(src.ringA, src.ringB, src.evalMode, uint32_t(s->trig.ring_size), s->size,
                             reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(s->d_state) + offsetof(ScopeDev, frontCursor)),
                             ext.n, -ext.bufferOffset, columns, src.key, src.colRing, d_xyz, d_rgba, s->d_dense, points, s->stream));
    return SGZ_OK;
}

sgz_status sgz_scope_dense_vertices(sgz_scope *s, uint32_t columns, uint32_t evaluator, uint32_t channel, float *xyz, uint8_t *rgba,
                                    uint32_t *count)
{
    if (!s || !xyz || !count) return fail(SGZ_EINVAL, "null argument");
    size_t need = 0, points = 0;
    if (sgz_status st = scopeDenseCheck(s, columns, evaluator, channel, &need); st != SGZ_OK) return st;
    if (need > *count) { *count = uint32_t(need); return fail(SGZ_EINVAL, "vertex buffer too small (count holds the required size)"); }
    void *mx = mappedDevicePointer(xyz, s->stream), *mc = rgba ? mappedDevicePointer(rgba, s->stream) : nullptr;
    if (mx && (!rgba || mc)) {                                // pinned, device-mapped (or device) buffers: the kernel writes them itself
        if (sgz_status sd = scopeDenseInto(s, columns, evaluator, channel, static_cast<float *>(mx), static_cast<uint32_t *>(mc), &points); sd != SGZ_OK)
            return sd;
        SGZ_HIP(hipStreamSynchronize(s->stream));
        *count = uint32_t(points);
        return SGZ_OK;
    }
    if (sgz_status rs = scopeReserveVertices(s, need); rs != SGZ_OK) return rs;
    if (sgz_status st = scopeDenseInto(s, columns, evaluator, channel, s->d_xyz, rgba ? s->d_rgba : nullptr, &points); st != SGZ_OK) return st;
    if (sgz_status rb = readBack(xyz, s->d_xyz, points * 3 * sizeof(float), rgba, s->d_rgba, points * sizeof(uint32_t), s->h_out, s->stream);
        rb != SGZ_OK) return rb;
    *count = uint32_t(points);
    return SGZ_OK;
}

sgz_status sgz_scope_dense_vertices_all(sgz_scope *s, uint32_t columns, uint32_t items, const uint32_t *evaluators, const uint32_t *channels,
                                        float *const *xyz, uint8_t *const *rgba, uint32_t *counts)
{
    if (!s || !evaluators || !channels || !xyz || !counts) return fail(SGZ_EINVAL, "null argument");
    if (columns == 0) return fail(SGZ_EINVAL, "columns == 0");
    size_t need = 0;
    bool small = false, direct = true;
    for (uint32_t k = 0; k < items; ++k) {
        if (!xyz[k]) return fail(SGZ_EINVAL, "null argument");
        if (sgz_status st = scopeDenseCheck(s, columns, evaluators[k], channels[k], &need); st != SGZ_OK) return st;
    }
    for (uint32_t k = 0; k < items; ++k) {
        if (need > counts[k]) { counts[k] = uint32_t(need); small = true; }
        direct = direct && mappedDevicePointer(xyz[k], s->stream) && (!rgba || !rgba[k] || mappedDevicePointer(rgba[k], s->stream));
    }
    if (small) return fail(SGZ_EINVAL, "vertex buffer too small (counts hold the required size)");
    if (!direct) {                                            // a pageable buffer among them: item by item through the bounce buffer
        for (uint32_t k = 0; k < items; ++k) {
            const sgz_status st = sgz_scope_dense_vertices(s, columns, evaluators[k], channels[k], xyz[k], rgba ? rgba[k] : nullptr, &counts[k]);
            if (st != SGZ_OK) return st;
        }
        return SGZ_OK;
    }
    for (uint32_t k = 0; k < items; ++k) {
        size_t points = 0;
        const sgz_status st = scopeDenseInto(s, columns, evaluators[k], channels[k], static_cast<float *>(mappedDevicePointer(xyz[k], s->stream)),
                                             rgba && rgba[k] ? static_cast<uint32_t *>(mappedDevicePointer(rgba[k], s->stream)) : nullptr, &points);
        if (st != SGZ_OK) { (void)hipStreamSynchronize(s->stream); return st; }
        counts[k] = uint32_t(points);
    }
    SGZ_HIP(hipStreamSynchronize(s->stream));
    return SGZ_OK;
}

sgz_status sgz_scope_dense_vertices_device(sgz_scope *s, uint32_t columns, uint32_t evaluator, uint32_t channel, float *d_xyz, uint8_t *d_rgba,
                                           uint32_t *count)
{
    if (!s || !d_xyz || !count) return fail(SGZ_EINVAL, "null argument");
    if ((reinterpret_cast<uintptr_t>(d_xyz) & 3) || (reinterpret_cast<uintptr_t>(d_rgba) & 3)) return fail(SGZ_EINVAL, "4-byte aligned buffers");
    size_t need = 0, points = 0;
    if (sgz_status st = scopeDenseCheck(s, columns, evaluator, channel, &need); st != SGZ_OK) return st;
    if (need > *count) { *count = uint32_t(need); return fail(SGZ_EINVAL, "vertex buffer too small (count holds the required size)"); }
    if (sgz_status st = scopeDenseInto(s, columns, evaluator, channel, d_xyz, reinterpret_cast<uint32_t *>(d_rgba), &points); st != SGZ_OK) return st;
    SGZ_HIP(hipStreamSynchronize(s->stream));                 // the vertices are in place when the call returns
    *count = uint32_t(points);
    return SGZ_OK;
}

}  // extern "C"
