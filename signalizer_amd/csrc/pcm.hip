// pcm.hip -- interleaved PCM in (include/sgz.h "interleaved PCM in"): the convert-and-de-interleave kernel, and the stream handle that
// cuts a feed into pieces and runs upload / convert + render / read-back of neighbouring pieces side by side on three streams.  Both kinds
// of feed (frames, overview columns) go through ONE piece loop, pcmPieces, and differ in the Part they hand it: what to render from a piece
// and which rows to read back.  Every output of a piece -- image, lines, overview image, overview peaks, waveform columns, track records --
// is a PcmOut: device block, pinned twin, pending host copy.  Armed, the waveform lane (wave_columns.hip) and the level lane
// (level_columns.hip) reduce every piece's new samples behind the converter and the track lane (tracker.hip) searches every piece's line
// results behind its render; the true-peak lane (truepeak_columns.hip) filters every piece's new samples behind them, and the loudness lane
// (loudness_columns.hip) behind that one.  All ride the same read-back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>
#include <new>

#include "rt_common.hpp"       // isPinnedHost
#include "runtime.hpp"
#include "scope_ring.hpp"     // StreamScratch

namespace sgz {

// ---- the converter ---------------------------------------------------------------------------------------------------------------------
// A transposition whose input rows (one sample of every source channel: a "frame" of frameBytes = src_channels * sample_bytes, 1 .. 512
// bytes, 3, 9, 15 ... for S24) are much shorter than a wave's access.  One workgroup takes a tile of tileSamples consecutive frames:
//   load   the tile's bytes as 16-byte chunks at 16-byte-aligned ADDRESSES, whatever the frame size and wherever d_pcm starts, lane after
//          lane (1 KiB per wave instruction), into LDS at the same offsets -- the tile's first byte sits `lead` = address & 15 bytes in.
//          A chunk that reaches over either end of the PCM buffer (the first chunk of the first tile, the last of the last) is read byte by
//          byte instead: nothing outside [d_pcm, d_pcm + nsamples * frameBytes) is touched.  Chunks that reach into a NEIGHBOURING tile are
//          read whole (those bytes are the buffer's own).
//   store  a wave takes one (destination row, 64 consecutive samples) unit at a time: lane l reads its sample from LDS -- any byte address:
//          the word that holds it and, for S24 / F64, the next one -- converts, and the wave stores 64 consecutive floats of that row.
// All byte offsets are 64-bit (a tile's start: tile * tileSamples * frameBytes).
constexpr int kPcmThreads = 256;
constexpr uint32_t kPcmMaxChannels = 64;
constexpr uint32_t kPcmTileBytes = 16384;       // the tile's target size; one frame group of 64 samples is the least (up to 32 KiB: 64 x F64)
constexpr uint32_t kPcmMaxTileSamples = 4096;

struct PcmMap { uint32_t src[kPcmMaxChannels]; };

// bytes of one sample of a format; 0: no such format
static constexpr uint32_t pcmSampleBytes(uint32_t format)
{
    switch (format) {
    case SGZ_PCM_F32: case SGZ_PCM_S32: return 4;
    case SGZ_PCM_U8: return 1;
    case SGZ_PCM_S16: return 2;
    case SGZ_PCM_S24: return 3;
    case SGZ_PCM_F64: return 8;
    default: return 0;
    }
}

// the sample at LDS byte offset `at` (a multiple of the sample's natural alignment) as the fp32 word sgz.h defines
template <uint32_t FORMAT>
__device__ __forceinline__ uint32_t pcmSample(const uint32_t *words, uint32_t at)
{
    const uint32_t w = at >> 2, sh = (at & 3u) * 8u;
    if constexpr (FORMAT == SGZ_PCM_F32) {
        return words[w];                                                   // the bits themselves: no arithmetic touches a NaN
    } else if constexpr (FORMAT == SGZ_PCM_S32) {
        return __float_as_uint(float(int32_t(words[w])) * 0x1p-31f);       // v_cvt_f32_i32 rounds to nearest even
    } else if constexpr (FORMAT == SGZ_PCM_S16) {
        return __float_as_uint(float(int32_t(int16_t(words[w] >> sh))) * 0x1p-15f);
    } else if constexpr (FORMAT == SGZ_PCM_U8) {
        return __float_as_uint(float(int32_t((words[w] >> sh) & 0xffu) - 128) * 0x1p-7f);
    } else if constexpr (FORMAT == SGZ_PCM_S24) {
        // three bytes anywhere in two words (the second one is read even where the sample ends in the first: the tile has a pad word)
        const uint64_t two = uint64_t(words[w]) | uint64_t(words[w + 1]) << 32;
        const int32_t x = int32_t(uint32_t(two >> sh) << 8) >> 8;
        return __float_as_uint(float(x) * 0x1p-23f);
    } else {
        const double v = __longlong_as_double((long long)(uint64_t(words[w]) | uint64_t(words[w + 1]) << 32));
        return __float_as_uint(float(v));                                  // v_cvt_f32_f64: nearest even, denormal results kept
    }
}

template <uint32_t FORMAT>
__global__ __launch_bounds__(kPcmThreads) void pcmToPlanarKernel(const uint8_t *__restrict__ pcm, uint64_t nsamples, uint32_t srcChannels,
                                                                 uint32_t tileSamples, PcmMap map, uint32_t numChannels,
                                                                 uint32_t *__restrict__ planar, uint64_t channelStride)
{
    extern __shared__ uint4 pcmTile[];                                     // [lead + tile bytes, rounded up to chunks] + one pad chunk
    constexpr uint32_t kBytes = pcmSampleBytes(FORMAT);
    const uint32_t frameBytes = srcChannels * kBytes;
    const uint64_t first = uint64_t(blockIdx.x) * tileSamples;             // the tile's first sample
    const uint32_t count = uint32_t(min(uint64_t(tileSamples), nsamples - first));
    const uint64_t bufBegin = reinterpret_cast<uint64_t>(pcm), bufEnd = bufBegin + nsamples * frameBytes;
    const uint64_t tileBegin = bufBegin + first * frameBytes, tileEnd = tileBegin + uint64_t(count) * frameBytes;
    const uint64_t aligned = tileBegin & ~uint64_t(15);
    const uint32_t lead = uint32_t(tileBegin - aligned);
    const uint32_t chunks = uint32_t((tileEnd - aligned + 15) >> 4);
    for (uint32_t k = threadIdx.x; k < chunks; k += kPcmThreads) {
        const uint64_t a = aligned + uint64_t(k) * 16;
        uint4 v;
        if (a >= bufBegin && a + 16 <= bufEnd) {
            v = *reinterpret_cast<const uint4 *>(pcm + int64_t(a - bufBegin));
        } else {                                                           // at most two chunks of a launch: the buffer's own bytes, one by one
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t b = 0; b < 16; ++b)
                if (a + b >= bufBegin && a + b < bufEnd) w[b >> 2] |= uint32_t(pcm[int64_t(a + b - bufBegin)]) << ((b & 3u) * 8u);
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        pcmTile[k] = v;
    }
    __syncthreads();
    const uint32_t *words = reinterpret_cast<const uint32_t *>(pcmTile);
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (uniform: map.src[d] is a scalar load)
    const uint32_t groups = (count + 63u) >> 6;
    for (uint32_t u = wave; u < groups * numChannels; u += kPcmThreads / 64) {
        const uint32_t d = u / groups, i = (u - d * groups) * 64u + lane;  // (d and the group are the same in every lane of the wave)
        if (i < count) planar[uint64_t(d) * channelStride + first + i] = pcmSample<FORMAT>(words, lead + (i * srcChannels + map.src[d]) * kBytes);
    }
}

static uint32_t pcmTileSamples(uint32_t frameBytes)
{
    return std::min(kPcmMaxTileSamples, 64u * std::max(1u, kPcmTileBytes / (64u * frameBytes)));
}

// the alignment d_pcm needs: the sample's own size, none for the packed three bytes of S24
static uint32_t pcmAlignment(uint32_t format) { return pcmSampleBytes(format) == 3 ? 1u : pcmSampleBytes(format); }

// everything the converter refuses that does not depend on the buffers (the stream handle checks it at create)
static sgz_status checkPcmLayout(uint32_t format, uint32_t srcChannels, const uint32_t *channelMap, uint32_t numChannels, PcmMap &map)
{
    if (pcmSampleBytes(format) == 0) return fail(SGZ_EINVAL, "unknown PCM format");
    if (srcChannels == 0 || srcChannels > kPcmMaxChannels || numChannels == 0 || numChannels > kPcmMaxChannels)
        return fail(SGZ_EINVAL, "PCM: 1 .. 64 source channels and 1 .. 64 destination rows");
    if (!channelMap && srcChannels < numChannels) return fail(SGZ_EINVAL, "PCM: the identity map needs src_channels >= num_channels");
    for (uint32_t d = 0; d < numChannels; ++d) {
        map.src[d] = channelMap ? channelMap[d] : d;
        if (map.src[d] >= srcChannels) return fail(SGZ_EINVAL, "PCM: channel_map entry >= src_channels");
    }
    for (uint32_t d = numChannels; d < kPcmMaxChannels; ++d) map.src[d] = 0;
    return SGZ_OK;
}

static sgz_status launchPcmToPlanar(const void *d_pcm, uint32_t format, uint32_t srcChannels, size_t nsamples, const PcmMap &map,
                                    uint32_t numChannels, float *d_planar, size_t channelStride, hipStream_t stream)
{
    if (!d_pcm || !d_planar) return fail(SGZ_EINVAL, "null buffer");
    if (channelStride < nsamples) return fail(SGZ_EINVAL, "PCM: channel_stride < nsamples");
    if (reinterpret_cast<uintptr_t>(d_pcm) % pcmAlignment(format)) return fail(SGZ_EINVAL, "PCM: d_pcm is not aligned to its sample type");
    if (nsamples == 0) return SGZ_OK;
    const uint32_t frameBytes = srcChannels * pcmSampleBytes(format);
    const uint32_t tileSamples = pcmTileSamples(frameBytes);
    const size_t tiles = (nsamples + tileSamples - 1) / tileSamples;
    if (tiles > 0x7fffffffu) return fail(SGZ_EINVAL, "PCM: too many samples for one launch");
    // 15 bytes of lead at most, the tile, rounded up to whole chunks; one more chunk so that the word behind the last sample exists
    const uint32_t lds = ((15u + tileSamples * frameBytes + 15u) & ~15u) + 16u;
    uint32_t *out = reinterpret_cast<uint32_t *>(d_planar);
    const uint8_t *in = static_cast<const uint8_t *>(d_pcm);
    const dim3 grid{uint32_t(tiles)}, block{uint32_t(kPcmThreads)};
#define SGZ_PCM_LAUNCH(F) hipLaunchKernelGGL(pcmToPlanarKernel<F>, grid, block, lds, stream, in, uint64_t(nsamples), srcChannels, tileSamples, map, numChannels, out, uint64_t(channelStride))
    switch (format) {
    case SGZ_PCM_F32: SGZ_PCM_LAUNCH(SGZ_PCM_F32); break;
    case SGZ_PCM_U8: SGZ_PCM_LAUNCH(SGZ_PCM_U8); break;
    case SGZ_PCM_S16: SGZ_PCM_LAUNCH(SGZ_PCM_S16); break;
    case SGZ_PCM_S24: SGZ_PCM_LAUNCH(SGZ_PCM_S24); break;
    case SGZ_PCM_S32: SGZ_PCM_LAUNCH(SGZ_PCM_S32); break;
    default: SGZ_PCM_LAUNCH(SGZ_PCM_F64); break;
    }
#undef SGZ_PCM_LAUNCH
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

static sgz_status streamStep(uint32_t W, uint32_t hop, uint64_t held, uint64_t incoming, uint64_t *frames, uint64_t *keep)
{
    if (W == 0 || hop == 0 || hop > W || !frames || !keep) return fail(SGZ_EINVAL, "sgz_stream_step: window_size >= hop >= 1, results non-null");
    const uint64_t total = held + incoming;
    *frames = total >= W ? (total - W) / hop + 1 : 0;
    *keep = total - *frames * hop;
    return SGZ_OK;
}

}  // namespace sgz

using namespace sgz;

// ---- the stream handle -----------------------------------------------------------------------------------------------------------------
namespace {
// The default piece: 2^20 samples, less where a slot of that many frames would pass 256 MiB (64-channel F64: 2^19).  A kept stream fed cfg2's
// 60 s of stereo S16 (tools/bench_pcm_render.py): 5.1 / 2.5 / 1.4 / 0.93 / 0.67 / 0.65 / 0.66 ms at 2^16 .. 2^22 -- a piece costs the host
// and the streams ~0.1 ms whatever its size, which 2^20 samples (21 frames' worth of upload at cfg2, 128 frames to render) bury.
constexpr size_t kPcmDefaultChunk = size_t(1) << 20;
constexpr size_t kPcmDefaultSlotBytes = size_t(256) << 20;
constexpr size_t kPcmMaxChunk = size_t(1) << 26;

// The outputs of a piece.  Image [maxFrames][P][4] and Lines [maxFrames][C][graphs][P][2] are the feed's; OvImage [columns][P][4] and OvPeaks
// [columns][C][P] the overview feed's, ceil(maxFrames / k) + 1 columns of them; Wave float2 [ceil(chunk / m) + 1][channels] the waveform
// lane's; Track sgz_line_peak [maxFrames][pairs] the track lane's; Level sgz_level_record [ceil(chunk / m) + 1][pairs] the level lane's;
// TruePeak sgz_truepeak_record [ceil(chunk / m) + 1][channels] the true-peak lane's.
// Loudness sgz_loudness_record [ceil(chunk / m) + 1][channels] the loudness lane's.
enum PcmOutKind { kOutImage, kOutLines, kOutOvImage, kOutOvPeaks, kOutWave, kOutTrack, kOutLevel, kOutTruePeak, kOutLoudness, kPcmOuts };

// One output of a slot: a device block, its pinned twin, and the host's part of a read-back -- the copy out of the twin that the drain
// performs when the caller's memory is pageable.  Capacities in bytes.  The image's device block is made at create, every other block on
// first need; a block grows when a later feed needs more (the slot is idle then: nothing in flight reads the old one).
struct PcmOut {
    void *dev = nullptr, *twin = nullptr;
    size_t devCap = 0, twinCap = 0;
    void *dst = nullptr; size_t bytes = 0;              // pending: `bytes` of the twin -> dst

    template <typename T> T *as() const { return static_cast<T *>(dev); }
    // a device block of at least n bytes; the twin as well when the destination is pageable
    sgz_status reserve(size_t n, bool pageable)
    {
        if (devCap < n) {
            if (dev) { (void)hipFree(dev); dev = nullptr; devCap = 0; }
            SGZ_HIP(hipMalloc(&dev, n));
            devCap = n;
        }
        if (pageable && twinCap < n) {
            if (twin) { (void)hipHostFree(twin); twin = nullptr; twinCap = 0; }
            SGZ_HIP(hipHostMalloc(&twin, n, hipHostMallocDefault));
            twinCap = n;
        }
        return SGZ_OK;
    }
    // the block's first n bytes on their way to `to`: straight there when it is pinned, else to the twin, and the drain copies
    sgz_status readBack(void *to, size_t n, bool pinned, hipStream_t stream)
    {
        SGZ_HIP(hipMemcpyAsync(pinned ? to : twin, dev, n, hipMemcpyDeviceToHost, stream));
        dst = pinned ? nullptr : to; bytes = n;
        return SGZ_OK;
    }
    void drain() { if (dst) std::memcpy(dst, twin, bytes); dst = nullptr; }
    void release() { if (dev) (void)hipFree(dev); if (twin) (void)hipHostFree(twin); *this = PcmOut{}; }
};

struct PcmSlot {                        // what one piece in flight owns; a slot is reused by the piece after next
    void *h_pcm = nullptr;              // pinned [chunk][frameBytes], made when the first pageable feed arrives
    void *d_pcm = nullptr;
    PcmOut out[kPcmOuts];
    hipEvent_t ev[7] = {};              // upload begin / END (copy stream); convert begin, convert end, render END (compute); read-back begin / END
                                        // (the capitals order the streams; the others are recorded for a caller that asks for timing only: a
                                        // marker costs the stream it sits on microseconds, api.hip sgz_render_queue_submit)
    bool timed = false;
    bool busy = false, rendered = false;            // rendered: the piece has a read-back (any output at all), ev[6] is recorded
};
}  // namespace

struct sgz_pcm_stream {
    sgz_spectrum_config cfg{};
    sgz_plan *plan = nullptr;
    uint32_t format = 0, srcChannels = 0, frameBytes = 0, numChannels = 0;
    PcmMap map{};
    size_t chunk = 0, stride = 0, maxFrames = 0;
    hipStream_t copy = nullptr, compute = nullptr, back = nullptr;
    PcmSlot slot[2];
    float *d_planar[2] = {nullptr, nullptr};            // [numChannels][stride] each: the held tail moves from one to the front of the other
    float *d_state = nullptr;
    int cur = 0;
    uint64_t held = 0, pieces = 0;
    // the overview inside the stream: the open column's V [pairs][P], its frame count and its k (meaningful while ovOpen > 0)
    float *d_ovCarry = nullptr;
    uint64_t ovOpen = 0; uint32_t ovK = 0;
    // the waveform lane (m > 0: armed): the caller's columns and the cursor in them, the open column's sample count and its (lo, hi) per channel
    // in d_wvCarry [2][channels] float2 -- a piece reads half wvCur and writes the other, so no launch reads what it writes
    uint32_t wvM = 0;
    float *wvOut = nullptr;
    uint64_t wvCap = 0, wvCursor = 0, wvOpen = 0;
    bool wvPinned = false;
    float *d_wvCarry = nullptr;
    int wvCur = 0;
    // the track lane (trArmed): the graph and mouse position searched, the caller's records [trCap][pairs] and the cursor in them, in frames
    bool trArmed = false, trPinned = false;
    uint32_t trGraph = 0;
    double trFraction = 0;
    sgz_line_peak *trOut = nullptr;
    uint64_t trCap = 0, trCursor = 0;
    // the level lane (lvM > 0: armed), as the waveform lane with an m of its own: the caller's records and the cursor in them, the open column's
    // sample count and its record per pair in d_lvCarry [2][pairs] -- a piece reads half lvCur and writes the other
    uint32_t lvM = 0;
    sgz_level_record *lvOut = nullptr;
    uint64_t lvCap = 0, lvCursor = 0, lvOpen = 0;
    bool lvPinned = false;
    sgz_level_record *d_lvCarry = nullptr;
    int lvCur = 0;
    // the true-peak lane (tpM > 0: armed), as the level lane per channel; its carry d_tpCarry [2][channels] also holds the filter's history, so
    // every piece with samples writes the other half and the halves alternate.  tpContinued: half tpCur holds the samples before the next one
    // (false after arming or a reset: the history is zeros)
    uint32_t tpM = 0;
    sgz_truepeak_record *tpOut = nullptr;
    uint64_t tpCap = 0, tpCursor = 0, tpOpen = 0;
    bool tpPinned = false, tpContinued = false;
    sgz_truepeak_carry *d_tpCarry = nullptr;
    int tpCur = 0;
    // the loudness lane (ldM > 0: armed), as the true-peak lane; its carry d_ldCarry holds two halves of loudnessCarryBytes(ldFilter) * channels
    // bytes (ldCarryCap: what is allocated).  ldIndex: the lane's samples so far -- the absolute index of the next one, which a flush does not move
    uint32_t ldM = 0;
    sgz_loudness_filter ldFilter{};
    sgz_loudness_record *ldOut = nullptr;
    uint64_t ldCap = 0, ldCursor = 0, ldOpen = 0, ldIndex = 0;
    bool ldPinned = false, ldContinued = false;
    uint8_t *d_ldCarry = nullptr;
    size_t ldCarryCap = 0;
    // the lane's scratch (q of a piece's samples, partial records), kept: every piece's launches are on the compute stream, one behind the other
    void *d_ldScratch = nullptr;
    size_t ldScratchCap = 0;
    int ldCur = 0;
};

struct sgz_plan { Plan impl; };

using PcmClock = std::chrono::steady_clock;
static double pcmMsSince(PcmClock::time_point t0) { return std::chrono::duration<double, std::milli>(PcmClock::now() - t0).count(); }

static size_t pcmStateBytes(const sgz_pcm_stream &s) { return size_t(s.cfg.num_pairs) * SGZ_NUM_GRAPHS * s.cfg.axis_points * 2 * sizeof(float); }
static size_t pcmLinesFloats(const sgz_pcm_stream &s, uint64_t frames) { return size_t(frames) * s.cfg.num_pairs * SGZ_NUM_GRAPHS * s.cfg.axis_points * 2; }
static size_t pcmImageBytes(const sgz_pcm_stream &s, uint64_t columns) { return size_t(columns) * s.cfg.axis_points * 4; }
static size_t pcmPeaksFloats(const sgz_pcm_stream &s, uint64_t columns) { return size_t(columns) * s.cfg.num_pairs * s.cfg.axis_points; }

// waits for the piece that used the slot, hands its outputs to the caller (pageable destinations) and adds its event intervals up
static sgz_status pcmDrain(PcmSlot &sl, sgz_pcm_timing *timing)
{
    if (!sl.busy) return SGZ_OK;
    sl.busy = false;
    SGZ_HIP(hipEventSynchronize(sl.ev[sl.rendered ? 6 : 4]));
    for (PcmOut &o : sl.out) o.drain();
    if (timing && sl.timed) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sl.ev[0], sl.ev[1]) == hipSuccess) timing->h2d_ms += ms;
        if (hipEventElapsedTime(&ms, sl.ev[2], sl.ev[3]) == hipSuccess) timing->convert_ms += ms;
        if (hipEventElapsedTime(&ms, sl.ev[3], sl.ev[4]) == hipSuccess) timing->render_ms += ms;
        if (sl.rendered && hipEventElapsedTime(&ms, sl.ev[5], sl.ev[6]) == hipSuccess) timing->d2h_ms += ms;
    }
    return SGZ_OK;
}

// ---- the waveform lane inside the stream (sgz.h, "The waveform lane") -----------------------------------------------------------------------
static float *pcmWaveCarry(const sgz_pcm_stream &s, int half) { return s.d_wvCarry + size_t(half) * 2 * s.numChannels; }

// what a feed checks for the lane before anything is consumed: the columns its samples close fit behind the cursor
static sgz_status pcmWaveFits(const sgz_pcm_stream &s, size_t nsamples)
{
    if (s.wvM && (s.wvOpen + nsamples) / s.wvM > s.wvCap - s.wvCursor)
        return fail(SGZ_EINVAL, "sgz_pcm_stream: the feed closes more waveform columns than the buffer has left (sgz_pcm_stream_waveform_for; re-arm with sgz_pcm_stream_set_waveform)");
    return SGZ_OK;
}

// a slot's columns of a piece, ceil(chunk / m) + 1 of them (both slots are idle between feeds)
static sgz_status pcmWaveBuffers(sgz_pcm_stream &s, PcmSlot &sl)
{
    return s.wvM ? sl.out[kOutWave].reserve(((s.chunk + s.wvM - 1) / s.wvM + 1) * s.numChannels * 2 * sizeof(float), !s.wvPinned) : SGZ_OK;
}

// the lane's part of a piece, on the compute stream: the n samples the converter just wrote at `fresh` -> the columns they close, into the slot;
// the open one into the carry
static sgz_status pcmWavePiece(sgz_pcm_stream &s, PcmSlot &sl, const float *fresh, size_t n, uint64_t *columns)
{
    *columns = 0;
    if (!s.wvM || n == 0) return SGZ_OK;
    const WaveColumnsShape sh = waveColumnsShape(s.numChannels, n, s.wvM, uint32_t(s.wvOpen), 0, 0);
    StreamScratch scratch(s.compute);
    if (sh.scratchBytes) SGZ_HIP(scratch.get(sh.scratchBytes));
    const sgz_status st = runWaveColumns(sh, fresh, s.stride, s.numChannels, n, s.wvM, uint32_t(s.wvOpen), pcmWaveCarry(s, s.wvCur), pcmWaveCarry(s, s.wvCur ^ 1),
                                         sl.out[kOutWave].as<float>(), scratch.p, s.compute);
    if (st != SGZ_OK) return st;
    if (sh.open) s.wvCur ^= 1;
    s.wvOpen = (s.wvOpen + n) % s.wvM;
    *columns = sh.closed;
    return SGZ_OK;
}

// the piece's columns to the caller's buffer at the cursor, on the read-back stream
static sgz_status pcmWaveReadBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t columns)
{
    if (!columns) return SGZ_OK;
    const size_t column = size_t(s.numChannels) * 2;
    const sgz_status st = sl.out[kOutWave].readBack(s.wvOut + size_t(s.wvCursor) * column, size_t(columns) * column * sizeof(float), s.wvPinned, s.back);
    if (st == SGZ_OK) s.wvCursor += columns;
    return st;
}

// ---- the level lane inside the stream (sgz.h, "The level lane") ----------------------------------------------------------------------------
static sgz_level_record *pcmLevelCarry(const sgz_pcm_stream &s, int half) { return s.d_lvCarry + size_t(half) * s.cfg.num_pairs; }

// what a feed checks for the lane before anything is consumed: the columns its samples close fit behind the cursor
static sgz_status pcmLevelFits(const sgz_pcm_stream &s, size_t nsamples)
{
    if (s.lvM && (s.lvOpen + nsamples) / s.lvM > s.lvCap - s.lvCursor)
        return fail(SGZ_EINVAL, "sgz_pcm_stream: the feed closes more level columns than the buffer has left (sgz_pcm_stream_level_for; re-arm with sgz_pcm_stream_set_level)");
    return SGZ_OK;
}

// a slot's records of a piece, ceil(chunk / m) + 1 columns of them (both slots are idle between feeds)
static sgz_status pcmLevelBuffers(sgz_pcm_stream &s, PcmSlot &sl)
{
    return s.lvM ? sl.out[kOutLevel].reserve(((s.chunk + s.lvM - 1) / s.lvM + 1) * s.cfg.num_pairs * sizeof(sgz_level_record), !s.lvPinned) : SGZ_OK;
}

// the lane's part of a piece, on the compute stream: the n samples the converter just wrote at `fresh` -> the records they close, into the slot;
// the open one into the carry
static sgz_status pcmLevelPiece(sgz_pcm_stream &s, PcmSlot &sl, const float *fresh, size_t n, uint64_t *columns)
{
    *columns = 0;
    if (!s.lvM || n == 0) return SGZ_OK;
    const LevelColumnsShape sh = levelColumnsShape(s.cfg.num_pairs, n, s.lvM, uint32_t(s.lvOpen), 0, 0);
    StreamScratch scratch(s.compute);
    if (sh.scratchBytes) SGZ_HIP(scratch.get(sh.scratchBytes));
    const sgz_status st = runLevelColumns(sh, fresh, s.stride, s.cfg.num_pairs, n, s.lvM, uint32_t(s.lvOpen), pcmLevelCarry(s, s.lvCur), pcmLevelCarry(s, s.lvCur ^ 1),
                                          sl.out[kOutLevel].as<sgz_level_record>(), scratch.p, s.compute);
    if (st != SGZ_OK) return st;
    if (sh.open) s.lvCur ^= 1;
    s.lvOpen = (s.lvOpen + n) % s.lvM;
    *columns = sh.closed;
    return SGZ_OK;
}

// the piece's records to the caller's buffer at the cursor, on the read-back stream
static sgz_status pcmLevelReadBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t columns)
{
    if (!columns) return SGZ_OK;
    const size_t column = s.cfg.num_pairs;
    const sgz_status st = sl.out[kOutLevel].readBack(s.lvOut + size_t(s.lvCursor) * column, size_t(columns) * column * sizeof(sgz_level_record), s.lvPinned, s.back);
    if (st == SGZ_OK) s.lvCursor += columns;
    return st;
}

// ---- the true-peak lane inside the stream (sgz.h, "The true-peak lane") --------------------------------------------------------------------
static sgz_truepeak_carry *pcmTruePeakCarry(const sgz_pcm_stream &s, int half) { return s.d_tpCarry + size_t(half) * s.numChannels; }

// what a feed checks for the lane before anything is consumed: the columns its samples close fit behind the cursor
static sgz_status pcmTruePeakFits(const sgz_pcm_stream &s, size_t nsamples)
{
    if (s.tpM && (s.tpOpen + nsamples) / s.tpM > s.tpCap - s.tpCursor)
        return fail(SGZ_EINVAL, "sgz_pcm_stream: the feed closes more true-peak columns than the buffer has left (sgz_pcm_stream_truepeak_for; re-arm with sgz_pcm_stream_set_truepeak)");
    return SGZ_OK;
}

// a slot's records of a piece, ceil(chunk / m) + 1 columns of them (both slots are idle between feeds)
static sgz_status pcmTruePeakBuffers(sgz_pcm_stream &s, PcmSlot &sl)
{
    return s.tpM ? sl.out[kOutTruePeak].reserve(((s.chunk + s.tpM - 1) / s.tpM + 1) * s.numChannels * sizeof(sgz_truepeak_record), !s.tpPinned) : SGZ_OK;
}

// the lane's part of a piece, on the compute stream: the n samples the converter just wrote at `fresh` -> the records they close, into the slot;
// the open one and the new history into the other half of the carry
static sgz_status pcmTruePeakPiece(sgz_pcm_stream &s, PcmSlot &sl, const float *fresh, size_t n, uint64_t *columns)
{
    *columns = 0;
    if (!s.tpM || n == 0) return SGZ_OK;
    const TruePeakColumnsShape sh = truePeakColumnsShape(s.numChannels, n, s.tpM, uint32_t(s.tpOpen), 0, 0);
    StreamScratch scratch(s.compute);
    if (sh.scratchBytes) SGZ_HIP(scratch.get(sh.scratchBytes));
    const sgz_status st = runTruePeakColumns(sh, fresh, s.stride, s.numChannels, n, s.tpM, uint32_t(s.tpOpen), s.tpContinued ? 1u : 0u, pcmTruePeakCarry(s, s.tpCur),
                                             pcmTruePeakCarry(s, s.tpCur ^ 1), sl.out[kOutTruePeak].as<sgz_truepeak_record>(), scratch.p, s.compute);
    if (st != SGZ_OK) return st;
    s.tpCur ^= 1;                                                                   // (the history moved, whether or not a column stays open)
    s.tpContinued = true;
    s.tpOpen = (s.tpOpen + n) % s.tpM;
    *columns = sh.closed;
    return SGZ_OK;
}

// the piece's records to the caller's buffer at the cursor, on the read-back stream
static sgz_status pcmTruePeakReadBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t columns)
{
    if (!columns) return SGZ_OK;
    const size_t column = s.numChannels;
    const sgz_status st = sl.out[kOutTruePeak].readBack(s.tpOut + size_t(s.tpCursor) * column, size_t(columns) * column * sizeof(sgz_truepeak_record), s.tpPinned, s.back);
    if (st == SGZ_OK) s.tpCursor += columns;
    return st;
}

// ---- the loudness lane inside the stream (sgz.h, "The loudness lane") ------------------------------------------------------------------------
static uint8_t *pcmLoudnessCarry(const sgz_pcm_stream &s, int half) { return s.d_ldCarry + size_t(half) * loudnessCarryBytes(s.ldFilter) * s.numChannels; }

// what a feed checks for the lane before anything is consumed: the columns its samples close fit behind the cursor
static sgz_status pcmLoudnessFits(const sgz_pcm_stream &s, size_t nsamples)
{
    if (s.ldM && (s.ldOpen + nsamples) / s.ldM > s.ldCap - s.ldCursor)
        return fail(SGZ_EINVAL, "sgz_pcm_stream: the feed closes more loudness columns than the buffer has left (sgz_pcm_stream_loudness_for; re-arm with sgz_pcm_stream_set_loudness)");
    return SGZ_OK;
}

// a slot's records of a piece, ceil(chunk / m) + 1 columns of them (both slots are idle between feeds)
static sgz_status pcmLoudnessBuffers(sgz_pcm_stream &s, PcmSlot &sl)
{
    return s.ldM ? sl.out[kOutLoudness].reserve(((s.chunk + s.ldM - 1) / s.ldM + 1) * s.numChannels * sizeof(sgz_loudness_record), !s.ldPinned) : SGZ_OK;
}

// the lane's part of a piece, on the compute stream: the n samples the converter just wrote at `fresh` -> the records they close, into the slot;
// the open one and the new history into the other half of the carry
static sgz_status pcmLoudnessPiece(sgz_pcm_stream &s, PcmSlot &sl, const float *fresh, size_t n, uint64_t *columns)
{
    *columns = 0;
    if (!s.ldM || n == 0) return SGZ_OK;
    const LoudnessColumnsShape sh = loudnessColumnsShape(s.numChannels, n, s.ldM, uint32_t(s.ldOpen), 0, 0);
    if (sh.scratchBytes > s.ldScratchCap) {                                         // (the first piece of a feed is its largest: this happens once)
        SGZ_HIP(hipStreamSynchronize(s.compute));
        if (s.d_ldScratch) { (void)hipFree(s.d_ldScratch); s.d_ldScratch = nullptr; s.ldScratchCap = 0; }
        SGZ_HIP(hipMalloc(&s.d_ldScratch, sh.scratchBytes));
        s.ldScratchCap = sh.scratchBytes;
    }
    const sgz_status st = runLoudnessColumns(sh, s.ldFilter, fresh, s.stride, s.numChannels, n, s.ldIndex, s.ldM, uint32_t(s.ldOpen), s.ldContinued ? 1u : 0u,
                                             pcmLoudnessCarry(s, s.ldCur), pcmLoudnessCarry(s, s.ldCur ^ 1), sl.out[kOutLoudness].as<sgz_loudness_record>(),
                                             s.d_ldScratch, s.compute);
    if (st != SGZ_OK) return st;
    s.ldCur ^= 1;                                                                   // (the history moved, whether or not a column stays open)
    s.ldContinued = true;
    s.ldOpen = (s.ldOpen + n) % s.ldM;
    s.ldIndex += n;
    *columns = sh.closed;
    return SGZ_OK;
}

// the piece's records to the caller's buffer at the cursor, on the read-back stream
static sgz_status pcmLoudnessReadBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t columns)
{
    if (!columns) return SGZ_OK;
    const size_t column = s.numChannels;
    const sgz_status st = sl.out[kOutLoudness].readBack(s.ldOut + size_t(s.ldCursor) * column, size_t(columns) * column * sizeof(sgz_loudness_record), s.ldPinned, s.back);
    if (st == SGZ_OK) s.ldCursor += columns;
    return st;
}

// ---- the track lane inside the stream (sgz.h, "The track lane") ----------------------------------------------------------------------------
// what a feed checks for the lane before anything is consumed: the frames its samples complete fit behind the cursor
static sgz_status pcmTrackFits(const sgz_pcm_stream &s, uint64_t frames)
{
    if (s.trArmed && frames > s.trCap - s.trCursor)
        return fail(SGZ_EINVAL, "sgz_pcm_stream: the feed completes more frames than the track buffer has left (sgz_pcm_stream_track_for; re-arm with sgz_pcm_stream_set_track)");
    return SGZ_OK;
}

// a slot's records of a piece, maxFrames * pairs of them (both slots are idle between feeds)
static sgz_status pcmTrackBuffers(sgz_pcm_stream &s, PcmSlot &sl)
{
    return s.trArmed ? sl.out[kOutTrack].reserve(s.maxFrames * s.cfg.num_pairs * sizeof(sgz_line_peak), !s.trPinned) : SGZ_OK;
}

// the records of the piece's `frames` frames to the caller's buffer at the cursor, on the read-back stream
static sgz_status pcmTrackReadBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t frames)
{
    if (!frames) return SGZ_OK;
    const size_t record = s.cfg.num_pairs;
    const sgz_status st = sl.out[kOutTrack].readBack(s.trOut + size_t(s.trCursor) * record, size_t(frames) * record * sizeof(sgz_line_peak), s.trPinned, s.back);
    if (st == SGZ_OK) s.trCursor += frames;
    return st;
}

// ---- the piece loop ------------------------------------------------------------------------------------------------------------------------
// What both feeds do once they have refused what they refuse.  The feed is cut into pieces of at most `chunk` samples; piece i uses slot i & 1:
//   1. upload            copy stream: the samples to the slot (through its pinned block when the caller's are pageable)
//   2. convert + render  compute stream, behind ev[1]: the converter behind the held tail, the waveform and level lanes on the new samples, the Part's
//                        render of what became complete (armed, the track lane's search with it), the new tail to the other planar buffer
//   3. read back         read-back stream, behind ev[4]: the Part's rows, the track's records, the waveform's columns, the level's records
// The two kinds of feed differ in their Part alone: reserve(s, sl) makes its outputs in a slot before anything is consumed; render(s, sl,
// planar, total, frames, last, &units) enqueues the render of a piece's frames and says how many rows -- `units`, what the feed counts and its
// timing reports -- it leaves in the slot; readBack(s, sl, done, units) enqueues their copies behind the feed's `done` earlier rows.
// emptyPiece: a feed without samples has one piece all the same (the overview's flush of an open column).
template <typename Part>
static sgz_status pcmFeed(sgz_pcm_stream &s, const void *pcm, size_t nsamples, bool emptyPiece, Part &part, uint64_t *unitsOut, sgz_pcm_timing *timing,
                          PcmClock::time_point t0)
{
    if (timing) *timing = sgz_pcm_timing{};
    const bool pcmPinned = nsamples && isPinnedHost(pcm);
    // (the pinned blocks are made on first need: a caller with pinned memory of its own never pays for them)
    for (PcmSlot &sl : s.slot) {
        if (nsamples && !pcmPinned && !sl.h_pcm) SGZ_HIP(hipHostMalloc(&sl.h_pcm, s.chunk * s.frameBytes, hipHostMallocDefault));
        if (sgz_status st = part.reserve(s, sl); st != SGZ_OK) return st;
        if (sgz_status st = pcmWaveBuffers(s, sl); st != SGZ_OK) return st;
        if (sgz_status st = pcmTrackBuffers(s, sl); st != SGZ_OK) return st;
        if (sgz_status st = pcmLevelBuffers(s, sl); st != SGZ_OK) return st;
        if (sgz_status st = pcmTruePeakBuffers(s, sl); st != SGZ_OK) return st;
        if (sgz_status st = pcmLoudnessBuffers(s, sl); st != SGZ_OK) return st;
    }
    const uint8_t *src = static_cast<const uint8_t *>(pcm);
    uint64_t done = 0, chunks = 0;
    auto pieces = [&]() -> sgz_status {
        for (size_t at = 0; at < nsamples || (emptyPiece && chunks == 0); ) {
            const size_t n = std::min(s.chunk, nsamples - at);
            PcmSlot &sl = s.slot[s.pieces & 1];
            if (sgz_status st = pcmDrain(sl, timing); st != SGZ_OK) return st;      // the one wait inside a feed: the piece before last
            uint64_t frames = 0, keep = 0;
            if (sgz_status st = streamStep(s.cfg.window_size, s.cfg.hop, s.held, n, &frames, &keep); st != SGZ_OK) return st;
            sl.timed = timing != nullptr;
            // 1. upload (a piece without samples has none, and the compute stream nothing to wait for; timed, it still has its interval)
            const void *from = n ? src + at * s.frameBytes : nullptr;
            if (n && !pcmPinned) { std::memcpy(sl.h_pcm, from, n * s.frameBytes); from = sl.h_pcm; }
            if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[0], s.copy));
            if (n) SGZ_HIP(hipMemcpyAsync(sl.d_pcm, from, n * s.frameBytes, hipMemcpyHostToDevice, s.copy));
            if (n || sl.timed) SGZ_HIP(hipEventRecord(sl.ev[1], s.copy));
            if (n) SGZ_HIP(hipStreamWaitEvent(s.compute, sl.ev[1], 0));
            // 2. convert behind the held tail, render what became complete, move the new tail to the front of the other planar buffer
            float *planar = s.d_planar[s.cur];
            if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[2], s.compute));
            if (n)
                if (sgz_status st = launchPcmToPlanar(sl.d_pcm, s.format, s.srcChannels, n, s.map, s.numChannels, planar + s.held, s.stride, s.compute); st != SGZ_OK) return st;
            if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[3], s.compute));
            uint64_t waveColumns = 0, levelColumns = 0, truePeakColumns = 0, loudnessColumns = 0, units = 0;
            if (sgz_status st = pcmWavePiece(s, sl, planar + s.held, n, &waveColumns); st != SGZ_OK) return st;
            if (sgz_status st = pcmLevelPiece(s, sl, planar + s.held, n, &levelColumns); st != SGZ_OK) return st;
            if (sgz_status st = pcmTruePeakPiece(s, sl, planar + s.held, n, &truePeakColumns); st != SGZ_OK) return st;
            if (sgz_status st = pcmLoudnessPiece(s, sl, planar + s.held, n, &loudnessColumns); st != SGZ_OK) return st;
            const uint64_t total = s.held + n;
            if (sgz_status st = part.render(s, sl, planar, size_t(total), frames, at + n == nsamples, &units); st != SGZ_OK) return st;
            if (frames) {
                if (keep) SGZ_HIP(hipMemcpy2DAsync(s.d_planar[s.cur ^ 1], s.stride * sizeof(float), planar + (total - keep), s.stride * sizeof(float),
                                                   size_t(keep) * sizeof(float), s.numChannels, hipMemcpyDeviceToDevice, s.compute));
                s.cur ^= 1;
            }                                                                      // (no frame: the tail just grew where it is)
            s.held = keep;
            SGZ_HIP(hipEventRecord(sl.ev[4], s.compute));
            // 3. read back (a piece may close waveform or level columns and complete no frame, or complete frames whose records are all it returns)
            const uint64_t trackFrames = s.trArmed ? frames : 0;
            sl.rendered = units > 0 || waveColumns > 0 || trackFrames > 0 || levelColumns > 0 || truePeakColumns > 0 || loudnessColumns > 0;
            if (sl.rendered) {
                SGZ_HIP(hipStreamWaitEvent(s.back, sl.ev[4], 0));
                if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[5], s.back));
                if (units)
                    if (sgz_status st = part.readBack(s, sl, done, units); st != SGZ_OK) return st;
                if (sgz_status st = pcmTrackReadBack(s, sl, trackFrames); st != SGZ_OK) return st;
                if (sgz_status st = pcmWaveReadBack(s, sl, waveColumns); st != SGZ_OK) return st;
                if (sgz_status st = pcmLevelReadBack(s, sl, levelColumns); st != SGZ_OK) return st;
                if (sgz_status st = pcmTruePeakReadBack(s, sl, truePeakColumns); st != SGZ_OK) return st;
                if (sgz_status st = pcmLoudnessReadBack(s, sl, loudnessColumns); st != SGZ_OK) return st;
                SGZ_HIP(hipEventRecord(sl.ev[6], s.back));
            }
            sl.busy = true;
            done += units; ++chunks; ++s.pieces; at += n;
        }
        // the end of the feed: both slots, the older piece first
        for (uint64_t i = 0; i < 2; ++i)
            if (sgz_status st = pcmDrain(s.slot[(s.pieces + i) & 1], timing); st != SGZ_OK) return st;
        return SGZ_OK;
    };
    if (const sgz_status st = pieces(); st != SGZ_OK) {
        // a failure among the pieces: nothing stays in flight, and both slots forget their pending host copies WITHOUT performing them -- those
        // point into this call's output buffers, which the caller may free once it has the status (g_lastError stays the failure's)
        for (hipStream_t q : {s.copy, s.compute, s.back}) (void)hipStreamSynchronize(q);
        for (PcmSlot &sl : s.slot) { sl.busy = false; for (PcmOut &o : sl.out) o.dst = nullptr; }
        return st;
    }
    if (unitsOut) *unitsOut = done;
    if (timing) { timing->frames = done; timing->chunks = chunks; timing->wall_ms = pcmMsSince(t0); }
    return SGZ_OK;
}

// sgz_pcm_stream_feed's part: frames into the slot's image, and into its lines when the caller or the track lane wants them
struct PcmFramesPart {
    uint8_t *rgba; float *lines;
    uint64_t need;                                                // the frames the whole feed yields
    bool rgbaPinned, linesPinned;

    sgz_status reserve(sgz_pcm_stream &s, PcmSlot &sl) const
    {
        if (!need) return SGZ_OK;
        const sgz_status st = sl.out[kOutImage].reserve(pcmImageBytes(s, s.maxFrames), !rgbaPinned);
        if (st != SGZ_OK || (!lines && !s.trArmed)) return st;    // (the track lane searches the line results: rendered, never read back for it)
        return sl.out[kOutLines].reserve(pcmLinesFloats(s, s.maxFrames) * sizeof(float), lines && !linesPinned);
    }
    sgz_status render(sgz_pcm_stream &s, PcmSlot &sl, const float *planar, size_t total, uint64_t frames, bool, uint64_t *units) const
    {
        *units = frames;
        if (!frames) return SGZ_OK;
        float *d_lines = (lines || s.trArmed) ? sl.out[kOutLines].as<float>() : nullptr;
        const sgz_status st = sgz_spectrogram_render_device(s.plan, planar, s.stride, total, sl.out[kOutImage].as<uint8_t>(), d_lines, s.d_state, s.compute);
        if (st != SGZ_OK || !s.trArmed) return st;
        return runTrackPeaksLines(s.plan->impl, d_lines, size_t(frames), s.trGraph, s.trFraction, sl.out[kOutTrack].as<sgz_line_peak>(), s.compute);
    }
    sgz_status readBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t done, uint64_t frames) const
    {
        const sgz_status st = sl.out[kOutImage].readBack(rgba + pcmImageBytes(s, done), pcmImageBytes(s, frames), rgbaPinned, s.back);
        if (st != SGZ_OK || !lines) return st;
        return sl.out[kOutLines].readBack(lines + pcmLinesFloats(s, done), pcmLinesFloats(s, frames) * sizeof(float), linesPinned, s.back);
    }
};

// sgz_pcm_stream_feed_overview's part: frames slab by slab into the columns they close, the open column in the stream's carry
struct PcmColumnsPart {
    uint8_t *rgba; float *peaks;
    uint32_t k; int flush;
    uint64_t need;                                                // the columns the whole feed yields
    bool rgbaPinned, peaksPinned;

    sgz_status reserve(sgz_pcm_stream &s, PcmSlot &sl) const
    {
        if (!s.d_ovCarry) SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s.d_ovCarry), pcmPeaksFloats(s, 1) * sizeof(float)));
        if (!need) return SGZ_OK;                                 // (no column closes: nothing is written or read back)
        // the most columns one piece can close: floor((k - 1 + maxFrames) / k) = ceil(maxFrames / k), and one more from a flush
        const size_t columns = (s.maxFrames + k - 1) / k + 1;
        const sgz_status st = rgba ? sl.out[kOutOvImage].reserve(pcmImageBytes(s, columns), !rgbaPinned) : SGZ_OK;
        if (st != SGZ_OK || !peaks) return st;
        return sl.out[kOutOvPeaks].reserve(pcmPeaksFloats(s, columns) * sizeof(float), !peaksPinned);
    }
    sgz_status render(sgz_pcm_stream &s, PcmSlot &sl, const float *planar, size_t total, uint64_t frames, bool last, uint64_t *units) const
    {
        const int pieceFlush = flush && last;
        const uint64_t t = s.ovOpen + frames;
        *units = t / k + ((pieceFlush && t % k) ? 1u : 0u);
        uint8_t *d_rgba = rgba ? sl.out[kOutOvImage].as<uint8_t>() : nullptr;
        float *d_peaks = peaks ? sl.out[kOutOvPeaks].as<float>() : nullptr;
        sgz_status st = SGZ_OK;
        if (frames) {
            const SlabTrack track{s.trGraph, s.trFraction, sl.out[kOutTrack].as<sgz_line_peak>()};
            st = runOverviewSlabs(s.plan, planar, s.stride, total, long(frames), k, uint32_t(s.ovOpen), pieceFlush, s.d_ovCarry, s.d_state, d_rgba, d_peaks,
                                  s.compute, s.trArmed ? &track : nullptr);
        } else if (*units) {                                       // no frame arrives and the open column is flushed
            st = runOverviewColumns(s.plan->impl, nullptr, 0, k, uint32_t(s.ovOpen), 1, 0, s.d_ovCarry, d_rgba, d_peaks, s.compute);
        }
        if (st != SGZ_OK) return st;
        s.ovOpen = pieceFlush ? 0 : t % k;
        s.ovK = k;
        return SGZ_OK;
    }
    sgz_status readBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t done, uint64_t columns) const
    {
        const sgz_status st = rgba ? sl.out[kOutOvImage].readBack(rgba + pcmImageBytes(s, done), pcmImageBytes(s, columns), rgbaPinned, s.back) : SGZ_OK;
        if (st != SGZ_OK || !peaks) return st;
        return sl.out[kOutOvPeaks].readBack(peaks + pcmPeaksFloats(s, done), pcmPeaksFloats(s, columns) * sizeof(float), peaksPinned, s.back);
    }
};

// what the two one-shot calls share: a stream with no more device and pinned memory than the buffer needs, SGZ_SKIPPED_FRAME where nothing
// comes out, the feed, and the wall time around all of it.  units(s): what the feed will yield; feed(s, units): the feed call
template <typename Units, typename Feed>
static sgz_status pcmOneShot(const sgz_spectrum_config *cfg, uint32_t format, uint32_t src_channels, const uint32_t *channel_map, size_t nsamples,
                             sgz_pcm_timing *timing, Units units, Feed feed)
{
    const auto t0 = PcmClock::now();
    sgz_pcm_stream *s = nullptr;
    const uint32_t frameBytes = std::max(1u, src_channels * pcmSampleBytes(format));
    const size_t chunk = std::min(std::min(kPcmDefaultChunk, kPcmDefaultSlotBytes / frameBytes), std::max<size_t>(nsamples, 1));
    if (sgz_status st = sgz_pcm_stream_create(cfg, format, src_channels, channel_map, chunk, &s); st != SGZ_OK) return st;
    const uint64_t yields = units(s);
    sgz_status st = SGZ_SKIPPED_FRAME;
    if (yields == 0) { if (timing) *timing = sgz_pcm_timing{}; }
    else st = feed(s, yields);
    const std::string keep = g_lastError;
    sgz_pcm_stream_destroy(s);
    g_lastError = keep;
    if (timing && st == SGZ_OK) timing->wall_ms = pcmMsSince(t0);
    return st;
}

// columns a feed of nsamples yields at k with the stream as it is; false: k == 0, or a k other than the open column's
static bool pcmOverviewNeed(const sgz_pcm_stream *s, size_t nsamples, uint32_t k, int flush, uint64_t *columns)
{
    if (!s || k == 0 || (s->ovOpen && k != s->ovK)) return false;
    const uint64_t t = s->ovOpen + sgz_pcm_stream_frames_for(s, nsamples);
    *columns = t / k + ((flush && t % k) ? 1u : 0u);
    return true;
}

extern "C" {

uint32_t sgz_pcm_sample_bytes(uint32_t format) { return pcmSampleBytes(format); }

sgz_status sgz_stream_step(uint32_t window_size, uint32_t hop, uint64_t held, uint64_t incoming, uint64_t *frames, uint64_t *keep)
{
    return streamStep(window_size, hop, held, incoming, frames, keep);
}

sgz_status sgz_pcm_to_planar_device(const void *d_pcm, uint32_t format, uint32_t src_channels, size_t nsamples, const uint32_t *channel_map,
                                    uint32_t num_channels, float *d_planar, size_t channel_stride, void *stream)
{
    PcmMap map;
    if (sgz_status st = checkPcmLayout(format, src_channels, channel_map, num_channels, map); st != SGZ_OK) return st;
    return launchPcmToPlanar(d_pcm, format, src_channels, nsamples, map, num_channels, d_planar, channel_stride, reinterpret_cast<hipStream_t>(stream));
}

void sgz_pcm_stream_destroy(sgz_pcm_stream *s)
{
    if (!s) return;
    for (hipStream_t q : {s->copy, s->compute, s->back}) if (q) (void)hipStreamSynchronize(q);
    for (PcmSlot &sl : s->slot) {
        if (sl.h_pcm) (void)hipHostFree(sl.h_pcm);
        if (sl.d_pcm) (void)hipFree(sl.d_pcm);
        for (PcmOut &o : sl.out) o.release();
        for (hipEvent_t e : sl.ev) if (e) (void)hipEventDestroy(e);
    }
    for (void *p : {(void *)s->d_planar[0], (void *)s->d_planar[1], (void *)s->d_state, (void *)s->d_ovCarry, (void *)s->d_wvCarry, (void *)s->d_lvCarry, (void *)s->d_tpCarry, (void *)s->d_ldCarry, s->d_ldScratch}) if (p) (void)hipFree(p);
    for (hipStream_t q : {s->copy, s->compute, s->back}) if (q) (void)hipStreamDestroy(q);
    if (s->plan) sgz_plan_destroy(s->plan);
    delete s;
}

sgz_status sgz_pcm_stream_create(const sgz_spectrum_config *cfg, uint32_t format, uint32_t src_channels, const uint32_t *channel_map,
                                 size_t chunk_samples, sgz_pcm_stream **out)
{
    if (!cfg || !out) return fail(SGZ_EINVAL, "null argument");
    sgz_pcm_stream *s = new (std::nothrow) sgz_pcm_stream();
    if (!s) return fail(SGZ_ENOMEM, "out of memory");
    auto bail = [&](sgz_status st) { const std::string keep = g_lastError; sgz_pcm_stream_destroy(s); g_lastError = keep; return st; };
    if (sgz_status st = sgz_plan_create(cfg, &s->plan); st != SGZ_OK) return bail(st);
    if (cfg->algorithm == SGZ_ALGO_RSNT)
        return bail(fail(SGZ_EUNSUPPORTED, "sgz_pcm_stream: RSNT launches chain their frames within an fp32 bar, a chunked render would not equal the single one"));
    if (cfg->hop > cfg->window_size) return bail(fail(SGZ_EUNSUPPORTED, "sgz_pcm_stream: hop > window_size"));
    if (cfg->num_pairs > kPcmMaxChannels / 2) return bail(fail(SGZ_EINVAL, "sgz_pcm_stream: at most 32 pairs"));
    s->cfg = *cfg; s->format = format; s->srcChannels = src_channels; s->numChannels = 2 * cfg->num_pairs;
    if (sgz_status st = checkPcmLayout(format, src_channels, channel_map, s->numChannels, s->map); st != SGZ_OK) return bail(st);
    if (chunk_samples > kPcmMaxChunk) return bail(fail(SGZ_EINVAL, "sgz_pcm_stream: chunk_samples above 2^26"));
    s->frameBytes = src_channels * pcmSampleBytes(format);
    s->chunk = chunk_samples ? chunk_samples : std::min(kPcmDefaultChunk, kPcmDefaultSlotBytes / s->frameBytes);
    s->stride = (size_t(cfg->window_size) - 1 + s->chunk + 63) & ~size_t(63);       // the held tail (< W) and a piece behind it; 256-byte rows
    s->maxFrames = (s->chunk - 1) / cfg->hop + 1;
    if (sgz_status st = sgz_plan_upload(s->plan); st != SGZ_OK) return bail(st);
#define SGZ_PCM_TRY(call) do { if (hipError_t e_ = (call); e_ != hipSuccess) return bail(hipFail(e_, #call)); } while (0)
    for (hipStream_t *q : {&s->copy, &s->compute, &s->back}) SGZ_PCM_TRY(hipStreamCreateWithFlags(q, hipStreamNonBlocking));
    for (PcmSlot &sl : s->slot) {
        for (hipEvent_t &e : sl.ev) SGZ_PCM_TRY(hipEventCreate(&e));
        SGZ_PCM_TRY(hipMalloc(&sl.d_pcm, s->chunk * s->frameBytes));
        if (sgz_status st = sl.out[kOutImage].reserve(pcmImageBytes(*s, s->maxFrames), false); st != SGZ_OK) return bail(st);
    }
    for (float *&p : s->d_planar) SGZ_PCM_TRY(hipMalloc(reinterpret_cast<void **>(&p), size_t(s->numChannels) * s->stride * sizeof(float)));
    SGZ_PCM_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_state), pcmStateBytes(*s)));
    SGZ_PCM_TRY(hipMemset(s->d_state, 0, pcmStateBytes(*s)));
#undef SGZ_PCM_TRY
    *out = s;
    return SGZ_OK;
}

uint64_t sgz_pcm_stream_frames_for(const sgz_pcm_stream *s, size_t nsamples)
{
    uint64_t frames = 0, keep = 0;
    if (!s || streamStep(s->cfg.window_size, s->cfg.hop, s->held, nsamples, &frames, &keep) != SGZ_OK) return 0;
    return frames;
}

sgz_status sgz_pcm_stream_reset(sgz_pcm_stream *s)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    SGZ_HIP(hipMemsetAsync(s->d_state, 0, pcmStateBytes(*s), s->compute));          // (in order behind whatever the last feed left there: nothing)
    SGZ_HIP(hipStreamSynchronize(s->compute));
    s->held = 0;
    s->ovOpen = 0;                                                                  // an open overview column is dropped
    s->wvOpen = 0; s->wvCursor = 0;                                                 // and the waveform's; its columns start over
    s->trCursor = 0;                                                                // the track's records too; the lane stays armed
    s->lvOpen = 0; s->lvCursor = 0;                                                 // the level lane as the waveform's
    s->tpOpen = 0; s->tpCursor = 0; s->tpContinued = false;                         // the true-peak lane too, and its history is zeros again
    s->ldOpen = 0; s->ldCursor = 0; s->ldIndex = 0; s->ldContinued = false;         // the loudness lane as that one; its samples count from 0 again
    return SGZ_OK;
}

sgz_status sgz_pcm_stream_feed(sgz_pcm_stream *s, const void *pcm, size_t nsamples, uint8_t *rgba_out, float *lines_out,
                               uint64_t capacity_frames, uint64_t *frames_out, sgz_pcm_timing *timing)
{
    const auto t0 = PcmClock::now();
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (!pcm && nsamples) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: null pcm");
    if (s->ovOpen) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: an overview column is open -- flush it (sgz_pcm_stream_feed_overview) or reset the stream first");
    const uint64_t need = sgz_pcm_stream_frames_for(s, nsamples);
    if (frames_out) *frames_out = need;
    if (capacity_frames < need) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: capacity_frames below what this feed yields (see *frames_out)");
    if (need && !rgba_out) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: null rgba_out");
    if (sgz_status st = pcmWaveFits(*s, nsamples); st != SGZ_OK) return st;
    if (sgz_status st = pcmLevelFits(*s, nsamples); st != SGZ_OK) return st;
    if (sgz_status st = pcmTruePeakFits(*s, nsamples); st != SGZ_OK) return st;
    if (sgz_status st = pcmLoudnessFits(*s, nsamples); st != SGZ_OK) return st;
    if (sgz_status st = pcmTrackFits(*s, need); st != SGZ_OK) return st;
    PcmFramesPart part{rgba_out, lines_out, need, need && isPinnedHost(rgba_out), need && lines_out && isPinnedHost(lines_out)};
    return pcmFeed(*s, pcm, nsamples, false, part, frames_out, timing, t0);
}

sgz_status sgz_spectrogram_render_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                      const uint32_t *channel_map, size_t nsamples, uint8_t *rgba_out, float *lines_out, sgz_pcm_timing *timing)
{
    if (!cfg || !pcm || !rgba_out) return fail(SGZ_EINVAL, "null argument");
    return pcmOneShot(cfg, format, src_channels, channel_map, nsamples, timing,
                      [&](sgz_pcm_stream *s) { return sgz_pcm_stream_frames_for(s, nsamples); },
                      [&](sgz_pcm_stream *s, uint64_t frames) { return sgz_pcm_stream_feed(s, pcm, nsamples, rgba_out, lines_out, frames, &frames, timing); });
}

// ---- the overview inside the stream (sgz.h, "the overview inside sgz_pcm_stream") ----------------------------------------------------------
uint64_t sgz_pcm_stream_columns_for(const sgz_pcm_stream *s, size_t nsamples, uint32_t k, int flush)
{
    uint64_t columns = 0;
    return pcmOverviewNeed(s, nsamples, k, flush, &columns) ? columns : 0;
}

uint64_t sgz_pcm_stream_open_frames(const sgz_pcm_stream *s) { return s ? s->ovOpen : 0; }

sgz_status sgz_pcm_stream_set_option(sgz_pcm_stream *s, uint32_t option, uint32_t value)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    return sgz_plan_set_option(s->plan, option, value);
}

sgz_status sgz_pcm_stream_feed_overview(sgz_pcm_stream *s, const void *pcm, size_t nsamples, uint32_t k, int flush, uint8_t *rgba_out, float *peaks_out,
                                        uint64_t capacity_columns, uint64_t *columns_out, sgz_pcm_timing *timing)
{
    const auto t0 = PcmClock::now();
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (!pcm && nsamples) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview: null pcm");
    if (k == 0) return fail(SGZ_EINVAL, "overview: k >= 1 frames per column");
    if (!rgba_out && !peaks_out) return fail(SGZ_EINVAL, "overview: an image, the peaks or both");
    if (s->ovOpen && k != s->ovK) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview: k differs from the open column's -- flush or reset first");
    uint64_t need = 0;
    (void)pcmOverviewNeed(s, nsamples, k, flush, &need);
    if (columns_out) *columns_out = need;
    if (capacity_columns < need) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview: capacity_columns below what this feed yields (see *columns_out)");
    if (sgz_status st = pcmWaveFits(*s, nsamples); st != SGZ_OK) return st;
    if (sgz_status st = pcmLevelFits(*s, nsamples); st != SGZ_OK) return st;
    if (sgz_status st = pcmTruePeakFits(*s, nsamples); st != SGZ_OK) return st;
    if (sgz_status st = pcmLoudnessFits(*s, nsamples); st != SGZ_OK) return st;
    if (sgz_status st = pcmTrackFits(*s, sgz_pcm_stream_frames_for(s, nsamples)); st != SGZ_OK) return st;
    PcmColumnsPart part{rgba_out, peaks_out, k, flush, need, need && rgba_out && isPinnedHost(rgba_out), need && peaks_out && isPinnedHost(peaks_out)};
    // (a feed without samples still has one piece when it flushes an open column)
    return pcmFeed(*s, pcm, nsamples, flush && s->ovOpen, part, columns_out, timing, t0);
}

sgz_status sgz_spectrogram_overview_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                        const uint32_t *channel_map, size_t nsamples, uint32_t k, uint8_t *rgba_out, float *peaks_out, sgz_pcm_timing *timing)
{
    if (!cfg || !pcm) return fail(SGZ_EINVAL, "null argument");
    if (k == 0) return fail(SGZ_EINVAL, "overview: k >= 1 frames per column");
    if (!rgba_out && !peaks_out) return fail(SGZ_EINVAL, "overview: an image, the peaks or both");
    return pcmOneShot(cfg, format, src_channels, channel_map, nsamples, timing,
                      [&](sgz_pcm_stream *s) { return sgz_pcm_stream_columns_for(s, nsamples, k, 1); },
                      [&](sgz_pcm_stream *s, uint64_t columns) { return sgz_pcm_stream_feed_overview(s, pcm, nsamples, k, 1, rgba_out, peaks_out, columns, &columns, timing); });
}

// ---- the waveform lane's calls ----------------------------------------------------------------------------------------------------------------
sgz_status sgz_pcm_stream_set_waveform(sgz_pcm_stream *s, uint32_t m, float *wave_out, uint64_t capacity_columns)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (m == 0) {                                                  // off: the open column is dropped
        s->wvM = 0; s->wvOut = nullptr; s->wvCap = s->wvCursor = s->wvOpen = 0;
        return SGZ_OK;
    }
    if (!wave_out && capacity_columns) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_waveform: null wave_out");
    if (reinterpret_cast<uintptr_t>(wave_out) % alignof(float)) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_waveform: wave_out is not aligned to float");
    if (s->wvOpen && m != s->wvM) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_waveform: m differs from the open column's -- flush it (sgz_pcm_stream_flush_waveform), disarm or reset first");
    if (!s->d_wvCarry) SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_wvCarry), size_t(2) * s->numChannels * 2 * sizeof(float)));
    s->wvM = m; s->wvOut = wave_out; s->wvCap = capacity_columns; s->wvCursor = 0;
    s->wvPinned = capacity_columns && isPinnedHost(wave_out);
    return SGZ_OK;
}

uint64_t sgz_pcm_stream_waveform_for(const sgz_pcm_stream *s, size_t nsamples, int flush)
{
    if (!s || !s->wvM) return 0;
    const uint64_t t = s->wvOpen + nsamples;
    return t / s->wvM + ((flush && t % s->wvM) ? 1u : 0u);
}

sgz_status sgz_pcm_stream_waveform_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (columns_written) *columns_written = s->wvCursor;
    if (open_samples) *open_samples = s->wvOpen;
    return SGZ_OK;
}

sgz_status sgz_pcm_stream_flush_waveform(sgz_pcm_stream *s)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (!s->wvM) return fail(SGZ_EINVAL, "sgz_pcm_stream_flush_waveform: the lane is off (sgz_pcm_stream_set_waveform)");
    if (!s->wvOpen) return SGZ_OK;
    if (s->wvCursor >= s->wvCap) return fail(SGZ_EINVAL, "sgz_pcm_stream_flush_waveform: no column left in the buffer (re-arm with sgz_pcm_stream_set_waveform)");
    PcmSlot &sl = s->slot[0];                                      // (both slots are idle between feeds)
    if (sgz_status st = pcmWaveBuffers(*s, sl); st != SGZ_OK) return st;
    const WaveColumnsShape sh = waveColumnsShape(s->numChannels, 0, s->wvM, uint32_t(s->wvOpen), 1, 0);
    const sgz_status st = runWaveColumns(sh, s->d_planar[s->cur], s->stride, s->numChannels, 0, s->wvM, uint32_t(s->wvOpen), pcmWaveCarry(*s, s->wvCur),
                                         pcmWaveCarry(*s, s->wvCur ^ 1), sl.out[kOutWave].as<float>(), nullptr, s->compute);
    if (st != SGZ_OK) return st;
    // the one column behind the launch on the compute stream itself, and waited for
    const size_t column = size_t(s->numChannels) * 2;
    PcmOut &out = sl.out[kOutWave];
    if (sgz_status rb = out.readBack(s->wvOut + size_t(s->wvCursor) * column, column * sizeof(float), s->wvPinned, s->compute); rb != SGZ_OK) return rb;
    if (const hipError_t e = hipStreamSynchronize(s->compute); e != hipSuccess) { out.dst = nullptr; return hipFail(e, "hipStreamSynchronize(s->compute)"); }
    out.drain();
    s->wvOpen = 0;
    ++s->wvCursor;
    return SGZ_OK;
}

// ---- the level lane's calls -------------------------------------------------------------------------------------------------------------------
sgz_status sgz_pcm_stream_set_level(sgz_pcm_stream *s, uint32_t m, sgz_level_record *level_out, uint64_t capacity_columns)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (m == 0) {                                                  // off: the open column is dropped
        s->lvM = 0; s->lvOut = nullptr; s->lvCap = s->lvCursor = s->lvOpen = 0;
        return SGZ_OK;
    }
    if (!level_out && capacity_columns) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_level: null level_out");
    if (reinterpret_cast<uintptr_t>(level_out) % alignof(sgz_level_record)) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_level: level_out is not aligned to 8 bytes");
    if (s->lvOpen && m != s->lvM) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_level: m differs from the open column's -- flush it (sgz_pcm_stream_flush_level), disarm or reset first");
    if (!s->d_lvCarry) SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_lvCarry), size_t(2) * s->cfg.num_pairs * sizeof(sgz_level_record)));
    s->lvM = m; s->lvOut = level_out; s->lvCap = capacity_columns; s->lvCursor = 0;
    s->lvPinned = capacity_columns && isPinnedHost(level_out);
    return SGZ_OK;
}

uint64_t sgz_pcm_stream_level_for(const sgz_pcm_stream *s, size_t nsamples, int flush)
{
    if (!s || !s->lvM) return 0;
    const uint64_t t = s->lvOpen + nsamples;
    return t / s->lvM + ((flush && t % s->lvM) ? 1u : 0u);
}

sgz_status sgz_pcm_stream_level_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (columns_written) *columns_written = s->lvCursor;
    if (open_samples) *open_samples = s->lvOpen;
    return SGZ_OK;
}

sgz_status sgz_pcm_stream_flush_level(sgz_pcm_stream *s)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (!s->lvM) return fail(SGZ_EINVAL, "sgz_pcm_stream_flush_level: the lane is off (sgz_pcm_stream_set_level)");
    if (!s->lvOpen) return SGZ_OK;
    if (s->lvCursor >= s->lvCap) return fail(SGZ_EINVAL, "sgz_pcm_stream_flush_level: no column left in the buffer (re-arm with sgz_pcm_stream_set_level)");
    PcmSlot &sl = s->slot[0];                                      // (both slots are idle between feeds)
    if (sgz_status st = pcmLevelBuffers(*s, sl); st != SGZ_OK) return st;
    const uint32_t pairs = s->cfg.num_pairs;
    const LevelColumnsShape sh = levelColumnsShape(pairs, 0, s->lvM, uint32_t(s->lvOpen), 1, 0);
    const sgz_status st = runLevelColumns(sh, s->d_planar[s->cur], s->stride, pairs, 0, s->lvM, uint32_t(s->lvOpen), pcmLevelCarry(*s, s->lvCur),
                                          pcmLevelCarry(*s, s->lvCur ^ 1), sl.out[kOutLevel].as<sgz_level_record>(), nullptr, s->compute);
    if (st != SGZ_OK) return st;
    // the one column behind the launch on the compute stream itself, and waited for
    PcmOut &out = sl.out[kOutLevel];
    if (sgz_status rb = out.readBack(s->lvOut + size_t(s->lvCursor) * pairs, pairs * sizeof(sgz_level_record), s->lvPinned, s->compute); rb != SGZ_OK) return rb;
    if (const hipError_t e = hipStreamSynchronize(s->compute); e != hipSuccess) { out.dst = nullptr; return hipFail(e, "hipStreamSynchronize(s->compute)"); }
    out.drain();
    s->lvOpen = 0;
    ++s->lvCursor;
    return SGZ_OK;
}

// ---- the true-peak lane's calls ---------------------------------------------------------------------------------------------------------------
sgz_status sgz_pcm_stream_set_truepeak(sgz_pcm_stream *s, uint32_t m, sgz_truepeak_record *out, uint64_t capacity_columns)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (m == 0) {                                                  // off: the open column and the history are dropped
        s->tpM = 0; s->tpOut = nullptr; s->tpCap = s->tpCursor = s->tpOpen = 0; s->tpContinued = false;
        return SGZ_OK;
    }
    if (!out && capacity_columns) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_truepeak: null out");
    if (reinterpret_cast<uintptr_t>(out) % alignof(sgz_truepeak_record)) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_truepeak: out is not aligned to 8 bytes");
    if (s->tpOpen && m != s->tpM) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_truepeak: m differs from the open column's -- flush it (sgz_pcm_stream_flush_truepeak), disarm or reset first");
    if (!s->d_tpCarry) SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_tpCarry), size_t(2) * s->numChannels * sizeof(sgz_truepeak_carry)));
    if (m != s->tpM) s->tpContinued = false;                       // (arming: the lane starts at the next sample with a zero history; the same m keeps it)
    s->tpM = m; s->tpOut = out; s->tpCap = capacity_columns; s->tpCursor = 0;
    s->tpPinned = capacity_columns && isPinnedHost(out);
    return SGZ_OK;
}

uint64_t sgz_pcm_stream_truepeak_for(const sgz_pcm_stream *s, size_t nsamples, int flush)
{
    if (!s || !s->tpM) return 0;
    const uint64_t t = s->tpOpen + nsamples;
    return t / s->tpM + ((flush && t % s->tpM) ? 1u : 0u);
}

sgz_status sgz_pcm_stream_truepeak_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (columns_written) *columns_written = s->tpCursor;
    if (open_samples) *open_samples = s->tpOpen;
    return SGZ_OK;
}

sgz_status sgz_pcm_stream_flush_truepeak(sgz_pcm_stream *s)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (!s->tpM) return fail(SGZ_EINVAL, "sgz_pcm_stream_flush_truepeak: the lane is off (sgz_pcm_stream_set_truepeak)");
    if (!s->tpOpen) return SGZ_OK;
    if (s->tpCursor >= s->tpCap) return fail(SGZ_EINVAL, "sgz_pcm_stream_flush_truepeak: no column left in the buffer (re-arm with sgz_pcm_stream_set_truepeak)");
    PcmSlot &sl = s->slot[0];                                      // (both slots are idle between feeds)
    if (sgz_status st = pcmTruePeakBuffers(*s, sl); st != SGZ_OK) return st;
    const uint32_t channels = s->numChannels;
    // the emit launch alone, on the open column of the current half; the carry, and with it the history, stays where it is
    const TruePeakColumnsShape sh = truePeakColumnsShape(channels, 0, s->tpM, uint32_t(s->tpOpen), 1, 0);
    const sgz_status st = runTruePeakColumns(sh, s->d_planar[s->cur], s->stride, channels, 0, s->tpM, uint32_t(s->tpOpen), 1u, pcmTruePeakCarry(*s, s->tpCur),
                                             pcmTruePeakCarry(*s, s->tpCur ^ 1), sl.out[kOutTruePeak].as<sgz_truepeak_record>(), nullptr, s->compute);
    if (st != SGZ_OK) return st;
    // the one column behind the launch on the compute stream itself, and waited for
    PcmOut &out = sl.out[kOutTruePeak];
    if (sgz_status rb = out.readBack(s->tpOut + size_t(s->tpCursor) * channels, channels * sizeof(sgz_truepeak_record), s->tpPinned, s->compute); rb != SGZ_OK) return rb;
    if (const hipError_t e = hipStreamSynchronize(s->compute); e != hipSuccess) { out.dst = nullptr; return hipFail(e, "hipStreamSynchronize(s->compute)"); }
    out.drain();
    s->tpOpen = 0;
    ++s->tpCursor;
    return SGZ_OK;
}

// ---- the loudness lane's calls ----------------------------------------------------------------------------------------------------------------
sgz_status sgz_pcm_stream_set_loudness(sgz_pcm_stream *s, const sgz_loudness_filter *filter, uint32_t m, sgz_loudness_record *out, uint64_t capacity_columns)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (m == 0) {                                                  // off: the open column, the history and the index are dropped
        s->ldM = 0; s->ldOut = nullptr; s->ldCap = s->ldCursor = s->ldOpen = s->ldIndex = 0; s->ldContinued = false;
        return SGZ_OK;
    }
    if (!filter) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_loudness: null filter");
    if (!out && capacity_columns) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_loudness: null out");
    if (reinterpret_cast<uintptr_t>(out) % alignof(sgz_loudness_record)) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_loudness: out is not aligned to 8 bytes");
    const bool same = s->ldM == m && std::memcmp(&s->ldFilter, filter, sizeof *filter) == 0;
    if (s->ldOpen && !same) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_loudness: m or the filter differs from the open column's -- flush it (sgz_pcm_stream_flush_loudness), disarm or reset first");
    if (!same) {
        // (what the stage call refuses, and the tap table: a refused filter arms nothing)
        size_t bytes = 0;
        if (sgz_status st = sgz_loudness_columns_limits(filter, s->numChannels, nullptr, nullptr, &bytes); st != SGZ_OK) return st;
        std::vector<int32_t> taps(size_t(4) * filter->W);
        if (sgz_status st = sgz_loudness_taps(filter, taps.data()); st != SGZ_OK) return st;
        if (s->ldCarryCap < 2 * bytes) {
            // (both slots are idle between feeds, but a flush's launch may still read the old block: wait for it)
            SGZ_HIP(hipStreamSynchronize(s->compute));
            if (s->d_ldCarry) { (void)hipFree(s->d_ldCarry); s->d_ldCarry = nullptr; s->ldCarryCap = 0; }
            SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_ldCarry), 2 * bytes));
            s->ldCarryCap = 2 * bytes;
        }
        s->ldFilter = *filter;
        s->ldContinued = false;                                    // (arming: the lane starts at the next sample, index 0, with a zero history)
        s->ldIndex = 0; s->ldCur = 0;
    }
    s->ldM = m; s->ldOut = out; s->ldCap = capacity_columns; s->ldCursor = 0;
    s->ldPinned = capacity_columns && isPinnedHost(out);
    return SGZ_OK;
}

uint64_t sgz_pcm_stream_loudness_for(const sgz_pcm_stream *s, size_t nsamples, int flush)
{
    if (!s || !s->ldM) return 0;
    const uint64_t t = s->ldOpen + nsamples;
    return t / s->ldM + ((flush && t % s->ldM) ? 1u : 0u);
}

sgz_status sgz_pcm_stream_loudness_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (columns_written) *columns_written = s->ldCursor;
    if (open_samples) *open_samples = s->ldOpen;
    return SGZ_OK;
}

sgz_status sgz_pcm_stream_flush_loudness(sgz_pcm_stream *s)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (!s->ldM) return fail(SGZ_EINVAL, "sgz_pcm_stream_flush_loudness: the lane is off (sgz_pcm_stream_set_loudness)");
    if (!s->ldOpen) return SGZ_OK;
    if (s->ldCursor >= s->ldCap) return fail(SGZ_EINVAL, "sgz_pcm_stream_flush_loudness: no column left in the buffer (re-arm with sgz_pcm_stream_set_loudness)");
    PcmSlot &sl = s->slot[0];                                      // (both slots are idle between feeds)
    if (sgz_status st = pcmLoudnessBuffers(*s, sl); st != SGZ_OK) return st;
    const uint32_t channels = s->numChannels;
    // the emit launch alone, on the open column of the current half; the carry, and with it the history and the segment grid, stays where it is
    const LoudnessColumnsShape sh = loudnessColumnsShape(channels, 0, s->ldM, uint32_t(s->ldOpen), 1, 0);
    const sgz_status st = runLoudnessColumns(sh, s->ldFilter, s->d_planar[s->cur], s->stride, channels, 0, s->ldIndex, s->ldM, uint32_t(s->ldOpen), 1u,
                                             pcmLoudnessCarry(*s, s->ldCur), pcmLoudnessCarry(*s, s->ldCur ^ 1), sl.out[kOutLoudness].as<sgz_loudness_record>(),
                                             nullptr, s->compute);
    if (st != SGZ_OK) return st;
    // the one column behind the launch on the compute stream itself, and waited for
    PcmOut &out = sl.out[kOutLoudness];
    if (sgz_status rb = out.readBack(s->ldOut + size_t(s->ldCursor) * channels, channels * sizeof(sgz_loudness_record), s->ldPinned, s->compute); rb != SGZ_OK) return rb;
    if (const hipError_t e = hipStreamSynchronize(s->compute); e != hipSuccess) { out.dst = nullptr; return hipFail(e, "hipStreamSynchronize(s->compute)"); }
    out.drain();
    s->ldOpen = 0;
    ++s->ldCursor;
    return SGZ_OK;
}

// ---- the track lane's calls -------------------------------------------------------------------------------------------------------------------
sgz_status sgz_pcm_stream_set_track(sgz_pcm_stream *s, uint32_t graph, double mouse_fraction, sgz_line_peak *track_out, uint64_t capacity_frames)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (graph >= SGZ_NUM_GRAPHS) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_track: graph");
    if (!std::isfinite(mouse_fraction)) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_track: mouse_fraction");
    if (!track_out && capacity_frames) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_track: null track_out");
    if (reinterpret_cast<uintptr_t>(track_out) % alignof(sgz_line_peak)) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_track: track_out is not aligned to double");
    s->trArmed = track_out != nullptr;                             // NULL with capacity 0: off
    s->trGraph = graph; s->trFraction = mouse_fraction; s->trOut = track_out; s->trCap = capacity_frames; s->trCursor = 0;
    s->trPinned = capacity_frames && isPinnedHost(track_out);
    return SGZ_OK;
}

uint64_t sgz_pcm_stream_track_for(const sgz_pcm_stream *s, size_t nsamples)
{
    return s && s->trArmed ? sgz_pcm_stream_frames_for(s, nsamples) : 0;
}

sgz_status sgz_pcm_stream_track_state(const sgz_pcm_stream *s, uint64_t *frames_written)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (frames_written) *frames_written = s->trCursor;
    return SGZ_OK;
}

}  // extern "C"
