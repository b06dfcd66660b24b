// pcm.hip -- interleaved PCM in (include/sgz.h "interleaved PCM in"): the convert-and-de-interleave kernel, and the stream handle that
// cuts a feed into pieces and runs upload / convert + render / read-back of neighbouring pieces side by side on three streams; armed, the
// waveform lane (wave_columns.hip) reduces every piece's new samples behind the converter and its columns ride the same read-back; armed, the
// track lane (tracker.hip) searches every piece's line results behind its render and its records ride it too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
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

template <uint32_t FORMAT> struct PcmBytes;
template <> struct PcmBytes<SGZ_PCM_F32> { static constexpr uint32_t value = 4; };
template <> struct PcmBytes<SGZ_PCM_U8> { static constexpr uint32_t value = 1; };
template <> struct PcmBytes<SGZ_PCM_S16> { static constexpr uint32_t value = 2; };
template <> struct PcmBytes<SGZ_PCM_S24> { static constexpr uint32_t value = 3; };
template <> struct PcmBytes<SGZ_PCM_S32> { static constexpr uint32_t value = 4; };
template <> struct PcmBytes<SGZ_PCM_F64> { static constexpr uint32_t value = 8; };

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
    constexpr uint32_t kBytes = PcmBytes<FORMAT>::value;
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

static uint32_t pcmAlignment(uint32_t format)
{
    return format == SGZ_PCM_S16 ? 2u : (format == SGZ_PCM_S32 || format == SGZ_PCM_F32) ? 4u : format == SGZ_PCM_F64 ? 8u : 1u;
}

static uint32_t pcmSampleBytes(uint32_t format)
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

struct PcmSlot {                        // what one piece in flight owns; a slot is reused by the piece after next
    void *h_pcm = nullptr;              // pinned [chunk][frameBytes], made when the first pageable feed arrives
    void *d_pcm = nullptr;
    uint8_t *d_rgba = nullptr, *h_rgba = nullptr;       // [maxFrames][P][4]; the pinned twin when rgba_out is pageable
    float *d_lines = nullptr, *h_lines = nullptr;       // [maxFrames][C][graphs][P][2], made when lines are first asked for
    hipEvent_t ev[7] = {};              // upload begin / END (copy stream); convert begin, convert end, render END (compute); read-back begin / END
                                        // (the capitals order the streams; the others are recorded for a caller that asks for timing only: a
                                        // marker costs the stream it sits on microseconds, api.hip sgz_render_queue_submit)
    bool timed = false;
    bool busy = false, rendered = false;            // rendered: the piece has a read-back (frames, overview or waveform columns), ev[6] is recorded
    // the host's part of the read-back, done when the slot is drained
    uint8_t *rgbaDst = nullptr; float *linesDst = nullptr; size_t rgbaBytes = 0, linesBytes = 0;
    const uint8_t *rgbaFrom = nullptr; const float *linesFrom = nullptr;       // the pinned twins the drain copies from
    // the overview's columns of one piece (sgz_pcm_stream_feed_overview): [ovCap][P][4] and V [ovCap][C][P] with their pinned twins, made on
    // first need and grown when a later k needs more columns per piece
    uint8_t *d_ovRgba = nullptr, *h_ovRgba = nullptr; float *d_ovPeaks = nullptr, *h_ovPeaks = nullptr;
    size_t ovRgbaCap = 0, ovRgbaPinnedCap = 0, ovPeaksCap = 0, ovPeaksPinnedCap = 0;       // columns
    // the waveform lane's columns of one piece (sgz_pcm_stream_set_waveform): float2 [waveCap][channels] with its pinned twin, made on first
    // need and grown when a later m needs more columns per piece; waveDst: where the drain copies the twin's waveBytes to
    float *d_wave = nullptr, *h_wave = nullptr, *waveDst = nullptr;
    size_t waveCap = 0, wavePinnedCap = 0, waveBytes = 0;
    // the track lane's records of one piece (sgz_pcm_stream_set_track): sgz_line_peak [maxFrames][pairs] with its pinned twin, made on first
    // need; trackDst: where the drain copies the twin's trackBytes to
    sgz_line_peak *d_track = nullptr, *h_track = nullptr, *trackDst = nullptr;
    size_t trackCap = 0, trackPinnedCap = 0, trackBytes = 0;
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
};

struct sgz_plan { Plan impl; };

static size_t pcmStateBytes(const sgz_pcm_stream &s) { return size_t(s.cfg.num_pairs) * SGZ_NUM_GRAPHS * s.cfg.axis_points * 2 * sizeof(float); }
static size_t pcmLinesFloats(const sgz_pcm_stream &s, uint64_t frames) { return size_t(frames) * s.cfg.num_pairs * SGZ_NUM_GRAPHS * s.cfg.axis_points * 2; }

// waits for the piece that used the slot, hands its columns to the caller (pageable destinations) and adds its event intervals up
static sgz_status pcmDrain(PcmSlot &sl, sgz_pcm_timing *timing)
{
    if (!sl.busy) return SGZ_OK;
    sl.busy = false;
    SGZ_HIP(hipEventSynchronize(sl.ev[sl.rendered ? 6 : 4]));
    if (sl.rgbaDst) std::memcpy(sl.rgbaDst, sl.rgbaFrom, sl.rgbaBytes);
    if (sl.linesDst) std::memcpy(sl.linesDst, sl.linesFrom, sl.linesBytes);
    if (sl.waveDst) std::memcpy(sl.waveDst, sl.h_wave, sl.waveBytes);
    if (sl.trackDst) std::memcpy(sl.trackDst, sl.h_track, sl.trackBytes);
    sl.rgbaDst = nullptr; sl.linesDst = nullptr; sl.waveDst = nullptr; sl.trackDst = nullptr;
    if (timing && sl.timed) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sl.ev[0], sl.ev[1]) == hipSuccess) timing->h2d_ms += ms;
        if (hipEventElapsedTime(&ms, sl.ev[2], sl.ev[3]) == hipSuccess) timing->convert_ms += ms;
        if (hipEventElapsedTime(&ms, sl.ev[3], sl.ev[4]) == hipSuccess) timing->render_ms += ms;
        if (sl.rendered && hipEventElapsedTime(&ms, sl.ev[5], sl.ev[6]) == hipSuccess) timing->d2h_ms += ms;
    }
    return SGZ_OK;
}

// a device or pinned block of at least `need` columns of `bytes` each (the slot is idle: nothing in flight reads the old one)
template <typename T>
static sgz_status pcmGrow(T **buf, size_t *cap, size_t need, size_t bytes, bool pinned)
{
    if (*cap >= need) return SGZ_OK;
    if (*buf) { (void)(pinned ? hipHostFree(*buf) : hipFree(*buf)); *buf = nullptr; *cap = 0; }
    if (pinned) SGZ_HIP(hipHostMalloc(reinterpret_cast<void **>(buf), need * bytes, hipHostMallocDefault));
    else SGZ_HIP(hipMalloc(reinterpret_cast<void **>(buf), need * bytes));
    *cap = need;
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
    if (!s.wvM) return SGZ_OK;
    const size_t columns = (s.chunk + s.wvM - 1) / s.wvM + 1, bytes = size_t(s.numChannels) * 2 * sizeof(float);
    if (sgz_status st = pcmGrow(&sl.d_wave, &sl.waveCap, columns, bytes, false); st != SGZ_OK) return st;
    return s.wvPinned ? SGZ_OK : pcmGrow(&sl.h_wave, &sl.wavePinnedCap, columns, bytes, true);
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
                                         sl.d_wave, scratch.p, s.compute);
    if (st != SGZ_OK) return st;
    if (sh.open) s.wvCur ^= 1;
    s.wvOpen = (s.wvOpen + n) % s.wvM;
    *columns = sh.closed;
    return SGZ_OK;
}

// the piece's columns to the caller's buffer at the cursor, on the read-back stream (behind ev[4]); pageable: to the twin, the drain copies
static sgz_status pcmWaveReadBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t columns)
{
    if (!columns) return SGZ_OK;
    const size_t column = size_t(s.numChannels) * 2;
    float *at = s.wvOut + size_t(s.wvCursor) * column;
    sl.waveBytes = size_t(columns) * column * sizeof(float);
    SGZ_HIP(hipMemcpyAsync(s.wvPinned ? at : sl.h_wave, sl.d_wave, sl.waveBytes, hipMemcpyDeviceToHost, s.back));
    sl.waveDst = s.wvPinned ? nullptr : at;
    s.wvCursor += columns;
    return SGZ_OK;
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
    if (!s.trArmed) return SGZ_OK;
    const size_t bytes = size_t(s.cfg.num_pairs) * sizeof(sgz_line_peak);
    if (sgz_status st = pcmGrow(&sl.d_track, &sl.trackCap, s.maxFrames, bytes, false); st != SGZ_OK) return st;
    return s.trPinned ? SGZ_OK : pcmGrow(&sl.h_track, &sl.trackPinnedCap, s.maxFrames, bytes, true);
}

// the piece's records to the caller's buffer at the cursor, on the read-back stream (behind ev[4]); pageable: to the twin, the drain copies
static sgz_status pcmTrackReadBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t frames)
{
    if (!s.trArmed || !frames) return SGZ_OK;
    sgz_line_peak *at = s.trOut + size_t(s.trCursor) * s.cfg.num_pairs;
    sl.trackBytes = size_t(frames) * s.cfg.num_pairs * sizeof(sgz_line_peak);
    SGZ_HIP(hipMemcpyAsync(s.trPinned ? at : sl.h_track, sl.d_track, sl.trackBytes, hipMemcpyDeviceToHost, s.back));
    sl.trackDst = s.trPinned ? nullptr : at;
    s.trCursor += frames;
    return SGZ_OK;
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
        for (void *p : {sl.h_pcm, (void *)sl.h_rgba, (void *)sl.h_lines, (void *)sl.h_ovRgba, (void *)sl.h_ovPeaks, (void *)sl.h_wave, (void *)sl.h_track}) if (p) (void)hipHostFree(p);
        for (void *p : {sl.d_pcm, (void *)sl.d_rgba, (void *)sl.d_lines, (void *)sl.d_ovRgba, (void *)sl.d_ovPeaks, (void *)sl.d_wave, (void *)sl.d_track}) if (p) (void)hipFree(p);
        for (hipEvent_t e : sl.ev) if (e) (void)hipEventDestroy(e);
    }
    for (void *p : {(void *)s->d_planar[0], (void *)s->d_planar[1], (void *)s->d_state, (void *)s->d_ovCarry, (void *)s->d_wvCarry}) if (p) (void)hipFree(p);
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
        SGZ_PCM_TRY(hipMalloc(reinterpret_cast<void **>(&sl.d_rgba), s->maxFrames * cfg->axis_points * 4));
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
    return SGZ_OK;
}

sgz_status sgz_pcm_stream_feed(sgz_pcm_stream *s, const void *pcm, size_t nsamples, uint8_t *rgba_out, float *lines_out,
                               uint64_t capacity_frames, uint64_t *frames_out, sgz_pcm_timing *timing)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (!pcm && nsamples) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: null pcm");
    if (s->ovOpen) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: an overview column is open -- flush it (sgz_pcm_stream_feed_overview) or reset the stream first");
    const uint64_t need = sgz_pcm_stream_frames_for(s, nsamples);
    if (frames_out) *frames_out = need;
    if (capacity_frames < need) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: capacity_frames below what this feed yields (see *frames_out)");
    if (need && !rgba_out) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: null rgba_out");
    if (sgz_status st = pcmWaveFits(*s, nsamples); st != SGZ_OK) return st;
    if (sgz_status st = pcmTrackFits(*s, need); st != SGZ_OK) return st;
    if (timing) *timing = sgz_pcm_timing{};
    const uint32_t W = s->cfg.window_size, hop = s->cfg.hop, P = s->cfg.axis_points;
    const bool wantLines = lines_out || s->trArmed;             // the track lane searches the line results: rendered, never read back for it
    const bool pcmPinned = nsamples && isPinnedHost(pcm);
    const bool rgbaPinned = need && isPinnedHost(rgba_out), linesPinned = need && lines_out && isPinnedHost(lines_out);
    // (the pinned slots and the lines buffers are made on first need: a caller with pinned memory of its own never pays for them)
    for (PcmSlot &sl : s->slot) {
        if (nsamples && !pcmPinned && !sl.h_pcm) SGZ_HIP(hipHostMalloc(&sl.h_pcm, s->chunk * s->frameBytes, hipHostMallocDefault));
        if (need && !rgbaPinned && !sl.h_rgba) SGZ_HIP(hipHostMalloc(reinterpret_cast<void **>(&sl.h_rgba), s->maxFrames * P * 4, hipHostMallocDefault));
        if (need && wantLines && !sl.d_lines) SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&sl.d_lines), pcmLinesFloats(*s, s->maxFrames) * sizeof(float)));
        if (need && lines_out && !linesPinned && !sl.h_lines)
            SGZ_HIP(hipHostMalloc(reinterpret_cast<void **>(&sl.h_lines), pcmLinesFloats(*s, s->maxFrames) * sizeof(float), hipHostMallocDefault));
        if (sgz_status st = pcmWaveBuffers(*s, sl); st != SGZ_OK) return st;
        if (sgz_status st = pcmTrackBuffers(*s, sl); st != SGZ_OK) return st;
    }
    const uint8_t *src = static_cast<const uint8_t *>(pcm);
    uint64_t framesDone = 0, chunks = 0;
    for (size_t at = 0; at < nsamples; ) {
        const size_t n = std::min(s->chunk, nsamples - at);
        PcmSlot &sl = s->slot[s->pieces & 1];
        if (sgz_status st = pcmDrain(sl, timing); st != SGZ_OK) return st;          // the one wait inside a feed: the piece before last
        uint64_t frames = 0, keep = 0;
        if (sgz_status st = streamStep(W, hop, s->held, n, &frames, &keep); st != SGZ_OK) return st;
        const size_t bytes = n * s->frameBytes;
        const void *from = src + at * s->frameBytes;
        if (!pcmPinned) { std::memcpy(sl.h_pcm, from, bytes); from = sl.h_pcm; }
        // 1. upload
        sl.timed = timing != nullptr;
        if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[0], s->copy));
        SGZ_HIP(hipMemcpyAsync(sl.d_pcm, from, bytes, hipMemcpyHostToDevice, s->copy));
        SGZ_HIP(hipEventRecord(sl.ev[1], s->copy));
        // 2. convert behind the held tail, render what became complete, move the new tail to the front of the other planar buffer
        float *planar = s->d_planar[s->cur];
        SGZ_HIP(hipStreamWaitEvent(s->compute, sl.ev[1], 0));
        if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[2], s->compute));
        if (sgz_status st = launchPcmToPlanar(sl.d_pcm, s->format, s->srcChannels, n, s->map, s->numChannels, planar + s->held, s->stride, s->compute); st != SGZ_OK) return st;
        if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[3], s->compute));
        uint64_t waveColumns = 0;
        if (sgz_status st = pcmWavePiece(*s, sl, planar + s->held, n, &waveColumns); st != SGZ_OK) return st;
        const uint64_t total = s->held + n;
        sl.rendered = frames > 0 || waveColumns > 0;               // (a piece may close waveform columns and complete no frame)
        if (frames) {
            sgz_status st = sgz_spectrogram_render_device(s->plan, planar, s->stride, size_t(total), sl.d_rgba, wantLines ? sl.d_lines : nullptr, s->d_state, s->compute);
            if (st != SGZ_OK) return st;
            if (s->trArmed && (st = runTrackPeaksLines(s->plan->impl, sl.d_lines, size_t(frames), s->trGraph, s->trFraction, sl.d_track, s->compute)) != SGZ_OK) return st;
            if (keep) SGZ_HIP(hipMemcpy2DAsync(s->d_planar[s->cur ^ 1], s->stride * sizeof(float), planar + (total - keep), s->stride * sizeof(float),
                                               size_t(keep) * sizeof(float), s->numChannels, hipMemcpyDeviceToDevice, s->compute));
            s->cur ^= 1;
        }                                                                          // (no frame: the tail just grew where it is)
        s->held = keep;
        SGZ_HIP(hipEventRecord(sl.ev[4], s->compute));
        // 3. read back
        if (sl.rendered) {
            SGZ_HIP(hipStreamWaitEvent(s->back, sl.ev[4], 0));
            if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[5], s->back));
            if (frames) {
                sl.rgbaBytes = size_t(frames) * P * 4; sl.linesBytes = pcmLinesFloats(*s, frames) * sizeof(float);
                uint8_t *rgbaAt = rgba_out + size_t(framesDone) * P * 4;
                float *linesAt = lines_out ? lines_out + pcmLinesFloats(*s, framesDone) : nullptr;
                SGZ_HIP(hipMemcpyAsync(rgbaPinned ? rgbaAt : sl.h_rgba, sl.d_rgba, sl.rgbaBytes, hipMemcpyDeviceToHost, s->back));
                if (lines_out) SGZ_HIP(hipMemcpyAsync(linesPinned ? linesAt : sl.h_lines, sl.d_lines, sl.linesBytes, hipMemcpyDeviceToHost, s->back));
                sl.rgbaDst = rgbaPinned ? nullptr : rgbaAt; sl.rgbaFrom = sl.h_rgba;
                sl.linesDst = (lines_out && !linesPinned) ? linesAt : nullptr; sl.linesFrom = sl.h_lines;
            }
            if (sgz_status st = pcmTrackReadBack(*s, sl, frames); st != SGZ_OK) return st;
            if (sgz_status st = pcmWaveReadBack(*s, sl, waveColumns); st != SGZ_OK) return st;
            SGZ_HIP(hipEventRecord(sl.ev[6], s->back));
        }
        sl.busy = true;
        framesDone += frames; ++chunks; ++s->pieces; at += n;
    }
    // the end of the feed: both slots, the older piece first
    for (uint64_t k = 0; k < 2; ++k)
        if (sgz_status st = pcmDrain(s->slot[(s->pieces + k) & 1], timing); st != SGZ_OK) return st;
    if (frames_out) *frames_out = framesDone;
    if (timing) {
        timing->frames = framesDone; timing->chunks = chunks;
        timing->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return SGZ_OK;
}

sgz_status sgz_spectrogram_render_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                      const uint32_t *channel_map, size_t nsamples, uint8_t *rgba_out, float *lines_out, sgz_pcm_timing *timing)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!cfg || !pcm || !rgba_out) return fail(SGZ_EINVAL, "null argument");
    sgz_pcm_stream *s = nullptr;
    // (no more device and pinned memory than the buffer needs)
    const uint32_t frameBytes = std::max(1u, src_channels * sgz_pcm_sample_bytes(format));
    const size_t chunk = std::min(std::min(kPcmDefaultChunk, kPcmDefaultSlotBytes / frameBytes), std::max<size_t>(nsamples, 1));
    if (sgz_status st = sgz_pcm_stream_create(cfg, format, src_channels, channel_map, chunk, &s); st != SGZ_OK) return st;
    uint64_t frames = sgz_pcm_stream_frames_for(s, nsamples);
    sgz_status st = SGZ_SKIPPED_FRAME;
    if (frames == 0) { if (timing) *timing = sgz_pcm_timing{}; }
    else st = sgz_pcm_stream_feed(s, pcm, nsamples, rgba_out, lines_out, frames, &frames, timing);
    const std::string keep = g_lastError;
    sgz_pcm_stream_destroy(s);
    g_lastError = keep;
    if (timing && st == SGZ_OK) timing->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
}

// ---- the overview inside the stream (sgz.h, "the overview inside sgz_pcm_stream") ----------------------------------------------------------
// columns a feed of nsamples yields at k with the stream as it is; false: k == 0, or a k other than the open column's
static bool pcmOverviewNeed(const sgz_pcm_stream *s, size_t nsamples, uint32_t k, int flush, uint64_t *columns)
{
    if (!s || k == 0 || (s->ovOpen && k != s->ovK)) return false;
    const uint64_t t = s->ovOpen + sgz_pcm_stream_frames_for(s, nsamples);
    *columns = t / k + ((flush && t % k) ? 1u : 0u);
    return true;
}

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
    const auto t0 = std::chrono::steady_clock::now();
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
    if (sgz_status st = pcmTrackFits(*s, sgz_pcm_stream_frames_for(s, nsamples)); st != SGZ_OK) return st;
    if (timing) *timing = sgz_pcm_timing{};
    const uint32_t W = s->cfg.window_size, hop = s->cfg.hop, P = s->cfg.axis_points, C = s->cfg.num_pairs;
    const bool pcmPinned = nsamples && isPinnedHost(pcm);
    const bool rgbaPinned = need && rgba_out && isPinnedHost(rgba_out), peaksPinned = need && peaks_out && isPinnedHost(peaks_out);
    // the most columns one piece can close: floor((k - 1 + maxFrames) / k) = ceil(maxFrames / k), and one more from a flush
    const size_t slotColumns = (s->maxFrames + k - 1) / k + 1;
    if (!s->d_ovCarry) SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&s->d_ovCarry), size_t(C) * P * sizeof(float)));
    for (PcmSlot &sl : s->slot) {                                 // (both slots are idle between feeds)
        if (nsamples && !pcmPinned && !sl.h_pcm) SGZ_HIP(hipHostMalloc(&sl.h_pcm, s->chunk * s->frameBytes, hipHostMallocDefault));
        sgz_status st = pcmWaveBuffers(*s, sl);
        if (st != SGZ_OK) return st;
        if ((st = pcmTrackBuffers(*s, sl)) != SGZ_OK) return st;
        if (!need) continue;                                      // (no column closes: nothing is written or read back)
        if (rgba_out && (st = pcmGrow(&sl.d_ovRgba, &sl.ovRgbaCap, slotColumns, size_t(P) * 4, false)) != SGZ_OK) return st;
        if (rgba_out && !rgbaPinned && (st = pcmGrow(&sl.h_ovRgba, &sl.ovRgbaPinnedCap, slotColumns, size_t(P) * 4, true)) != SGZ_OK) return st;
        if (peaks_out && (st = pcmGrow(&sl.d_ovPeaks, &sl.ovPeaksCap, slotColumns, size_t(C) * P * sizeof(float), false)) != SGZ_OK) return st;
        if (peaks_out && !peaksPinned && (st = pcmGrow(&sl.h_ovPeaks, &sl.ovPeaksPinnedCap, slotColumns, size_t(C) * P * sizeof(float), true)) != SGZ_OK) return st;
    }
    const uint8_t *src = static_cast<const uint8_t *>(pcm);
    uint64_t columnsDone = 0, chunks = 0;
    // (a feed without samples still has one piece when it flushes an open column)
    for (size_t at = 0; at < nsamples || (chunks == 0 && flush && s->ovOpen); ) {
        const size_t n = std::min(s->chunk, nsamples - at);
        const bool last = at + n == nsamples;
        PcmSlot &sl = s->slot[s->pieces & 1];
        if (sgz_status st = pcmDrain(sl, timing); st != SGZ_OK) return st;          // the one wait inside a feed: the piece before last
        uint64_t frames = 0, keep = 0;
        if (sgz_status st = streamStep(W, hop, s->held, n, &frames, &keep); st != SGZ_OK) return st;
        sl.timed = timing != nullptr;
        // 1. upload
        if (n) {
            const size_t bytes = n * s->frameBytes;
            const void *from = src + at * s->frameBytes;
            if (!pcmPinned) { std::memcpy(sl.h_pcm, from, bytes); from = sl.h_pcm; }
            if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[0], s->copy));
            SGZ_HIP(hipMemcpyAsync(sl.d_pcm, from, bytes, hipMemcpyHostToDevice, s->copy));
            SGZ_HIP(hipEventRecord(sl.ev[1], s->copy));
            SGZ_HIP(hipStreamWaitEvent(s->compute, sl.ev[1], 0));
        } else if (sl.timed) {
            SGZ_HIP(hipEventRecord(sl.ev[0], s->copy));
            SGZ_HIP(hipEventRecord(sl.ev[1], s->copy));
        }
        // 2. convert behind the held tail, render what became complete slab by slab into the columns, move the new tail
        float *planar = s->d_planar[s->cur];
        if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[2], s->compute));
        if (n)
            if (sgz_status st = launchPcmToPlanar(sl.d_pcm, s->format, s->srcChannels, n, s->map, s->numChannels, planar + s->held, s->stride, s->compute); st != SGZ_OK) return st;
        if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[3], s->compute));
        uint64_t waveColumns = 0;
        if (sgz_status st = pcmWavePiece(*s, sl, planar + s->held, n, &waveColumns); st != SGZ_OK) return st;
        const uint64_t total = s->held + n;
        const int pieceFlush = flush && last;
        const uint64_t t = s->ovOpen + frames;
        const uint64_t columns = t / k + ((pieceFlush && t % k) ? 1u : 0u);
        uint8_t *d_rgba = rgba_out ? sl.d_ovRgba : nullptr;
        float *d_peaks = peaks_out ? sl.d_ovPeaks : nullptr;
        if (frames) {
            const SlabTrack track{s->trGraph, s->trFraction, sl.d_track};
            const sgz_status st = runOverviewSlabs(s->plan, planar, s->stride, size_t(total), long(frames), k, uint32_t(s->ovOpen), pieceFlush, s->d_ovCarry,
                                                   s->d_state, d_rgba, d_peaks, s->compute, s->trArmed ? &track : nullptr);
            if (st != SGZ_OK) return st;
            if (keep) SGZ_HIP(hipMemcpy2DAsync(s->d_planar[s->cur ^ 1], s->stride * sizeof(float), planar + (total - keep), s->stride * sizeof(float),
                                               size_t(keep) * sizeof(float), s->numChannels, hipMemcpyDeviceToDevice, s->compute));
            s->cur ^= 1;
        } else if (columns) {                                                      // no frame arrives and the open column is flushed
            const sgz_status st = runOverviewColumns(s->plan->impl, nullptr, 0, k, uint32_t(s->ovOpen), 1, 0, s->d_ovCarry, d_rgba, d_peaks, s->compute);
            if (st != SGZ_OK) return st;
        }
        s->held = keep;
        s->ovOpen = pieceFlush ? 0 : t % k;
        s->ovK = k;
        SGZ_HIP(hipEventRecord(sl.ev[4], s->compute));
        // 3. read back the columns that closed
        const uint64_t trackFrames = s->trArmed ? frames : 0;      // (a piece may complete frames and close no column)
        sl.rendered = columns > 0 || waveColumns > 0 || trackFrames > 0;
        if (sl.rendered) {
            SGZ_HIP(hipStreamWaitEvent(s->back, sl.ev[4], 0));
            if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[5], s->back));
            if (columns) {
                sl.rgbaBytes = size_t(columns) * P * 4; sl.linesBytes = size_t(columns) * C * P * sizeof(float);
                uint8_t *rgbaAt = rgba_out ? rgba_out + size_t(columnsDone) * P * 4 : nullptr;
                float *peaksAt = peaks_out ? peaks_out + size_t(columnsDone) * C * P : nullptr;
                if (rgba_out) SGZ_HIP(hipMemcpyAsync(rgbaPinned ? rgbaAt : sl.h_ovRgba, sl.d_ovRgba, sl.rgbaBytes, hipMemcpyDeviceToHost, s->back));
                if (peaks_out) SGZ_HIP(hipMemcpyAsync(peaksPinned ? peaksAt : sl.h_ovPeaks, sl.d_ovPeaks, sl.linesBytes, hipMemcpyDeviceToHost, s->back));
                sl.rgbaDst = (rgba_out && !rgbaPinned) ? rgbaAt : nullptr; sl.rgbaFrom = sl.h_ovRgba;
                sl.linesDst = (peaks_out && !peaksPinned) ? peaksAt : nullptr; sl.linesFrom = sl.h_ovPeaks;
            }
            if (sgz_status st = pcmTrackReadBack(*s, sl, trackFrames); st != SGZ_OK) return st;
            if (sgz_status st = pcmWaveReadBack(*s, sl, waveColumns); st != SGZ_OK) return st;
            SGZ_HIP(hipEventRecord(sl.ev[6], s->back));
        }
        sl.busy = true;
        columnsDone += columns; ++chunks; ++s->pieces; at += n;
    }
    for (uint64_t i = 0; i < 2; ++i)
        if (sgz_status st = pcmDrain(s->slot[(s->pieces + i) & 1], timing); st != SGZ_OK) return st;
    if (columns_out) *columns_out = columnsDone;
    if (timing) {
        timing->frames = columnsDone; timing->chunks = chunks;
        timing->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return SGZ_OK;
}

sgz_status sgz_spectrogram_overview_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                        const uint32_t *channel_map, size_t nsamples, uint32_t k, uint8_t *rgba_out, float *peaks_out, sgz_pcm_timing *timing)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!cfg || !pcm) return fail(SGZ_EINVAL, "null argument");
    if (k == 0) return fail(SGZ_EINVAL, "overview: k >= 1 frames per column");
    if (!rgba_out && !peaks_out) return fail(SGZ_EINVAL, "overview: an image, the peaks or both");
    sgz_pcm_stream *s = nullptr;
    const uint32_t frameBytes = std::max(1u, src_channels * sgz_pcm_sample_bytes(format));
    const size_t chunk = std::min(std::min(kPcmDefaultChunk, kPcmDefaultSlotBytes / frameBytes), std::max<size_t>(nsamples, 1));
    if (sgz_status st = sgz_pcm_stream_create(cfg, format, src_channels, channel_map, chunk, &s); st != SGZ_OK) return st;
    uint64_t columns = sgz_pcm_stream_columns_for(s, nsamples, k, 1);
    sgz_status st = SGZ_SKIPPED_FRAME;
    if (columns == 0) { if (timing) *timing = sgz_pcm_timing{}; }
    else st = sgz_pcm_stream_feed_overview(s, pcm, nsamples, k, 1, rgba_out, peaks_out, columns, &columns, timing);
    const std::string keep = g_lastError;
    sgz_pcm_stream_destroy(s);
    g_lastError = keep;
    if (timing && st == SGZ_OK) timing->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
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
                                         pcmWaveCarry(*s, s->wvCur ^ 1), sl.d_wave, nullptr, s->compute);
    if (st != SGZ_OK) return st;
    const size_t bytes = size_t(s->numChannels) * 2 * sizeof(float);
    float *at = s->wvOut + size_t(s->wvCursor) * s->numChannels * 2;
    SGZ_HIP(hipMemcpyAsync(s->wvPinned ? at : sl.h_wave, sl.d_wave, bytes, hipMemcpyDeviceToHost, s->compute));
    SGZ_HIP(hipStreamSynchronize(s->compute));
    if (!s->wvPinned) std::memcpy(at, sl.h_wave, bytes);
    s->wvOpen = 0;
    ++s->wvCursor;
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
