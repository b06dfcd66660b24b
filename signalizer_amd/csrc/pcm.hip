// pcm.hip -- interleaved PCM in (include/sgz.h "interleaved PCM in"): the convert-and-de-interleave kernel, and the stream handle that
// cuts a feed into pieces and runs upload / convert + render / read-back of neighbouring pieces side by side on three streams.  Both kinds
// of feed (frames, overview columns) go through ONE piece loop, pcmPieces, and differ in the Part they hand it: what to render from a piece
// and which rows to read back.  Every output of a piece -- image, lines, overview image, overview peaks, a lane's columns or records --
// is a PcmOut: device block, pinned twin, pending host copy.  Every lane is a PcmSink: the caller's buffer, the cursor in it, and the PcmOut its
// units pass through; the track lane (tracker.hip), which searches every piece's line results behind its render, is a sink of frames, and the
// eight column lanes -- waveform, level, true-peak, loudness, stereo-field, band, histogram, run (<lane>_columns.hip; their entry points: column_lanes.hpp),
// which reduce every piece's new samples behind the converter in that order -- are ONE PcmLane type, a sink of columns with the open column's
// carry, and differ in a hook that makes the one call of their reduction: one of two templates, for the two carry rules.  The feed walks the
// lanes; all ride the same read-back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>
#include <new>

#include "rt_common.hpp"       // isPinnedHost
#include "column_lanes.hpp"    // the column lanes' entry points

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
struct sgz_pcm_stream;
struct PcmLane;

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
// Field sgz_field_record [ceil(chunk / m) + 1][pairs] the stereo-field lane's.
// Band sgz_band_record [ceil(chunk / m) + 1][channels] the band lane's.
// Hist sgz_hist_record [ceil(chunk / m) + 1][channels] the histogram lane's.
// Run sgz_run_record [ceil(chunk / m) + 1][channels] the run lane's.
// OvStats sgz_overview_stat_record [columns][C][P] and OvMeans float [columns][C][P] the stats feed's, beside its OvImage.
// OvPower sgz_overview_power_record [columns][C][sides][P] and OvLevels float [columns][C][sides][P] the power feed's, beside its OvImage.
// OvCross sgz_overview_cross_record [columns][C][bands] the cross feed's.
// OvFlux sgz_overview_flux_record [columns][C][sides] the flux feed's.
// OvPct sgz_overview_pct_record [columns][C][P] and OvPctValues + j, float [columns][C][P], value plane j of the percentile feed's, beside its
// OvImage: a plane is a block of its own, because its columns go to a part of the caller's buffer of their own.
constexpr int kPcmPctPlanes = SGZ_OVERVIEW_PCT_MAX_QUANTILES;
enum PcmOutKind { kOutImage, kOutLines, kOutOvImage, kOutOvPeaks, kOutOvStats, kOutOvMeans, kOutOvPower, kOutOvLevels, kOutOvCross, kOutOvFlux, kOutOvPct,
                  kOutOvPctValues, kOutOvPctValuesEnd = kOutOvPctValues + kPcmPctPlanes, kOutWave = kOutOvPctValuesEnd, kOutTrack, kOutLevel, kOutTruePeak, kOutLoudness, kOutField, kOutBand, kOutHist, kOutRun, kPcmOuts };

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

// What every lane has: the caller's buffer and the cursor in it, in units -- columns, or frames for the track lane -- of `unit` bytes, and the
// PcmOut of a slot that a piece's units pass through.  most: the most units one piece yields, which is what a slot's block holds; 0: off
struct PcmSink {
    PcmOutKind kind = kPcmOuts;
    size_t unit = 0;
    uint64_t most = 0;
    uint8_t *out = nullptr;
    uint64_t cap = 0, cursor = 0;
    bool pinned = false;

    void arm(uint64_t mostUnits, void *to, uint64_t capacity)
    {
        most = mostUnits; out = static_cast<uint8_t *>(to); cap = capacity; cursor = 0;
        pinned = capacity && isPinnedHost(to);
    }
    void disarm() { most = 0; out = nullptr; cap = cursor = 0; }
    bool armed() const { return most != 0; }
    // what a feed checks before anything is consumed: the n units it yields fit behind the cursor
    bool fits(uint64_t n) const { return !armed() || n <= cap - cursor; }
    // the slot's block of `most` units (both slots are idle between feeds)
    sgz_status reserve(PcmSlot &sl) const { return most ? sl.out[kind].reserve(size_t(most) * unit, !pinned) : SGZ_OK; }
    // the first n units of the slot's block to the caller's buffer at the cursor, on `stream`
    sgz_status readBack(PcmSlot &sl, uint64_t n, hipStream_t stream)
    {
        if (!n) return SGZ_OK;
        const sgz_status st = sl.out[kind].readBack(out + size_t(cursor) * unit, size_t(n) * unit, pinned, stream);
        if (st == SGZ_OK) cursor += n;
        return st;
    }
};

// The sinks in the order a feed refuses them; the eight column lanes come first and are the stream's lane[] in this order
enum PcmSinkId { kSinkWave, kSinkLevel, kSinkTruePeak, kSinkLoudness, kSinkField, kSinkBand, kSinkHist, kSinkRun, kSinkTrack, kPcmSinks, kPcmLanes = kSinkTrack };
constexpr PcmSinkId kReserveOrder[kPcmSinks] = {kSinkWave, kSinkTrack, kSinkLevel, kSinkTruePeak, kSinkLoudness, kSinkField, kSinkBand, kSinkHist, kSinkRun};
constexpr PcmSinkId kReadBackOrder[kPcmSinks] = {kSinkTrack, kSinkWave, kSinkLevel, kSinkTruePeak, kSinkLoudness, kSinkField, kSinkBand, kSinkHist, kSinkRun};

// A lane's hook: the one call of its reduction, run<Lane>Columns, on the compute stream.  (n samples at `in`, flush 0) is a piece's step: the
// columns they close go to d_out, the open one to the other half of the carry; (0 samples, flush 1) is the flush's emit launch, which leaves the
// carry where it is.  The hook keeps what is the lane's own: the carry's layout, its scratch, and whether a step moves to the other half
using PcmLaneRun = sgz_status (*)(sgz_pcm_stream &s, PcmLane &l, const float *in, size_t n, int flush, void *d_out, uint64_t *closed);
}  // namespace

// A column lane (m > 0: armed): a sink of columns of m samples.  open: the open column's sample count; its state is in half `cur` of d_carry
// [2][...] -- a step reads that half and writes the other, so no launch reads what it writes.  The true-peak, loudness and band carries hold
// the filter's history too, so every piece with samples writes the other half and the halves alternate.  continued: half `cur` holds the
// samples before the next one (false after arming or a reset: the history is zeros); index: the lane's samples so far -- the absolute index
// of the next one, which a flush does not move (the loudness and band lanes' segment phase)
struct PcmLane {
    PcmSink sink;
    const char *word = "", *call = "";                  // for messages: "true-peak", and the calls' suffix, "truepeak"
    PcmLaneRun run = nullptr;
    uint32_t m = 0;
    uint64_t open = 0;
    int cur = 0;
    void *d_carry = nullptr;
    size_t carryCap = 0;                                // what is allocated, where the carry's size depends on a filter (loudness, band)
    bool continued = false;
    uint64_t index = 0;
    // the loudness and band lanes' scratch (q of a piece's samples, partial records), kept: every piece's launches are on the compute
    // stream, one behind the other
    void *d_scratch = nullptr;
    size_t scratchCap = 0;
};

// how a refusal names an open column's kind (plan.hpp OverviewKind), and the feed that flushes it
static const struct { const char *word, *call; } kPcmOvKindText[kOverviewKinds] = {
    {"peak-hold", "sgz_pcm_stream_feed_overview"},       {"mean", "sgz_pcm_stream_feed_overview_stats"}, {"power", "sgz_pcm_stream_feed_overview_power"},
    {"cross", "sgz_pcm_stream_feed_overview_cross"},     {"flux", "sgz_pcm_stream_feed_overview_flux"}, {"percentile", "sgz_pcm_stream_feed_overview_pct"},
};

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
    // the overview inside the stream: the open column's frame count, its k and its kind (meaningful while ovOpen > 0), and every kind's carry,
    // made on first use: the peak hold's V [pairs][P], the mean overview's records [pairs][P] (sgz.h, "The mean overview"), the power overview's
    // [pairs][sides][P] ("The power overview"), the cross overview's [pairs][bands], by the band table of the stream's plan and made with it ("The
    // cross overview"), the flux overview's [pairs][sides] ("The flux overview"), the percentile overview's records [pairs][P] ("The percentile
    // overview")
    uint64_t ovOpen = 0; uint32_t ovK = 0;
    OverviewKind ovKind = kOvPeaks;
    void *d_ovCarry[kOverviewKinds] = {};
    // The flux overview also keeps, across feeds, the last frame's mapped magnitudes [pairs][sides][P] in d_ovFluxPrev -- fluxLinked: they are the
    // frame in front of the next one, which no reset and no feed of another kind has consumed frames since -- and frameIndex, the frames the
    // stream has completed since it was made or reset, in any kind of feed
    float *d_ovFluxPrev = nullptr;
    bool fluxLinked = false;
    uint64_t frameIndex = 0;
    // the column lanes: waveform (carry float2 [2][channels]), level (sgz_level_record [2][pairs]), true-peak (sgz_truepeak_carry [2][channels]),
    // stereo-field (sgz_field_record [2][pairs]), histogram (sgz_hist_record [2][channels]), run (sgz_run_carry [2][channels]), loudness and
    // band (two halves of <lane>CarryBytes(filter) * channels bytes), and the two filters
    PcmLane lane[kPcmLanes];
    sgz_loudness_filter ldFilter{};
    sgz_band_filter bdFilter{};
    sgz_run_params rnParams{};                          // the run lane's thresholds
    // the track lane (track.most > 0: armed): a sink of frames, and the graph and mouse position searched
    PcmSink track;
    uint32_t trGraph = 0;
    double trFraction = 0;

    PcmSink &sink(int id) { return id < kPcmLanes ? lane[id].sink : track; }
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

// ---- the lanes inside the stream (sgz.h, "The waveform lane" ... "The loudness lane", "The track lane") -----------------------------------------
// The hooks are two templates over what a lane's two steps are called, for the two carry rules.
// The waveform, level, stereo-field and histogram carries hold the open column alone: a step moves to the other half only when a column stays open.
// Record: the element of the carry and of the output, PerCell of them per channel (or, OfPairs, per pair); Shape, Run: the lane's two steps
template <class Record, size_t PerCell, bool OfPairs, auto Shape, auto Run>
static sgz_status pcmOpenColumnRun(sgz_pcm_stream &s, PcmLane &l, const float *in, size_t n, int flush, void *d_out, uint64_t *closed)
{
    const uint32_t cells = OfPairs ? s.cfg.num_pairs : s.numChannels, open = uint32_t(l.open);
    const ColumnsShape sh = Shape(cells, n, l.m, open, flush, 0);
    StreamScratch scratch(s.compute);
    if (sh.scratchBytes) SGZ_HIP(scratch.get(sh.scratchBytes));
    Record *carry = static_cast<Record *>(l.d_carry);
    const size_t half = PerCell * cells;
    const sgz_status st = Run(sh, in, s.stride, cells, n, l.m, open, carry + l.cur * half, carry + (l.cur ^ 1) * half, static_cast<Record *>(d_out),
                              scratch.p, s.compute);
    if (st != SGZ_OK) return st;
    if (sh.open) l.cur ^= 1;
    *closed = sh.closed;
    return SGZ_OK;
}

// The true-peak, loudness and band carries hold the filter's history too: every step with samples moves to the other half, whether or not a
// column stays open.  A flush emits the open column of the current half as continued and leaves the carry, and with it the history, where it
// is.  Lane: shape, the lane's <lane>ColumnsShape; carryBytes(s), a channel's carry; keptScratch (else stream-ordered); run(...), the lane's
// run<Lane>Columns with what it takes from the stream (the filter, the sample index)
struct PcmTruePeak {
    static constexpr bool keptScratch = false;
    static constexpr auto shape = truePeakColumnsShape;
    static size_t carryBytes(const sgz_pcm_stream &) { return sizeof(sgz_truepeak_carry); }
    static sgz_status run(sgz_pcm_stream &s, PcmLane &l, const ColumnsShape &sh, const float *in, size_t n, uint32_t continued, const void *carryIn,
                          void *carryOut, void *d_out, void *scratch)
    {
        return runTruePeakColumns(sh, in, s.stride, s.numChannels, n, l.m, uint32_t(l.open), continued, static_cast<const sgz_truepeak_carry *>(carryIn),
                                  static_cast<sgz_truepeak_carry *>(carryOut), static_cast<sgz_truepeak_record *>(d_out), scratch, s.compute);
    }
};
struct PcmRun {
    static constexpr bool keptScratch = false;
    static constexpr auto shape = runColumnsShape;
    static size_t carryBytes(const sgz_pcm_stream &) { return sizeof(sgz_run_carry); }
    static sgz_status run(sgz_pcm_stream &s, PcmLane &l, const ColumnsShape &sh, const float *in, size_t n, uint32_t continued, const void *carryIn,
                          void *carryOut, void *d_out, void *scratch)
    {
        return runRunColumns(sh, s.rnParams, in, s.stride, s.numChannels, n, l.m, uint32_t(l.open), continued, static_cast<const sgz_run_carry *>(carryIn),
                             static_cast<sgz_run_carry *>(carryOut), static_cast<sgz_run_record *>(d_out), scratch, s.compute);
    }
};
struct PcmLoudness {
    static constexpr bool keptScratch = true;
    static constexpr auto shape = loudnessColumnsShape;
    static size_t carryBytes(const sgz_pcm_stream &s) { return loudnessCarryBytes(s.ldFilter); }
    static sgz_status run(sgz_pcm_stream &s, PcmLane &l, const ColumnsShape &sh, const float *in, size_t n, uint32_t continued, const void *carryIn,
                          void *carryOut, void *d_out, void *scratch)
    {
        return runLoudnessColumns(sh, s.ldFilter, in, s.stride, s.numChannels, n, l.index, l.m, uint32_t(l.open), continued, carryIn, carryOut,
                                  static_cast<sgz_loudness_record *>(d_out), scratch, s.compute);
    }
};
struct PcmBand {
    static constexpr bool keptScratch = true;
    static constexpr auto shape = bandColumnsShape;
    static size_t carryBytes(const sgz_pcm_stream &s) { return bandCarryBytes(s.bdFilter); }
    static sgz_status run(sgz_pcm_stream &s, PcmLane &l, const ColumnsShape &sh, const float *in, size_t n, uint32_t continued, const void *carryIn,
                          void *carryOut, void *d_out, void *scratch)
    {
        return runBandColumns(sh, s.bdFilter, in, s.stride, s.numChannels, n, l.index, l.m, uint32_t(l.open), continued, carryIn, carryOut,
                              static_cast<sgz_band_record *>(d_out), scratch, s.compute);
    }
};

template <class Lane>
static sgz_status pcmHistoryRun(sgz_pcm_stream &s, PcmLane &l, const float *in, size_t n, int flush, void *d_out, uint64_t *closed)
{
    const uint32_t channels = s.numChannels;
    const ColumnsShape sh = Lane::shape(channels, n, l.m, uint32_t(l.open), flush, 0);
    StreamScratch ordered(s.compute);
    void *scratch = nullptr;
    if constexpr (Lane::keptScratch) {
        if (sh.scratchBytes > l.scratchCap) {                                       // (the first piece of a feed is its largest: this happens once)
            SGZ_HIP(hipStreamSynchronize(s.compute));
            if (l.d_scratch) { (void)hipFree(l.d_scratch); l.d_scratch = nullptr; l.scratchCap = 0; }
            SGZ_HIP(hipMalloc(&l.d_scratch, sh.scratchBytes));
            l.scratchCap = sh.scratchBytes;
        }
        scratch = flush ? nullptr : l.d_scratch;
    } else {
        if (sh.scratchBytes) SGZ_HIP(ordered.get(sh.scratchBytes));
        scratch = ordered.p;
    }
    uint8_t *carry = static_cast<uint8_t *>(l.d_carry);
    const size_t half = Lane::carryBytes(s) * channels;
    const sgz_status st = Lane::run(s, l, sh, in, n, (flush || l.continued) ? 1u : 0u, carry + l.cur * half, carry + (l.cur ^ 1) * half, d_out, scratch);
    if (st != SGZ_OK) return st;
    if (!flush) { l.cur ^= 1; l.continued = true; l.index += n; }
    *closed = sh.closed;
    return SGZ_OK;
}

// what both feeds refuse for the lanes before anything is consumed, in the sinks' order: the columns the samples close and the frames they
// complete fit behind every armed lane's cursor
static sgz_status pcmLanesFit(const sgz_pcm_stream &s, size_t nsamples, uint64_t frames)
{
    for (const PcmLane &l : s.lane)
        if (l.m && !l.sink.fits((l.open + nsamples) / l.m))
            return fail(SGZ_EINVAL, std::string("sgz_pcm_stream: the feed closes more ") + l.word + " columns than the buffer has left (sgz_pcm_stream_" + l.call +
                                        "_for; re-arm with sgz_pcm_stream_set_" + l.call + ")");
    if (!s.track.fits(frames))
        return fail(SGZ_EINVAL, "sgz_pcm_stream: the feed completes more frames than the track buffer has left (sgz_pcm_stream_track_for; re-arm with sgz_pcm_stream_set_track)");
    return SGZ_OK;
}

// a lane's part of a piece, on the compute stream: the n samples the converter just wrote at `fresh` -> the columns they close, into the slot
static sgz_status pcmLanePiece(sgz_pcm_stream &s, PcmLane &l, PcmSlot &sl, const float *fresh, size_t n, uint64_t *columns)
{
    *columns = 0;
    if (!l.m || n == 0) return SGZ_OK;
    if (sgz_status st = l.run(s, l, fresh, n, 0, sl.out[l.sink.kind].dev, columns); st != SGZ_OK) return st;
    l.open = (l.open + n) % l.m;
    return SGZ_OK;
}

// the tail of sgz_pcm_stream_set_<lane> (pcmLaneSet) behind its checks: m, the caller's columns, the cursor at 0; a slot holds the
// ceil(chunk / m) + 1 columns a piece can close
static void pcmLaneArm(sgz_pcm_stream &s, PcmLane &l, uint32_t m, void *out, uint64_t capacity)
{
    l.m = m;
    l.sink.arm((s.chunk + m - 1) / m + 1, out, capacity);
}
static void pcmLaneDisarm(PcmLane &l) { l.m = 0; l.open = 0; l.continued = false; l.index = 0; l.sink.disarm(); }     // off: the open column, the history and the index are dropped

static uint64_t pcmLaneFor(const sgz_pcm_stream *s, int id, size_t nsamples, int flush)
{
    if (!s || !s->lane[id].m) return 0;
    const PcmLane &l = s->lane[id];
    const uint64_t t = l.open + nsamples;
    return t / l.m + ((flush && t % l.m) ? 1u : 0u);
}

static sgz_status pcmLaneState(const sgz_pcm_stream *s, int id, uint64_t *columns_written, uint64_t *open_samples)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (columns_written) *columns_written = s->lane[id].sink.cursor;
    if (open_samples) *open_samples = s->lane[id].open;
    return SGZ_OK;
}

// sgz_pcm_stream_flush_<lane>: the emit launch alone, the one column behind it on the compute stream itself, and waited for
static sgz_status pcmLaneFlush(sgz_pcm_stream *s, int id)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    PcmLane &l = s->lane[id];
    // (the message is put together only where it is needed: a flush with nothing open is a microsecond)
    const auto refuse = [&l](const char *why) { return fail(SGZ_EINVAL, std::string("sgz_pcm_stream_flush_") + l.call + why + "sgz_pcm_stream_set_" + l.call + ")"); };
    if (!l.m) return refuse(": the lane is off (");
    if (!l.open) return SGZ_OK;
    if (l.sink.cursor >= l.sink.cap) return refuse(": no column left in the buffer (re-arm with ");
    PcmSlot &sl = s->slot[0];                                      // (both slots are idle between feeds)
    if (sgz_status st = l.sink.reserve(sl); st != SGZ_OK) return st;
    PcmOut &out = sl.out[l.sink.kind];
    uint64_t closed = 0;
    if (sgz_status st = l.run(*s, l, s->d_planar[s->cur], 0, 1, out.dev, &closed); st != SGZ_OK) return st;
    if (sgz_status rb = l.sink.readBack(sl, 1, s->compute); rb != SGZ_OK) return rb;
    if (const hipError_t e = hipStreamSynchronize(s->compute); e != hipSuccess) {
        out.dst = nullptr; --l.sink.cursor;                        // (nothing arrived: the column is not counted)
        return hipFail(e, "hipStreamSynchronize(s->compute)");
    }
    out.drain();
    l.open = 0;
    return SGZ_OK;
}

// ---- the piece loop ------------------------------------------------------------------------------------------------------------------------
// What both feeds do once they have refused what they refuse.  The feed is cut into pieces of at most `chunk` samples; piece i uses slot i & 1:
//   1. upload            copy stream: the samples to the slot (through its pinned block when the caller's are pageable)
//   2. convert + render  compute stream, behind ev[1]: the converter behind the held tail, the column lanes on the new samples, the Part's
//                        render of what became complete (armed, the track lane's search with it), the new tail to the other planar buffer
//   3. read back         read-back stream, behind ev[4]: the Part's rows, then every sink's units in kReadBackOrder
// The two kinds of feed differ in their Part alone: reserve(s, sl) makes its outputs in a slot before anything is consumed; render(s, sl,
// planar, total, frames, last, &units) enqueues the render of a piece's frames and says how many rows -- `units`, what the feed counts and its
// timing reports -- it leaves in the slot; readBack(s, sl, done, units) enqueues their copies behind the feed's `done` earlier rows;
// fluxPiece(): its pieces leave the stream's last frame where the next flux feed finds it.
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
        for (PcmSinkId id : kReserveOrder)
            if (sgz_status st = s.sink(id).reserve(sl); st != SGZ_OK) return st;
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
            uint64_t yields[kPcmSinks] = {}, units = 0;                             // what the piece leaves for every sink, and for the Part
            for (int id = 0; id < kPcmLanes; ++id)
                if (sgz_status st = pcmLanePiece(s, s.lane[id], sl, planar + s.held, n, &yields[id]); st != SGZ_OK) return st;
            const uint64_t total = s.held + n;
            if (sgz_status st = part.render(s, sl, planar, size_t(total), frames, at + n == nsamples, &units); st != SGZ_OK) return st;
            s.frameIndex += frames;
            if (frames) s.fluxLinked = part.fluxPiece();                            // (the flux overview's previous frame is the stream's last only behind a flux piece)
            if (frames) {
                if (keep) SGZ_HIP(hipMemcpy2DAsync(s.d_planar[s.cur ^ 1], s.stride * sizeof(float), planar + (total - keep), s.stride * sizeof(float),
                                                   size_t(keep) * sizeof(float), s.numChannels, hipMemcpyDeviceToDevice, s.compute));
                s.cur ^= 1;
            }                                                                      // (no frame: the tail just grew where it is)
            s.held = keep;
            SGZ_HIP(hipEventRecord(sl.ev[4], s.compute));
            // 3. read back (a piece may close a lane's columns and complete no frame, or complete frames whose records are all it returns)
            yields[kSinkTrack] = s.track.armed() ? frames : 0;
            sl.rendered = units > 0 || std::any_of(yields, yields + kPcmSinks, [](uint64_t y) { return y > 0; });
            if (sl.rendered) {
                SGZ_HIP(hipStreamWaitEvent(s.back, sl.ev[4], 0));
                if (sl.timed) SGZ_HIP(hipEventRecord(sl.ev[5], s.back));
                if (units)
                    if (sgz_status st = part.readBack(s, sl, done, units); st != SGZ_OK) return st;
                for (PcmSinkId id : kReadBackOrder)
                    if (sgz_status st = s.sink(id).readBack(sl, yields[id], s.back); st != SGZ_OK) return st;
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

    static bool fluxPiece() { return false; }
    sgz_status reserve(sgz_pcm_stream &s, PcmSlot &sl) const
    {
        if (!need) return SGZ_OK;
        const sgz_status st = sl.out[kOutImage].reserve(pcmImageBytes(s, s.maxFrames), !rgbaPinned);
        if (st != SGZ_OK || (!lines && !s.track.armed())) return st;    // (the track lane searches the line results: rendered, never read back for it)
        return sl.out[kOutLines].reserve(pcmLinesFloats(s, s.maxFrames) * sizeof(float), lines && !linesPinned);
    }
    sgz_status render(sgz_pcm_stream &s, PcmSlot &sl, const float *planar, size_t total, uint64_t frames, bool, uint64_t *units) const
    {
        *units = frames;
        if (!frames) return SGZ_OK;
        float *d_lines = (lines || s.track.armed()) ? sl.out[kOutLines].as<float>() : nullptr;
        const sgz_status st = sgz_spectrogram_render_device(s.plan, planar, s.stride, total, sl.out[kOutImage].as<uint8_t>(), d_lines, s.d_state, s.compute);
        if (st != SGZ_OK || !s.track.armed()) return st;
        return runTrackPeaksLines(s.plan->impl, d_lines, size_t(frames), s.trGraph, s.trFraction, sl.out[kOutTrack].as<sgz_line_peak>(), s.compute);
    }
    sgz_status readBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t done, uint64_t frames) const
    {
        const sgz_status st = sl.out[kOutImage].readBack(rgba + pcmImageBytes(s, done), pcmImageBytes(s, frames), rgbaPinned, s.back);
        if (st != SGZ_OK || !lines) return st;
        return sl.out[kOutLines].readBack(lines + pcmLinesFloats(s, done), pcmLinesFloats(s, frames) * sizeof(float), linesPinned, s.back);
    }
};

// The overview feeds' part, of any kind: frames slab by slab into the columns they close, the open column in the stream's carry of the kind.
// out[]: the outputs the call has, in the order the kind's hook takes them -- the slot's block, the bytes of one column, the caller's buffer
// (null: not asked for).  firstUse[]: the device blocks the kind makes on its first feed (the cross carry is made with the band table).
// run(part, s, sl, k, d_out, planar, total, frames, flush): frames > 0, the kind's slabs, on the compute stream; frames == 0, the Columns call that
// flushes the open column alone.  d_out[i]: out[i]'s block in the slot, null where the caller asked for none or no column closes in this feed.
// The power, cross and flux hooks have no K_B: the stream's decay state is neither read nor advanced, and there are no line results for a track
// lane to search (their feeds refuse one)
struct PcmOverviewPart {
    static constexpr int kMostOuts = 2 + kPcmPctPlanes;          // the percentile feed's: the image, the records, the value planes
    using Run = sgz_status (*)(const PcmOverviewPart &part, sgz_pcm_stream &s, PcmSlot &sl, uint32_t k, void *const d_out[kMostOuts], const float *planar, size_t total, uint64_t frames, int flush);
    OverviewKind kind;
    uint32_t k; int flush;
    Run run;
    uint64_t need = 0;                                            // the columns the whole feed yields
    struct Out { PcmOutKind slot; size_t unit; void *host; bool pinned; } out[kMostOuts] = {};
    int outs = 0;
    struct { void **block; size_t bytes; } firstUse[2] = {};
    const double *q = nullptr; uint32_t nq = 0;                   // the percentile feed's quantiles

    void add(PcmOutKind slot, size_t unit, void *host) { out[outs++] = {slot, unit, host, false}; }
    bool fluxPiece() const { return kind == kOvFlux; }
    sgz_status reserve(sgz_pcm_stream &s, PcmSlot &sl) const
    {
        for (const auto &f : firstUse)
            if (f.block && !*f.block) SGZ_HIP(hipMalloc(f.block, f.bytes));
        if (!need) return SGZ_OK;                                 // (no column closes: nothing is written or read back)
        // the most columns one piece can close: floor((k - 1 + maxFrames) / k) = ceil(maxFrames / k), and one more from a flush
        const size_t columns = (s.maxFrames + k - 1) / k + 1;
        for (int i = 0; i < outs; ++i)
            if (out[i].host)
                if (sgz_status st = sl.out[out[i].slot].reserve(columns * out[i].unit, !out[i].pinned); st != SGZ_OK) return st;
        return SGZ_OK;
    }
    sgz_status render(sgz_pcm_stream &s, PcmSlot &sl, const float *planar, size_t total, uint64_t frames, bool last, uint64_t *units) const
    {
        const int pieceFlush = flush && last;
        const uint64_t t = s.ovOpen + frames;
        *units = t / k + ((pieceFlush && t % k) ? 1u : 0u);
        void *d_out[kMostOuts] = {};
        for (int i = 0; i < outs; ++i) d_out[i] = (out[i].host && need) ? sl.out[out[i].slot].dev : nullptr;
        if (frames || *units)                                      // (no frame arrives: the open column is flushed, or nothing happens)
            if (sgz_status st = run(*this, s, sl, k, d_out, planar, total, frames, pieceFlush); st != SGZ_OK) return st;
        s.ovOpen = pieceFlush ? 0 : t % k;
        s.ovK = k;
        s.ovKind = kind;
        return SGZ_OK;
    }
    sgz_status readBack(sgz_pcm_stream &s, PcmSlot &sl, uint64_t done, uint64_t columns) const
    {
        for (int i = 0; i < outs; ++i)
            if (out[i].host)
                if (sgz_status st = sl.out[out[i].slot].readBack(static_cast<uint8_t *>(out[i].host) + done * out[i].unit, columns * out[i].unit, out[i].pinned, s.back); st != SGZ_OK) return st;
        return SGZ_OK;
    }
};

// the kinds' hooks.  The peak hold's and the mean overview's slabs render line results, which the track lane, armed, searches
static sgz_status pcmPeaksRun(const PcmOverviewPart &, sgz_pcm_stream &s, PcmSlot &sl, uint32_t k, void *const d[], const float *planar, size_t total, uint64_t frames, int flush)
{
    float *carry = static_cast<float *>(s.d_ovCarry[kOvPeaks]);
    uint8_t *d_rgba = static_cast<uint8_t *>(d[0]);
    float *d_peaks = static_cast<float *>(d[1]);
    if (!frames) return runOverviewColumns(s.plan->impl, nullptr, 0, k, uint32_t(s.ovOpen), 1, 0, carry, d_rgba, d_peaks, s.compute);
    const SlabTrack track{s.trGraph, s.trFraction, sl.out[kOutTrack].as<sgz_line_peak>()};
    return runOverviewSlabs(s.plan, planar, s.stride, total, long(frames), k, uint32_t(s.ovOpen), flush, carry, s.d_state, d_rgba, d_peaks, s.compute,
                            s.track.armed() ? &track : nullptr);
}
static sgz_status pcmStatsRun(const PcmOverviewPart &, sgz_pcm_stream &s, PcmSlot &sl, uint32_t k, void *const d[], const float *planar, size_t total, uint64_t frames, int flush)
{
    using Record = sgz_overview_stat_record;
    Record *carry = static_cast<Record *>(s.d_ovCarry[kOvStats]), *d_stats = static_cast<Record *>(d[1]);
    uint8_t *d_rgba = static_cast<uint8_t *>(d[0]);
    float *d_means = static_cast<float *>(d[2]);
    if (!frames) return runOverviewStatsColumns(s.plan->impl, nullptr, 0, k, uint32_t(s.ovOpen), 1, 0, carry, d_rgba, d_stats, d_means, s.compute);
    const SlabTrack track{s.trGraph, s.trFraction, sl.out[kOutTrack].as<sgz_line_peak>()};
    return runOverviewStatsSlabs(s.plan, planar, s.stride, total, long(frames), k, uint32_t(s.ovOpen), flush, carry, s.d_state, d_rgba, d_stats, d_means,
                                 s.compute, s.track.armed() ? &track : nullptr);
}
static sgz_status pcmPowerRun(const PcmOverviewPart &, sgz_pcm_stream &s, PcmSlot &, uint32_t k, void *const d[], const float *planar, size_t, uint64_t frames, int flush)
{
    using Record = sgz_overview_power_record;
    Record *carry = static_cast<Record *>(s.d_ovCarry[kOvPower]), *d_power = static_cast<Record *>(d[1]);
    uint8_t *d_rgba = static_cast<uint8_t *>(d[0]);
    float *d_levels = static_cast<float *>(d[2]);
    if (!frames) return runOverviewPowerColumns(s.plan->impl, nullptr, 0, k, uint32_t(s.ovOpen), 1, 0, carry, d_rgba, d_power, d_levels, s.compute);
    return runOverviewPowerSlabs(s.plan, planar, s.stride, long(frames), k, uint32_t(s.ovOpen), flush, carry, d_rgba, d_power, d_levels, s.compute);
}
static sgz_status pcmCrossRun(const PcmOverviewPart &, sgz_pcm_stream &s, PcmSlot &, uint32_t k, void *const d[], const float *planar, size_t, uint64_t frames, int flush)
{
    using Record = sgz_overview_cross_record;
    Record *carry = static_cast<Record *>(s.d_ovCarry[kOvCross]), *d_cross = static_cast<Record *>(d[0]);
    if (!frames) return runOverviewCrossColumns(s.plan->impl, nullptr, 0, k, uint32_t(s.ovOpen), 1, 0, carry, d_cross, s.compute);
    return runOverviewCrossSlabs(s.plan, planar, s.stride, long(frames), k, uint32_t(s.ovOpen), flush, carry, d_cross, s.compute);
}
// (d[2 + j]: value plane j's block; the quantiles are the feed's)
static sgz_status pcmPctRun(const PcmOverviewPart &part, sgz_pcm_stream &s, PcmSlot &sl, uint32_t k, void *const d[], const float *planar, size_t total, uint64_t frames, int flush)
{
    using Record = sgz_overview_pct_record;
    Record *carry = static_cast<Record *>(s.d_ovCarry[kOvPct]), *d_records = static_cast<Record *>(d[1]);
    uint8_t *d_rgba = static_cast<uint8_t *>(d[0]);
    PctPlanes planes{};
    for (uint32_t j = 0; j < part.nq; ++j) planes.p[j] = static_cast<float *>(d[2 + j]);
    if (!frames) return runOverviewPctColumns(s.plan->impl, nullptr, 0, k, uint32_t(s.ovOpen), 1, 0, part.q, part.nq, carry, d_rgba, d_records, planes, s.compute);
    const SlabTrack track{s.trGraph, s.trFraction, sl.out[kOutTrack].as<sgz_line_peak>()};
    return runOverviewPctSlabs(s.plan, planar, s.stride, total, long(frames), k, uint32_t(s.ovOpen), flush, part.q, part.nq, carry, s.d_state, d_rgba, d_records,
                               planes, s.compute, s.track.armed() ? &track : nullptr);
}
// (the previous frame and the frame index are the stream's: pcmFeed moves both on behind every piece)
static sgz_status pcmFluxRun(const PcmOverviewPart &, sgz_pcm_stream &s, PcmSlot &, uint32_t k, void *const d[], const float *planar, size_t, uint64_t frames, int flush)
{
    using Record = sgz_overview_flux_record;
    Record *carry = static_cast<Record *>(s.d_ovCarry[kOvFlux]), *d_flux = static_cast<Record *>(d[0]);
    if (!frames) return runOverviewFluxColumns(s.plan->impl, nullptr, 0, k, uint32_t(s.ovOpen), 1, s.frameIndex, 0, nullptr, false, carry, d_flux, s.compute);
    return runOverviewFluxSlabs(s.plan, planar, s.stride, long(frames), k, uint32_t(s.ovOpen), flush, s.frameIndex, s.d_ovFluxPrev, s.fluxLinked, carry, d_flux,
                                s.compute);
}

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

// The refusal of a feed while a column of another kind is open, written once: `feed` the refusing call's name; own: the kind the call could
// continue (kOverviewKinds: none -- sgz_pcm_stream_feed, whose text names the column first).  SGZ_OK: nothing stands in the way
static sgz_status pcmOpenColumnRefusal(const sgz_pcm_stream &s, const char *feed, int own)
{
    if (!s.ovOpen || s.ovKind == own) return SGZ_OK;
    const auto &kind = kPcmOvKindText[s.ovKind];
    const std::string tail = std::string(" -- flush it (") + kind.call + ") or reset the stream first";
    if (own == kOverviewKinds)
        return fail(SGZ_EINVAL, std::string(feed) + (s.ovKind == kOvPeaks ? ": an overview column" : std::string(": a ") + kind.word + " overview's column") + " is open" + tail);
    return fail(SGZ_EINVAL, std::string(feed) + ": the open column is a " + kind.word + " overview's" + tail);
}

// columns a feed of nsamples yields at k with the stream as it is; false: k == 0, or a k other than the open column's
static bool pcmOverviewNeed(const sgz_pcm_stream *s, size_t nsamples, uint32_t k, int flush, uint64_t *columns)
{
    if (!s || k == 0 || (s->ovOpen && k != s->ovK)) return false;
    const uint64_t t = s->ovOpen + sgz_pcm_stream_frames_for(s, nsamples);
    *columns = t / k + ((flush && t % k) ? 1u : 0u);
    return true;
}

// What the six overview feeds share, in the order every one of them refuses: the stream, the samples, k, then own() -- the call's checks of
// its outputs and of the plan, which also fills part.out[] and part.firstUse[] --, a column of another kind, another k, the capacity, a missing
// output the feed would write (text.nullOut; null: the call has refused a call without outputs before), the lanes.  The texts that name the call
// are the call's own
struct PcmOvTexts { const char *nullPcm, *kDiffers, *capacity, *nullOut; };
template <typename Own>
static sgz_status pcmOverviewFeed(sgz_pcm_stream *s, const void *pcm, size_t nsamples, const PcmOvTexts &text, PcmOverviewPart &part, uint64_t capacity_columns,
                                  uint64_t *columns_out, sgz_pcm_timing *timing, Own own)
{
    const auto t0 = PcmClock::now();
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (!pcm && nsamples) return fail(SGZ_EINVAL, text.nullPcm);
    if (part.k == 0) return fail(SGZ_EINVAL, "overview: k >= 1 frames per column");
    if (sgz_status st = own(); st != SGZ_OK) return st;
    if (sgz_status st = pcmOpenColumnRefusal(*s, kPcmOvKindText[part.kind].call, part.kind); st != SGZ_OK) return st;
    if (s->ovOpen && part.k != s->ovK) return fail(SGZ_EINVAL, text.kDiffers);
    (void)pcmOverviewNeed(s, nsamples, part.k, part.flush, &part.need);
    if (columns_out) *columns_out = part.need;
    if (capacity_columns < part.need) return fail(SGZ_EINVAL, text.capacity);
    if (text.nullOut && part.need && !part.out[0].host) return fail(SGZ_EINVAL, text.nullOut);
    if (sgz_status st = pcmLanesFit(*s, nsamples, sgz_pcm_stream_frames_for(s, nsamples)); st != SGZ_OK) return st;
    for (int i = 0; i < part.outs; ++i) part.out[i].pinned = part.need && part.out[i].host && isPinnedHost(part.out[i].host);
    // (a feed without samples still has one piece when it flushes an open column)
    return pcmFeed(*s, pcm, nsamples, part.flush && s->ovOpen, part, columns_out, timing, t0);
}

// ... and the six one-shots: the null arguments, k, own() -- the call's other refusals --, and the stream of pcmOneShot around feed(s, columns)
template <typename Own, typename Feed>
static sgz_status pcmOverviewOneShot(bool nullArgument, const sgz_spectrum_config *cfg, uint32_t format, uint32_t src_channels, const uint32_t *channel_map,
                                     size_t nsamples, uint32_t k, sgz_pcm_timing *timing, Own own, Feed feed)
{
    if (nullArgument) return fail(SGZ_EINVAL, "null argument");
    if (k == 0) return fail(SGZ_EINVAL, "overview: k >= 1 frames per column");
    if (sgz_status st = own(); st != SGZ_OK) return st;
    return pcmOneShot(cfg, format, src_channels, channel_map, nsamples, timing, [&](sgz_pcm_stream *s) { return sgz_pcm_stream_columns_for(s, nsamples, k, 1); }, feed);
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
    for (void *p : {(void *)s->d_planar[0], (void *)s->d_planar[1], (void *)s->d_state, (void *)s->d_ovFluxPrev}) if (p) (void)hipFree(p);
    for (void *p : s->d_ovCarry) if (p) (void)hipFree(p);
    for (PcmLane &l : s->lane)
        for (void *p : {l.d_carry, l.d_scratch}) if (p) (void)hipFree(p);
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
    // the lanes: the word for messages, the calls' suffix, the slot's output, the bytes of one column (a record per channel or pair), the hook
    const struct { const char *word, *call; PcmOutKind kind; size_t unit; PcmLaneRun run; } lanes[kPcmLanes] = {
        {"waveform", "waveform", kOutWave, s->numChannels * 2 * sizeof(float), pcmOpenColumnRun<float, 2, false, waveColumnsShape, runWaveColumns>},
        {"level", "level", kOutLevel, cfg->num_pairs * sizeof(sgz_level_record), pcmOpenColumnRun<sgz_level_record, 1, true, levelColumnsShape, runLevelColumns>},
        {"true-peak", "truepeak", kOutTruePeak, s->numChannels * sizeof(sgz_truepeak_record), pcmHistoryRun<PcmTruePeak>},
        {"loudness", "loudness", kOutLoudness, s->numChannels * sizeof(sgz_loudness_record), pcmHistoryRun<PcmLoudness>},
        {"stereo-field", "field", kOutField, cfg->num_pairs * sizeof(sgz_field_record), pcmOpenColumnRun<sgz_field_record, 1, true, fieldColumnsShape, runFieldColumns>},
        {"band", "band", kOutBand, s->numChannels * sizeof(sgz_band_record), pcmHistoryRun<PcmBand>},
        {"histogram", "hist", kOutHist, s->numChannels * sizeof(sgz_hist_record), pcmOpenColumnRun<sgz_hist_record, 1, false, histColumnsShape, runHistColumns>},
        {"run", "run", kOutRun, s->numChannels * sizeof(sgz_run_record), pcmHistoryRun<PcmRun>},
    };
    for (int id = 0; id < kPcmLanes; ++id) {
        PcmLane &l = s->lane[id];
        l.word = lanes[id].word; l.call = lanes[id].call; l.run = lanes[id].run;
        l.sink.kind = lanes[id].kind; l.sink.unit = lanes[id].unit;
    }
    s->track.kind = kOutTrack; s->track.unit = cfg->num_pairs * sizeof(sgz_line_peak);
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
    s->ovOpen = 0; s->ovKind = kOvPeaks;                                            // an open overview column, of any kind, is dropped
    s->fluxLinked = false; s->frameIndex = 0;                                       // ... and the flux overview's predecessor; the frames count from 0
    for (int id = 0; id < kPcmSinks; ++id) s->sink(id).cursor = 0;                  // every lane's columns and the track's records start over; all stay armed
    for (PcmLane &l : s->lane) { l.open = 0; l.continued = false; l.index = 0; }    // open columns are dropped, the histories are zeros again and the samples count from 0
    return SGZ_OK;
}

sgz_status sgz_pcm_stream_feed(sgz_pcm_stream *s, const void *pcm, size_t nsamples, uint8_t *rgba_out, float *lines_out,
                               uint64_t capacity_frames, uint64_t *frames_out, sgz_pcm_timing *timing)
{
    const auto t0 = PcmClock::now();
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (!pcm && nsamples) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: null pcm");
    if (sgz_status st = pcmOpenColumnRefusal(*s, "sgz_pcm_stream_feed", kOverviewKinds); st != SGZ_OK) return st;
    const uint64_t need = sgz_pcm_stream_frames_for(s, nsamples);
    if (frames_out) *frames_out = need;
    if (capacity_frames < need) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: capacity_frames below what this feed yields (see *frames_out)");
    if (need && !rgba_out) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed: null rgba_out");
    if (sgz_status st = pcmLanesFit(*s, nsamples, need); st != SGZ_OK) return st;
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
    static const PcmOvTexts text = {"sgz_pcm_stream_feed_overview: null pcm", "sgz_pcm_stream_feed_overview: k differs from the open column's -- flush or reset first",
                                    "sgz_pcm_stream_feed_overview: capacity_columns below what this feed yields (see *columns_out)", nullptr};
    PcmOverviewPart part{kOvPeaks, k, flush, pcmPeaksRun};
    return pcmOverviewFeed(s, pcm, nsamples, text, part, capacity_columns, columns_out, timing, [&]() -> sgz_status {
        if (!rgba_out && !peaks_out) return fail(SGZ_EINVAL, "overview: an image, the peaks or both");
        part.add(kOutOvImage, pcmImageBytes(*s, 1), rgba_out);
        part.add(kOutOvPeaks, pcmPeaksFloats(*s, 1) * sizeof(float), peaks_out);
        part.firstUse[0] = {&s->d_ovCarry[kOvPeaks], pcmPeaksFloats(*s, 1) * sizeof(float)};
        return SGZ_OK;
    });
}

sgz_status sgz_spectrogram_overview_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                        const uint32_t *channel_map, size_t nsamples, uint32_t k, uint8_t *rgba_out, float *peaks_out, sgz_pcm_timing *timing)
{
    return pcmOverviewOneShot(!cfg || !pcm, cfg, format, src_channels, channel_map, nsamples, k, timing,
                              [&] { return (!rgba_out && !peaks_out) ? fail(SGZ_EINVAL, "overview: an image, the peaks or both") : SGZ_OK; },
                              [&](sgz_pcm_stream *s, uint64_t columns) { return sgz_pcm_stream_feed_overview(s, pcm, nsamples, k, 1, rgba_out, peaks_out, columns, &columns, timing); });
}

// ---- the mean overview inside the stream (sgz.h, "The mean overview") ----------------------------------------------------------------------------
sgz_status sgz_pcm_stream_feed_overview_stats(sgz_pcm_stream *s, const void *pcm, size_t nsamples, uint32_t k, int flush, uint8_t *rgba_out,
                                              sgz_overview_stat_record *stats_out, float *means_out, uint64_t capacity_columns, uint64_t *columns_out,
                                              sgz_pcm_timing *timing)
{
    static const PcmOvTexts text = {"sgz_pcm_stream_feed_overview_stats: null pcm", "sgz_pcm_stream_feed_overview_stats: k differs from the open column's -- flush or reset first",
                                    "sgz_pcm_stream_feed_overview_stats: capacity_columns below what this feed yields (see *columns_out)", nullptr};
    PcmOverviewPart part{kOvStats, k, flush, pcmStatsRun};
    return pcmOverviewFeed(s, pcm, nsamples, text, part, capacity_columns, columns_out, timing, [&]() -> sgz_status {
        if (!rgba_out && !stats_out && !means_out) return fail(SGZ_EINVAL, "overview stats: an image, the records, the means or any of them");
        if (reinterpret_cast<uintptr_t>(stats_out) % alignof(sgz_overview_stat_record)) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview_stats: stats_out is not aligned to 8 bytes");
        const size_t records = pcmPeaksFloats(*s, 1);                // one per float of the peaks
        part.add(kOutOvImage, pcmImageBytes(*s, 1), rgba_out);
        part.add(kOutOvStats, records * sizeof(sgz_overview_stat_record), stats_out);
        part.add(kOutOvMeans, records * sizeof(float), means_out);
        part.firstUse[0] = {&s->d_ovCarry[kOvStats], records * sizeof(sgz_overview_stat_record)};
        return SGZ_OK;
    });
}

sgz_status sgz_spectrogram_overview_stats_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                              const uint32_t *channel_map, size_t nsamples, uint32_t k, uint8_t *rgba_out,
                                              sgz_overview_stat_record *stats_out, float *means_out, sgz_pcm_timing *timing)
{
    return pcmOverviewOneShot(!cfg || !pcm, cfg, format, src_channels, channel_map, nsamples, k, timing,
                              [&] { return (!rgba_out && !stats_out && !means_out) ? fail(SGZ_EINVAL, "overview stats: an image, the records, the means or any of them") : SGZ_OK; },
                              [&](sgz_pcm_stream *s, uint64_t columns) { return sgz_pcm_stream_feed_overview_stats(s, pcm, nsamples, k, 1, rgba_out, stats_out, means_out, columns, &columns, timing); });
}

// ---- the percentile overview inside the stream (sgz.h, "The percentile overview") ----------------------------------------------------------------
sgz_status sgz_pcm_stream_feed_overview_pct(sgz_pcm_stream *s, const void *pcm, size_t nsamples, uint32_t k, int flush, const double *q, uint32_t nq,
                                            uint8_t *rgba_out, sgz_overview_pct_record *records_out, float *values_out, uint64_t capacity_columns,
                                            uint64_t *columns_out, sgz_pcm_timing *timing)
{
    static const PcmOvTexts text = {"sgz_pcm_stream_feed_overview_pct: null pcm", "sgz_pcm_stream_feed_overview_pct: k differs from the open column's -- flush or reset first",
                                    "sgz_pcm_stream_feed_overview_pct: capacity_columns below what this feed yields (see *columns_out)", nullptr};
    PcmOverviewPart part{kOvPct, k, flush, pcmPctRun};
    return pcmOverviewFeed(s, pcm, nsamples, text, part, capacity_columns, columns_out, timing, [&]() -> sgz_status {
        if (!validPctQuantiles(q, nq)) return fail(SGZ_EINVAL, "overview pct: 1 .. 8 quantiles, each in [0, 1]");
        if (!rgba_out && !records_out && !values_out) return fail(SGZ_EINVAL, "overview pct: an image, the records, the values or any of them");
        if (reinterpret_cast<uintptr_t>(records_out) % alignof(sgz_overview_pct_record)) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview_pct: records_out is not aligned to 4 bytes");
        const size_t records = pcmPeaksFloats(*s, 1);                // one per float of the peaks
        part.q = q; part.nq = nq;
        part.add(kOutOvImage, pcmImageBytes(*s, 1), rgba_out);
        part.add(kOutOvPct, records * sizeof(sgz_overview_pct_record), records_out);
        for (uint32_t j = 0; j < nq; ++j)                            // plane j of the caller's buffer: capacity_columns columns behind plane j - 1
            part.add(PcmOutKind(kOutOvPctValues + j), records * sizeof(float), values_out ? values_out + size_t(j) * size_t(capacity_columns) * records : nullptr);
        part.firstUse[0] = {&s->d_ovCarry[kOvPct], records * sizeof(sgz_overview_pct_record)};
        return SGZ_OK;
    });
}

sgz_status sgz_spectrogram_overview_pct_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                            const uint32_t *channel_map, size_t nsamples, uint32_t k, const double *q, uint32_t nq, uint8_t *rgba_out,
                                            sgz_overview_pct_record *records_out, float *values_out, sgz_pcm_timing *timing)
{
    return pcmOverviewOneShot(!cfg || !pcm, cfg, format, src_channels, channel_map, nsamples, k, timing,
                              [&]() -> sgz_status {
                                  if (!validPctQuantiles(q, nq)) return fail(SGZ_EINVAL, "overview pct: 1 .. 8 quantiles, each in [0, 1]");
                                  return (!rgba_out && !records_out && !values_out) ? fail(SGZ_EINVAL, "overview pct: an image, the records, the values or any of them") : SGZ_OK;
                              },
                              [&](sgz_pcm_stream *s, uint64_t columns) { return sgz_pcm_stream_feed_overview_pct(s, pcm, nsamples, k, 1, q, nq, rgba_out, records_out, values_out, columns, &columns, timing); });
}

// ---- the power overview inside the stream (sgz.h, "The power overview") --------------------------------------------------------------------------
sgz_status sgz_pcm_stream_feed_overview_power(sgz_pcm_stream *s, const void *pcm, size_t nsamples, uint32_t k, int flush, uint8_t *rgba_out,
                                              sgz_overview_power_record *power_out, float *levels_out, uint64_t capacity_columns, uint64_t *columns_out,
                                              sgz_pcm_timing *timing)
{
    static const PcmOvTexts text = {"sgz_pcm_stream_feed_overview_power: null pcm", "sgz_pcm_stream_feed_overview_power: k differs from the open column's -- flush or reset first",
                                    "sgz_pcm_stream_feed_overview_power: capacity_columns below what this feed yields (see *columns_out)", nullptr};
    PcmOverviewPart part{kOvPower, k, flush, pcmPowerRun};
    return pcmOverviewFeed(s, pcm, nsamples, text, part, capacity_columns, columns_out, timing, [&]() -> sgz_status {
        if (!rgba_out && !power_out && !levels_out) return fail(SGZ_EINVAL, "overview power: an image, the records, the levels or any of them");
        if (reinterpret_cast<uintptr_t>(power_out) % alignof(sgz_overview_power_record)) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview_power: power_out is not aligned to 8 bytes");
        if (sgz_status st = powerOverviewSupported(s->plan->impl); st != SGZ_OK) return st;
        if (s->track.armed()) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview_power: the track lane is armed and a power feed has no line results to search -- disarm it (sgz_pcm_stream_set_track) first");
        const size_t records = pcmPeaksFloats(*s, 1) * size_t(s->plan->impl.sides);
        part.add(kOutOvImage, pcmImageBytes(*s, 1), rgba_out);
        part.add(kOutOvPower, records * sizeof(sgz_overview_power_record), power_out);
        part.add(kOutOvLevels, records * sizeof(float), levels_out);
        part.firstUse[0] = {&s->d_ovCarry[kOvPower], records * sizeof(sgz_overview_power_record)};
        return SGZ_OK;
    });
}

sgz_status sgz_spectrogram_overview_power_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                              const uint32_t *channel_map, size_t nsamples, uint32_t k, uint8_t *rgba_out,
                                              sgz_overview_power_record *power_out, float *levels_out, sgz_pcm_timing *timing)
{
    return pcmOverviewOneShot(!cfg || !pcm, cfg, format, src_channels, channel_map, nsamples, k, timing,
                              [&]() -> sgz_status {
                                  if (!rgba_out && !power_out && !levels_out) return fail(SGZ_EINVAL, "overview power: an image, the records, the levels or any of them");
                                  if (cfg->algorithm == SGZ_ALGO_RSNT) return fail(SGZ_EUNSUPPORTED, "the power overview reduces transform magnitudes: RSNT plans are not supported");
                                  if (cfg->channel_mode == SGZ_CH_PHASE) return fail(SGZ_EUNSUPPORTED, "the power overview reduces magnitudes: Phase mode's second plane is none");
                                  return SGZ_OK;
                              },
                              [&](sgz_pcm_stream *s, uint64_t columns) { return sgz_pcm_stream_feed_overview_power(s, pcm, nsamples, k, 1, rgba_out, power_out, levels_out, columns, &columns, timing); });
}

// ---- the cross overview inside the stream (sgz.h, "The cross overview") --------------------------------------------------------------------------
sgz_status sgz_pcm_stream_set_cross_edges(sgz_pcm_stream *s, const uint32_t *edges, uint32_t bands)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (sgz_status st = crossOverviewSupported(s->plan->impl); st != SGZ_OK) return st;
    if (s->ovOpen && s->ovKind == kOvCross) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_cross_edges: a cross overview's column is open -- flush it (sgz_pcm_stream_feed_overview_cross) or reset the stream first");
    if (sgz_status st = sgz_plan_set_cross_edges(s->plan, edges, bands); st != SGZ_OK) return st;
    void *&carry = s->d_ovCarry[kOvCross];
    if (carry) { (void)hipFree(carry); carry = nullptr; }
    SGZ_HIP(hipMalloc(&carry, size_t(s->cfg.num_pairs) * bands * sizeof(sgz_overview_cross_record)));
    return SGZ_OK;
}

sgz_status sgz_pcm_stream_feed_overview_cross(sgz_pcm_stream *s, const void *pcm, size_t nsamples, uint32_t k, int flush,
                                              sgz_overview_cross_record *cross_out, uint64_t capacity_columns, uint64_t *columns_out,
                                              sgz_pcm_timing *timing)
{
    static const PcmOvTexts text = {"sgz_pcm_stream_feed_overview_cross: null pcm", "sgz_pcm_stream_feed_overview_cross: k differs from the open column's -- flush or reset first",
                                    "sgz_pcm_stream_feed_overview_cross: capacity_columns below what this feed yields (see *columns_out)", "sgz_pcm_stream_feed_overview_cross: null cross_out"};
    PcmOverviewPart part{kOvCross, k, flush, pcmCrossRun};
    return pcmOverviewFeed(s, pcm, nsamples, text, part, capacity_columns, columns_out, timing, [&]() -> sgz_status {
        if (sgz_status st = crossOverviewSupported(s->plan->impl); st != SGZ_OK) return st;
        if (!s->plan->impl.crossBands || !s->d_ovCarry[kOvCross]) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview_cross: the stream has no band table (sgz_pcm_stream_set_cross_edges)");
        if (reinterpret_cast<uintptr_t>(cross_out) % alignof(sgz_overview_cross_record)) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview_cross: cross_out is not aligned to 8 bytes");
        if (s->track.armed()) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview_cross: the track lane is armed and a cross feed has no line results to search -- disarm it (sgz_pcm_stream_set_track) first");
        part.add(kOutOvCross, size_t(s->cfg.num_pairs) * s->plan->impl.crossBands * sizeof(sgz_overview_cross_record), cross_out);
        return SGZ_OK;
    });
}

sgz_status sgz_spectrogram_overview_cross_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                              const uint32_t *channel_map, size_t nsamples, const uint32_t *edges, uint32_t bands, uint32_t k,
                                              sgz_overview_cross_record *cross_out, sgz_pcm_timing *timing)
{
    return pcmOverviewOneShot(!cfg || !pcm || !edges || !cross_out, cfg, format, src_channels, channel_map, nsamples, k, timing,
                              [&]() -> sgz_status {
                                  if (cfg->algorithm == SGZ_ALGO_RSNT) return fail(SGZ_EUNSUPPORTED, "the cross overview reduces transform bins: RSNT plans are not supported");
                                  if (cfg->channel_mode != SGZ_CH_PHASE) return fail(SGZ_EUNSUPPORTED, "the cross overview reduces the complex bins of both channels: only SGZ_CH_PHASE plans keep them");
                                  return SGZ_OK;
                              },
                              [&](sgz_pcm_stream *s, uint64_t columns) {
                                  if (sgz_status st = sgz_pcm_stream_set_cross_edges(s, edges, bands); st != SGZ_OK) return st;
                                  return sgz_pcm_stream_feed_overview_cross(s, pcm, nsamples, k, 1, cross_out, columns, &columns, timing);
                              });
}

// ---- the flux overview inside the stream (sgz.h, "The flux overview") ----------------------------------------------------------------------------
sgz_status sgz_pcm_stream_feed_overview_flux(sgz_pcm_stream *s, const void *pcm, size_t nsamples, uint32_t k, int flush, sgz_overview_flux_record *flux_out,
                                             uint64_t capacity_columns, uint64_t *columns_out, sgz_pcm_timing *timing)
{
    static const PcmOvTexts text = {"sgz_pcm_stream_feed_overview_flux: null pcm", "sgz_pcm_stream_feed_overview_flux: k differs from the open column's -- flush or reset first",
                                    "sgz_pcm_stream_feed_overview_flux: capacity_columns below what this feed yields (see *columns_out)", "sgz_pcm_stream_feed_overview_flux: null flux_out"};
    PcmOverviewPart part{kOvFlux, k, flush, pcmFluxRun};
    return pcmOverviewFeed(s, pcm, nsamples, text, part, capacity_columns, columns_out, timing, [&]() -> sgz_status {
        if (reinterpret_cast<uintptr_t>(flux_out) % alignof(sgz_overview_flux_record)) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview_flux: flux_out is not aligned to 8 bytes");
        if (sgz_status st = fluxOverviewSupported(s->plan->impl); st != SGZ_OK) return st;
        if (s->track.armed()) return fail(SGZ_EINVAL, "sgz_pcm_stream_feed_overview_flux: the track lane is armed and a flux feed has no line results to search -- disarm it (sgz_pcm_stream_set_track) first");
        const size_t records = size_t(s->cfg.num_pairs) * size_t(s->plan->impl.sides);
        part.add(kOutOvFlux, records * sizeof(sgz_overview_flux_record), flux_out);
        part.firstUse[0] = {&s->d_ovCarry[kOvFlux], records * sizeof(sgz_overview_flux_record)};
        part.firstUse[1] = {reinterpret_cast<void **>(&s->d_ovFluxPrev), records * s->cfg.axis_points * sizeof(float)};
        return SGZ_OK;
    });
}

sgz_status sgz_spectrogram_overview_flux_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                             const uint32_t *channel_map, size_t nsamples, uint32_t k, sgz_overview_flux_record *flux_out,
                                             sgz_pcm_timing *timing)
{
    return pcmOverviewOneShot(!cfg || !pcm || !flux_out, cfg, format, src_channels, channel_map, nsamples, k, timing,
                              [&]() -> sgz_status {
                                  if (cfg->algorithm == SGZ_ALGO_RSNT) return fail(SGZ_EUNSUPPORTED, "the flux overview reduces transform magnitudes: RSNT plans are not supported");
                                  if (cfg->channel_mode == SGZ_CH_PHASE) return fail(SGZ_EUNSUPPORTED, "the flux overview reduces magnitudes: Phase mode's second plane is none");
                                  return SGZ_OK;
                              },
                              [&](sgz_pcm_stream *s, uint64_t columns) { return sgz_pcm_stream_feed_overview_flux(s, pcm, nsamples, k, 1, flux_out, columns, &columns, timing); });
}

}  // extern "C"

// ---- the lanes' calls ---------------------------------------------------------------------------------------------------------------------------
namespace {

// What sgz_pcm_stream_set_<lane> differs in.  leastM, leastWhy: "m >= leastM samples per column (leastWhy)" (1: any m); out, alignedTo: the
// output argument's name and how its alignment is worded; cellBytes: of the carry per channel or pair (0: by the filter, made by the lane's own
// `fresh`); history: the carry holds a history, which an arming unlike the last one begins anew; differs: what an open column refuses
struct PcmLaneSetting {
    PcmSinkId id;
    uint32_t leastM;
    const char *leastWhy, *out;
    size_t align;
    const char *alignedTo;
    size_t cellBytes;
    bool ofPairs, history;
    const char *differs;
};
constexpr const char *kMDiffers = "m differs from";
const PcmLaneSetting kSetWave{kSinkWave, 1, "", "wave_out", alignof(float), "float", 2 * sizeof(float), false, false, kMDiffers};
const PcmLaneSetting kSetLevel{kSinkLevel, 1, "", "level_out", alignof(sgz_level_record), "8 bytes", sizeof(sgz_level_record), true, false, kMDiffers};
const PcmLaneSetting kSetTruePeak{kSinkTruePeak, 1, "", "out", alignof(sgz_truepeak_record), "8 bytes", sizeof(sgz_truepeak_carry), false, true, kMDiffers};
const PcmLaneSetting kSetLoudness{kSinkLoudness, 1, "", "out", alignof(sgz_loudness_record), "8 bytes", 0, false, true, "m or the filter differs from"};
const PcmLaneSetting kSetField{kSinkField, 64, "a 528-byte record per pair for fewer would read back more than the samples", "field_out", alignof(sgz_field_record), "8 bytes", sizeof(sgz_field_record), true, false, kMDiffers};
const PcmLaneSetting kSetBand{kSinkBand, 64, "a 64-byte record per channel for fewer would read back more than the samples", "out", alignof(sgz_band_record), "8 bytes", 0, false, true, "m or the filter differs from"};
const PcmLaneSetting kSetHist{kSinkHist, 128, "a 448-byte record per channel for fewer than 112 samples would read back more than the samples", "hist_out", alignof(sgz_hist_record), "4 bytes", sizeof(sgz_hist_record), false, false, kMDiffers};
const PcmLaneSetting kSetRun{kSinkRun, 32, "a 96-byte record per channel for fewer would read back more than the samples", "out", alignof(sgz_run_record), "4 bytes", sizeof(sgz_run_carry), false, true, "m or the params differ from"};

// sgz_pcm_stream_set_<lane>, once.  keyCheck(who): the check of what the lane takes beside m (a filter, the thresholds), between the least m
// and the output's checks; same(l): the lane is armed with this m (and filter, thresholds) already; fresh(l): what an arming unlike the last
// one does of its own, behind every refusal (the key kept; the filter's carry).  The tail is pcmLaneArm
template <class KeyCheck, class Same, class Fresh>
sgz_status pcmLaneSet(sgz_pcm_stream *s, const PcmLaneSetting &d, uint32_t m, void *out, uint64_t capacity, KeyCheck keyCheck, Same same, Fresh fresh)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    PcmLane &l = s->lane[d.id];
    if (m == 0) { pcmLaneDisarm(l); return SGZ_OK; }
    const auto who = [&l] { return std::string("sgz_pcm_stream_set_") + l.call; };
    if (m < d.leastM) return fail(SGZ_EINVAL, who() + ": m >= " + std::to_string(d.leastM) + " samples per column (" + d.leastWhy + ")");
    if (sgz_status st = keyCheck(who); st != SGZ_OK) return st;
    if (!out && capacity) return fail(SGZ_EINVAL, who() + ": null " + d.out);
    if (reinterpret_cast<uintptr_t>(out) % d.align) return fail(SGZ_EINVAL, who() + ": " + d.out + " is not aligned to " + d.alignedTo);
    const bool asBefore = same(l);
    if (l.open && !asBefore)
        return fail(SGZ_EINVAL, who() + ": " + d.differs + " the open column's -- flush it (sgz_pcm_stream_flush_" + l.call + "), disarm or reset first");
    if (d.cellBytes && !l.d_carry) SGZ_HIP(hipMalloc(&l.d_carry, size_t(2) * (d.ofPairs ? s->cfg.num_pairs : s->numChannels) * d.cellBytes));
    if (!asBefore) {
        if (sgz_status st = fresh(l); st != SGZ_OK) return st;
        if (d.history) { l.continued = false; l.index = 0; }       // (the lane starts at the next sample, index 0, with an empty history; the same arming keeps it)
    }
    pcmLaneArm(*s, l, m, out, capacity);
    return SGZ_OK;
}

// ... the lanes that take m alone
sgz_status pcmLaneSet(sgz_pcm_stream *s, const PcmLaneSetting &d, uint32_t m, void *out, uint64_t capacity)
{
    return pcmLaneSet(s, d, m, out, capacity, [](auto) { return SGZ_OK; }, [m](const PcmLane &l) { return l.m == m; }, [](PcmLane &) { return SGZ_OK; });
}

// ... and the loudness and the band lane.  kept: the stream's filter; limits, taps: the lane's sgz_<lane>_columns_limits and sgz_<lane>_taps;
// rows: of the tap table (4 or 16)
template <class Filter, class Limits, class Taps>
sgz_status pcmTwinSet(sgz_pcm_stream *s, const PcmLaneSetting &d, Filter sgz_pcm_stream::*kept, const Filter *filter, Limits limits, Taps taps, uint32_t rows,
                      uint32_t m, void *out, uint64_t capacity)
{
    return pcmLaneSet(
        s, d, m, out, capacity, [&](auto who) { return filter ? SGZ_OK : fail(SGZ_EINVAL, who() + ": null filter"); },
        [&](const PcmLane &l) { return l.m == m && std::memcmp(&(s->*kept), filter, sizeof *filter) == 0; },
        [&](PcmLane &l) {
            // (what the stage call refuses, and the tap table: a refused filter arms nothing)
            size_t bytes = 0;
            if (sgz_status st = limits(filter, s->numChannels, nullptr, nullptr, &bytes); st != SGZ_OK) return st;
            std::vector<int32_t> table(size_t(rows) * filter->W);
            if (sgz_status st = taps(filter, table.data()); st != SGZ_OK) return st;
            if (l.carryCap < 2 * bytes) {
                // (both slots are idle between feeds, but a flush's launch may still read the old block: wait for it)
                SGZ_HIP(hipStreamSynchronize(s->compute));
                if (l.d_carry) { (void)hipFree(l.d_carry); l.d_carry = nullptr; l.carryCap = 0; }
                SGZ_HIP(hipMalloc(&l.d_carry, 2 * bytes));
                l.carryCap = 2 * bytes;
            }
            s->*kept = *filter;
            l.cur = 0;
            return SGZ_OK;
        });
}

}  // namespace

extern "C" {

sgz_status sgz_pcm_stream_set_waveform(sgz_pcm_stream *s, uint32_t m, float *wave_out, uint64_t capacity_columns) { return pcmLaneSet(s, kSetWave, m, wave_out, capacity_columns); }
sgz_status sgz_pcm_stream_set_level(sgz_pcm_stream *s, uint32_t m, sgz_level_record *level_out, uint64_t capacity_columns) { return pcmLaneSet(s, kSetLevel, m, level_out, capacity_columns); }
sgz_status sgz_pcm_stream_set_truepeak(sgz_pcm_stream *s, uint32_t m, sgz_truepeak_record *out, uint64_t capacity_columns) { return pcmLaneSet(s, kSetTruePeak, m, out, capacity_columns); }
sgz_status sgz_pcm_stream_set_field(sgz_pcm_stream *s, uint32_t m, sgz_field_record *field_out, uint64_t capacity_columns) { return pcmLaneSet(s, kSetField, m, field_out, capacity_columns); }
sgz_status sgz_pcm_stream_set_hist(sgz_pcm_stream *s, uint32_t m, sgz_hist_record *hist_out, uint64_t capacity_columns) { return pcmLaneSet(s, kSetHist, m, hist_out, capacity_columns); }

sgz_status sgz_pcm_stream_set_loudness(sgz_pcm_stream *s, const sgz_loudness_filter *filter, uint32_t m, sgz_loudness_record *out, uint64_t capacity_columns)
{
    return pcmTwinSet(s, kSetLoudness, &sgz_pcm_stream::ldFilter, filter, sgz_loudness_columns_limits, sgz_loudness_taps, 4, m, out, capacity_columns);
}

sgz_status sgz_pcm_stream_set_band(sgz_pcm_stream *s, const sgz_band_filter *filter, uint32_t m, sgz_band_record *out, uint64_t capacity_columns)
{
    return pcmTwinSet(s, kSetBand, &sgz_pcm_stream::bdFilter, filter, sgz_band_columns_limits, sgz_band_taps, 16, m, out, capacity_columns);
}

sgz_status sgz_pcm_stream_set_run(sgz_pcm_stream *s, const sgz_run_params *params, uint32_t m, sgz_run_record *out, uint64_t capacity_columns)
{
    return pcmLaneSet(
        s, kSetRun, m, out, capacity_columns, [&](auto who) { return runParamsCheck(params, who().c_str()); },
        [&](const PcmLane &l) { return l.m == m && std::memcmp(&s->rnParams, params, sizeof *params) == 0; },
        [&](PcmLane &) { s->rnParams = *params; return SGZ_OK; });
}

uint64_t sgz_pcm_stream_waveform_for(const sgz_pcm_stream *s, size_t nsamples, int flush) { return pcmLaneFor(s, kSinkWave, nsamples, flush); }
uint64_t sgz_pcm_stream_level_for(const sgz_pcm_stream *s, size_t nsamples, int flush) { return pcmLaneFor(s, kSinkLevel, nsamples, flush); }
uint64_t sgz_pcm_stream_truepeak_for(const sgz_pcm_stream *s, size_t nsamples, int flush) { return pcmLaneFor(s, kSinkTruePeak, nsamples, flush); }
uint64_t sgz_pcm_stream_loudness_for(const sgz_pcm_stream *s, size_t nsamples, int flush) { return pcmLaneFor(s, kSinkLoudness, nsamples, flush); }
uint64_t sgz_pcm_stream_field_for(const sgz_pcm_stream *s, size_t nsamples, int flush) { return pcmLaneFor(s, kSinkField, nsamples, flush); }
uint64_t sgz_pcm_stream_band_for(const sgz_pcm_stream *s, size_t nsamples, int flush) { return pcmLaneFor(s, kSinkBand, nsamples, flush); }
uint64_t sgz_pcm_stream_hist_for(const sgz_pcm_stream *s, size_t nsamples, int flush) { return pcmLaneFor(s, kSinkHist, nsamples, flush); }
uint64_t sgz_pcm_stream_run_for(const sgz_pcm_stream *s, size_t nsamples, int flush) { return pcmLaneFor(s, kSinkRun, nsamples, flush); }

sgz_status sgz_pcm_stream_waveform_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples) { return pcmLaneState(s, kSinkWave, columns_written, open_samples); }
sgz_status sgz_pcm_stream_level_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples) { return pcmLaneState(s, kSinkLevel, columns_written, open_samples); }
sgz_status sgz_pcm_stream_truepeak_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples) { return pcmLaneState(s, kSinkTruePeak, columns_written, open_samples); }
sgz_status sgz_pcm_stream_loudness_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples) { return pcmLaneState(s, kSinkLoudness, columns_written, open_samples); }
sgz_status sgz_pcm_stream_field_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples) { return pcmLaneState(s, kSinkField, columns_written, open_samples); }
sgz_status sgz_pcm_stream_band_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples) { return pcmLaneState(s, kSinkBand, columns_written, open_samples); }
sgz_status sgz_pcm_stream_hist_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples) { return pcmLaneState(s, kSinkHist, columns_written, open_samples); }
sgz_status sgz_pcm_stream_run_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples) { return pcmLaneState(s, kSinkRun, columns_written, open_samples); }

sgz_status sgz_pcm_stream_flush_waveform(sgz_pcm_stream *s) { return pcmLaneFlush(s, kSinkWave); }
sgz_status sgz_pcm_stream_flush_level(sgz_pcm_stream *s) { return pcmLaneFlush(s, kSinkLevel); }
sgz_status sgz_pcm_stream_flush_truepeak(sgz_pcm_stream *s) { return pcmLaneFlush(s, kSinkTruePeak); }
sgz_status sgz_pcm_stream_flush_loudness(sgz_pcm_stream *s) { return pcmLaneFlush(s, kSinkLoudness); }
sgz_status sgz_pcm_stream_flush_field(sgz_pcm_stream *s) { return pcmLaneFlush(s, kSinkField); }
sgz_status sgz_pcm_stream_flush_band(sgz_pcm_stream *s) { return pcmLaneFlush(s, kSinkBand); }
sgz_status sgz_pcm_stream_flush_hist(sgz_pcm_stream *s) { return pcmLaneFlush(s, kSinkHist); }
sgz_status sgz_pcm_stream_flush_run(sgz_pcm_stream *s) { return pcmLaneFlush(s, kSinkRun); }

// ---- the track lane's calls -------------------------------------------------------------------------------------------------------------------
sgz_status sgz_pcm_stream_set_track(sgz_pcm_stream *s, uint32_t graph, double mouse_fraction, sgz_line_peak *track_out, uint64_t capacity_frames)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (graph >= SGZ_NUM_GRAPHS) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_track: graph");
    if (!std::isfinite(mouse_fraction)) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_track: mouse_fraction");
    if (!track_out && capacity_frames) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_track: null track_out");
    if (reinterpret_cast<uintptr_t>(track_out) % alignof(sgz_line_peak)) return fail(SGZ_EINVAL, "sgz_pcm_stream_set_track: track_out is not aligned to double");
    s->trGraph = graph; s->trFraction = mouse_fraction;
    s->track.arm(track_out ? s->maxFrames : 0, track_out, capacity_frames);                // NULL with capacity 0: off; a slot holds a piece's frames
    return SGZ_OK;
}

uint64_t sgz_pcm_stream_track_for(const sgz_pcm_stream *s, size_t nsamples)
{
    return s && s->track.armed() ? sgz_pcm_stream_frames_for(s, nsamples) : 0;
}

sgz_status sgz_pcm_stream_track_state(const sgz_pcm_stream *s, uint64_t *frames_written)
{
    if (!s) return fail(SGZ_EINVAL, "null stream");
    if (frames_written) *frames_written = s->track.cursor;
    return SGZ_OK;
}

}  // extern "C"
