// runtime.hpp -- internal helpers shared by api.hip and realtime.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "kernels.hpp"
#include "plan.hpp"

namespace sgz {
extern thread_local std::string g_lastError;
sgz_status fail(sgz_status st, const std::string &msg);
sgz_status hipFail(hipError_t e, const char *what);
#define SGZ_HIP(call)                                        \
    do {                                                     \
        hipError_t _e = (call);                              \
        if (_e != hipSuccess) return ::sgz::hipFail(_e, #call); \
    } while (0)

constexpr size_t kExportGranule = size_t(2) << 20;      // allocations that are exported as dma-buf fds: whole 2 MiB blocks (sgz_export_alloc)
sgz_status ensureCap(float **buf, size_t *cap, size_t need);
// line_graph.hip: the line graph's vertex kernel (sgz_line_graph_vertices_device; the spectrum handle's render_line_vertices)
sgz_status launchLineGraphVertices(const float *d_lines, uint32_t pairs, uint32_t P, uint32_t mode, uint32_t flood, float *d_xyz,
                                   hipStream_t stream);
// view_translate.hip: the spectrogram image following a change of view (sgz_view_translate_device; the spectrum handle's set_view).
// translateViewImage waits for its result; scratch / scratchCap (floats) are grown as needed and stay the caller's
bool validViewRect(double left, double right);
sgz_status translateViewImage(uint8_t *image, uint32_t columns, size_t pitch, uint32_t P, const double oldView[2], const double newView[2],
                              float **scratch, size_t *scratchCap, hipStream_t stream);
// image_resize.hip: the spectrogram image following a resize (sgz_image_resize_device; the spectrum handle's resize).  resizeImage waits for
// its result; src and dst may share memory; scratch / scratchCap (floats, imageResizeScratchFloats of them) are grown as needed and stay
// the caller's
bool validAxisPoints(uint32_t P);
bool validImageLayout(const void *d_image, uint32_t columns, size_t pitch);
bool imageResizeFits(uint32_t C0, uint32_t C1, uint32_t P1);         // the kernel's grid and the int32 column table
size_t imageResizeScratchFloats(uint32_t P0, uint32_t C0, uint32_t P1, uint32_t C1);
sgz_status resizeImage(const uint8_t *src, uint32_t C0, size_t srcPitch, uint32_t P0, uint32_t x0, uint8_t *dst, uint32_t C1,
                       size_t dstPitch, uint32_t P1, uint32_t *x1, float **scratch, size_t *scratchCap, hipStream_t stream);
// ring_resize.hip: the real-time Spectrum's mirrored ring [channels][2 cap] at a new capacity, its newest samples kept (sgz_ring_resize_device;
// the spectrum handle's update).  resizeRing enqueues on `stream` and waits for nothing
bool validRingResize(const float *d_old, uint32_t oldCap, const float *d_new, uint32_t newCap, uint32_t channels);
sgz_status resizeRing(const float *d_old, uint32_t oldCap, float *d_new, uint32_t newCap, uint32_t channels, uint64_t written, hipStream_t stream);
// spectrum_present.hip: renderColourSpectrum's frame pacing (:687 / :730 and round(framesPerUpdate), :688), the columns of one video frame
// into the image in one launch (column k = d_columns[(slot0 + k) mod ring], at texel column (x0 + k) mod columns) and drawCircular
// (sgz_columns_to_image_device / sgz_image_unroll_device; the spectrum handle's render_columns / present).  The launches enqueue on
// `stream` and wait for nothing; their arguments are the stage calls', checked by the caller
bool validSmoothing(double smoothing);
double pacedFramesPerUpdate(uint64_t approximateFrames, double smoothing, double framesPerUpdate);
uint64_t pacedFramesThisTime(double framesPerUpdate);
bool imagesOverlap(const void *a, size_t aPitch, uint32_t aColumns, const void *b, size_t bPitch, uint32_t bColumns, uint32_t P);
sgz_status launchColumnsToImage(const uint8_t *d_columns, uint32_t slot0, uint32_t ring, size_t n, uint32_t P, uint8_t *d_image,
                                uint32_t columns, size_t pitch, uint32_t x0, hipStream_t stream);
sgz_status launchImageUnroll(const uint8_t *d_src, uint32_t columns, size_t srcPitch, uint32_t P, uint32_t x, uint8_t *d_dst, size_t dstPitch,
                             hipStream_t stream);
int numCUs();
// K_A over `frames` frames (ideal STFT framing from d_planar); any of mapped/binsOut may be null
// deferLate: the caller's next call is runDecayColour on the same d_mapped with only an image wanted -- a channel-split launch may then
// leave its late pixels (late_fix.hpp) to K_B's fused kernel instead of a launch of its own (runDecayColour checks Plan::lateDeferred)
// imageOnly: nothing but that image is read from d_mapped (side 0 of every pair, and both channels' Nyquist bins through the late pixels):
// an eligible channel-split launch may skip side 1's transform (RealParams::nyFrames).  Set by the caller, never inferred from deferLate
// (the real-time handle defers its late pixels too, and keeps both sides).
// the plan's second stream and the fork / join events that tie it to the caller's (created on first use, destroyed with the plan)
sgz_status ensureSecondStream(Plan &p);
sgz_status resetResonator(Plan &p, hipStream_t stream);
// RSNT, line-graph mode: the resonators advance over one host block of `nsamples` (sample by sample from the carried state); d_mapped
// [C][sides][P] receives the windowed state afterwards
sgz_status runResonatorAdvance(Plan &p, const float *d_planar, size_t chStride, uint32_t nsamples, float *d_mapped, hipStream_t stream);
// sharded RSNT render (api.hip): this rank's chunk from rest without the window kernel; then the carry of the ranks in front + the windows
sgz_status checkResonatorShardBound(const Plan &p, long frames);
sgz_status runResonatorFromRest(Plan &p, const float *d_planar, size_t chStride, long frames, float *d_mapped, hipStream_t stream);
sgz_status runResonatorJoin(Plan &p, long frames, float *d_mapped, const float *d_allEnd, const long long *framesPerRank, uint32_t world, uint32_t rank,
                            float *d_carry, hipStream_t stream);
sgz_status runStft(Plan &p, const float *d_planar, size_t chStride, long frames, float *d_mapped,
                   float *d_binsOut, const float *d_binsIn, hipStream_t stream, unsigned long long *d_phaseClock = nullptr,
                   bool deferLate = false, bool imageOnly = false);
#ifdef SGZ_DEBUG
extern uint32_t g_ablate;   // debug only (tools/ablate.py)
#endif
// K_B: decay recurrence + dB map + colour blend
sgz_status runDecayColour(Plan &p, const float *d_mapped, long frames, uint8_t *d_rgba, float *d_lines,
                          float *d_state, hipStream_t stream, bool magnitudeOnly = false);
sgz_status runDecayEmitWithCarry(Plan &p, const float *d_mapped, long frames, const float *d_carry, uint8_t *d_rgba, float *d_lines,
                                 float *d_stateOut, hipStream_t stream);
// frequency tracker (tracker.hip): peak search + parabolic fit on one (frame, pair)'s csf magnitudes; d_out: DEVICE sgz_peak
sgz_status runTrackPeak(const Plan &p, const float *d_bins, double mouseFraction, sgz_peak *d_out, hipStream_t stream);
// the batched forms: one workgroup per record, asynchronous on `stream`, nothing allocated; d_out: DEVICE [records] / [frames][pairs]
sgz_status runTrackPeaks(const Plan &p, const float *d_bins, size_t records, double mouseFraction, sgz_peak *d_out, hipStream_t stream);
sgz_status runTrackPeaksLines(const Plan &p, const float *d_lines, size_t frames, uint32_t graph, double mouseFraction, sgz_line_peak *d_out,
                              hipStream_t stream);
// ... and the line-results search over value planes d_values [records][P] float (the peaks of any overview or view call); d_out: DEVICE [records]
sgz_status runTrackPeaksValues(const Plan &p, const float *d_values, size_t records, double mouseFraction, sgz_line_peak *d_out, hipStream_t stream);
// the overview's reduction (overview.hip): k frames of line results per column -> image columns / peaks, the open column in d_carry; the
// arguments are sgz_stage_overview's, checked by the caller; asynchronous on `stream`, plan scratch grows on demand
sgz_status runOverviewColumns(Plan &p, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices, float *d_carry,
                              uint8_t *d_rgba, float *d_peaks, hipStream_t stream);
uint32_t overviewAutoSlices(long columns, uint32_t blocks, uint32_t k, size_t frames, int cus);
// the view of kept peaks (overview.hip): d_src [m][pairs][P], the range's first source column -> cols <= m output columns; the arguments are
// sgz_stage_overview_view's, checked by the caller; asynchronous on `stream`, plan scratch grows on demand
sgz_status checkViewRange(uint64_t n, uint64_t x0, uint64_t x1, uint32_t outColumns, uint64_t *cols);
sgz_status checkOverviewStep(uint32_t k, uint64_t held, uint64_t frames);          // what every overview stage call refuses first: k == 0, held >= k
bool bytesOverlap(const void *a, size_t aBytes, const void *b, size_t bBytes);       // two non-null byte ranges share a byte (the views' outputs against their source)
sgz_status runOverviewView(Plan &p, const float *d_src, size_t m, size_t cols, uint32_t slices, uint8_t *d_rgba, float *d_peaksOut, hipStream_t stream);
// The kinds' run...Slabs below are one slab loop (api.hip, overviewSlabs) with the kind's two steps: `frames` frames from d_planar behind `held`
// frames of an open column whose reduction is in d_carry; the columns that close go to the outputs from their first element on, the open one
// stays in d_carry unless `flush`.  What a kind's sgz_spectrogram_overview..._device and sgz_pcm_stream share; the caller has checked the plan
// (powerOverviewSupported, crossOverviewSupported and the band table, fluxOverviewSupported).  The peak hold and the mean overview render
// K_A and K_B per slab -- d_state: the decay state in and out, or null (from rest; kept in plan scratch between slabs) --, the others K_A
// alone: mapped magnitudes with the late pixels completed (power, flux) or complex bins (cross), no decay state.
// track: null, or where the tracker's record of every (frame, pair) goes -- runTrackPeaksLines behind every slab's render on the slab's line
// results, into d_out [frames][pairs] at the slab's frame offset (stream order alone keeps the next slab's render behind it)
struct SlabTrack { uint32_t graph; double mouseFraction; sgz_line_peak *d_out; };
sgz_status runOverviewSlabs(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, long frames, uint32_t k, uint32_t held,
                            int flush, float *d_carry, float *d_state, uint8_t *d_rgba, float *d_peaks, hipStream_t stream,
                            const SlabTrack *track = nullptr);
// the mean overview (overview_stats.hip): the twins of runOverviewColumns and runOverviewView on sgz_overview_stat_record, with the means as
// one more output; the arguments are sgz_stage_overview_stats' / sgz_stage_overview_stats_view's, checked by the caller
sgz_status runOverviewStatsColumns(Plan &p, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                   sgz_overview_stat_record *d_carry, uint8_t *d_rgba, sgz_overview_stat_record *d_stats, float *d_means,
                                   hipStream_t stream);
sgz_status runOverviewStatsView(Plan &p, const sgz_overview_stat_record *d_src, size_t m, size_t cols, uint32_t slices, uint8_t *d_rgba,
                                sgz_overview_stat_record *d_statsOut, float *d_means, hipStream_t stream);
sgz_status runOverviewStatsSlabs(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, long frames, uint32_t k, uint32_t held,
                                 int flush, sgz_overview_stat_record *d_carry, float *d_state, uint8_t *d_rgba, sgz_overview_stat_record *d_stats,
                                 float *d_means, hipStream_t stream, const SlabTrack *track = nullptr);
// the power overview (overview_power.hip): the same twins on sgz_overview_power_record over the mapped magnitudes d_mapped
// [frames][pairs][sides][P], with the levels as the third output; the arguments are sgz_stage_overview_power's / sgz_stage_overview_power_view's,
// checked by the caller
sgz_status runOverviewPowerColumns(Plan &p, const float *d_mapped, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                   sgz_overview_power_record *d_carry, uint8_t *d_rgba, sgz_overview_power_record *d_power, float *d_levels,
                                   hipStream_t stream);
sgz_status runOverviewPowerView(Plan &p, const sgz_overview_power_record *d_src, size_t m, size_t cols, uint32_t slices, uint8_t *d_rgba,
                                sgz_overview_power_record *d_powerOut, float *d_levels, hipStream_t stream);
sgz_status powerOverviewSupported(const Plan &p);                 // Phase and RSNT plans: SGZ_EUNSUPPORTED
sgz_status runOverviewPowerSlabs(sgz_plan *plan, const float *d_planar, size_t channel_stride, long frames, uint32_t k, uint32_t held, int flush,
                                 sgz_overview_power_record *d_carry, uint8_t *d_rgba, sgz_overview_power_record *d_power, float *d_levels,
                                 hipStream_t stream);
// the cross overview (overview_cross.hip): the reduction of the complex bins d_bins [frames][pairs][N + 1] float2 of an SGZ_CH_PHASE plan into
// sgz_overview_cross_record [columns][pairs][bands] by the plan's band table; the arguments are sgz_stage_overview_cross', checked by the caller
sgz_status crossOverviewSupported(const Plan &p);                 // FFT, SGZ_CH_PHASE, N = 2^n: everything else SGZ_EUNSUPPORTED
sgz_status runOverviewCrossColumns(Plan &p, const float *d_bins, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                   sgz_overview_cross_record *d_carry, sgz_overview_cross_record *d_cross, hipStream_t stream);
sgz_status runOverviewCrossSlabs(sgz_plan *plan, const float *d_planar, size_t channel_stride, long frames, uint32_t k, uint32_t held, int flush,
                                 sgz_overview_cross_record *d_carry, sgz_overview_cross_record *d_cross, hipStream_t stream);
// the flux overview (overview_flux.hip): the reduction of the mapped magnitudes d_mapped [frames][pairs][sides][P] into sgz_overview_flux_record
// [columns][pairs][sides]; the arguments are sgz_stage_overview_flux's, checked by the caller, but for d_prev [pairs][sides][P], which is read only
// where prevValid (the frame before frame 0) and written with the call's last frame wherever it is non-null and frames arrive
sgz_status fluxOverviewSupported(const Plan &p);                  // Phase and RSNT plans: SGZ_EUNSUPPORTED
sgz_status runOverviewFluxColumns(Plan &p, const float *d_mapped, size_t frames, uint32_t k, uint32_t held, int flush, uint64_t firstFrame, uint32_t slices,
                                  float *d_prev, bool prevValid, sgz_overview_flux_record *d_carry, sgz_overview_flux_record *d_flux, hipStream_t stream);
// (its slabs keep a slab's last frame in d_prev for the next slab's first; firstFrame: the index of frame 0 in the file)
sgz_status runOverviewFluxSlabs(sgz_plan *plan, const float *d_planar, size_t channel_stride, long frames, uint32_t k, uint32_t held, int flush,
                                uint64_t firstFrame, float *d_prev, bool prevValid, sgz_overview_flux_record *d_carry, sgz_overview_flux_record *d_flux,
                                hipStream_t stream);
// the percentile overview (overview_pct.hip): the mean overview's twin on sgz_overview_pct_record, with nq value planes as the third output.
// PctPlanes: where the call's first column of every plane goes (all null: no values) -- the planes of a render lie a whole render's columns
// apart, those of a stream's slot in blocks of their own; the other arguments are sgz_stage_overview_pct's, checked by the caller
struct PctPlanes { float *p[SGZ_OVERVIEW_PCT_MAX_QUANTILES]; };
inline PctPlanes pctPlanes(float *d_values, size_t offset, size_t planeStride, uint32_t nq)
{
    PctPlanes planes{};
    for (uint32_t j = 0; d_values && j < nq; ++j) planes.p[j] = d_values + size_t(j) * planeStride + offset;
    return planes;
}
bool validPctQuantiles(const double *q, uint32_t nq);              // a host pointer to 1 .. 8 values in [0, 1]
sgz_status runOverviewPctColumns(Plan &p, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices, const double *q,
                                 uint32_t nq, sgz_overview_pct_record *d_carry, uint8_t *d_rgba, sgz_overview_pct_record *d_records,
                                 const PctPlanes &planes, hipStream_t stream);
// (planes: the render's first column of every plane; the slabs move on in each)
sgz_status runOverviewPctSlabs(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, long frames, uint32_t k, uint32_t held,
                               int flush, const double *q, uint32_t nq, sgz_overview_pct_record *d_carry, float *d_state, uint8_t *d_rgba,
                               sgz_overview_pct_record *d_records, const PctPlanes &planes, hipStream_t stream, const SlabTrack *track = nullptr);
// what the overview kinds' files share beside the declarations above (the step, the bounds, the kernel bodies, the launch front): overview_kinds.hpp
// the column lanes' reductions (wave, level, true-peak, loudness, stereo-field, band): column_lanes.hpp
sgz_status trackPeakLines(const Plan &p, const float *results /*host float2 [P]*/, double mouseFraction, sgz_line_peak *out);   // tracker.hip
sgz_status trackPeakValues(const Plan &p, const float *values /*host float [P]*/, double mouseFraction, sgz_line_peak *out);
}  // namespace sgz
