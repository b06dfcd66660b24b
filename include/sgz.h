/*
 * sgz.h -- C ABI of libsgz.so, the MI355X (gfx950) DSP back end for Signalizer's visualiser hot path.
 *
 * Drop-in boundary.  Every entry point names the reference interface it
 * replaces (paths relative to jthorborg/signalizer v0.4.3).  Plain pointers and sizes only: no C++
 * types, no torch types, no exceptions cross this boundary.  All functions return an sgz_status;
 * sgz_last_error() gives the text of the last failure on the calling thread.
 *
 * Pointer spaces: parameters named `d_*` are DEVICE (HBM) pointers, everything else is host memory.
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).
 */
#ifndef SGZ_H
#define SGZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: sgz_spectrum_config grew algorithm / free_q, sgz_scope_config custom_trigger / custom_trigger_frequency (round 3);
 * 4: sgz_spectrum_config grew display_mode (ZERO = the line graph, as in the reference's enum), sgz_spectrum_render_lines,
 *    sgz_spectrum_set_option (round 4);
 * 5: sgz_scope_set_option / sgz_vector_set_option (SGZ_RT_OPT_DEFER_SUBMIT, SGZ_RT_OPT_PARK_PUSHES), sgz_spectrum_track_peak_lines, plan option
 *    SGZ_OPT_WIDE_GROUPS; the Oscilloscope / Vectorscope readers flush the host FIFO as well; SGZ_OPT_RESONATOR_SLAB bounds the sharded RSNT render (round 5; its own option SGZ_OPT_RESONATOR_SHARD_BOUND from round 6);
 * (5, later: sgz_scope_set_mix / sgz_vector_set_mix were added without a version change: no existing entry point or struct changed;
 *  a binding that needs them looks the symbols up.)
 * (5, later: the Oscilloscope's time modes -- sgz_scope_config grew time_mode at its end (SGZ_TIME_*; 0 = the behaviour before), and
 *  sgz_scope_set_tempo, sgz_scope_effective_window and sgz_scope_time_window were added.  The version number stays 5, which the
 *  suite pins; a binding built against an older header passes the shorter sgz_scope_config and must not be mixed with this library.)
 * (5, later: plan option SGZ_OPT_IMAGE_ONLY_SPLIT and the test hook sgz_stage_nyquist.  No existing entry point or struct changed and
 *  the suite pins 5; a binding that sets the option on an older library gets SGZ_EINVAL, "unknown plan option", and looks the hook up.)
 * (5, later: sgz_spectrum_update, sgz_spectrum_update_effects (SGZ_UPDATE_*) and the stage call sgz_ring_resize_device.  No existing
 *  entry point or struct changed and the suite pins 5; a binding that needs them looks the symbols up.)
 * (5, later: interleaved PCM in -- SGZ_PCM_*, sgz_pcm_sample_bytes, sgz_pcm_to_planar_device, the sgz_pcm_stream handle, sgz_stream_step and
 *  sgz_spectrogram_render_pcm.  No existing entry point or struct changed and the suite pins 5; a binding that needs them looks the
 *  symbols up.)
 * (5, later: the overview render -- sgz_overview_step, sgz_stage_overview, sgz_spectrogram_overview_device / _host and plan option
 *  SGZ_OPT_OVERVIEW_SLAB.  No existing entry point or struct changed and the suite pins 5; a binding that needs them looks the symbols
 *  up, and one that sets the option on an older library gets SGZ_EINVAL, "unknown plan option".)
 * (5, later: the file lane -- the view of kept peaks (sgz_overview_view_columns, sgz_stage_overview_view, sgz_overview_view_host) and the
 *  overview inside the PCM stream (sgz_pcm_stream_feed_overview, sgz_pcm_stream_columns_for, sgz_pcm_stream_open_frames,
 *  sgz_pcm_stream_set_option, sgz_spectrogram_overview_pcm).  No struct changed and the suite pins 5; the one new refusal on an existing call, sgz_pcm_stream_feed
 *  while an overview column is open, cannot be reached without the new calls.  A binding that needs them looks the symbols up.)
 * (5, later: the waveform lane -- sgz_stage_wave_columns, sgz_wave_columns_limits and, on the PCM stream, sgz_pcm_stream_set_waveform,
 *  sgz_pcm_stream_waveform_for, sgz_pcm_stream_waveform_state, sgz_pcm_stream_flush_waveform.  No existing entry point or struct changed and
 *  the suite pins 5; a stream that was never armed enqueues what it did before.  A binding that needs them looks the symbols up.)
 * (5, later: the track lane -- sgz_track_peak_values, sgz_stage_track_peaks_values and, on the PCM stream, sgz_pcm_stream_set_track,
 *  sgz_pcm_stream_track_for, sgz_pcm_stream_track_state.  No existing entry point or struct changed and the suite pins 5; a stream that was
 *  never armed enqueues what it did before.  A binding that needs them looks the symbols up.)
 * (5, later: the level lane -- sgz_level_record, sgz_level_reading, sgz_stage_level_columns, sgz_level_columns_limits, the host helpers
 *  sgz_level_fold and sgz_level_readout and, on the PCM stream, sgz_pcm_stream_set_level, sgz_pcm_stream_level_for,
 *  sgz_pcm_stream_level_state, sgz_pcm_stream_flush_level.  No existing entry point or struct changed and the suite pins 5; a stream that
 *  was never armed enqueues what it did before.  A binding that needs them looks the symbols up.)
 * (5, later: the true-peak lane -- sgz_truepeak_record, sgz_truepeak_carry, sgz_stage_truepeak_columns, sgz_truepeak_columns_limits, the
 *  host helpers sgz_truepeak_taps, sgz_truepeak_fold and sgz_truepeak_readout and, on the PCM stream, sgz_pcm_stream_set_truepeak,
 *  sgz_pcm_stream_truepeak_for, sgz_pcm_stream_truepeak_state, sgz_pcm_stream_flush_truepeak.  No existing entry point or struct changed and
 *  the suite pins 5; a stream that was never armed enqueues what it did before.  A binding that needs them looks the symbols up.)
 * (5, later: the loudness lane -- sgz_loudness_filter, sgz_loudness_record, sgz_stage_loudness_columns, sgz_loudness_columns_limits, the host
 *  helpers sgz_loudness_filter_for_rate, sgz_loudness_taps, sgz_loudness_fold, sgz_loudness_readout and sgz_loudness_integrated and, on the
 *  PCM stream, sgz_pcm_stream_set_loudness, sgz_pcm_stream_loudness_for, sgz_pcm_stream_loudness_state, sgz_pcm_stream_flush_loudness.  No
 *  existing entry point or struct changed and the suite pins 5; a stream that was never armed enqueues what it did before.)
 * (5, later: the stereo-field lane -- SGZ_FIELD_SECTORS, sgz_field_record, sgz_field_reading, sgz_stage_field_columns,
 *  sgz_field_columns_limits, the host helpers sgz_field_boundaries, sgz_field_fold and sgz_field_readout and, on the PCM stream,
 *  sgz_pcm_stream_set_field, sgz_pcm_stream_field_for, sgz_pcm_stream_field_state, sgz_pcm_stream_flush_field.  No existing entry point or
 *  struct changed and the suite pins 5; a stream that was never armed enqueues what it did before.)
 * (5, later: the band lane -- sgz_band_filter, sgz_band_record, sgz_stage_band_columns, sgz_band_columns_limits, the host helpers
 *  sgz_band_filter_for_rate, sgz_band_taps, sgz_band_fold, sgz_band_readout and sgz_band_colours and, on the PCM stream,
 *  sgz_pcm_stream_set_band, sgz_pcm_stream_band_for, sgz_pcm_stream_band_state, sgz_pcm_stream_flush_band.  No existing entry point or
 *  struct changed and the suite pins 5; a stream that was never armed enqueues what it did before.)
 * (5, later: the mean overview -- sgz_overview_stat_record, sgz_stage_overview_stats, sgz_spectrogram_overview_stats_device / _host,
 *  sgz_stage_overview_stats_view, sgz_overview_stats_view_host, the host helpers sgz_overview_stats_fold and sgz_overview_stats_readout and,
 *  on the PCM stream, sgz_pcm_stream_feed_overview_stats and sgz_spectrogram_overview_stats_pcm.  No existing entry point or struct changed
 *  and the suite pins 5; the one new refusal on an existing call, sgz_pcm_stream_feed_overview while a stats column is open, cannot be
 *  reached without the new calls.  A binding that needs them looks the symbols up.)
 * (5, later: the histogram lane -- SGZ_HIST_BUCKETS, sgz_hist_record, sgz_hist_reading, sgz_stage_hist_columns, sgz_hist_columns_limits, the
 *  host helpers sgz_hist_edges, sgz_hist_fold, sgz_hist_percentile and sgz_hist_readout and, on the PCM stream, sgz_pcm_stream_set_hist,
 *  sgz_pcm_stream_hist_for, sgz_pcm_stream_hist_state, sgz_pcm_stream_flush_hist.  No existing entry point or struct changed and the suite
 *  pins 5; a stream that was never armed enqueues what it did before.)
 * (5, later: the power overview -- sgz_overview_power_record, sgz_stage_overview_power, sgz_spectrogram_overview_power_device / _host,
 *  sgz_stage_overview_power_view, sgz_overview_power_view_host, the host helpers sgz_overview_power_quantise, sgz_overview_power_fold,
 *  sgz_overview_power_readout and sgz_overview_power_levels and, on the PCM stream, sgz_pcm_stream_feed_overview_power and
 *  sgz_spectrogram_overview_power_pcm.  No existing entry point or struct changed and the suite pins 5; the new refusals on existing calls,
 *  a feed of another kind while a power column is open, cannot be reached without the new calls.  A binding that needs them looks the
 *  symbols up.)
 * (5, later: the cross overview -- sgz_overview_cross_record, sgz_overview_cross_reading, sgz_plan_set_cross_edges, sgz_stage_overview_cross,
 *  sgz_spectrogram_overview_cross_device / _host, the host helpers sgz_overview_cross_quantise, sgz_overview_cross_fold,
 *  sgz_overview_cross_readout, sgz_overview_cross_unit and sgz_cross_edges_octave and, on the PCM stream, sgz_pcm_stream_set_cross_edges,
 *  sgz_pcm_stream_feed_overview_cross and sgz_spectrogram_overview_cross_pcm.  No existing entry point or struct changed and the suite pins 5;
 *  the new refusals on existing calls, a feed of another kind while a cross column is open, cannot be reached without the new calls.  A
 *  binding that needs them looks the symbols up.)
 * (5, later: the flux overview -- sgz_overview_flux_record, sgz_stage_overview_flux, sgz_spectrogram_overview_flux_device / _host, the host
 *  helpers sgz_overview_flux_quantise, sgz_overview_flux_fold, sgz_overview_flux_readout and sgz_overview_flux_hz and, on the PCM stream,
 *  sgz_pcm_stream_feed_overview_flux and sgz_spectrogram_overview_flux_pcm.  No existing entry point or struct changed and the suite pins 5;
 *  the new refusals on existing calls, a feed of another kind while a flux column is open, cannot be reached without the new calls.  A
 *  binding that needs them looks the symbols up.)
 * (5, later: the run lane -- SGZ_RUN_HOT / _QUIET / _FLAT, SGZ_RUN_NAN, sgz_run_params, sgz_run_of, sgz_run_record, sgz_run_carry,
 *  sgz_run_reading, sgz_stage_run_columns, sgz_run_columns_limits, the host helpers sgz_run_params_default, sgz_run_fold and
 *  sgz_run_readout and, on the PCM stream, sgz_pcm_stream_set_run, sgz_pcm_stream_run_for, sgz_pcm_stream_run_state,
 *  sgz_pcm_stream_flush_run.  No existing entry point or struct changed and the suite pins 5; a stream that was never armed enqueues what
 *  it did before.)
 * (5, later: the percentile overview -- SGZ_OVERVIEW_PCT_BUCKETS, SGZ_OVERVIEW_PCT_MAX_QUANTILES, sgz_overview_pct_record,
 *  sgz_stage_overview_pct, sgz_spectrogram_overview_pct_device / _host, the host helpers sgz_overview_pct_bucket, sgz_overview_pct_fold and
 *  sgz_overview_pct_readout and, on the PCM stream, sgz_pcm_stream_feed_overview_pct and sgz_spectrogram_overview_pct_pcm.  No existing
 *  entry point or struct changed and the suite pins 5; the new refusals on existing calls, a feed of another kind while a percentile
 *  column is open, cannot be reached without the new calls.  A binding that needs them looks the symbols up.)
 * a binding compares sgz_abi_version() with the header it was compiled against */
#define SGZ_ABI_VERSION 5

typedef enum sgz_status {
    SGZ_OK = 0,
    SGZ_EMPTY = 1,          /* nothing to pop (frameQueue empty)                              */
    SGZ_SKIPPED_FRAME = 2,  /* prepareTransform returned false, TransformDSP.inl:45-46          */
    SGZ_BUSY = 3,           /* a real-time push found the GPU several blocks behind (or a reconfiguration in progress): the block
                               was NOT taken -- push never waits                                   */
    SGZ_EINVAL = -1,
    SGZ_EHIP = -2,          /* a HIP runtime call failed / no gfx950 device                     */
    SGZ_ENOMEM = -3,
    SGZ_EUNSUPPORTED = -4   /* e.g. line results from a folded carry in SpectrumChannels::Phase     */
} sgz_status;

/* SpectrumChannels, Source/Common/CommonSignalizer.h:495-539 */
enum { SGZ_CH_LEFT = 0, SGZ_CH_RIGHT, SGZ_CH_MERGE, SGZ_CH_SIDE, SGZ_CH_PHASE, SGZ_CH_SEPARATE,
       SGZ_CH_MIDSIDE, SGZ_CH_COMPLEX };
/* SpectrumContent::TransformAlgorithm, Source/Spectrum/SpectrumParameters.h:66-69.  RSNT ("Resonator"): a bank of complex
 * one-pole resonators, one per axis point, advanced by every sample (TransformPair::resonatingDispatch, TransformDSP.inl:1213-1295);
 * a frame is the windowed resonator state every `hop` samples (audioEntryPoint :1172-1201, mapToLinearSpace :1103-1133).  The
 * resonator itself is cpl::dsp::CComplexResonator (absent submodule): restated from its published mathematics, see resonator.hip.
 * EXPERIMENTAL as a drop-in: Signalizer's own part of this algorithm (dispatch, cadence, Phase post-processing, everything behind the
 * frame) follows the reference line by line, but the bank's constants -- bandwidth = spacing to the next axis point, the Q bound by the
 * window size, pole radius exp(-pi B / fs), gain 1 - r, V = 2 K - 1 detuned vectors with the cosine-sum weights a_m / 2, the ignored
 * vectorLength argument of mapSystemHz -- are this build's reading of what such a bank must be, checked against mathematics (an
 * exponentially windowed DFT) and against nothing of cpl's.  A maintainer with the cpl sources should compare
 * sgz_plan_get_resonator() with CComplexResonator::Constant after mapSystemHz (and the vector count with
 * cpl::dsp::windowCoefficients(window).second) before shipping it; the FFT algorithm carries no such caveat beyond "parity unpinned". */
enum { SGZ_ALGO_FFT = 0, SGZ_ALGO_RSNT = 1 };
/* SpectrumContent::DisplayMode, Source/Spectrum/SpectrumParameters.h:60-64 (constant.displayMode, Spectrum.cpp:439).  Only the real-time
 * handle reads it: LINE_GRAPH -- the audio thread transforms nothing (TransformDSP.inl:1167; RSNT: it keeps the resonators running,
 * :1206-1209) and the render thread transforms the current history once per video frame (sgz_spectrum_render_lines =
 * SpectrumRendering.cpp:617-635); COLOUR_SPECTRUM -- a frame every `hop` samples on the audio thread, columns through the frame queue.
 * Plans and the offline / stage entry points ignore it (they are the colour spectrum's chain). */
enum { SGZ_DISPLAY_LINE_GRAPH = 0, SGZ_DISPLAY_COLOUR_SPECTRUM = 1 };
/* SpectrumContent::BinInterpolation */
enum { SGZ_INTERP_NONE = 0, SGZ_INTERP_LINEAR, SGZ_INTERP_LANCZOS };
/* SpectrumContent::ViewScaling */
enum { SGZ_VIEW_LINEAR = 0, SGZ_VIEW_LOG };
/* window shapes / symmetry (stand-in for cpl::dsp::WindowTypes, which lives in the missing cpl) */
enum { SGZ_WIN_RECT = 0, SGZ_WIN_HANN, SGZ_WIN_HAMMING, SGZ_WIN_FLATTOP, SGZ_WIN_BLACKMAN,
       SGZ_WIN_EXACT_BLACKMAN, SGZ_WIN_NUTTALL, SGZ_WIN_BLACKMAN_NUTTALL, SGZ_WIN_BLACKMAN_HARRIS,
       SGZ_WIN_TRIANGULAR, SGZ_WIN_WELCH, SGZ_WIN_GAUSSIAN, SGZ_WIN_KAISER, SGZ_WIN_END };
enum { SGZ_WIN_SYMMETRIC = 0, SGZ_WIN_PERIODIC };
/* OscChannels, Source/Common/CommonSignalizer.h:458-493 */
enum { SGZ_OSC_LEFT = 0, SGZ_OSC_RIGHT, SGZ_OSC_MID, SGZ_OSC_SIDE, SGZ_OSC_SEPARATE, SGZ_OSC_MIDSIDE };

/* OscilloscopeContent::TriggeringMode, Source/Oscilloscope/OscilloscopeParameters.h:50-58 */
enum { SGZ_TRIG_NONE = 0, SGZ_TRIG_SPECTRAL, SGZ_TRIG_WINDOW, SGZ_TRIG_ENVELOPE_HOLD, SGZ_TRIG_ZERO_CROSSING };
/* OscilloscopeContent::TimeMode, Source/Oscilloscope/OscilloscopeParameters.h:60: what sgz_scope_config::window_size counts */
enum { SGZ_TIME_TIME = 0, SGZ_TIME_CYCLES, SGZ_TIME_BEATS };
/* EnvelopeModes / SubSampleInterpolation, Source/Common/CommonSignalizer.h:72-85 */
enum { SGZ_ENV_NONE = 0, SGZ_ENV_RMS, SGZ_ENV_PEAK_DECAY };
enum { SGZ_SUBSAMPLE_NONE = 0, SGZ_SUBSAMPLE_RECTANGULAR, SGZ_SUBSAMPLE_LINEAR, SGZ_SUBSAMPLE_LANCZOS };

#define SGZ_NUM_SPEC_COLOURS 5   /* SpectrumContent::numSpectrumColours */
#define SGZ_NUM_GRAPHS 2         /* SpectrumContent::LineGraphs::LineEnd (LineMain, LineSecond) */

/* POD mirror of Signalizer::TransformConstant<float> inputs
 * (Source/Spectrum/TransformConstant.h:190-239, filled by Spectrum::handleFlagUpdates,
 *  Source/Spectrum/Spectrum.cpp:351-616). */
typedef struct sgz_spectrum_config {
    float    sample_rate;
    uint32_t window_size;        /* W; transform size N = max(32, nextPow2(W)), TransformConstant.h:84 */
    uint32_t hop;                /* sampleBufferSize, SpectrumDSP.cpp:51-54                           */
    uint32_t axis_points;        /* P, Spectrum.cpp:445                                               */
    uint32_t channel_mode;       /* SGZ_CH_*                                                          */
    uint32_t bin_interp;         /* SGZ_INTERP_*                                                      */
    uint32_t view_scaling;       /* SGZ_VIEW_*                                                        */
    uint32_t window_type;        /* SGZ_WIN_*                                                         */
    uint32_t window_symmetry;
    uint32_t num_pairs;          /* stereo pairs (numChannels/2), SpectrumDSP.cpp:65-72               */
    double   window_alpha, window_beta;
    double   view_left, view_right;
    double   min_log_freq;
    double   low_db, high_db, clip_db;
    double   slope_a, slope_b;
    float    pole[SGZ_NUM_GRAPHS];                    /* constant.filter[k].pole                      */
    uint8_t  colours[SGZ_NUM_SPEC_COLOURS + 1][3];    /* [0] background, [1..5] gradient stops (RGB8) */
    uint8_t  _pad[2];
    double   ratios[SGZ_NUM_SPEC_COLOURS];            /* content->specRatios (normalised values)      */
    uint32_t algorithm;          /* SGZ_ALGO_*: constant.algo, Spectrum.cpp:367                                  */
    uint32_t free_q;             /* RSNT: content->freeQ (Spectrum.cpp:593): bandwidths not bounded by the window */
    uint32_t display_mode;       /* SGZ_DISPLAY_*: constant.displayMode (real-time handle only)                   */
    uint32_t _reserved;
} sgz_spectrum_config;

typedef struct sgz_timing {         /* filled by the batch entry points when non-NULL */
    double h2d_ms, kernel_ms, d2h_ms;
    uint64_t frames;
} sgz_timing;

const char *sgz_last_error(void);
int         sgz_abi_version(void);
/* number of visible gfx950 devices (0 when no GPU: every compute entry point then fails with SGZ_EHIP;
 * there is NO CPU fallback in this library). */
int         sgz_device_count(void);
sgz_status  sgz_set_device(int device);

/* ------------------------------------------------------------------------------------------------
 * Spectrum "constant block": replaces TransformConstant<float> + its (re)build in
 * Spectrum::handleFlagUpdates (Spectrum.cpp:489 setStorage, :573 remapFrequencies,
 * :580 generateSlopeMap, :586 regenerateWindowKernel, :226-246 colour ratios).
 * Host-side tables are built on the CPU in fp64 with the reference's expression order and uploaded
 * once; the query functions below expose them for parity tests (they need no GPU).
 *
 * Threading: a plan belongs to the device that was current at its first compute call, and owns the
 * per-launch scratch of its kernels -- like the reference's TransformConstant + TransformPair, which one
 * audio thread uses at a time.  One host thread / stream per plan at a time; concurrent renders use one plan
 * each (the tables are small).  The library itself keeps no process-wide device state: the stage calls'
 * scratch is stream-ordered, the real-time handles own theirs.
 */
typedef struct sgz_plan sgz_plan;
sgz_status sgz_plan_create(const sgz_spectrum_config *cfg, sgz_plan **out);   /* host tables only, no GPU needed */
void       sgz_plan_destroy(sgz_plan *plan);
sgz_status sgz_plan_upload(sgz_plan *plan);                                   /* device tables; needs a GPU */
uint32_t   sgz_plan_transform_size(const sgz_plan *plan);
double     sgz_plan_window_scale(const sgz_plan *plan);                        /* windowKernelScale */
uint32_t   sgz_plan_break_pixel(const sgz_plan *plan);                         /* first max-of-bins pixel */
/* which K_A implementation the transform size and channel mode select: SGZ_PATH_FUSED: N = R^3
 * (4096, 32768) in one workgroup; SGZ_PATH_HALVES: N = 2 R^3 (8192, 65536) as two half-frame workgroups + a map kernel;
 * SGZ_PATH_GENERIC: HBM-resident passes (every other size, and Phase at any size).  Bit SGZ_PATH_SIDE_MAP: the halves /
 * generic path can use the LDS-staged per-side map kernel (the view's records stay inside the staged csf range). */
#define SGZ_PATH_GENERIC  0u
#define SGZ_PATH_FUSED    1u
#define SGZ_PATH_HALVES   2u
#define SGZ_PATH_SIDE_MAP 4u
#define SGZ_PATH_CHANNEL_SPLIT 8u   /* N = 16384 / 32768 / 65536, W == N, even hop: the real-input kernel (spectrum_real.hip) -- Separate: one
                                       workgroup per (frame, pair, channel); Left / Right / Merge / Side: one per (frame, pair) on the mixed
                                       signal -- takes the place of the kernels above, whatever the row layout
                                       (at N = 32768 in Separate mode: for launches of up to 1024 tasks) */
uint32_t   sgz_plan_path(const sgz_plan *plan);
/* frames an offline render / stage call produces from `nsamples` samples per channel: FFT: sgz_num_frames(nsamples, W, hop);
 * RSNT: nsamples / hop (a frame after every hop samples, no window history) */
uint64_t   sgz_plan_num_frames(const sgz_plan *plan, size_t nsamples);
/* RSNT plans: the resonator bank CComplexResonator::Constant::mapSystemHz builds (TransformConstant.h:120-123) -- `vectors` detuned
 * resonators per axis point: coeff [vectors][P] (re, im) pole positions, gain [P], weights [vectors] of the frequency-domain window.
 * Any output may be NULL; returns SGZ_EINVAL on an FFT plan. */
sgz_status sgz_plan_get_resonator(const sgz_plan *plan, uint32_t *vectors, float *coeff, float *gain, float *weights);
/* RSNT plans carry the resonator state between calls (the reference's TransformPair::cresonator).  sgz_stage_mapped and renders without
 * a carried decay state (d_state == NULL) start from rest by themselves; a render WITH d_state continues the stream, resonators
 * included.  This call puts them to rest explicitly (TransformPair.h:183 resetState); no-op on FFT plans. */
sgz_status sgz_plan_reset_resonator(sgz_plan *plan, void *stream);
/* Per-plan switches (all default to what is fastest; the parity tests and measurements flip them):
 *   SGZ_OPT_CHANNEL_SPLIT  1 (default): eligible plans run the real-input channel-split kernels (SGZ_PATH_CHANNEL_SPLIT); 0: never
 *   SGZ_OPT_FUSED_COLOUR   1 (default): an image-only K_B of one pair runs as the single fused launch, a workgroup per 4 pixels; 8 / 16:
 *                          the same with 8 / 16 pixels per workgroup (fewer, longer workgroups: slower on an idle device, but less of
 *                          the chip is taken from kernels that run beside it -- what sgz_render_queue lanes use); 0: scan + emit launches
 *   SGZ_OPT_FETCH_WINDOW   0 (default): Hann / Hamming periodic windows at W == N are evaluated inside K_A; 1: fetched from the table
 * Call between sgz_plan_create and the first compute call on the plan (same threading rule as every other plan call). */
#define SGZ_OPT_CHANNEL_SPLIT 1u
#define SGZ_OPT_FUSED_COLOUR  2u
#define SGZ_OPT_FETCH_WINDOW  3u
#define SGZ_OPT_MATRIX_RESONATOR 4u /* RSNT launches of several frames at a hop that is a multiple of 1024: every frame starts from rest as block
                                      sums on the matrix cores and the frames are chained afterwards (a one-frame launch -- the real-time case --
                                      is always the reference's recurrence sample by sample).  2 (default): the fp32 matrix cores
                                      (resonateMfmaKernel, exact fp32 multiply-add chains); 1: the bf16 matrix cores, every fp32 sample and
                                      weight as the exact sum of three bf16 parts, six part products (fp32-equivalent accuracy, twice as fast:
                                      resonator.hip resonateMfmaBf16Kernel) -- OPT-IN since round 6: on the MI355X boxes this was measured on, FFT
                                      kernels that run on the device at the same time (another stream, another process; this library's and
                                      rocFFT's alike) came back with a wrong cache line's worth of values in 2 of 100 000 launches while this
                                      kernel ran in its round-4 form, and in every second launch with other instruction orders of the same
                                      kernel; the form shipped now (four idle cycles behind every matrix instruction, the middle of a range
                                      that was clean in 350 000 launches) showed none -- a measurement, not a guarantee: choose it when nothing
                                      else shares the device (NOTES.md, "A matrix-core kernel that disturbs its neighbours"); 0: the
                                      vector-ALU block form everywhere (frame 0 of a launch then continues the carried state sample by sample) */
#define SGZ_OPT_RESONATOR_SLAB 5u   /* RSNT: frames per slab of a long render (the per-frame resonator states between the kernels are held for one
                                      slab at a time; 0, the default: as many frames as fit 256 MiB).  A slab continues the state the one
                                      before it left.  It plays no part in the sharded render (SGZ_OPT_RESONATOR_SHARD_BOUND) */
#define SGZ_OPT_WIDE_GROUPS 6u       /* retired: N = 32768 channel-split plans always run the 512-thread form (spectrum_real.hip).  The 1024-thread form
                                      this selected measured 7-12 % slower; the option is accepted for source compatibility, any
                                      value returns SGZ_OK and changes nothing */
#define SGZ_OPT_RESONATOR_SHARD_BOUND 7u /* RSNT, sgz_spectrogram_render_sharded only: that render holds the per-frame resonator states of a rank's WHOLE
                                      chunk between its two halves (from rest ... carry + windows) and cannot cut it, so this is a bound, in frames
                                      (0, the default: 8 GiB worth): a rank's chunk above it is refused with SGZ_EUNSUPPORTED on every rank before
                                      anything is allocated or exchanged (round 6; rounds 4-5 read SGZ_OPT_RESONATOR_SLAB here) */
#define SGZ_OPT_PIPELINED 8u          /* 1: other launches run beside this plan's (a lane of an sgz_render_queue sets it): K_A without the tunings of a launch
                                      that has the chip to itself (the second generation's delayed start, the wave priorities).  Same results. */
#define SGZ_OPT_IMAGE_ONLY_SPLIT 9u   /* 1 (default): a render that asks for the image alone (sgz_spectrogram_render_device / sgz_spectrogram_render
                                      without lines or state, sgz_render_queue) of a one-pair Separate plan at N = 32768 with an evaluated window, no
                                      low pixels and the fused colour K_B transforms the pair's first channel only, and takes the second channel's
                                      Nyquist bin -- the one number of it the image reads -- from workgroups that sum it without a transform.  Every
                                      input sample is still read; the image is byte-identical.  0: both channels' transforms (for A/B and tests);
                                      2 <= n <= 4096: as 1, with n frames per Nyquist workgroup instead of the automatic size (a render of fewer
                                      frames uses its frame count); larger values are refused with SGZ_EINVAL.  Other renders, the stage calls
                                      and the real-time handles are not affected. */
#define SGZ_OPT_OVERVIEW_SLAB 10u     /* sgz_spectrogram_overview_device / _host, FFT plans: frames per slab of the render (0, the default: as many as
                                      fit 64 MiB of line results, frames * pairs * graphs * P * 8 bytes).  Any value gives the same bytes; the
                                      plan's scratch is bounded by the slab, not by the buffer.  RSNT plans render one slab whatever it says. */
sgz_status sgz_plan_set_option(sgz_plan *plan, uint32_t option, uint32_t value);
/* The pixels whose filter taps or arg-max run reach a csf entry the reference leaves complex -- Complex: csf[0] = Z[0]/2
 * (TransformDSP.inl:993); Left / Right / Merge / Side: csf[N/2 .. N-1] (:553-560), reached by windows that wrap below bin 0 or
 * sit at Nyquist -- redone as complex sums after the magnitude-only mapping.  Returns their count; writes at most `cap`. */
uint32_t   sgz_plan_dc_pixels(const sgz_plan *plan, uint32_t *out, uint32_t cap);
sgz_status sgz_plan_get_window(const sgz_plan *plan, float *out /*N*/);
sgz_status sgz_plan_get_mapped_frequencies(const sgz_plan *plan, float *out /*P*/);
sgz_status sgz_plan_get_slope_map(const sgz_plan *plan, float *out /*P*/);
sgz_status sgz_plan_get_colour_ratios(const sgz_plan *plan, float *out /*6*/);
sgz_status sgz_plan_get_colour_table(const sgz_plan *plan, uint32_t pair, float *out /*6*3*/);
/* juce::Colour::withRotatedHue restated (juce_Colour.cpp:33-107,:331-336) */
void       sgz_rotate_hue_rgb8(const uint8_t rgb[3], float amount, uint8_t out[3]);
long       sgz_num_frames(size_t nsamples, uint32_t window_size, uint32_t hop);

/* ------------------------------------------------------------------------------------------------
 * Offline / batch spectrogram: TransformPair::audioEntryPoint (TransformDSP.inl:1165-1211) +
 * AudioDispatcher::blendAndDispatchSpectrums (SpectrumDSP.cpp:111-206) over a whole buffer with ideal
 * STFT framing (frame f = samples [f*hop, f*hop+W)).
 *
 * d_planar:   DEVICE fp32, channel c at d_planar + c*channel_stride, 2*num_pairs channels, nsamples each.
 * d_rgba:     DEVICE RGBA8 [frames][P][4]        (the columns oglImage.updateSingleColumn receives)
 * d_lines:    optional DEVICE float2 [frames][pairs][graphs][P] (lineGraphs[k].results, TransformPair.h:63-94)
 * d_state:    optional DEVICE float2 [pairs][graphs][P] peak-decay state, read as carry-in and
 *             updated to the state after the last frame (lineGraphs[k].states); NULL = start from zero.
 * Asynchronous on `stream`; the caller synchronises.  Fewer samples than one window: nothing is rendered and the call
 * returns SGZ_SKIPPED_FRAME (prepareTransform returns false, TransformDSP.inl:45-46); sgz_spectrogram_render likewise.
 */
sgz_status sgz_spectrogram_render_device(sgz_plan *plan, const float *d_planar, size_t channel_stride,
                                         size_t nsamples, uint8_t *d_rgba, float *d_lines,
                                         float *d_state, void *stream);
/* ---- render queue: a job of MANY buffers, several renders in flight (round 6) ------------------------------------------------------
 * One render of BASELINE configs[1] is 696 workgroups on 512 slots: two full generations and a third that leaves two thirds of the
 * chip idle, then K_B's dependent chain.  A job of many buffers (a folder of files, the channel pairs of a session rendered to separate
 * images, a long buffer cut into independent images) need not pay that per buffer: the queue owns `depth` lanes -- a plan (a plan owns
 * its scratch) and a stream each -- and submits round-robin, so that one buffer's K_B and the partly filled last generation of its K_A
 * run beside the next buffers' K_A.  Measured (tools/pipeline_depth.py, input rotated past the Infinity Cache): 33.3 us per render one
 * after the other, 25.3-26.1 us at depth >= 3: +27 ... 31 % frames/s.  The reference has no counterpart (it transforms one frame per
 * audio callback, TransformDSP.inl:1165-1211); results per buffer are those of sgz_spectrogram_render_device(plan, ..., d_lines = NULL,
 * d_state = NULL, ...) byte for byte (every buffer is a job of its own: decay states start from zero).
 *   submit   never waits for the GPU (a lane that is still busy simply queues the work behind its previous render).  The samples must be
 *            complete -- and d_rgba free of pending work of other streams (a fill, an earlier reader) -- when the render starts:
 *            `after_stream` (may be NULL) is the caller's stream that produced / last touched them; the lane waits for what that stream
 *            holds at the time of the call.  *ticket (optional) numbers the submission, from 1.
 *   wait     host wait until submission `ticket` has finished (0: everything submitted so far)
 *   join     makes `stream` (the caller's) wait for everything submitted so far, without a host wait
 * One thread at a time per queue.  depth 1 .. 16 (3 or more reaches the plateau). */
typedef struct sgz_render_queue sgz_render_queue;
sgz_status sgz_render_queue_create(const sgz_spectrum_config *cfg, uint32_t depth, sgz_render_queue **out);
void       sgz_render_queue_destroy(sgz_render_queue *q);
sgz_status sgz_render_queue_submit(sgz_render_queue *q, const float *d_planar, size_t channel_stride, size_t nsamples,
                                   uint8_t *d_rgba /*[frames][P][4]*/, void *after_stream, uint64_t *ticket);
sgz_status sgz_render_queue_wait(sgz_render_queue *q, uint64_t ticket);
sgz_status sgz_render_queue_join(sgz_render_queue *q, void *stream);
/* Lanes whose streams run side by side.  The runtime maps streams onto a few hardware queues (4 by default; GPU_MAX_HW_QUEUES) and two
 * lanes on one queue run one after the other, so sgz_render_queue_create picks its streams by measurement (a 100 us spin kernel per
 * stream); with depth above the number of hardware queues the remaining lanes share.  Diagnostic. */
uint32_t   sgz_render_queue_distinct_lanes(const sgz_render_queue *q);
/* the lane plans' option (sgz_plan_set_option on every lane; before the first submit) */
sgz_status sgz_render_queue_set_option(sgz_render_queue *q, uint32_t option, uint32_t value);

/* Host buffers in, host buffers out (H2D, render, D2H on a stream of the plan's own); `planar` are the reference's planar channel
 * pointers (AudioStream::Listener::onStreamAudio's float** buffer, Spectrum.h:370).  The plan keeps the device copies between calls:
 * repeated renders of the same shape allocate nothing and rebuild no tables.  sgz_spectrogram_render is the one-shot form (plan
 * built and destroyed inside the call: the fp64 constant block costs more than the render itself). */
sgz_status sgz_spectrogram_render_host(sgz_plan *plan, const float *const *planar, uint32_t num_channels, size_t nsamples,
                                       uint8_t *rgba_out, float *lines_out, sgz_timing *timing);
sgz_status sgz_spectrogram_render(const sgz_spectrum_config *cfg, const float *const *planar,
                                  uint32_t num_channels, size_t nsamples, uint8_t *rgba_out,
                                  float *lines_out, sgz_timing *timing);

/* ---- interleaved PCM in: the offline render fed as a decoder hands audio out ---------------------------------------------------------
 * Audio files hold interleaved integer PCM, often with more channels than the plan has; the planar fp32 the entry points above take is
 * what a caller would otherwise produce on the CPU (and then send 4 bytes per sample where 2 or 3 would do).  The reference has no
 * counterpart: its host hands planar float blocks to onStreamAudio (Spectrum.h:370).
 *
 * Formats: little-endian, sample i of source channel c at byte (i * src_channels + c) * sample_bytes.  The fp32 value is defined exactly:
 *   SGZ_PCM_U8   (x - 128) * 2^-7                    SGZ_PCM_S16  x * 2^-15                SGZ_PCM_S24  3 packed bytes, sign-extended, x * 2^-23
 *   SGZ_PCM_S32  (float) x, nearest even, * 2^-31    SGZ_PCM_F32  the 32 bits copied (NaN payloads, -0, denormals kept)
 *   SGZ_PCM_F64  rounded to nearest even (overflow to +-inf, underflow to a denormal or 0; a NaN stays a NaN, payload unspecified) */
enum { SGZ_PCM_F32 = 0, SGZ_PCM_U8, SGZ_PCM_S16, SGZ_PCM_S24, SGZ_PCM_S32, SGZ_PCM_F64, SGZ_PCM_END };
uint32_t   sgz_pcm_sample_bytes(uint32_t format);            /* 4, 1, 2, 3, 4, 8; 0 for an unknown format (host only) */
/* Convert and de-interleave on the device: row d of d_planar (d < num_channels, at d_planar + d * channel_stride) receives source channel
 * channel_map[d] (HOST array; NULL = identity).  A source channel may feed several rows or none.  Only d_planar[d * channel_stride + i],
 * i < nsamples, is written, and only the nsamples * src_channels * sample_bytes bytes at d_pcm are read.  Asynchronous on `stream`.
 * SGZ_EINVAL, nothing written: a null pointer, an unknown format, src_channels or num_channels of 0 or above 64, a map entry >= src_channels
 * (identity: src_channels < num_channels), channel_stride < nsamples, d_pcm not aligned to the sample's natural alignment (1 for U8 and
 * S24).  nsamples == 0: SGZ_OK, nothing is launched. */
sgz_status sgz_pcm_to_planar_device(const void *d_pcm, uint32_t format, uint32_t src_channels, size_t nsamples,
                                    const uint32_t *channel_map /*HOST [num_channels] or NULL = identity*/, uint32_t num_channels,
                                    float *d_planar, size_t channel_stride, void *stream);

/* The arithmetic of a streamed render (host only): `held` samples are waiting, `incoming` arrive; with total = held + incoming,
 * *frames = total >= window_size ? (total - window_size) / hop + 1 : 0 frames are complete (frame f = samples [f*hop, f*hop + W) of the
 * stream) and *keep = total - *frames * hop samples stay for the next step (keep < window_size; keep >= window_size - hop once a frame
 * was made).  SGZ_EINVAL: a zero window or hop, a null result, hop > window_size (samples between frames would have to be skipped:
 * not a stream this arithmetic describes). */
sgz_status sgz_stream_step(uint32_t window_size, uint32_t hop, uint64_t held, uint64_t incoming, uint64_t *frames, uint64_t *keep);

typedef struct sgz_pcm_timing {     /* filled by feed / render_pcm when non-NULL.  The four stage times are sums of event intervals on three */
    double wall_ms;                 /* streams that overlap: together they may exceed wall_ms (the host's clock around the call).  Asking for */
                                    /* it puts four more event markers per piece on the streams: time a run without it for the wall clock    */
    double h2d_ms, convert_ms, render_ms, d2h_ms;
    uint64_t frames, chunks;        /* columns returned; pieces the PCM was cut into */
} sgz_pcm_timing;

/* The stream handle: interleaved PCM in pieces of any size -> the spectrogram's columns (and line results) as they become complete.
 * Let the stream be everything fed since create or reset.  What all feeds returned, concatenated, equals what
 * sgz_spectrogram_render_host returns for the stream's converted planar floats, byte for byte, however the stream is cut into feeds
 * (empty, one-sample, shorter than the hop or than the held tail) and whatever chunk_samples is.  A feed returns exactly the frames that
 * became complete (sgz_stream_step; sgz_pcm_stream_frames_for tells how many the next feed of nsamples yields); a stream that never reaches
 * window_size samples yields none (feeds: SGZ_OK, *frames_out = 0).
 *   channel_map    HOST [2*num_pairs]: plan channel d is source channel channel_map[d]; NULL = identity
 *   chunk_samples  a feed is cut into pieces of at most this many samples; every piece is uploaded on a copy stream (from the caller's
 *                  memory when it is pinned -- hipHostMalloc / hipHostRegister --, else through one of two pinned slots), converted and
 *                  rendered with carried decay state on a compute stream, and read back on a third (into the caller's memory when pinned):
 *                  upload k+1, render k and read-back k-1 overlap; the host waits to reuse a slot and at the end of the feed.  Device and
 *                  pinned memory are bounded by chunk_samples and window_size, never by the stream's length.
 *                  0 = the default: 2^20 samples, less where a slot of that many frames would pass 256 MiB (64-channel F64: 2^19).  By
 *                  measurement (tools/bench_pcm_render.py, a kept stream fed cfg2's 60 s of stereo S16 at 2^16 .. 2^22: 5.1 / 2.5 / 1.4 /
 *                  0.93 / 0.67 / 0.65 / 0.66 ms): a piece costs ~0.1 ms of host and stream work whatever its size.  At most 2^26.
 *   rgba_out       HOST RGBA8 [capacity_frames][P][4]; lines_out: optional HOST float2 [capacity_frames][pairs][graphs][P]
 * Refusals consume nothing and leave the stream unchanged.  SGZ_EINVAL: what sgz_plan_create or the converter refuses, a null pcm with
 * nsamples > 0, capacity_frames below the need (*frames_out then holds the need), chunk_samples above 2^26.  SGZ_EUNSUPPORTED: an RSNT
 * configuration (its multi-frame launches chain frames from rest within an fp32 bar, not bit for bit: a chunked render would not equal
 * the single one), hop > window_size.  The FFT algorithm is taken in all eight channel modes.
 * reset: a new file -- held samples dropped, decay state zero.  One thread at a time per stream; streams are independent. */
typedef struct sgz_pcm_stream sgz_pcm_stream;
sgz_status sgz_pcm_stream_create(const sgz_spectrum_config *cfg, uint32_t format, uint32_t src_channels,
                                 const uint32_t *channel_map /*[2*num_pairs] or NULL*/, size_t chunk_samples /*0 = default*/,
                                 sgz_pcm_stream **out);
void       sgz_pcm_stream_destroy(sgz_pcm_stream *s);
uint64_t   sgz_pcm_stream_frames_for(const sgz_pcm_stream *s, size_t nsamples);   /* frames the next feed of nsamples yields */
sgz_status sgz_pcm_stream_feed(sgz_pcm_stream *s, const void *pcm /*HOST*/, size_t nsamples, uint8_t *rgba_out, float *lines_out /*or NULL*/,
                               uint64_t capacity_frames, uint64_t *frames_out, sgz_pcm_timing *timing /*or NULL*/);
sgz_status sgz_pcm_stream_reset(sgz_pcm_stream *s);
/* The overview inside the stream: the same pieces, three streams and two slots, but every piece's frames are reduced on the device to the
 * overview's columns of k frames (below, "The overview render") and only those are read back: the image, the peaks V or both.  Let the
 * stream be everything fed since create or reset.  The columns of all overview feeds, of which only the last flushes, concatenated, equal
 * what sgz_spectrogram_overview_host returns for the stream's converted planar floats, byte for byte, image and peaks, however the
 * stream is cut into feeds and whatever chunk_samples and SGZ_OPT_OVERVIEW_SLAB are.  A feed returns exactly the columns that closed; the
 * frames of a column that stays open are held on the device (their V, [pairs][P]) with their count.  flush != 0 closes the open column
 * early, the last frame of the feed included (the counts are those of sgz_overview_step chained over the feeds); the next frame opens a
 * new column.  A flush with no open column and no new frames returns none.
 *   rgba_out    HOST RGBA8 [capacity_columns][P][4]; peaks_out HOST float [capacity_columns][pairs][P]; either may be NULL, not both
 *   columns_for    columns the next feed of nsamples yields at k and flush (0 as well where the feed would be refused for its k)
 *   open_frames    frames of the open column
 * Per slot the columns of a piece take ceil(max frames of a piece / k) + 1 columns of device (and, for pageable outputs, pinned) memory,
 * made on first need and grown when a later k needs more; line results stay in the plan's slab scratch (SGZ_OPT_OVERVIEW_SLAB): memory
 * is bounded by chunk_samples, window_size and the slab, never by the stream's length.  sgz_pcm_timing.frames counts the columns returned.
 * Refusals consume nothing and leave the stream unchanged.  SGZ_EINVAL: a null stream, a null pcm with nsamples > 0, k == 0, both outputs
 * NULL, capacity_columns below the need (*columns_out then holds the need), a k other than the open column's while frames are open.  While a
 * column is open sgz_pcm_stream_feed is refused with SGZ_EINVAL (flush or reset first); reset drops the open column. */
sgz_status sgz_pcm_stream_feed_overview(sgz_pcm_stream *s, const void *pcm /*HOST*/, size_t nsamples, uint32_t k, int flush, uint8_t *rgba_out /*or NULL*/,
                                        float *peaks_out /*or NULL*/, uint64_t capacity_columns, uint64_t *columns_out, sgz_pcm_timing *timing /*or NULL*/);
uint64_t   sgz_pcm_stream_columns_for(const sgz_pcm_stream *s, size_t nsamples, uint32_t k, int flush);
uint64_t   sgz_pcm_stream_open_frames(const sgz_pcm_stream *s);
/* sgz_plan_set_option on the stream's own plan (SGZ_OPT_OVERVIEW_SLAB bounds the line results an overview feed keeps on the device; the bytes
 * do not depend on it).  Between feeds. */
sgz_status sgz_pcm_stream_set_option(sgz_pcm_stream *s, uint32_t option, uint32_t value);
/* One-shot: a stream with the default chunk_samples (the buffer's length if that is less), one feed of the whole buffer (rgba_out / lines_out hold
 * sgz_num_frames frames), destroyed.  Fewer samples than one window: SGZ_SKIPPED_FRAME, as sgz_spectrogram_render_host. */
sgz_status sgz_spectrogram_render_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                      const uint32_t *channel_map, size_t nsamples, uint8_t *rgba_out, float *lines_out, sgz_pcm_timing *timing);
/* One-shot overview: a stream with the default chunk_samples (the buffer's length if that is less), one flushed overview feed of the whole
 * buffer (rgba_out / peaks_out hold ceil(sgz_num_frames / k) columns; either may be NULL, not both), destroyed.  Fewer samples than one
 * window: SGZ_SKIPPED_FRAME. */
sgz_status sgz_spectrogram_overview_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                        const uint32_t *channel_map, size_t nsamples, uint32_t k, uint8_t *rgba_out, float *peaks_out,
                                        sgz_pcm_timing *timing);

/* Device memory for the display hand-off: `bytes` rounded up to whole 2 MiB blocks (*allocated), exported as a dma-buf
 * file descriptor (dmabuf_fd may be NULL: plain allocation) that the GL / Vulkan context of the display GPU -- an MI355X has no graphics
 * engine of its own -- or any other process imports (EXT_memory_object_fd, EGL_EXT_image_dma_buf_import, hipImportExternalMemory with
 * hipExternalMemoryHandleTypeOpaqueFd and size = *allocated).  Whole blocks because a dma-buf is a whole buffer object and the runtime
 * packs smaller allocations into shared ones: the importer sees the memory from offset 0 (tests/test_gpu_realtime.py imports the fd in
 * a second process and compares the texels).  The caller closes the fd and frees the memory with sgz_export_free. */
sgz_status sgz_export_alloc(size_t bytes, void **d_ptr, size_t *allocated, int *dmabuf_fd);
void       sgz_export_free(void *d_ptr);

/* Stage entry points (parity tests call these through the ABI; all DEVICE pointers, async on stream):
 *  bins:   per (frame,pair) the post-split magnitude array csf[0..N] of mapToLinearSpace
 *          (TransformDSP.inl:858-869 for Separate/MidSide; :553-560 mono modes) as float [N+1];
 *          Separate / MidSide: csf[0] and csf[N] signed (Re Z[0] / 2, Im Z[0] / 2), the rest magnitudes.  The entries the reference
 *          leaves complex are reported as magnitudes: Complex csf[0] = |Z[0]| / 2; Left / Right / Merge / Side csf[N/2] = |X[N/2]| / 2,
 *          csf[N/2 + 1 .. N - 1] = |X[k]|, csf[N] = 0 -- except on the channel-split kernel's mono form (SGZ_PATH_CHANNEL_SPLIT in
 *          those modes), which writes csf[0 .. N/2] only, with csf[N/2] = X[N/2] / 2 signed (real for a real signal, the value the
 *          reference holds), and leaves csf[N/2 + 1 .. N] untouched (its pixels take conj X[k] from held entries instead);
 *  mapped: csp magnitudes after pixel mapping (TransformDSP.inl:871-985), float [frames][pairs][2][P];
 *  decay+colour from given mapped magnitudes (TransformDSP.inl:1299-1435 + SpectrumDSP.cpp:111-206).
 * SGZ_CH_PHASE (TransformDSP.inl:643-853, :1393-1432): the bins stay complex -- `bins` is float2 [N+1] (re, im) after
 * separateTransformsIPL and the DC / Nyquist fix-ups; the two planes of `mapped` are wsp[2x] (magnitude) and wsp[2x+1]
 * (phase cancellation); state and line results hold (magnitude, phase) where the other modes hold (left, right). */
sgz_status sgz_stage_bins(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples,
                          float *d_bins /*[frames][pairs][N+1]*/, void *stream);
sgz_status sgz_stage_mapped(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples,
                            float *d_mapped /*[frames][pairs][2][P]*/, void *stream);
sgz_status sgz_stage_map_from_bins(sgz_plan *plan, const float *d_bins, size_t frames,
                                   float *d_mapped, void *stream);
/* K_A's dominant launch ALONE, for timing it with events on `stream` (bench.py's roofline line): on a channel-split plan the pixels
 * that need both channels (the top pixels csf[N/2] can win, taps that reach over bin 0) hold the values of the channel's own bins
 * only -- sgz_stage_mapped / the render calls complete them (a small follow-up launch, or K_B's fused kernel as it reads them);
 * on every other plan this is sgz_stage_mapped. */
sgz_status sgz_stage_mapped_dominant(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples,
                                     float *d_mapped /*[frames][pairs][2][P]*/, void *stream);
/* Test hook of a channel-split pair plan: the two channels' Nyquist bins X_L[M], X_R[M] per (frame, pair) as K_A leaves them for
 * csf[N/2], from the launch an image-only render runs (image_only != 0; SGZ_OPT_IMAGE_ONLY_SPLIT) or from the two-channel launch.
 * *ny_frames (may be NULL): frames per Nyquist workgroup of that launch, 0 for the two-channel form; *low_pixels (may be NULL): the
 * plan's pixels whose taps reach over bin 0 into the other channel (such plans keep the two-channel form). */
sgz_status sgz_stage_nyquist(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, int image_only,
                             float *d_ny /*[frames][pairs][2]*/, uint32_t *ny_frames, uint32_t *low_pixels, void *stream);
/* d_rgba and d_lines may both be NULL: a state-only pass that just advances d_state over `frames` frames (what the
 * multi-GPU carry exchange below needs from every rank before the real pass). */
sgz_status sgz_stage_decay_colour(sgz_plan *plan, const float *d_mapped, size_t frames,
                                  uint8_t *d_rgba, float *d_lines, float *d_state, void *stream);

/* Frequency tracker, the raw-FFT branch of Spectrum::drawFrequencyTracking (Source/Spectrum/SpectrumRendering.cpp:379-469; SURVEY 8(f)
 * #4): nearest peak of the raw transform around the mouse position (fraction of the frequency axis, :267 / :292), walk along a rising
 * edge at the range boundary, parabolic fit in the dB domain.  peak_dbs is the value before the slope correction (:453: the caller
 * adds 20 log10(slopeMap[x])).  d_bins: DEVICE csf magnitudes [N + 1] of one (frame, pair) as sgz_stage_bins writes them.
 * Magnitude modes except Complex (:301).  The call waits for its result. */
typedef struct sgz_peak {
    double peak_offset;          /* bin of the peak                         */
    double peak_fraction;        /* 2 (bin + phi) / N                       */
    double peak_frequency;       /* Hz                                      */
    double peak_dbs;
    double alpha, beta, gamma;   /* 20 log10 of the three bins around it    */
    double phi;                  /* fractional bin offset of the parabola   */
} sgz_peak;
sgz_status sgz_stage_track_peak(sgz_plan *plan, const float *d_bins, double mouse_fraction, sgz_peak *out, void *stream);
/* The tracker's OTHER branch (SpectrumRendering.cpp:300-377): in Complex mode, for the RSNT algorithm and for the LineMain / LineSecond
 * graphs the reference looks for the peak in lineGraphs[graph].getResults(axisPoints) -- the displayed line -- instead of the raw bins:
 * first largest leftMagnitude within +-3 % of the axis around the mouse position, the walk along a still rising edge at a boundary of
 * that range, then peakFrequency = mapFrequency(peak), peakDeviance from the neighbouring axis points (for the FFT algorithm with a
 * non-Lanczos bin interpolation at least half a bin in axis points, :355-358), peakFractionY = the line's value there and its dB
 * value on the view's dB range.  `results`: HOST float2 [P] as sgz_spectrum_line_results / sgz_spectrum_render_lines deliver them --
 * the reference reads the same host-resident display results on its GUI thread; this is host arithmetic on a few thousand floats,
 * nothing is launched.  (peak_dbs = low_db + y (high_db - low_db): cpl::Math::UnityScale::linear, absent, by its name.) */
typedef struct sgz_line_peak {
    double peak_offset;          /* axis point of the peak (peakX)               */
    double peak_frequency;       /* mappedFrequencies[peak], Hz                  */
    double peak_deviance;        /* Hz                                           */
    double peak_fraction_y;      /* results[peak].leftMagnitude                  */
    double peak_dbs;
    double peak_slope;           /* slopeMap[peak]                               */
} sgz_line_peak;
sgz_status sgz_track_peak_lines(const sgz_plan *plan, const float *results /*HOST float2 [P]*/, double mouse_fraction, sgz_line_peak *out);
/* Both branches for a whole render: one peak per record, on the device.  One workgroup per record, asynchronous on `stream`; nothing is
 * allocated, nothing is waited for.  The definitions are the single-frame calls above, byte for byte (NaN payloads included):
 *  sgz_stage_track_peaks        d_bins: DEVICE float [records][N + 1], records = frames * pairs, as sgz_stage_bins writes them; d_out: DEVICE
 *                               sgz_peak [records].  Record r == sgz_stage_track_peak(plan, d_bins + r * (N + 1), mouse_fraction, &out, stream)
 *                               (SpectrumRendering.cpp:379-469 per record), with its refusals: Phase / Complex SGZ_EUNSUPPORTED, a non-finite
 *                               mouse_fraction SGZ_EINVAL.  records == 0: SGZ_OK, nothing launched.
 *  sgz_stage_track_peaks_lines  d_lines: DEVICE float2 [frames][pairs][graphs][P] as every render writes them; record (f, p) searches graph
 *                               `graph`.  d_out: DEVICE sgz_line_peak [frames][pairs].  Record (f, p) == sgz_track_peak_lines(plan, <that
 *                               record's P float2 on the host>, mouse_fraction, &out) (:300-377 per record): all six fields, the confinement
 *                               for fewer than 17 axis points, the first largest, both boundary walks; a comparison with a NaN is false, so a
 *                               NaN wins only where the host's loop starts on it and never stops a walk.  graph >= SGZ_NUM_GRAPHS or a
 *                               non-finite mouse_fraction: SGZ_EINVAL.
 * The boundary walks are cooperative (256 neighbour pairs per step): a silent or constant record, whose walk runs to the end of the axis,
 * costs P / 256 steps, not P dependent loads. */
sgz_status sgz_stage_track_peaks(sgz_plan *plan, const float *d_bins, size_t records, double mouse_fraction, sgz_peak *d_out, void *stream);
sgz_status sgz_stage_track_peaks_lines(sgz_plan *plan, const float *d_lines, size_t frames, uint32_t graph, double mouse_fraction,
                                       sgz_line_peak *d_out, void *stream);
/* The offline render, with the line-results tracker applied to every frame on the device: d_track / track_out [frames][pairs] sgz_line_peak,
 * equal to sgz_spectrogram_render_host(..., lines_out) followed by sgz_track_peak_lines per (frame, pair) on graph `graph`, byte for byte.
 * d_rgba / rgba_out may be NULL (track only); an image asked for is that render's image.  Everything else as
 * sgz_spectrogram_render_device / _host (SGZ_SKIPPED_FRAME and nothing written for fewer samples than a window; d_state carry-in / out).
 * Every channel mode and RSNT (every render produces line results; in Phase the searched value is the magnitude half, as in the
 * reference).  The line results stay on the device, in plan-owned scratch that is kept between calls and is PROPORTIONAL TO THE FRAME
 * COUNT (frames * pairs * graphs * P * 8 bytes): the first call, and any call with more frames than every call before it, allocates it
 * and therefore synchronises the device; calls that fit enqueue and return.  _host reads back the track (48 bytes per record) and the image if one was asked for. */
sgz_status sgz_spectrogram_track_device(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, uint32_t graph,
                                        double mouse_fraction, uint8_t *d_rgba, float *d_state, sgz_line_peak *d_track, void *stream);
sgz_status sgz_spectrogram_track_host(sgz_plan *plan, const float *const *planar, uint32_t num_channels, size_t nsamples, uint32_t graph,
                                      double mouse_fraction, uint8_t *rgba_out, sgz_line_peak *track_out, sgz_timing *timing);
/* The line-results search on value planes: float [P] per record instead of float2 -- the layout of V / V', the peaks every overview and view
 * call below writes (d_peaks, peaks_out, d_peaks_out: [columns][pairs][P], records = columns * pairs).  A track drawn over a zoomed-out
 * lane is not a fold of per-frame tracks: the track that belongs on an overview or view column is the tracker applied to that column.
 * Definition (exact, no tolerance): record r == sgz_track_peak_lines(plan, L, mouse_fraction, &out) with L[i] = (values[r][i], anything),
 * byte for byte in all six fields (the confinement below 17 axis points, the first largest, both boundary walks, the NaN rules, the
 * deviance floor); the plan only has to agree in axis_points.
 *  sgz_track_peak_values         host arithmetic on a HOST record, nothing launched.  SGZ_EINVAL: a null argument, a non-finite mouse_fraction.
 *  sgz_stage_track_peaks_values  DEVICE pointers; one workgroup per record (trackLinePeaksKernel's body on the other layout), asynchronous on
 *                                `stream`, nothing allocated, nothing waited for.  SGZ_EINVAL, nothing launched: a null argument, a non-finite
 *                                mouse_fraction.  records == 0: SGZ_OK, nothing launched. */
sgz_status sgz_track_peak_values(const sgz_plan *plan, const float *values /*HOST float [P]*/, double mouse_fraction, sgz_line_peak *out);
sgz_status sgz_stage_track_peaks_values(sgz_plan *plan, const float *d_values /*DEVICE float [records][P]*/, size_t records, double mouse_fraction,
                                        sgz_line_peak *d_out /*DEVICE [records]*/, void *stream);

/* The overview render: an image with k frames per column, reduced and coloured on the device -- what a host draws as a file's
 * spectrogram in a lane, a thumbnail or a zoomed-out view, without reading back one column per frame.  The reference has no counterpart
 * (renderColourSpectrum draws one column per audio frame, Source/Spectrum/SpectrumRendering.cpp:696-721); the colouring is its own.
 * Definition (exact, no tolerance): with L[f][p][g][i] the float2 line results every render writes and F frames,
 *   columns = ceil(F / k); column c covers frames c k <= f < min((c + 1) k, F) (the last one may be partial);
 *   V[c][p][i] = the greatest of L[f][p][0][i].x over the column's frames -- a peak hold of graph 0 (LineMain), first component, the value
 *     the image is coloured from in every channel mode, Phase included.  "Greatest" is a total order, so that any split of the work
 *     gives the same bits: NaNs take no part; the others compare by bits ^ (sign ? 0xFFFFFFFF : 0x80000000) as unsigned (IEEE order
 *     with -0 below +0); a group of NaNs alone yields the quiet NaN 0x7FC00000;
 *   pixel (c, i) = the additive blend of the pairs' colours at V[c][p][i], p = 0 .. pairs - 1 in order, from a black column buffer,
 *     then the 8-bit conversion (SpectrumDSP.cpp:119-198, as K_B does it for a frame).
 * For k == 1 the image is sgz_spectrogram_render_device's byte for byte and V is the line results' first components bit for bit.
 *  sgz_overview_step   host arithmetic, the twin of sgz_stream_step: `held` frames of an open column plus `frames` new ones, t = held +
 *                      frames: *columns = t / k, plus one if flush and t % k != 0; *held_out = flush ? 0 : t % k.  SGZ_EINVAL: k == 0,
 *                      held >= k, a null result.
 *  sgz_stage_overview  the reduction on given line results d_lines [frames][pairs][graphs][P] float2.  d_carry: DEVICE float [pairs][P], the
 *                      open column's V so far -- read iff held > 0, written iff frames stay open afterwards (no flush, t % k != 0), NULL
 *                      allowed when neither applies; a carried column continues exactly as if its frames had come in one call.  d_rgba
 *                      [columns][P][4] and d_peaks float [columns][pairs][P] = V, columns as sgz_overview_step counts them; either may be
 *                      NULL, not both.  slices: 0 = the library's choice, 1 .. 64 forced (few columns of many frames are reduced in that
 *                      many slices per column into plan scratch, then folded) -- identical results.  Only the documented bytes are
 *                      written.  SGZ_EINVAL, nothing launched or written: a null plan or d_lines, k == 0, held >= k, slices > 64, both
 *                      outputs NULL, a needed d_carry that is NULL.  frames == 0 without a column to flush: SGZ_OK, nothing launched.
 *                      Asynchronous on `stream`, nothing is waited for; plan scratch grows on demand (only growth synchronises).
 *  sgz_spectrogram_overview_device / _host   the render: columns = ceil(F / k), the last column flushed; d_rgba / rgba_out [columns][P][4],
 *                      d_peaks / peaks_out float [columns][pairs][P], either may be NULL, not both.  Everything else as
 *                      sgz_spectrogram_render_device / _host: SGZ_SKIPPED_FRAME and nothing written for fewer samples than a window,
 *                      d_state carry-in / out, the host form on the plan's own stream with kept device copies -- it reads back the
 *                      columns and nothing else.  FFT plans render in slabs of frames (SGZ_OPT_OVERVIEW_SLAB; by default 64 MiB of
 *                      line results) with the decay state carried from slab to slab (in a plan-owned buffer when d_state is NULL) and
 *                      the open column carried across the cut: neither the read-back nor the plan's scratch grows with the frame
 *                      count, and the bytes do not depend on the slab.  RSNT plans render ONE slab (their launches chain the frames
 *                      within an fp32 bar, a cut would move the bits -- why sgz_pcm_stream refuses them): their line-result scratch is
 *                      PROPORTIONAL TO THE FRAME COUNT (frames * pairs * graphs * P * 8 bytes), as the tracker's.  The first call,
 *                      and any call that needs more scratch than every call before it, allocates and therefore synchronises the
 *                      device; calls that fit enqueue and return. */
sgz_status sgz_overview_step(uint32_t k, uint64_t held, uint64_t frames, int flush, uint64_t *columns, uint64_t *held_out);
sgz_status sgz_stage_overview(sgz_plan *plan, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                              float *d_carry, uint8_t *d_rgba, float *d_peaks, void *stream);
sgz_status sgz_spectrogram_overview_device(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, uint32_t k,
                                           uint8_t *d_rgba, float *d_peaks, float *d_state, void *stream);
sgz_status sgz_spectrogram_overview_host(sgz_plan *plan, const float *const *planar, uint32_t num_channels, size_t nsamples, uint32_t k,
                                         uint8_t *rgba_out, float *peaks_out, sgz_timing *timing);

/* The mean overview: mean and range of k frames per image column -- the second reduction of the overview render, of the same line results
 * over the same columns.  A peak hold shows transients; at a few hundred frames per column dense material saturates it, and a tone in one
 * frame of 500 looks like a tone in all 500.  This is the "average" every analyser offers beside "peak", with the minimum and the maximum
 * it draws the average between.  One pass over a file gives mean, least and greatest; the image is coloured from the mean.
 * Definition (exact, no tolerance).  L[f][p][g][i], F and k as in the overview render; columns and their frames are counted exactly as
 * there (sgz_overview_step).  Let x = L[f][p][0][i].x.
 *   quantiser  a NaN takes no part in sum, count, lo or hi; it is counted in nans.  Otherwise t = (double)x * 2^20 (exact; +-inf stays
 *              +-inf);  q = 2^31 - 1 if t >= 2^31 - 1;  q = -(2^31 - 1) if t <= -(2^31 - 1);  otherwise q = rint(t), ties to even.
 *              Line results are values on the normalised dB axis: |x| < 2048 covers a clip of -1000 dB over a 1 dB range, at a
 *              resolution of 1e-6 of the axis.
 *   record     per (column, pair, pixel) one sgz_overview_stat_record: sum = the sum of q; count = the non-NaN frames; nans = the NaN
 *              frames; hi the greatest and lo the least of the non-NaN x under the overview's total order (-0 below +0), both
 *              0x7FC00000 when count == 0.  hi is therefore V of the peak-hold overview, bit for bit.  |sum| < 2^63 for every count
 *              below 2^32.
 *   mean       count == 0: the bits 0x7FC00000; otherwise (float)(((double)sum / (double)count) * 2^-20), every conversion and the
 *              division rounded to nearest even, nothing contracted.
 *   pixel      the additive blend of the pairs' colours at the mean, p = 0 .. pairs - 1 in order, from a black column buffer, then the
 *              8-bit conversion -- the overview render's pixel with the mean in V's place; a NaN mean is coloured as a NaN V is.
 *   fold       field-wise: sum, count and nans add, lo is the least of the los, hi the greatest of the his.  All are associative and
 *              commutative: every cut (slices, calls, slabs, feeds, chunk sizes) gives the same bytes, and a coarser column is exactly
 *              the fold of the finer ones it covers -- any zoom from one streamed pass, as for the kept peaks.
 * For k == 1: hi == lo == x bit for bit for a non-NaN x, sum == q(x) and count == 1.  The image is in general NOT the frame render's byte
 * for byte: the mean is the quantised value.
 * The mean is a mean of displayed (dB-axis) values, hence the geometric mean of the magnitudes: it is defined on what every render writes
 * and what the colour map takes.  A power-domain mean needs magnitudes from before the dB map: that is the power overview below, which
 * reduces K_A's mapped magnitudes.  (Percentiles and the median were out of scope here: they are "The percentile overview" below.)
 * The calls follow their peak-hold twins argument for argument: float *d_peaks becomes sgz_overview_stat_record *d_stats, and every call
 * has one more optional output, the means float [columns][pairs][P] -- value planes as V is (sgz_stage_track_peaks_values takes them).
 * Of image, records and means at least one must be non-NULL.  The carry is sgz_overview_stat_record [pairs][P].
 *  sgz_stage_overview_stats   refusals, slices (0, 1 .. 64, identical bits), asynchrony and "only the documented bytes are written" as for
 *                      sgz_stage_overview.
 *  sgz_spectrogram_overview_stats_device / _host   as sgz_spectrogram_overview_device / _host: slabs with the decay state and the open
 *                      column carried, bytes independent of SGZ_OPT_OVERVIEW_SLAB, RSNT plans in one slab; carry and partial scratch of
 *                      their own in the plan.
 *  sgz_stage_overview_stats_view / sgz_overview_stats_view_host   any range [x0, x1) of kept records [n][pairs][P] at any width, in the
 *                      plan's colours, by the boundary rule of sgz_overview_view_columns: the image, the folded records and the means.
 *                      Outputs that overlap the source range are refused.  The counts of a folded column are the caller's to keep below
 *                      2^32 (they are not checked on the device; sgz_overview_stats_fold checks them).
 *  sgz_overview_stats_fold    host, no GPU: columns [x0, x1) of in [n][width] (width = pairs * P records per column) into cols =
 *                      min(out_columns, x1 - x0) columns of out by the same boundary rule.  SGZ_EINVAL, nothing written: a null argument,
 *                      width == 0, what sgz_overview_view_columns refuses, a folded count or nans above 2^32 - 1.
 *  sgz_overview_stats_readout host, no GPU: `count` records into the float planes mean, lo and hi by the definition; any of the three may
 *                      be NULL, not all.
 *  sgz_pcm_stream_feed_overview_stats / sgz_spectrogram_overview_stats_pcm   the overview inside sgz_pcm_stream with this reduction:
 *                      the concatenated columns of all feeds equal sgz_spectrogram_overview_stats_host of the converted planar floats,
 *                      byte for byte, however the stream is cut.  An open column is of one kind: a peak-hold feed while a stats column is
 *                      open, and the reverse, is refused with SGZ_EINVAL, consumes nothing and says so in sgz_last_error.
 *                      sgz_pcm_stream_columns_for and sgz_pcm_stream_open_frames serve both kinds; sgz_pcm_stream_reset drops the open
 *                      column; sgz_pcm_stream_feed stays refused while any column is open.  An armed lane runs in a stats feed exactly as
 *                      in a peak-hold feed (the track lane searches every slab's line results). */
typedef struct sgz_overview_stat_record {
    int64_t sum;        /* the sum of q over the column's non-NaN frames                              */
    uint32_t count;     /* non-NaN frames                                                            */
    uint32_t nans;      /* NaN frames                                                                */
    float lo, hi;       /* the least / the greatest non-NaN value; both 0x7FC00000 when count == 0   */
} sgz_overview_stat_record;                /* 24 bytes, 8-aligned */
#ifdef __cplusplus
static_assert(sizeof(sgz_overview_stat_record) == 24 && alignof(sgz_overview_stat_record) == 8, "sgz_overview_stat_record: 24 bytes, 8-aligned");
static_assert(offsetof(sgz_overview_stat_record, sum) == 0 && offsetof(sgz_overview_stat_record, count) == 8 && offsetof(sgz_overview_stat_record, nans) == 12 &&
              offsetof(sgz_overview_stat_record, lo) == 16 && offsetof(sgz_overview_stat_record, hi) == 20, "sgz_overview_stat_record: offsets");
#endif
sgz_status sgz_stage_overview_stats(sgz_plan *plan, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                    sgz_overview_stat_record *d_carry, uint8_t *d_rgba, sgz_overview_stat_record *d_stats, float *d_means, void *stream);
sgz_status sgz_spectrogram_overview_stats_device(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, uint32_t k,
                                                 uint8_t *d_rgba, sgz_overview_stat_record *d_stats, float *d_means, float *d_state, void *stream);
sgz_status sgz_spectrogram_overview_stats_host(sgz_plan *plan, const float *const *planar, uint32_t num_channels, size_t nsamples, uint32_t k,
                                               uint8_t *rgba_out, sgz_overview_stat_record *stats_out, float *means_out, sgz_timing *timing);
sgz_status sgz_stage_overview_stats_view(sgz_plan *plan, const sgz_overview_stat_record *d_stats, size_t n, size_t x0, size_t x1, uint32_t out_columns,
                                         uint32_t slices, uint8_t *d_rgba, sgz_overview_stat_record *d_stats_out, float *d_means, void *stream);
sgz_status sgz_overview_stats_view_host(sgz_plan *plan, const sgz_overview_stat_record *stats, size_t n, size_t x0, size_t x1, uint32_t out_columns,
                                        uint8_t *rgba_out, sgz_overview_stat_record *stats_out, float *means_out, sgz_timing *timing);
sgz_status sgz_overview_stats_fold(const sgz_overview_stat_record *in, size_t n, size_t width, size_t x0, size_t x1, uint32_t out_columns,
                                   sgz_overview_stat_record *out);
sgz_status sgz_overview_stats_readout(const sgz_overview_stat_record *in, size_t count, float *mean, float *lo, float *hi);
sgz_status sgz_pcm_stream_feed_overview_stats(sgz_pcm_stream *s, const void *pcm /*HOST*/, size_t nsamples, uint32_t k, int flush, uint8_t *rgba_out /*or NULL*/,
                                              sgz_overview_stat_record *stats_out /*or NULL*/, float *means_out /*or NULL*/, uint64_t capacity_columns,
                                              uint64_t *columns_out, sgz_pcm_timing *timing);
sgz_status sgz_spectrogram_overview_stats_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                              const uint32_t *channel_map, size_t nsamples, uint32_t k, uint8_t *rgba_out,
                                              sgz_overview_stat_record *stats_out, float *means_out, sgz_pcm_timing *timing);

/* The percentile overview: how a pixel's level is distributed over the k frames of a column -- the noise floor per frequency (the 10 %
 * level), the median spectrum, which is robust against the bursts that saturate a peak hold, and the "95 % ceiling".  No associative fold
 * of bounded size gives an order statistic exactly; a histogram over fixed buckets is such a fold, exact at the bucket's resolution, and
 * every cut gives the same bytes (the histogram lane's answer for samples, applied to the spectrum).
 * Definition (exact, no tolerance).  L[f][p][g][i], F and k as in the overview render; columns and their frames are counted exactly as
 * there (sgz_overview_step).  Let x = L[f][p][0][i].x, the mean overview's input.
 *   bucket     of a non-NaN x, SGZ_OVERVIEW_PCT_BUCKETS = 66 of them: bucket 0 takes x < 0 (-inf and the clip value included), bucket 65
 *              takes x >= 1 (+inf included), otherwise the bucket is 1 + floor(64 x).  64 x and the floor are exact in fp32: there is no
 *              rounding to argue about.  -0 lies in bucket 1; a value exactly on an edge j/64 lies in the upper bucket.  A bucket is 1/64
 *              of the displayed dB axis -- 1.875 dB at a 120 dB range -- and gets finer as the user narrows the range.
 *   record     per (column, pair, pixel) one sgz_overview_pct_record: bucket[b] = the frames whose x lies in bucket b; nans = the NaN
 *              frames; reserved = 0.  count is the sum of the buckets.
 *   fold       every word adds.  The fold is associative and commutative: every cut (slices, calls, slabs, feeds, chunk sizes) gives
 *              the same bytes, and a coarser column is exactly the fold of the finer ones it covers.
 *   quantile   q in [0, 1] of a record.  count == 0: the bits 0x7FC00000.  Otherwise r = the least integer >= q count, clamped to
 *              [1, count] (the product is one fp64 multiply: sgz_hist_percentile's rule); b = the least bucket whose cumulative count is
 *              >= r; before = the cumulative count below b.  The value is -2^-6 for b == 0, 1.0f for b == 65, and otherwise
 *              (float)(((double)(b - 1) + ((double)(r - before) - 0.5) / (double)bucket[b]) * 2^-6), every conversion and the division
 *              rounded to nearest even, nothing contracted.
 *              Consequence: for a record whose non-NaN values all lie in [0, 1) the value is within 1/64 of the exact order statistic
 *              sorted(x)[r - 1] (both lie in bucket b).  For any input the value is monotone in q.
 *   pixel      the additive blend of the pairs' colours at quantile 0's value (q[0]), p = 0 .. pairs - 1 in order, from a black column
 *              buffer, then the 8-bit conversion -- the mean overview's pixel with that value in the mean's place.
 * The calls mirror the mean overview's argument for argument: sgz_overview_stat_record becomes sgz_overview_pct_record, float *d_means
 * becomes float *d_values [nq][columns][pairs][P] -- each plane a value plane that sgz_stage_track_peaks_values takes and
 * sgz_overview_view_host colours --, and every call gains const double *q, uint32_t nq behind its last scalar argument: q is a HOST pointer
 * to nq = 1 .. SGZ_OVERVIEW_PCT_MAX_QUANTILES quantiles, each in [0, 1] and not a NaN, else SGZ_EINVAL.  The quantiles travel by value in
 * the launch arguments: the stage call stays asynchronous and q may be reused at once.  Of image, records and values at least one must be
 * non-NULL.  DEVICE pointers to records (d_carry, d_records) are 16-byte aligned; anything else is refused with SGZ_EINVAL.  The carry is
 * sgz_overview_pct_record [pairs][P].
 *  sgz_stage_overview_pct   refusals, slices (0, 1 .. 64, identical bytes), asynchrony and "only the documented bytes are written" as for
 *                      sgz_stage_overview_stats; `columns` of d_values' layout is the columns this call closes.  With slices == 0 the
 *                      library chooses the form: slices only where one launch would leave compute units idle, none shorter than 64 frames
 *                      (a partial record, written and read, costs 68 row loads), and never more than 64 MiB of partial records in plan
 *                      scratch.  An explicit slices takes slices x columns x pairs x P x 272 bytes.
 *  sgz_spectrogram_overview_pct_device / _host   as sgz_spectrogram_overview_stats_device / _host: slabs with the decay state and the open
 *                      column carried, bytes independent of SGZ_OPT_OVERVIEW_SLAB, RSNT plans in one slab; carry and partial scratch of
 *                      their own in the plan.  `columns` of the values' layout is ceil(F / k).
 *  sgz_overview_pct_bucket   host, no GPU: the bucket of x.  SGZ_EINVAL, *b untouched: b NULL, x a NaN.
 *  sgz_overview_pct_fold     host, no GPU: columns [x0, x1) of in [n][width] (width = pairs * P records per column) into cols =
 *                      min(out_columns, x1 - x0) columns of out by the boundary rule of sgz_overview_view_columns.  SGZ_EINVAL, nothing
 *                      written: a null argument, width == 0, what sgz_overview_view_columns refuses, a folded word above 2^32 - 1.  The
 *                      fold plus the readout is the zoom: there is no device view of kept records.
 *  sgz_overview_pct_readout  host, no GPU: `count` records into values [nq][count] by the definition.  SGZ_EINVAL, nothing written: a null
 *                      argument, q or nq as above, a record whose buckets sum above 2^32 - 1.
 *  sgz_pcm_stream_feed_overview_pct / sgz_spectrogram_overview_pct_pcm   the overview inside sgz_pcm_stream with this reduction, a sixth
 *                      kind of open column: the concatenated columns of all feeds equal sgz_spectrogram_overview_pct_host of the converted
 *                      planar floats, byte for byte, however the stream is cut.  In a feed value plane j starts at values_out + j x
 *                      capacity_columns x pairs x P and receives the feed's columns from there; in the one-shot call at j x ceil(F / k) x
 *                      pairs x P.  records_out is a host pointer and needs 4-byte alignment only.  A feed of another kind while a
 *                      percentile column is open, and the reverse, is refused with SGZ_EINVAL, consumes nothing and says so in
 *                      sgz_last_error.  An armed lane runs in a percentile feed exactly as in a stats feed. */
#define SGZ_OVERVIEW_PCT_BUCKETS 66
#define SGZ_OVERVIEW_PCT_MAX_QUANTILES 8
typedef struct sgz_overview_pct_record {
    uint32_t bucket[SGZ_OVERVIEW_PCT_BUCKETS];  /* frames per bucket; count = their sum */
    uint32_t nans;                              /* NaN frames                           */
    uint32_t reserved;                          /* 0                                    */
} sgz_overview_pct_record;                 /* 272 bytes */
#ifdef __cplusplus
static_assert(sizeof(sgz_overview_pct_record) == 272, "sgz_overview_pct_record: 272 bytes");
static_assert(offsetof(sgz_overview_pct_record, bucket) == 0 && offsetof(sgz_overview_pct_record, nans) == 264 &&
              offsetof(sgz_overview_pct_record, reserved) == 268, "sgz_overview_pct_record: offsets");
#endif
sgz_status sgz_stage_overview_pct(sgz_plan *plan, const float *d_lines, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                  const double *q /*HOST*/, uint32_t nq, sgz_overview_pct_record *d_carry, uint8_t *d_rgba,
                                  sgz_overview_pct_record *d_records, float *d_values, void *stream);
sgz_status sgz_spectrogram_overview_pct_device(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, uint32_t k,
                                               const double *q /*HOST*/, uint32_t nq, uint8_t *d_rgba, sgz_overview_pct_record *d_records,
                                               float *d_values, float *d_state, void *stream);
sgz_status sgz_spectrogram_overview_pct_host(sgz_plan *plan, const float *const *planar, uint32_t num_channels, size_t nsamples, uint32_t k,
                                             const double *q, uint32_t nq, uint8_t *rgba_out, sgz_overview_pct_record *records_out,
                                             float *values_out, sgz_timing *timing);
sgz_status sgz_overview_pct_bucket(float x, uint32_t *b);
sgz_status sgz_overview_pct_fold(const sgz_overview_pct_record *in, size_t n, size_t width, size_t x0, size_t x1, uint32_t out_columns,
                                 sgz_overview_pct_record *out);
sgz_status sgz_overview_pct_readout(const sgz_overview_pct_record *records, size_t count, const double *q, uint32_t nq, float *values);
sgz_status sgz_pcm_stream_feed_overview_pct(sgz_pcm_stream *s, const void *pcm /*HOST*/, size_t nsamples, uint32_t k, int flush, const double *q,
                                            uint32_t nq, uint8_t *rgba_out /*or NULL*/, sgz_overview_pct_record *records_out /*or NULL*/,
                                            float *values_out /*or NULL*/, uint64_t capacity_columns, uint64_t *columns_out, sgz_pcm_timing *timing);
sgz_status sgz_spectrogram_overview_pct_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                            const uint32_t *channel_map, size_t nsamples, uint32_t k, const double *q, uint32_t nq,
                                            uint8_t *rgba_out, sgz_overview_pct_record *records_out, float *values_out, sgz_pcm_timing *timing);

/* The power overview: mean-square spectrum of k frames per image column -- the power-domain mean that every analyser calls "average": the
 * long-term average spectrum of a file, and the spectrum of a selection.  The mean overview above averages displayed (dB-axis) values, a
 * geometric mean of the magnitudes, which understates noise-like material by about 2.5 dB and lets one silent frame drag a column down by the
 * whole dB range.  This lane reduces the mapped magnitudes themselves, at the one boundary inside the library where they exist: K_A writes
 * them to device memory before K_B reads them.  It needs no decay state and no K_B launch.
 * Definition (exact, no tolerance).  M[f][p][s][i] are the mapped magnitudes of frame f, pair p, side s < sides, pixel i < P: exactly what
 * sgz_stage_mapped writes, bit for bit, on every path (on channel-split plans the completed values, not sgz_stage_mapped_dominant's).  sides is
 * 2 for Separate / MidSide and 1 otherwise; width = pairs * sides * P records per column.  Columns and their frames are counted by
 * sgz_overview_step, exactly as in the two other overviews.  Let x = M[f][p][s][i].
 *   quantiser  a NaN takes no part in sum, count, lo or hi; it is counted in nans.  Otherwise t = (double)x * (double)x (exact: 48
 *              significant bits);  u = t * 2^60 (exact; +inf stays +inf);  q = 2^64 - 2^11 (the largest double below 2^64) if u >= 2^64 -
 *              2^11;  otherwise q = rint(u) as a uint64.  A tie cannot occur: x^2 2^60 = m^2 2^(2e + 60) has an even exponent.  Range and
 *              resolution: values up to 4 (+12 dB over a full-scale sine), 2^-60 in power (-180 dB).
 *   record     per (column, pair, side, pixel) one sgz_overview_power_record: sum[0], sum[1] = the low and the high word of the 128-bit sum
 *              of q; count = the non-NaN frames; nans = the NaN frames; lo the least and hi the greatest non-NaN x under the overview's
 *              total order (-0 below +0), both 0x7FC00000 when count == 0.  sum < 2^96 for every count below 2^32.
 *   fold       field-wise: the 128-bit sums add, count and nans add, lo is the least of the los, hi the greatest of the his.  All are
 *              associative and commutative: every cut (slices, calls, slabs, feeds, chunk sizes) gives the same bytes, a coarser column
 *              is exactly the fold of the finer ones, and the whole file's average spectrum is the fold of all columns.
 *   readout    count == 0: rms has the bits 0x7FC00000.  Otherwise S = (double)sum[1] * 2^64 + (double)sum[0] (the first term is exact;
 *              the conversion of sum[0] and the addition round to nearest even);  ms = S / (double)count;  rms = (float)(sqrt(ms) *
 *              2^-30).  Division and root are correctly rounded, nothing is contracted.  The mean square as a double is ms * 2^-60.
 *   level      the value K_B writes as a line result for a frame of magnitude rms from a zero decay state: dbMap(slopeMap[i], rms), the
 *              render's own dB map; 0x7FC00000 when count == 0.  Both sides use slopeMap[i].
 *   pixel      the additive blend of the pairs' colours at the level of side 0, p = 0 .. pairs - 1 in order, from a black column buffer,
 *              then the 8-bit conversion -- the overview's pixel with the level in V's place.
 * For k == 1 and 2^-7 <= |x| < 4: rms == |x| bit for bit.  In general the image is NOT the frame render's: there is no decay, and the value
 * is quantised.
 * Argument order follows the mean overview's calls: d_power [columns][pairs][sides][P] records, d_levels the same shape in floats, the carry
 * sgz_overview_power_record [pairs][sides][P].  Of image, records and levels at least one must be non-NULL.
 *  sgz_stage_overview_power   d_mapped float [frames][pairs][sides][P], whatever floats they are.  Refusals (SGZ_EINVAL, nothing launched or
 *                      written), slices (0, 1 .. 64, identical bytes), asynchrony, the carry snapshot and "only the documented bytes are
 *                      written" as for sgz_stage_overview_stats.
 *  sgz_spectrogram_overview_power_device / _host   slabs of frames (SGZ_OPT_OVERVIEW_SLAB, or by default the overview's frame count): per
 *                      slab K_A into plan scratch with its late pixels completed (sgz_stage_mapped's call), then the reduction with the open
 *                      column carried; the bytes do not depend on the slab.  No K_B, no decay state, no d_state argument.  SGZ_CH_PHASE
 *                      (plane 1 is no magnitude) and RSNT plans: SGZ_EUNSUPPORTED before the device is touched.  Fewer samples than a
 *                      window: SGZ_SKIPPED_FRAME, nothing written.
 *  sgz_stage_overview_power_view / sgz_overview_power_view_host   any range [x0, x1) of kept records [n][pairs][sides][P] at any width, in
 *                      the plan's colours, by the boundary rule of sgz_overview_view_columns: the image, the folded records and the levels.
 *                      Outputs that overlap the source range are refused.  The counts of a folded column are the caller's to keep below
 *                      2^32 (sgz_overview_power_fold checks them).
 *  sgz_overview_power_quantise   host, no GPU: q of n floats by the definition (0 for a NaN, which has none).
 *  sgz_overview_power_fold    host, no GPU: columns [x0, x1) of in [n][width] into cols = min(out_columns, x1 - x0) columns of out by the
 *                      same boundary rule.  SGZ_EINVAL, nothing written: a null argument, width == 0, what sgz_overview_view_columns
 *                      refuses, a folded count or nans above 2^32 - 1.
 *  sgz_overview_power_readout host, no GPU: `count` records into the planes mean_square (ms * 2^-60; NaN when count == 0), rms, lo and hi;
 *                      any of the four may be NULL, not all.
 *  sgz_overview_power_levels  host, no GPU: the levels of in [columns][pairs][sides][P] by the plan's host slope table and scalars and
 *                      std::log(float) -- the spectrum of a selection is sgz_overview_power_fold, then this. */
typedef struct sgz_overview_power_record {
    uint64_t sum[2];    /* low word, high word of the 128-bit sum of q over the column's non-NaN frames */
    uint32_t count;     /* non-NaN frames                                                            */
    uint32_t nans;      /* NaN frames                                                                */
    float lo, hi;       /* the least / the greatest non-NaN value; both 0x7FC00000 when count == 0   */
} sgz_overview_power_record;               /* 32 bytes, 8-aligned */
#ifdef __cplusplus
static_assert(sizeof(sgz_overview_power_record) == 32 && alignof(sgz_overview_power_record) == 8, "sgz_overview_power_record: 32 bytes, 8-aligned");
static_assert(offsetof(sgz_overview_power_record, sum) == 0 && offsetof(sgz_overview_power_record, count) == 16 && offsetof(sgz_overview_power_record, nans) == 20 &&
              offsetof(sgz_overview_power_record, lo) == 24 && offsetof(sgz_overview_power_record, hi) == 28, "sgz_overview_power_record: offsets");
#endif
sgz_status sgz_stage_overview_power(sgz_plan *plan, const float *d_mapped, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                    sgz_overview_power_record *d_carry, uint8_t *d_rgba, sgz_overview_power_record *d_power, float *d_levels, void *stream);
sgz_status sgz_spectrogram_overview_power_device(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, uint32_t k,
                                                 uint8_t *d_rgba, sgz_overview_power_record *d_power, float *d_levels, void *stream);
sgz_status sgz_spectrogram_overview_power_host(sgz_plan *plan, const float *const *planar, uint32_t num_channels, size_t nsamples, uint32_t k,
                                               uint8_t *rgba_out, sgz_overview_power_record *power_out, float *levels_out, sgz_timing *timing);
sgz_status sgz_stage_overview_power_view(sgz_plan *plan, const sgz_overview_power_record *d_power, size_t n, size_t x0, size_t x1, uint32_t out_columns,
                                         uint32_t slices, uint8_t *d_rgba, sgz_overview_power_record *d_power_out, float *d_levels, void *stream);
sgz_status sgz_overview_power_view_host(sgz_plan *plan, const sgz_overview_power_record *power, size_t n, size_t x0, size_t x1, uint32_t out_columns,
                                        uint8_t *rgba_out, sgz_overview_power_record *power_out, float *levels_out, sgz_timing *timing);
sgz_status sgz_overview_power_quantise(const float *x, size_t n, uint64_t *q);
sgz_status sgz_overview_power_fold(const sgz_overview_power_record *in, size_t n, size_t width, size_t x0, size_t x1, uint32_t out_columns,
                                   sgz_overview_power_record *out);
sgz_status sgz_overview_power_readout(const sgz_overview_power_record *in, size_t count, double *mean_square, float *rms, float *lo, float *hi);
sgz_status sgz_overview_power_levels(const sgz_plan *plan, const sgz_overview_power_record *in, size_t columns, float *levels);
/*  sgz_pcm_stream_feed_overview_power / sgz_spectrogram_overview_power_pcm   the overview inside sgz_pcm_stream with this reduction: the
 *                      concatenated columns of all feeds equal sgz_spectrogram_overview_power_host of the converted planar floats, byte for
 *                      byte, however the stream is cut.  A power feed neither reads nor advances the stream's decay state: a plain feed
 *                      behind it continues the state of the last feed that rendered.  An open column is of one of three kinds (peak hold,
 *                      mean, power): a feed of another kind while a column is open is refused with SGZ_EINVAL, consumes nothing and names the
 *                      flush call that closes it in sgz_last_error.  sgz_pcm_stream_columns_for, sgz_pcm_stream_open_frames and
 *                      sgz_pcm_stream_reset serve all three kinds.  A power feed with the track lane armed is refused (SGZ_EINVAL): it has
 *                      no line results to search.  The seven column lanes run in it as in any feed.  Phase and RSNT streams:
 *                      SGZ_EUNSUPPORTED. */
sgz_status sgz_pcm_stream_feed_overview_power(sgz_pcm_stream *s, const void *pcm /*HOST*/, size_t nsamples, uint32_t k, int flush, uint8_t *rgba_out /*or NULL*/,
                                              sgz_overview_power_record *power_out /*or NULL*/, float *levels_out /*or NULL*/, uint64_t capacity_columns,
                                              uint64_t *columns_out, sgz_pcm_timing *timing);
sgz_status sgz_spectrogram_overview_power_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                              const uint32_t *channel_map, size_t nsamples, uint32_t k, uint8_t *rgba_out,
                                              sgz_overview_power_record *power_out, float *levels_out, sgz_pcm_timing *timing);

/* The cross overview: band power, coherence and phase per column -- how the two channels of a pair relate per frequency.  The level lane's
 * correlation is one number per column over all frequencies; Phase mode's second plane is a per-frame cancellation value; and the coherence of
 * a single frame is identically 1, so no pass over the other outputs can produce it.  The quantity needed is the averaged cross-spectrum: per
 * column of k frames and per frequency band, the sums of |L|^2, |R|^2, Re(L conj R) and Im(L conj R).  One such record yields the band levels
 * of L, R, Mid and Side (a 1/3-octave analyser of a file or of a selection), the magnitude-squared coherence, the inter-channel phase and the
 * per-band correlation.  It reduces the complex bins at the one place where both channels' exist: what sgz_stage_bins writes on an
 * SGZ_CH_PHASE plan.  There is no image (the reference has no colour rule for coherence) and no device-side view: the host fold is the zoom.
 * Definition (exact, no tolerance).
 *   plan       FFT algorithm, SGZ_CH_PHASE, N = 2^n (n >= 3).  Every other plan: SGZ_EUNSUPPORTED before the device is touched.  B[f][p][j],
 *              j = 0 .. N, is what sgz_stage_bins writes for frame f and pair p, as float2 (re, im).
 *   bins       1 <= k <= N/2 - 2 are admitted; DC, Nyquist and the Q3-halved entry N/2 - 1 are left out.  L = B[k], R = B[N - k].
 *   bands      a band table is bands + 1 uint32 edges with 1 <= edges[0] <= ... <= edges[bands] <= N/2 - 1 and 1 <= bands <= 4096.  Band b
 *              holds the bins edges[b] <= k < edges[b + 1]; an empty band is allowed.  sgz_plan_set_cross_edges sets it on the plan: a host
 *              call that copies to the device and may synchronise.  A table that breaks the rule: SGZ_EINVAL, the old table stays.  Calls on
 *              a plan without a table: SGZ_EINVAL.
 *   quantiser  on one bin of one frame, floats lr, li, rr, ri; the scale is s = 2^(62 - 2n), so that 2^60 is the power of a full-scale sine on
 *              a bin under a rectangular full window.  If any of the four floats is not finite the bin takes no part and is counted in
 *              skipped.  Otherwise, in fp64 with nothing contracted (each product exact, each sum rounded once):
 *              a = lr lr + li li;  b = rr rr + ri ri;  c = lr rr + li ri;  d = li rr - lr ri  -- L conj R, the phase positive where L leads;
 *              u = x s (exact);  q = rint(clamp(u, +-(2^63 - 2^10))), ties to even, as an int64.  q_a and q_b are never negative.
 *              Resolution: 2^-60 in power, -180 dB re a full-scale sine.  Range: 8 in power, +9 dB.
 *   record     one sgz_overview_cross_record per (column, pair, band): ll, rr, re, im the 128-bit sums of q_a, q_b, q_c, q_d, low word then
 *              high word, re and im in two's complement; count the bin-frames summed; skipped the bin-frames left out.  Columns and their
 *              frames are counted by sgz_overview_step, as in the three other overviews.
 *   fold       every field adds (the sums modulo 2^128): associative and commutative.  Slices, calls, slabs, feeds and chunk sizes all
 *              give the same bytes; a coarser column is the fold of the finer ones; a band whose range is the union of adjacent finer
 *              bands is the fold of their records.
 *   readout    host only, fp64, into sgz_overview_cross_reading.  S -> double as in the power overview: hi 2^64 + lo; the signed sums
 *              through their magnitude.  With A, B, C, D the doubles of ll, rr, re, im:  ll = A / count 2^-60, and likewise rr, re, im --
 *              the mean per bin-frame in unit power;  mid = max(0, S_ll + S_rr + 2 S_re) / count 2^-62, the integer sum exact in 128 bits;
 *              side the same with -2 S_re;  coherence = min(1, (C^2 + D^2) / (A B));  phase = atan2(D, C);  correlation = C / sqrt(A B).
 *              count == 0: every plane is NaN.  A B == 0: coherence and correlation are NaN.
 *   unit       sgz_overview_cross_unit returns (invSize N / 2)^2 in fp64 from the plan's host scalars: ll * unit is the mean of
 *              |X invSize|^2, the amplitude scale the render's dB map sees.  A band level is mean * (edges[b + 1] - edges[b]) * unit.
 *  sgz_stage_overview_cross   d_bins float2 [frames][pairs][N + 1], whatever floats they are; d_carry [pairs][bands], d_cross
 *                      [columns][pairs][bands].  Refusals (SGZ_EINVAL, nothing launched or written), slices (0, 1 .. 64, identical bytes),
 *                      asynchrony, the carry snapshot and "only the documented bytes are written" as for sgz_stage_overview_power.
 *  sgz_spectrogram_overview_cross_device / _host   slabs of frames (SGZ_OPT_OVERVIEW_SLAB, or by default as many whole frames as keep the
 *                      slab's bins within 256 MiB of plan scratch): per slab K_A's bins into that scratch (sgz_stage_bins' call), then the
 *                      reduction with the open column carried; the bytes do not depend on the slab.  No K_B, no decay state.  Fewer samples
 *                      than a window: SGZ_SKIPPED_FRAME, nothing written.
 *  sgz_overview_cross_quantise   host, no GPU: `count` bins of a transform of size 2^n -> q [count][4] (a, b, c, d) and skipped [count]
 *                      (1: the bin takes no part, its q are 0).
 *  sgz_overview_cross_fold    host, no GPU: columns [x0, x1) of in [n][pairs][bands] into cols = min(out_columns, x1 - x0) columns of out
 *                      by the boundary rule of sgz_overview_view_columns and, when coarse_edges is not NULL, into coarse_bands bands: every
 *                      coarse edge must be one of the fine `edges`, else SGZ_EINVAL.  out [cols][pairs][coarse_bands or bands].  edges may
 *                      be NULL when coarse_edges is.  SGZ_EINVAL, nothing written: a null argument, what sgz_overview_view_columns refuses,
 *                      a folded count above 2^64 - 1.
 *  sgz_overview_cross_readout host, no GPU: `count` records into `count` readings.
 *  sgz_cross_edges_octave     host, no GPU, all in fp64: the centres f_j = 1000 2^(j / b) for every integer j with f_lo <= f_j <= f_hi,
 *                      b = bands_per_octave in 1 .. 48;  edges[i] = clamp(ceil(f_j 2^(-1 / (2 b)) N / sample_rate), 1, N/2 - 1), the last
 *                      edge from the last centre with 2^(+1 / (2 b)).  *bands = the centres found; SGZ_EINVAL when there is none or
 *                      capacity < *bands + 1.  centres [*bands] may be NULL. */
typedef struct sgz_overview_cross_record {
    uint64_t ll[2], rr[2];  /* the 128-bit sums of q_a and q_b, low word then high word                  */
    uint64_t re[2], im[2];  /* ... of q_c and q_d, two's complement                                      */
    uint64_t count;         /* bin-frames summed                                                         */
    uint64_t skipped;       /* bin-frames left out: one of their four floats was not finite              */
} sgz_overview_cross_record;               /* 80 bytes, 8-aligned */
typedef struct sgz_overview_cross_reading {
    double ll, rr, mid, side, re, im;       /* means per bin-frame in unit power */
    double coherence, phase, correlation;
} sgz_overview_cross_reading;
#ifdef __cplusplus
static_assert(sizeof(sgz_overview_cross_record) == 80 && alignof(sgz_overview_cross_record) == 8, "sgz_overview_cross_record: 80 bytes, 8-aligned");
static_assert(offsetof(sgz_overview_cross_record, ll) == 0 && offsetof(sgz_overview_cross_record, rr) == 16 && offsetof(sgz_overview_cross_record, re) == 32 &&
              offsetof(sgz_overview_cross_record, im) == 48 && offsetof(sgz_overview_cross_record, count) == 64 && offsetof(sgz_overview_cross_record, skipped) == 72,
              "sgz_overview_cross_record: offsets");
static_assert(sizeof(sgz_overview_cross_reading) == 72, "sgz_overview_cross_reading: nine doubles");
#endif
sgz_status sgz_plan_set_cross_edges(sgz_plan *plan, const uint32_t *edges /*HOST [bands + 1]*/, uint32_t bands);
sgz_status sgz_stage_overview_cross(sgz_plan *plan, const float *d_bins, size_t frames, uint32_t k, uint32_t held, int flush, uint32_t slices,
                                    sgz_overview_cross_record *d_carry, sgz_overview_cross_record *d_cross, void *stream);
sgz_status sgz_spectrogram_overview_cross_device(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, uint32_t k,
                                                 sgz_overview_cross_record *d_cross, void *stream);
sgz_status sgz_spectrogram_overview_cross_host(sgz_plan *plan, const float *const *planar, uint32_t num_channels, size_t nsamples, uint32_t k,
                                               sgz_overview_cross_record *cross_out, sgz_timing *timing);
sgz_status sgz_overview_cross_quantise(uint32_t n, const float *lr, const float *li, const float *rr, const float *ri, size_t count,
                                       int64_t *q /*[count][4]*/, uint8_t *skipped /*[count]*/);
sgz_status sgz_overview_cross_fold(const sgz_overview_cross_record *in, size_t n, size_t pairs, const uint32_t *edges /*or NULL*/, uint32_t bands,
                                   size_t x0, size_t x1, uint32_t out_columns, const uint32_t *coarse_edges /*or NULL*/, uint32_t coarse_bands,
                                   sgz_overview_cross_record *out);
sgz_status sgz_overview_cross_readout(const sgz_overview_cross_record *in, size_t count, sgz_overview_cross_reading *out);
sgz_status sgz_overview_cross_unit(const sgz_plan *plan, double *unit);
sgz_status sgz_cross_edges_octave(double sample_rate, uint32_t N, uint32_t bands_per_octave, double f_lo, double f_hi, uint32_t *edges,
                                  uint32_t capacity, uint32_t *bands, double *centres /*or NULL*/);
/*  sgz_pcm_stream_set_cross_edges / sgz_pcm_stream_feed_overview_cross / sgz_spectrogram_overview_cross_pcm   the overview inside
 *                      sgz_pcm_stream with this reduction: the concatenated columns of all feeds equal sgz_spectrogram_overview_cross_host of
 *                      the converted planar floats, byte for byte, however the stream is cut.  The band table is set on the stream
 *                      (SGZ_EINVAL while a cross column is open); a cross feed neither reads nor advances the stream's decay state.  An open
 *                      column is of one of four kinds (peak hold, mean, power, cross): a feed of another kind while a column is open is
 *                      refused with SGZ_EINVAL, consumes nothing and names the flush call that closes it in sgz_last_error.
 *                      sgz_pcm_stream_columns_for, sgz_pcm_stream_open_frames and sgz_pcm_stream_reset serve all four kinds.  A cross feed
 *                      with the track lane armed is refused (SGZ_EINVAL): it has no line results to search.  The seven column lanes run in
 *                      it as in any feed.  Streams that are not SGZ_CH_PHASE FFT streams: SGZ_EUNSUPPORTED. */
sgz_status sgz_pcm_stream_set_cross_edges(sgz_pcm_stream *s, const uint32_t *edges /*HOST [bands + 1]*/, uint32_t bands);
sgz_status sgz_pcm_stream_feed_overview_cross(sgz_pcm_stream *s, const void *pcm /*HOST*/, size_t nsamples, uint32_t k, int flush,
                                              sgz_overview_cross_record *cross_out, uint64_t capacity_columns, uint64_t *columns_out,
                                              sgz_pcm_timing *timing);
sgz_status sgz_spectrogram_overview_cross_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                              const uint32_t *channel_map, size_t nsamples, const uint32_t *edges, uint32_t bands, uint32_t k,
                                              sgz_overview_cross_record *cross_out, sgz_pcm_timing *timing);

/* The flux overview: onset strength, centroid and spread of k frames per column -- the two curves a file view draws on top of a spectrogram:
 * a novelty curve with the strongest onset of each column, and a brightness line.  Every other lane and overview reduces one pixel, sample
 * or band over time; this one reduces along the frequency axis and compares a frame with the frame before it, which no host can do from what
 * the other overviews return (they fold frames first).  It reads the mapped magnitudes at the boundary the power overview reads them.
 * Definition (exact, no tolerance).  M[f][p][s][i] are the mapped magnitudes of frame f, pair p, side s < sides, pixel i < P as in the power
 * overview: what sgz_stage_mapped writes, bit for bit (completed values on channel-split plans).  sides is 2 for Separate / MidSide and 1
 * otherwise; width = pairs * sides records per column.  Columns and their frames are counted by sgz_overview_step.
 *   quantiser  a(x) = rint(min((double)|x| * 2^30, 2^34)) as a uint64.  The product is exact; ties go to even; +inf clamps.  A NaN gives 0
 *              and marks its frame.  Resolution 2^-30 in amplitude; the clamp is at |x| = 16.
 *   per frame and (pair, side)   A = sum_i a_i;  M1 = sum_i i a_i;  M2 = sum_i i^2 a_i;  F = sum_i max(0, a_i(f) - a_i(f - 1)) with integer
 *              subtraction (the half-wave rectified L1 flux), F = 0 for a frame without a predecessor.  The predecessor is the previous
 *              frame of the same (pair, side), whatever column it fell in.  With P <= 2^20: F < 2^54 and M2 < 2^94 per frame, and every
 *              sum stays below 2^128 over 2^32 frames.
 *   record     per (column, pair, side) one sgz_overview_flux_record: amp, mom1, mom2, flux = the low and the high word of the 128-bit sums
 *              of A, M1, M2 and F over the column's frames; flux_max the greatest F of the column; flux_at the absolute index of the first
 *              frame that attains it (UINT64_MAX when count == 0); count the frames; nans the frames with at least one NaN pixel.
 *   fold       field-wise: sums and counts add; of (flux_max, flux_at) the greater flux_max wins, at equal flux_max the smaller flux_at.
 *              All of it is associative and commutative: every cut (runs, slices, calls, slabs, feeds) gives the same bytes, and a coarser
 *              column is exactly the fold of the finer ones.
 *   readout    host, fp64, nothing contracted, in this order.  A 128-bit sum s becomes S(s) = (double)s[1] * 2^64 + (double)s[0] (the power
 *              overview's rule).  mean amplitude = S(amp) / ((double)count * (double)P) * 2^-30;  centroid c = S(mom1) / S(amp), in pixels;
 *              spread = sqrt(max(0, S(mom2) / S(amp) - c * c));  mean flux = S(flux) / (double)count * 2^-30;  relative flux = S(flux) /
 *              S(amp).  NaN: the mean amplitude and the mean flux when count == 0; the centroid, the spread and the relative flux when amp
 *              == 0 (which count == 0 implies).
 * There is no image and no device-side view: the host fold is the zoom, as in the cross overview.
 *  sgz_stage_overview_flux   d_mapped float [frames][pairs][sides][P], whatever floats they are; first_frame the absolute index of its frame
 *                      0.  d_prev float [pairs][sides][P] holds the frame before d_mapped[0]: NULL -- the first frame has no predecessor;
 *                      otherwise the call reads it and then overwrites it with its own last frame (frames > 0), so that calls chain through
 *                      it as they chain through d_carry, one sgz_overview_flux_record [pairs][sides].  A call may read and write the same
 *                      buffers (the carry-snapshot rule of the other stage calls); d_prev must not overlap d_mapped.  d_flux [columns][pairs]
 *                      [sides] receives the columns that close.  Refusals (SGZ_EINVAL, nothing launched or written): what
 *                      sgz_overview_step refuses, slices above 64, a NULL d_flux when a column closes, a NULL d_carry that would be read
 *                      or written, d_mapped / d_prev not 4-byte or d_carry / d_flux not 8-byte aligned.  slices (0: automatic, 1 .. 64:
 *                      identical bytes), asynchrony and "only the documented bytes are written" as for sgz_stage_overview_power.
 *  sgz_spectrogram_overview_flux_device / _host   slabs of frames (SGZ_OPT_OVERVIEW_SLAB, or by default the overview's frame count): per
 *                      slab K_A into plan scratch (sgz_stage_mapped's call), then the reduction, with the open column and the previous
 *                      frame carried in plan scratch; the bytes do not depend on the slab.  Frames count from 0.  No K_B, no decay state.
 *                      SGZ_CH_PHASE and RSNT plans: SGZ_EUNSUPPORTED before the device is touched.  Fewer samples than a window:
 *                      SGZ_SKIPPED_FRAME, nothing written.
 *  sgz_overview_flux_quantise   host, no GPU: a of n floats by the definition (0 for a NaN).
 *  sgz_overview_flux_fold     host, no GPU: columns [x0, x1) of in [n][width] into cols = min(out_columns, x1 - x0) columns of out by the
 *                      boundary rule of sgz_overview_view_columns.  SGZ_EINVAL, nothing written: a null argument, width == 0, what
 *                      sgz_overview_view_columns refuses, a folded count or nans above 2^32 - 1.
 *  sgz_overview_flux_readout  host, no GPU: `count` records of rows of `pixels` pixels into the five planes of the readout; any may be NULL,
 *                      not all; pixels >= 1 where the mean amplitude is wanted.
 *  sgz_overview_flux_hz       host, no GPU: n fractional pixels (a centroid) into Hz by linear interpolation of
 *                      sgz_plan_get_mapped_frequencies in fp64: with i = floor(x), hz = f[i] + (x - i) * (f[i + 1] - f[i]); x <= 0 gives
 *                      f[0], x >= P - 1 gives f[P - 1], a NaN stays a NaN. */
typedef struct sgz_overview_flux_record {
    uint64_t amp[2];    /* low word, high word of the 128-bit sum of A over the column's frames   */
    uint64_t mom1[2];   /* ... of M1 = sum_i i a_i                                                */
    uint64_t mom2[2];   /* ... of M2 = sum_i i^2 a_i                                              */
    uint64_t flux[2];   /* ... of F                                                               */
    uint64_t flux_max;  /* the greatest F of the column                                           */
    uint64_t flux_at;   /* absolute index of the first frame that attains it; UINT64_MAX: none    */
    uint32_t count;     /* frames                                                                 */
    uint32_t nans;      /* frames with at least one NaN pixel                                     */
} sgz_overview_flux_record;                /* 88 bytes, 8-aligned */
#ifdef __cplusplus
static_assert(sizeof(sgz_overview_flux_record) == 88 && alignof(sgz_overview_flux_record) == 8, "sgz_overview_flux_record: 88 bytes, 8-aligned");
static_assert(offsetof(sgz_overview_flux_record, amp) == 0 && offsetof(sgz_overview_flux_record, mom1) == 16 && offsetof(sgz_overview_flux_record, mom2) == 32 &&
              offsetof(sgz_overview_flux_record, flux) == 48 && offsetof(sgz_overview_flux_record, flux_max) == 64 && offsetof(sgz_overview_flux_record, flux_at) == 72 &&
              offsetof(sgz_overview_flux_record, count) == 80 && offsetof(sgz_overview_flux_record, nans) == 84, "sgz_overview_flux_record: offsets");
#endif
sgz_status sgz_stage_overview_flux(sgz_plan *plan, const float *d_mapped, size_t frames, uint32_t k, uint32_t held, int flush, uint64_t first_frame,
                                   uint32_t slices, float *d_prev /*or NULL*/, sgz_overview_flux_record *d_carry, sgz_overview_flux_record *d_flux, void *stream);
sgz_status sgz_spectrogram_overview_flux_device(sgz_plan *plan, const float *d_planar, size_t channel_stride, size_t nsamples, uint32_t k,
                                                sgz_overview_flux_record *d_flux, void *stream);
sgz_status sgz_spectrogram_overview_flux_host(sgz_plan *plan, const float *const *planar, uint32_t num_channels, size_t nsamples, uint32_t k,
                                              sgz_overview_flux_record *flux_out, sgz_timing *timing);
sgz_status sgz_overview_flux_quantise(const float *x, size_t n, uint64_t *a);
sgz_status sgz_overview_flux_fold(const sgz_overview_flux_record *in, size_t n, size_t width, size_t x0, size_t x1, uint32_t out_columns,
                                  sgz_overview_flux_record *out);
sgz_status sgz_overview_flux_readout(const sgz_overview_flux_record *in, size_t count, uint32_t pixels, double *mean_amplitude, double *centroid,
                                     double *spread, double *mean_flux, double *relative_flux);
sgz_status sgz_overview_flux_hz(const sgz_plan *plan, const double *pixel, size_t n, double *hz);
/*  sgz_pcm_stream_feed_overview_flux / sgz_spectrogram_overview_flux_pcm   the overview inside sgz_pcm_stream with this reduction: the
 *                      concatenated columns of all feeds equal sgz_spectrogram_overview_flux_host of the converted planar floats, byte for
 *                      byte, however the stream is cut.  The stream keeps the previous frame across feeds, and flux_at counts every frame
 *                      the stream has completed since it was made or reset, whichever kind of feed consumed it.  After
 *                      sgz_pcm_stream_reset, and after any feed of another kind that consumed frames, the next flux feed starts without a
 *                      predecessor: its first frame has F = 0.  A flux feed neither reads nor advances the stream's decay state.  An open
 *                      column is of one of five kinds (peak hold, mean, power, cross, flux): a feed of another kind while a column is open
 *                      is refused with SGZ_EINVAL, consumes nothing and names the flush call that closes it in sgz_last_error.
 *                      sgz_pcm_stream_columns_for, sgz_pcm_stream_open_frames and sgz_pcm_stream_reset serve all five kinds.  A flux feed
 *                      with the track lane armed is refused (SGZ_EINVAL): it has no line results to search.  The seven column lanes run in
 *                      it as in any feed.  Phase and RSNT streams: SGZ_EUNSUPPORTED. */
sgz_status sgz_pcm_stream_feed_overview_flux(sgz_pcm_stream *s, const void *pcm /*HOST*/, size_t nsamples, uint32_t k, int flush,
                                             sgz_overview_flux_record *flux_out, uint64_t capacity_columns, uint64_t *columns_out,
                                             sgz_pcm_timing *timing);
sgz_status sgz_spectrogram_overview_flux_pcm(const sgz_spectrum_config *cfg, const void *pcm, uint32_t format, uint32_t src_channels,
                                             const uint32_t *channel_map, size_t nsamples, uint32_t k, sgz_overview_flux_record *flux_out,
                                             sgz_pcm_timing *timing);

/* The waveform lane: a minimum and a maximum per screen column and channel of a file's samples -- what every editor draws beside the
 * spectrogram lane -- reduced on the device from the planar floats the streamed render has there anyway.  The reference has no counterpart
 * (its Oscilloscope draws a live ring, never a file; sgz_scope_dense_* is that ring's reduction).
 * Definition (exact, no tolerance): let x[d][i] be the fp32 samples of channel d < channels, S their count so far and m >= 1 the samples per
 * column.  Column c covers samples c m <= i < min((c + 1) m, S); only a flushed last column may be partial.  Wv[c][d] = (lo, hi): lo the
 * least and hi the greatest of the column's non-NaN samples under the overview's total order (above: bits ^ (sign ? 0xFFFFFFFF :
 * 0x80000000) compared as unsigned; NaNs take no part; -0 < +0); a column of NaNs alone gives lo = hi = 0x7FC00000.  The results are the
 * samples' own bits: denormals, +-inf and -0 are kept.  Layout float2 [columns][channels].  Least and greatest under a total order are
 * associative, so any cut of the stream (calls, pieces, feeds) or of a column (lanes, slices) gives the same bits; a coarser column is the
 * fold of the finer ones it covers (lo of the los, hi of the his), which is how a host zooms kept columns out.  The counts are
 * sgz_overview_step's with samples in the place of frames: (m, held, nsamples, flush) -> columns, held_out.
 *  sgz_stage_wave_columns  DEVICE pointers.  d_planar [channels][channel_stride], the first nsamples of each row (any 4-byte-aligned address).
 *                      held: samples of the open column that earlier calls took (< m).  d_carry: DEVICE float2 [channels], the open
 *                      column's (lo, hi) so far -- read iff held > 0, written iff samples stay open afterwards (no flush, (held +
 *                      nsamples) % m != 0), NULL allowed when neither applies; a carried column continues exactly as if its samples had
 *                      come in one call.  d_wave: DEVICE float2 [columns][channels], columns as sgz_overview_step counts them (NULL
 *                      allowed when none closes).  nsamples == 0 with held > 0 and flush: one column from the carry alone.  m up to
 *                      the switch-over (1024; sgz_wave_columns_limits) runs one workgroup per (channel, tile of 4096 / m whole columns);
 *                      longer columns are reduced in slices per column into scratch and folded by a second launch.  slices: 0 = the
 *                      library's choice (m above the switch-over: the fewest slices that give two workgroups per CU), 1 .. 64 forced
 *                      -- 2 and more take the sliced form whatever m is, 1 takes the form m implies -- identical bits.  Only the
 *                      documented bytes are written.  Asynchronous on `stream`, nothing is waited for; scratch is allocated and freed in
 *                      stream order.  SGZ_EINVAL, nothing launched or written: a null d_planar, channels == 0 or > 64, m == 0, held >= m,
 *                      channel_stride < nsamples, slices > 64, a needed d_carry or d_wave that is NULL, d_planar not aligned to 4
 *                      bytes, d_carry or d_wave not aligned to 8.  nsamples == 0 with nothing to flush: SGZ_OK, nothing launched.
 *  sgz_wave_columns_limits  the switch-over and the tile's samples (either result may be NULL).
 * The lane inside the sgz_pcm_stream handle -- above, "interleaved PCM in": while armed, every feed of either kind also reduces the new samples of
 * each piece -- the stream's converted floats, exactly sgz_pcm_to_planar_device's -- on the compute stream behind the conversion, and
 * reads the columns that closed back on the read-back stream into wave_out at a cursor.  The columns of all feeds and the final flush,
 * concatenated, are Wv of the stream's converted floats bit for bit, however it is cut into feeds and pieces and whichever kind the feeds
 * are; the image, lines, overview and peaks of an armed stream are those of an unarmed one byte for byte.
 *  sgz_pcm_stream_set_waveform   between feeds.  m > 0 arms: wave_out HOST float2 [capacity_columns][channels] (channels = 2 num_pairs;
 *                      pinned memory is written in place, pageable memory through a pinned twin per slot), the cursor restarts at 0.
 *                      The same m with another buffer keeps the open column: how a caller with a small buffer drains.  m == 0 disarms
 *                      and drops the open column.  SGZ_EINVAL: a null stream, a null wave_out with capacity_columns > 0, another m
 *                      while samples are open.
 *  sgz_pcm_stream_waveform_for   columns the next feed of nsamples closes (flush != 0: that feed followed by sgz_pcm_stream_flush_waveform);
 *                      0 when disarmed.
 *  sgz_pcm_stream_waveform_state columns written since the lane was armed (the cursor) and the open column's samples; either may be NULL.
 *  sgz_pcm_stream_flush_waveform closes the open column: one launch on the carry, one column read back, waits.  Nothing open: SGZ_OK,
 *                      nothing done.  SGZ_EINVAL: disarmed, no column left in the buffer.
 * A feed that would close more columns than the buffer has left is refused with SGZ_EINVAL before anything is consumed.  reset drops the
 * open column and restarts the cursor.  Per slot the columns of a piece take ceil(chunk_samples / m) + 1 columns of device (and, for a
 * pageable buffer, pinned) memory, made on first need and grown when a later m needs more: memory is bounded by chunk_samples and m. */
sgz_status sgz_stage_wave_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, uint32_t m, uint32_t held,
                                  int flush, uint32_t slices, float *d_carry /*float2 [channels]*/, float *d_wave /*float2 [columns][channels]*/,
                                  void *stream);
void       sgz_wave_columns_limits(uint32_t *switch_over, uint32_t *tile_samples);
sgz_status sgz_pcm_stream_set_waveform(sgz_pcm_stream *s, uint32_t m /*0 = off*/, float *wave_out /*HOST float2 [capacity][channels]*/,
                                       uint64_t capacity_columns);
uint64_t   sgz_pcm_stream_waveform_for(const sgz_pcm_stream *s, size_t nsamples, int flush);
sgz_status sgz_pcm_stream_waveform_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples);
sgz_status sgz_pcm_stream_flush_waveform(sgz_pcm_stream *s);

/* The level lane: exact RMS, DC, "overs" and stereo correlation per screen column and channel pair of a file's samples -- the RMS body an
 * editor draws inside the waveform lane's peak envelope, its DC line, its over marks and its correlation trace -- reduced on the device
 * from the same planar floats.  The reference has no counterpart: its meters are live (the Vectorscope's drawStereoMeters reads one-pole
 * filters, here sgz_vector_meters); nothing of them is reused or contradicted.
 * A floating-point sum has no cut-independent bits; an integer sum has.  Every sample is quantised ONCE to a fixed-point integer and every
 * quantity is a sum of integers.
 * Definition (exact, no tolerance): let x[d][i] be the fp32 samples of channel d (the stream's converted floats, exactly what
 * sgz_pcm_to_planar_device writes), pair p the channels (2p, 2p + 1) = (L, R), S the samples so far and m >= 1 the samples per column.
 * Column c covers samples c m <= i < min((c + 1) m, S), counted exactly as the waveform lane counts them; only a flushed last column may
 * be partial.  The quantiser (a NaN takes no part):
 *     v = (int32) clamp(rintf(x * 2^23), -2^26, +2^26)
 * -- the multiply is exact (a power of two), the rounding is to nearest, ties to even, the lane saturates at +-8.0 (+18 dBFS), +-inf
 * saturate, and denormals quantise to 0 whether or not the device flushes them.  At this scale the quantiser is the identity on 8-, 16-
 * and 24-bit integer PCM: for such files the lane is the file's level exactly.  One sgz_level_record per (column, pair), layout
 * [columns][pairs], 80 bytes, little-endian; arrays of it on the DEVICE are aligned to 16 bytes:
 *     sumsq[ch]  sum of v^2 of channel ch of the pair (0 = L, 1 = R), an unsigned 128-bit integer as (lo, hi)
 *     cross      sum of v_L v_R over the sample frames where neither side is a NaN, 128-bit two's complement as (lo, hi)
 *     sum[ch]    sum of v
 *     count[ch]  the non-NaN samples
 *     overs[ch]  the non-NaN samples with |v| >= 2^23 (at or over full scale)
 * Bounds, with m <= 2^32 - 1: count fits 32 bits, |sum| < 2^58, sumsq and |cross| < 2^84.  A column of NaNs alone is the all-zero record.
 * Integer sums are associative and commutative, so any cut of the stream (feeds, pieces, calls with a carry) or of a column (lanes,
 * slices) gives the same bits, and a coarser column is the field-wise sum of the finer ones it covers: how a host zooms kept records out
 * (sgz_level_fold).  The counts are sgz_overview_step's with samples in the place of frames: (m, held, nsamples, flush) -> columns,
 * held_out.
 *  sgz_stage_level_columns  DEVICE pointers.  d_planar [2 pairs][channel_stride], the first nsamples of each row (any 4-byte-aligned
 *                      address).  held: samples of the open column that earlier calls took (< m).  d_carry: DEVICE sgz_level_record
 *                      [pairs], the open column so far -- read iff held > 0, written iff samples stay open afterwards (no flush,
 *                      (held + nsamples) % m != 0), NULL allowed when neither applies; a carried column continues exactly as if its
 *                      samples had come in one call.  d_level: DEVICE sgz_level_record [columns][pairs], columns as sgz_overview_step
 *                      counts them (NULL allowed when none closes).  nsamples == 0 with held > 0 and flush: one column from the carry
 *                      alone.  m up to the switch-over (1024; sgz_level_columns_limits) runs one workgroup per (pair, tile of 4096 / m
 *                      whole columns of both rows); longer columns are reduced in slices per column into scratch and folded by a
 *                      second launch.  slices: 0 = the library's choice (m above the switch-over: the fewest slices that give two
 *                      workgroups per CU), 1 .. 64 forced -- 2 and more take the sliced form whatever m is, 1 takes the form m
 *                      implies -- identical bits.  Only the documented bytes are written.  Asynchronous on `stream`, nothing is waited
 *                      for; scratch is allocated and freed in stream order.  SGZ_EINVAL, nothing launched or written: a null d_planar,
 *                      pairs == 0 or > 32, m == 0, held >= m, channel_stride < nsamples, slices > 64, a needed d_carry or d_level that
 *                      is NULL, d_planar not aligned to 4 bytes, d_carry or d_level not aligned to 16.  nsamples == 0 with nothing to
 *                      flush: SGZ_OK, nothing launched.
 *  sgz_level_columns_limits  the switch-over and the tile's samples per row (either result may be NULL).
 * The lane inside the sgz_pcm_stream handle -- above, "interleaved PCM in": while armed, every feed of either kind also reduces the new samples of
 * each piece -- the stream's converted floats, exactly sgz_pcm_to_planar_device's -- on the compute stream behind the conversion, and
 * reads the records that closed back on the read-back stream into level_out at a cursor.  The records of all feeds and the final flush,
 * concatenated, are the lane of the stream's converted floats bit for bit, however it is cut into feeds and pieces and whichever kind the
 * feeds are; the image, lines, overview, peaks, waveform columns and track records of an armed stream are those of an unarmed one byte
 * for byte.  The lane's m is its own: the waveform lane may be armed beside it with another.
 *  sgz_pcm_stream_set_level   between feeds.  m > 0 arms: level_out HOST sgz_level_record [capacity_columns][pairs] (aligned to 8 bytes;
 *                      pinned memory is written in place, pageable memory through a pinned twin per slot), the cursor restarts at 0.
 *                      The same m with another buffer keeps the open column: how a caller with a small buffer drains.  m == 0 disarms
 *                      and drops the open column.  SGZ_EINVAL: a null stream, a null level_out with capacity_columns > 0, a level_out
 *                      that is not aligned, another m while samples are open.
 *  sgz_pcm_stream_level_for   columns the next feed of nsamples closes (flush != 0: that feed followed by sgz_pcm_stream_flush_level);
 *                      0 when disarmed.
 *  sgz_pcm_stream_level_state columns written since the lane was armed (the cursor) and the open column's samples; either may be NULL.
 *  sgz_pcm_stream_flush_level closes the open column: one launch on the carry, one column read back, waits.  Nothing open: SGZ_OK,
 *                      nothing done.  SGZ_EINVAL: disarmed, no column left in the buffer.
 * A feed that would close more columns than the buffer has left is refused with SGZ_EINVAL before anything is consumed.  reset drops the
 * open column and restarts the cursor.  Per slot the records of a piece take ceil(chunk_samples / m) + 1 columns of device (and, for a
 * pageable buffer, pinned) memory, made on first need and grown when a later m needs more: memory is bounded by chunk_samples and m.
 * Host arithmetic on HOST records, nothing launched:
 *  sgz_level_fold      the zoom: source columns [x0, x1) of in [n][pairs], w = x1 - x0, into cols = min(out_columns, w) columns of out
 *                      [cols][pairs]; output column b is the field-wise sum of source columns x0 + ceil(b w / cols) <= j < x0 +
 *                      ceil((b + 1) w / cols) -- the boundary rule of the view of kept peaks (sgz_overview_view_columns), so the lanes
 *                      of a file zoom together.  128-bit fields add with carry.  out must not overlap in.  SGZ_EINVAL, nothing
 *                      written: a null argument, pairs == 0, what sgz_overview_view_columns refuses, a folded count above 2^32 - 1.
 *  sgz_level_readout   what a host draws from one record, in fp64: per channel mean square = sumsq / (count 2^46), rms = its square
 *                      root, rms_db = 10 log10(mean square) (-inf for silence, NaN for count 0), dc = sum / (count 2^23) (NaN for
 *                      count 0); correlation = cross / sqrt(sumsq_L sumsq_R), 0 when either is 0.  1.0 is full scale.  A 128-bit value
 *                      becomes a double through its magnitude (a negative cross is negated first: hi 2^64 + lo of -5 would cancel to
 *                      0).  SGZ_EINVAL: a null argument. */
typedef struct sgz_level_record {
    uint64_t sumsq[2][2];   /* [channel of the pair][lo, hi] */
    uint64_t cross[2];      /* lo, hi */
    int64_t  sum[2];
    uint32_t count[2];
    uint32_t overs[2];
} sgz_level_record;         /* 80 bytes */
typedef struct sgz_level_reading {
    double rms[2], rms_db[2], dc[2];
    double correlation;
} sgz_level_reading;
sgz_status sgz_stage_level_columns(const float *d_planar, size_t channel_stride, uint32_t pairs, size_t nsamples, uint32_t m, uint32_t held,
                                   int flush, uint32_t slices, sgz_level_record *d_carry /*[pairs]*/, sgz_level_record *d_level /*[columns][pairs]*/,
                                   void *stream);
void       sgz_level_columns_limits(uint32_t *switch_over, uint32_t *tile_samples);
sgz_status sgz_pcm_stream_set_level(sgz_pcm_stream *s, uint32_t m /*0 = off*/, sgz_level_record *level_out /*HOST [capacity][pairs]*/,
                                    uint64_t capacity_columns);
uint64_t   sgz_pcm_stream_level_for(const sgz_pcm_stream *s, size_t nsamples, int flush);
sgz_status sgz_pcm_stream_level_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples);
sgz_status sgz_pcm_stream_flush_level(sgz_pcm_stream *s);
sgz_status sgz_level_fold(const sgz_level_record *in, size_t n, uint32_t pairs, size_t x0, size_t x1, uint32_t out_columns, sgz_level_record *out);
sgz_status sgz_level_readout(const sgz_level_record *rec, sgz_level_reading *out);

/* The true-peak lane: the peak of the 4x oversampled signal per screen column and channel of a file's samples -- the inter-sample peak a
 * mastering tool shows beside the level: the level lane's `overs` see only samples at or over full scale, and a sine at fs/4 sampled at
 * 45 degrees has sample peaks of 0.707 A and a true peak of A.  The reference has no counterpart: its meters are live one-pole filters
 * (here sgz_vector_meters); nothing of them is reused or contradicted.  The filter is NOT ITU-R BS.1770's printed coefficient table; it is
 * a filter of the same structure -- 4x oversampling, 48 taps, 12 per phase -- with the taps below.  Loudness weighting (K-filtering) is not
 * part of the lane: an IIR recurrence in fp32 has no cut-independent bits.  A polyphase FIR on quantised integers has: it is a sum of
 * integer products, exact in any order.
 * Definition (exact, no tolerance): let x[d][i] be the fp32 samples of channel d (the stream's converted floats, exactly what
 * sgz_pcm_to_planar_device writes), i counting the samples of the whole stream since the lane was armed or reset, S the samples so far
 * and m >= 1 the samples per column.  The quantiser is the level lane's,
 *     v = (int32) clamp(rintf(x * 2^23), -2^26, +2^26)
 * but a NaN gives v = 0 here: it enters the filter as silence, and it is not counted in `count`.  v[k] = 0 for k < 0.  The taps: T = 12
 * per phase, 4 phases, scale 2^20, c[q][j] = rint(2^20 L(j - 6 + q / 4)) with L(t) = sinc(t) sinc(t / 6) for |t| < 6 (Lanczos, a = 6).
 * This table is normative (sgz_truepeak_taps copies it):
 *     q = 0:  c[0][6] = 1048576, all other taps 0           (the delayed sample itself)
 *     q = 1:  -1780  12162  -29613  59093  -116769  306657  941356  -175616  82260  -42310  19798  -6258
 *     q = 2:  -5454  22259  -50264  98518  -200334  659945  659945  -200334  98518  -50264  22259  -5454
 *     q = 3:  c[3][j] = c[1][11 - j]
 * The sums of |c| per phase are 1048576, 1793672, 2073548 and 1793672, hence |y| <= 2^26 * 2073548 < 2^47: every partial sum is exact in
 * int64 (and in fp64).  The output:
 *     y[i][q] = sum over j = 0 .. 11 of c[q][j] v[i - j]
 * The filter is causal: y[i][.] estimates the signal around sample i - 6 and belongs to the column of sample i, so a peak shows up to 6
 * samples late -- which is what keeps the column counts those of every other lane.  Column c covers samples c m <= i < min((c + 1) m, S),
 * counted by sgz_overview_step with samples in the place of frames; only a flushed last column may be partial.  A flush closes the open
 * column as it stands: the 11 outputs of the filter's tail are not produced (a host that wants them feeds 11 zeros), and the history is
 * kept across a flush, because the stream may go on.  One sgz_truepeak_record per (column, channel), layout [columns][channels], 16
 * bytes, little-endian; arrays on the DEVICE are aligned to 16 bytes:
 *     peak    the greatest |y[i][q]| over the column's samples i and q = 0 .. 3; 2^43 is full scale; 0 for an empty column
 *     count   the column's non-NaN samples
 *     overs   the column's samples i with |y[i][q]| >= 2^43 for some q
 * Maximum and integer sum are associative and commutative, so any cut of the stream or of a column gives the same bytes, and a coarser
 * column is the fold of the finer ones: max of peak, sums of count and overs (sgz_truepeak_fold).  What a cut of the stream carries is
 * one 64-byte sgz_truepeak_carry per channel, aligned to 16: the open column so far, the last 11 quantised samples (oldest first), and a
 * reserved word written as 0.
 *  sgz_stage_truepeak_columns  DEVICE pointers; sgz_stage_level_columns' semantics in every point not named here.  d_planar [channels]
 *                      [channel_stride], the first nsamples of each row (any 4-byte-aligned address).  held: samples of the open
 *                      column that earlier calls took (< m).  continued == 0: the stream begins with this call, the history is zeros,
 *                      held must be 0.  continued != 0: d_carry[].hist holds the 11 samples before this call's first, d_carry[].open
 *                      is read iff held > 0.  d_carry: DEVICE sgz_truepeak_carry [channels], needed (not NULL) whenever continued != 0
 *                      or nsamples > 0.  After a call with nsamples > 0 all 64 bytes of every channel's carry are written: hist is the
 *                      last 11 of (the old history followed by the new samples) -- a call of fewer than 11 samples shifts it --,
 *                      open is the open column where samples stay open (no flush, (held + nsamples) % m != 0) and all zero
 *                      otherwise, reserved is 0.  The call reads a snapshot of the carry it was given, so no workgroup reads what
 *                      another one of the same launch writes.  nsamples == 0 with held > 0 and flush: one column from the carry
 *                      alone, the carry untouched.  d_peaks: DEVICE sgz_truepeak_record [columns][channels], columns as
 *                      sgz_overview_step counts them (NULL allowed when none closes).  m up to the switch-over (1024;
 *                      sgz_truepeak_columns_limits) runs one workgroup per (channel, tile of 4096 / m whole columns); longer columns
 *                      are reduced in slices per column into scratch and folded by a second launch; every tile and slice fetches its
 *                      own 11-sample halo.  slices: 0 = the library's choice, 1 .. 64 forced -- 2 and more take the sliced form
 *                      whatever m is, 1 takes the form m implies -- identical bits.  Only the documented bytes are written.
 *                      Asynchronous on `stream`, nothing is waited for; scratch is allocated and freed in stream order.  SGZ_EINVAL,
 *                      nothing launched or written: a null d_planar, channels == 0 or > 64, m == 0, held >= m, continued == 0 with
 *                      held > 0, channel_stride < nsamples, slices > 64, a needed d_carry or d_peaks that is NULL, d_planar not
 *                      aligned to 4 bytes, d_carry or d_peaks not aligned to 16.  nsamples == 0 with nothing to flush: SGZ_OK,
 *                      nothing launched.
 *  sgz_truepeak_columns_limits  the switch-over and the tile's samples (either result may be NULL).
 *  sgz_truepeak_taps   copies the table, c[q][j] at taps[q][j].
 * The lane inside the sgz_pcm_stream handle -- above, "interleaved PCM in": while armed, every feed of either kind also runs the
 * reduction on the new samples of each piece on the compute stream behind the conversion (and behind the other lanes' launches), and
 * reads the records that closed back on the read-back stream into `out` at a cursor.  The records of all feeds and the final flush,
 * concatenated, are the definition applied to the stream's converted floats, byte for byte, however the stream is cut into feeds and
 * pieces and whichever kind the feeds are; everything else an armed stream returns equals an unarmed stream's, byte for byte.  The
 * lane's m is its own.
 *  sgz_pcm_stream_set_truepeak   between feeds.  m > 0 arms: out HOST sgz_truepeak_record [capacity_columns][channels] (aligned to 8
 *                      bytes; pinned memory is written in place, pageable memory through a pinned twin per slot), the cursor
 *                      restarts at 0 and the lane starts at the next sample with a zero history.  The same m with another buffer
 *                      keeps the open column and the history: how a caller with a small buffer drains.  m == 0 disarms and drops
 *                      both.  SGZ_EINVAL: a null stream, a null out with capacity_columns > 0, an out that is not aligned, another m
 *                      while samples are open.
 *  sgz_pcm_stream_truepeak_for   columns the next feed of nsamples closes (flush != 0: that feed followed by
 *                      sgz_pcm_stream_flush_truepeak); 0 when disarmed.
 *  sgz_pcm_stream_truepeak_state columns written since the lane was armed (the cursor) and the open column's samples; either may be
 *                      NULL.
 *  sgz_pcm_stream_flush_truepeak closes the open column: one launch on the carry, one column read back, waits; the history is kept.
 *                      Nothing open: SGZ_OK, nothing done.  SGZ_EINVAL: disarmed, no column left in the buffer.
 * A feed that would close more columns than the buffer has left is refused with SGZ_EINVAL before anything is consumed.  reset drops
 * the open column, zeroes the history and restarts the cursor.  The carry is kept twice and alternated: a piece reads one and writes
 * the other.  Memory per slot as the level lane's, 16 bytes a record.
 * Host arithmetic on HOST records, nothing launched:
 *  sgz_truepeak_fold   the zoom, with sgz_level_fold's boundary rule: output column b is the fold of source columns x0 + ceil(b w /
 *                      cols) <= j < x0 + ceil((b + 1) w / cols), w = x1 - x0, cols = min(out_columns, w).  out must not overlap in.
 *                      SGZ_EINVAL, nothing written: a null argument, channels == 0, what sgz_overview_view_columns refuses, a folded
 *                      count or overs above 2^32 - 1.
 *  sgz_truepeak_readout  *peak = rec->peak / 2^43 (1.0 is full scale) and *dbtp = 20 log10(peak), -inf for 0, in fp64; either result
 *                      may be NULL.  SGZ_EINVAL: a null rec. */
typedef struct sgz_truepeak_record {
    uint64_t peak;    /* max over the column's samples i and q = 0..3 of |y[i][q]|; 2^43 is full scale; 0 for an empty column */
    uint32_t count;   /* the column's non-NaN samples */
    uint32_t overs;   /* the column's samples i with |y[i][q]| >= 2^43 for some q */
} sgz_truepeak_record;         /* 16 bytes */
typedef struct sgz_truepeak_carry {
    sgz_truepeak_record open;      /* the open column so far */
    int32_t             hist[11];  /* the last 11 quantised samples before the next one, oldest first */
    uint32_t            reserved;  /* written as 0 */
} sgz_truepeak_carry;          /* 64 bytes */
sgz_status sgz_stage_truepeak_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, uint32_t m, uint32_t held,
                                      int flush, uint32_t continued, uint32_t slices, sgz_truepeak_carry *d_carry /*[channels]*/,
                                      sgz_truepeak_record *d_peaks /*[columns][channels]*/, void *stream);
void       sgz_truepeak_columns_limits(uint32_t *switch_over, uint32_t *tile_samples);
void       sgz_truepeak_taps(int32_t taps[4][12]);
sgz_status sgz_truepeak_fold(const sgz_truepeak_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns,
                             sgz_truepeak_record *out);
sgz_status sgz_truepeak_readout(const sgz_truepeak_record *rec, double *peak /*1.0 = full scale*/, double *dbtp);
sgz_status sgz_pcm_stream_set_truepeak(sgz_pcm_stream *s, uint32_t m /*0 = off*/, sgz_truepeak_record *out /*HOST [capacity][channels]*/,
                                       uint64_t capacity_columns);
uint64_t   sgz_pcm_stream_truepeak_for(const sgz_pcm_stream *s, size_t nsamples, int flush);
sgz_status sgz_pcm_stream_truepeak_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples);
sgz_status sgz_pcm_stream_flush_truepeak(sgz_pcm_stream *s);

/* The loudness lane: K-weighted energy per screen column and channel of a file's samples -- what momentary, short-term and integrated
 * loudness after ITU-R BS.1770 / EBU R 128 are read from.  The reference has no counterpart.  An IIR recurrence in fp32 has no
 * cut-independent bits; this formulation has: the sample axis is cut into short segments on an absolute grid, the filter's state at the
 * start of every segment is an exact integer FIR over the last W quantised samples (64-bit, order-free), and the fp64 recurrence runs only
 * over the segment's L samples, in an order fixed here.  Every output then depends on nothing but the samples.
 * Definition (exact, no tolerance).
 *  Filter     sgz_loudness_filter: two biquads as doubles, b[2][3] and a[2][2] with a0 = 1, stage 0 the shelf and stage 1 the RLB
 *             high-pass; W, the memory in samples, and L, the segment length: powers of two, 16 <= L <= W <= 65536.  The coefficients are
 *             inputs; nothing is derived from a sample rate inside the definition.
 *  Quantiser  the true-peak lane's: v = (int32) clamp(rintf(x * 2^23), -2^26, +2^26), a NaN gives v = 0 and is not counted; v[k] = 0 for
 *             k < 0; i counts the samples since the lane was armed or reset.
 *  Step       transposed direct form II in fp64; every *, + and - is one IEEE operation rounded to nearest even, in this order, with no
 *             contraction:
 *                 y = b00*x + s1;   s1 = (b01*x - a00*y) + s2;   s2 = b02*x - a01*y;
 *                 z = b10*y + t1;   t1 = (b11*y - a10*z) + t2;   t2 = b12*y - a11*z;
 *             state (s1, s2, t1, t2), output z.
 *  Tap table  S = 32.  The step run from rest on x = 1, 0, 0, ..; h[c][k], c = 0 .. 3, k = 0 .. W - 1, is state component c after k + 1
 *             steps; C[c][k] = (int32) rint(2^32 h[c][k]).  The filter is accepted only if every C fits int32 and
 *             2^26 max_c sum_k |C[c][k]| < 2^62 (sgz_loudness_taps; SGZ_EINVAL otherwise).
 *  Segment    segment j covers samples j L <= i < (j + 1) L.  Its start state is
 *                 state_c = (double)(int64) (sum over k = 0 .. W - 1 of C[c][k] v[j L - 1 - k]) * 2^-32
 *             -- an exact 64-bit integer in any order, one conversion rounded to nearest even, an exact scale.
 *  Output     z[i] is the step's output when the segment is run from that state over x = (double) v[j L], .., (double) v[i];
 *             q[i] = (int64) rint(z[i]), ties to even, clamped to +-(2^31 - 1).
 *  Record     one sgz_loudness_record per (column, channel), 32 bytes, layout [columns][channels], little-endian, arrays on the DEVICE
 *             aligned to 16: sumsq = the sum of q^2 over the column as an unsigned 128-bit integer (low word first), count = the column's
 *             non-NaN samples, three reserved words written as 0.  Columns of m samples are counted exactly as the true-peak lane counts
 *             them (sgz_overview_step with samples in the place of frames; only a flushed last column may be partial).  A flush does not
 *             move the segment grid.
 * Integer sums make a coarser column the field-wise sum of the finer ones (sgz_loudness_fold) and any cut of the stream or of a column
 * gives the same bytes.  Readout: mean square = sumsq / count / 2^46 (1.0 = a full-scale square wave), loudness = -0.691 + 10 log10 of the
 * sum over channels of G_c ms_c.  Measured against the unsegmented fp64 recurrence the definition differs by less than 1e-4 dB in any
 * 100 ms block (tests/test_loudness_host.py).
 * What a cut of the stream carries, per channel: the open column's record, the last W + L - 1 quantised samples and a zero word --
 * 32 + 4 (W + L) bytes, [channels] of them, aligned to 16; the call re-runs the open segment from its start out of that history without
 * counting those samples again.  The carry is opaque but for its size (sgz_loudness_columns_limits).
 *  sgz_stage_loudness_columns  DEVICE pointers; sgz_stage_truepeak_columns' semantics and refusals in every point not named here.  filter:
 *                      HOST; its tap table is built and uploaded at the filter's first use on a device (the one blocking step) and kept.
 *                      first_index: the absolute index i of the call's first sample; only first_index % L matters.  continued == 0: the
 *                      samples before this call are zeros, held must be 0.  d_carry: needed whenever continued != 0 or nsamples > 0; after
 *                      a call with nsamples > 0 all of it is written (the open column or zeros, the history, the zero word).  The call
 *                      reads a snapshot of the carry it was given.  nsamples == 0 with held > 0 and flush: one column from the carry
 *                      alone, the carry untouched.  The launches: one workgroup per (tile of max(4096, L) samples on the segment grid,
 *                      channel) stages the tile behind its W-sample halo in LDS, forms the segment starts with 32 x 32 -> 64-bit integer
 *                      multiply-adds, runs one lane per segment and stores q as int32 to stream-ordered scratch; a second launch writes
 *                      the history; the column sums follow in the level lane's structure (m up to the switch-over, 1024, in tiles; longer
 *                      columns in slices and a folding launch).  slices: 0 = the library's choice, 1 .. 64 forced, identical bits.
 *                      SGZ_EINVAL, nothing launched or written: what sgz_stage_truepeak_columns refuses, a null or refused filter,
 *                      W > 16384 (the halo and a tile must fit the LDS; the host helpers take every W of the definition), nsamples
 *                      above 2^40, first_index above 2^62.
 *  sgz_loudness_columns_limits  the column sums' switch-over, the run tile's samples and the carry's bytes for `channels` channels (any
 *                      result may be NULL); SGZ_EINVAL where the stage call would refuse the filter or the channel count.
 * The lane inside the sgz_pcm_stream handle: as the true-peak lane, launched behind it.  sgz_pcm_stream_set_loudness(s, filter, m, out,
 * capacity_columns) arms (m > 0; the filter is copied, a refused one is SGZ_EINVAL), keeps the open column and the history where the
 * same m and the same filter come with another buffer (draining), refuses another m or another filter while samples are open, and disarms
 * with m == 0 (filter may be NULL then).  _loudness_for, _loudness_state and _flush_loudness are the true-peak lane's; a flush keeps the
 * history and the sample index, so the segment grid stays where it is.  reset drops the open column, zeroes the history and the index.
 * The carry is kept twice and alternated.  Everything an armed stream returns besides the records equals an unarmed stream's.
 * Host arithmetic, nothing launched:
 *  sgz_loudness_filter_for_rate  48000: ITU-R BS.1770-4's printed coefficients.  Any other rate in 200 .. 819200: the bilinear transform
 *                      of the analogue prototype (shelf 1681.974450955533 Hz, +3.999843853973347 dB, Q 0.7071752369554196; high-pass
 *                      38.13547087602444 Hz, Q 0.5003270373238773).  W = the smallest power of two >= 0.08 rate (at least 256), L = W / 16.
 *                      Not bit-normative (libm decides the last bits off 48000): a caller may pass any coefficients.
 *  sgz_loudness_taps   the normative table, C[c][k] at taps[c * W + k] (4 W words), or SGZ_EINVAL with nothing written.
 *  sgz_loudness_fold   the zoom, with sgz_level_fold's boundary rule; SGZ_EINVAL, nothing written: a null argument, channels == 0, what
 *                      sgz_overview_view_columns refuses, a folded count above 2^32 - 1.
 *  sgz_loudness_readout  reads ncols >= 1 consecutive columns [ncols][channels] together: *mean_square = sum_c G_c ms_c with ms_c the sum
 *                      of the columns' sumsq over the sum of their counts over 2^46 (0 for a channel without samples), *lufs = -0.691 +
 *                      10 log10 of it, -inf when it is 0.  weights: G_c [channels], NULL = all 1.  4 columns of 100 ms are momentary
 *                      loudness, 30 short-term.  Either result may be NULL.
 *  sgz_loudness_integrated  gated loudness of n columns meant to be 100 ms each: blocks of 4 columns with a step of 1; the absolute gate
 *                      at -70, then the relative gate 10 below the loudness of the absolutely gated blocks; -inf when no block passes
 *                      (or n < 4).  Only whole columns take part: the caller leaves a flushed partial last column out of n. */
typedef struct sgz_loudness_filter {
    double   b[2][3];   /* numerators: stage 0 the shelf, stage 1 the high-pass */
    double   a[2][2];   /* denominators a1, a2 of each stage (a0 = 1) */
    uint32_t W;         /* memory in samples, a power of two */
    uint32_t L;         /* segment length, a power of two, 16 <= L <= W <= 65536 */
} sgz_loudness_filter;         /* 88 bytes */
typedef struct sgz_loudness_record {
    uint64_t sumsq[2];     /* the sum of q^2 over the column, unsigned 128-bit, low word first */
    uint32_t count;        /* the column's non-NaN samples */
    uint32_t reserved[3];  /* written as 0 */
} sgz_loudness_record;         /* 32 bytes */
sgz_status sgz_stage_loudness_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples,
                                      const sgz_loudness_filter *filter, uint64_t first_index, uint32_t m, uint32_t held, int flush,
                                      uint32_t continued, uint32_t slices, void *d_carry, sgz_loudness_record *d_records /*[columns][channels]*/,
                                      void *stream);
sgz_status sgz_loudness_columns_limits(const sgz_loudness_filter *filter, uint32_t channels, uint32_t *switch_over, uint32_t *tile_samples,
                                       size_t *carry_bytes);
sgz_status sgz_loudness_filter_for_rate(double rate, sgz_loudness_filter *f);
sgz_status sgz_loudness_taps(const sgz_loudness_filter *f, int32_t *taps /*[4][W]*/);
sgz_status sgz_loudness_fold(const sgz_loudness_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns,
                             sgz_loudness_record *out);
sgz_status sgz_loudness_readout(const sgz_loudness_record *recs, size_t ncols, uint32_t channels, const double *weights /*[channels] or NULL*/,
                                double *lufs, double *mean_square);
sgz_status sgz_loudness_integrated(const sgz_loudness_record *recs, size_t n, uint32_t channels, const double *weights, double *lufs);
sgz_status sgz_pcm_stream_set_loudness(sgz_pcm_stream *s, const sgz_loudness_filter *filter, uint32_t m /*0 = off*/,
                                       sgz_loudness_record *out /*HOST [capacity][channels]*/, uint64_t capacity_columns);
uint64_t   sgz_pcm_stream_loudness_for(const sgz_pcm_stream *s, size_t nsamples, int flush);
sgz_status sgz_pcm_stream_loudness_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples);
sgz_status sgz_pcm_stream_flush_loudness(sgz_pcm_stream *s);

/* The stereo-field lane: a histogram over stereo direction per screen column and channel pair of a file's samples -- where the energy sits
 * between left and right, how wide it is, and whether something lives out of phase: what the Vectorscope's polar plot shows of a live
 * signal, kept per column of a file (the level lane's correlation is one number of it).  The reference has no counterpart: its polar plot
 * is live (drawPolarPlot); nothing of it is reused or contradicted.  The lane takes its geometry from it: direction from (L + R, L - R),
 * radius = max(|L|, |R|), left at negative angles.
 * Definition (exact, no tolerance).  Samples, pairs, columns and counts are the level lane's: x[d][i] are the stream's converted fp32
 * samples, pair p the channels (2p, 2p + 1) = (L, R), column c covers frames c m <= i < min((c + 1) m, S), only a flushed last column may
 * be partial, and the counts are sgz_overview_step's with samples in the place of frames.  The quantiser is the level lane's, unchanged:
 *     v = (int32) clamp(rintf(x * 2^23), -2^26, +2^26)
 * A frame where either side is a NaN is SKIPPED; a frame with vL = vR = 0 is SILENT; every other frame has a direction and a radius.
 * Direction: SGZ_FIELD_SECTORS = 32 sectors on the half circle of directions.  M = vL + vR and X = vR - vL are exact integers with
 * |.| <= 2^27; if M < 0, negate both; theta = atan2(X, M) lies in [-pi/2, pi/2].  Sector b is centred at (b - 16) pi / 32: mono is the
 * centre of sector 16, left-only of sector 8, right-only of sector 24, antiphase (theta = +-pi/2, the same line) of sector 0.  No
 * transcendental takes part: the boundaries are the 32 integer directions (C_k, S_k) = (rint(cos g_k 2^30), rint(sin g_k 2^30)) with
 * g_k = (k - 15.5) pi / 32, n = #{k : C_k X - S_k M >= 0} -- every product is below 2^57, exact in 64 bits -- and the sector is n mod 32.
 * The rounded directions increase strictly in angle, so the true tests form a prefix and a binary search finds n.  This table is
 * normative (sgz_field_boundaries copies it); it is symmetric, C_(31-k) = C_k and S_(31-k) = -S_k:
 *     k =  0: (52686014, -1072448455)     k =  1: (157550647, -1062120190)    k =  2: (260897982, -1041563127)
 *     k =  3: (361732726, -1010975242)    k =  4: (459083786, -970651112)     k =  5: (552013618, -920979082)
 *     k =  6: (639627258, -862437520)     k =  7: (721080937, -795590213)     k =  8: (795590213, -721080937)
 *     k =  9: (862437520, -639627258)     k = 10: (920979082, -552013618)     k = 11: (970651112, -459083786)
 *     k = 12: (1010975242, -361732726)    k = 13: (1041563127, -260897982)    k = 14: (1062120190, -157550647)
 *     k = 15: (1072448455, -52686014)     k = 16: (1072448455, 52686014)      k = 17: (1062120190, 157550647)
 *     k = 18: (1041563127, 260897982)     k = 19: (1010975242, 361732726)     k = 20: (970651112, 459083786)
 *     k = 21: (920979082, 552013618)      k = 22: (862437520, 639627258)      k = 23: (795590213, 721080937)
 *     k = 24: (721080937, 795590213)      k = 25: (639627258, 862437520)      k = 26: (552013618, 920979082)
 *     k = 27: (459083786, 970651112)      k = 28: (361732726, 1010975242)     k = 29: (260897982, 1041563127)
 *     k = 30: (157550647, 1062120190)     k = 31: (52686014, 1072448455)
 * Radius: r = max(|vL|, |vR|) <= 2^26, the reference's `length`.  One sgz_field_record per (column, pair), layout [columns][pairs], 528
 * bytes, little-endian; arrays of it on the DEVICE are aligned to 16 bytes:
 *     radius[b]  sum of r over the sector's frames, < 2^58 with m <= 2^32 - 1
 *     count[b]   the sector's frames
 *     peak[b]    max of r over the sector's frames, 0 when empty
 *     silent     frames with vL = vR = 0
 *     skipped    frames with a NaN on either side
 *     reserved   written as 0
 * A column of NaNs alone has only `skipped` set.  All fields are integer sums and maxima, associative and commutative, so any cut of the
 * stream (feeds, pieces, calls with a carry) or of a column (lanes, slices) gives the same bytes, and a coarser column is the fold of the
 * finer ones -- add, add, max, add, add (sgz_field_fold).
 *  sgz_stage_field_columns  DEVICE pointers; sgz_stage_level_columns' arguments and semantics to the letter, with sgz_field_record in the
 *                      place of sgz_level_record: d_planar [2 pairs][channel_stride] (any 4-byte-aligned address), held, the carry
 *                      d_carry [pairs] (read iff held > 0, written iff samples stay open), d_field [columns][pairs], flush, nsamples ==
 *                      0 with held > 0 and flush: one column from the carry alone.  m up to the switch-over (512;
 *                      sgz_field_columns_limits) runs one workgroup per (pair, tile of 4096 / m whole columns of both rows); longer
 *                      columns are reduced in slices per column into scratch and folded by a second launch.  slices: 0 = the library's
 *                      choice, 1 .. 64 forced -- 2 and more take the sliced form whatever m is, 1 takes the form m implies -- identical
 *                      bytes.  Only the documented bytes are written.  Asynchronous on `stream`, nothing is waited for; scratch is
 *                      allocated and freed in stream order.  SGZ_EINVAL, nothing launched or written: a null d_planar, pairs == 0 or
 *                      > 32, m == 0, held >= m, channel_stride < nsamples, slices > 64, a needed d_carry or d_field that is NULL,
 *                      d_planar not aligned to 4 bytes, d_carry or d_field not aligned to 16.  nsamples == 0 with nothing to flush:
 *                      SGZ_OK, nothing launched.  m = 1 is legal: it writes a 528-byte record per frame.
 *  sgz_field_columns_limits  the switch-over and the tile's sample frames (either result may be NULL).
 *  sgz_field_boundaries  copies the table, (C_k, S_k) at cs[k][0], cs[k][1].
 * The lane inside the sgz_pcm_stream handle -- above, "interleaved PCM in": the level lane's contract word for word, with
 * sgz_field_record in the place of sgz_level_record and one exception.  While armed, every feed of either kind also reduces the new
 * samples of each piece on the compute stream behind the conversion (and behind the other lanes' launches) and reads the records that
 * closed back on the read-back stream into field_out at a cursor.  The records of all feeds and the final flush, concatenated, are the
 * lane of the stream's converted floats byte for byte, however it is cut into feeds and pieces and whichever kind the feeds are; the
 * image, lines, overview, peaks and every other lane's records of an armed stream are those of an unarmed one byte for byte.  The lane's
 * m is its own.  The exception: the stream refuses 0 < m < 64 with SGZ_EINVAL -- a 528-byte record per pair for fewer than 64 frames would
 * read back more than the samples it describes (the stage call takes every m >= 1).
 *  sgz_pcm_stream_set_field   between feeds.  m >= 64 arms: field_out HOST sgz_field_record [capacity_columns][pairs] (aligned to 8
 *                      bytes; pinned memory is written in place, pageable memory through a pinned twin per slot), the cursor restarts
 *                      at 0.  The same m with another buffer keeps the open column: how a caller with a small buffer drains.  m == 0
 *                      disarms and drops the open column.  SGZ_EINVAL: a null stream, 0 < m < 64, a null field_out with
 *                      capacity_columns > 0, a field_out that is not aligned, another m while samples are open.
 *  sgz_pcm_stream_field_for   columns the next feed of nsamples closes (flush != 0: that feed followed by sgz_pcm_stream_flush_field);
 *                      0 when disarmed.
 *  sgz_pcm_stream_field_state columns written since the lane was armed (the cursor) and the open column's samples; either may be NULL.
 *  sgz_pcm_stream_flush_field closes the open column: one launch on the carry, one column read back, waits.  Nothing open: SGZ_OK,
 *                      nothing done.  SGZ_EINVAL: disarmed, no column left in the buffer.
 * A feed that would close more columns than the buffer has left is refused with SGZ_EINVAL before anything is consumed.  reset drops the
 * open column and restarts the cursor.  Memory per slot as the level lane's, 528 bytes a record.
 * Host arithmetic on HOST records, nothing launched:
 *  sgz_field_fold      the zoom, with sgz_level_fold's boundary rule: output column b is the fold of source columns x0 + ceil(b w /
 *                      cols) <= j < x0 + ceil((b + 1) w / cols), w = x1 - x0, cols = min(out_columns, w): radius and count add, peak
 *                      is the maximum, silent and skipped add, reserved is 0.  out must not overlap in.  SGZ_EINVAL, nothing written:
 *                      a null argument, pairs == 0, what sgz_overview_view_columns refuses, a folded count, silent or skipped above
 *                      2^32 - 1.
 *  sgz_field_readout   what a host draws from one record, in fp64: share[b] = count[b] / sum of count (0 when that is 0); mean[b] =
 *                      radius[b] / (count[b] 2^23), 0 when empty; peak[b] = peak[b] / 2^23 (1.0 is full scale).  With w_b =
 *                      radius[b] and theta_b = (b - 16) pi / 32: direction = atan2(sum w_b sin 2 theta_b, sum w_b cos 2 theta_b) / 2
 *                      in radians, negative = left; spread = 1 - hypot(the two sums) / sum w_b, 0 for a point source and towards 1 for
 *                      a diffuse field; both NaN where sum w_b = 0.  silent_share = silent / (sum of count + silent), 0 when that is
 *                      0.  SGZ_EINVAL: a null argument. */
#define SGZ_FIELD_SECTORS 32
typedef struct sgz_field_record {
    uint64_t radius[SGZ_FIELD_SECTORS];   /* sum of r over the sector's frames, < 2^58 */
    uint32_t count[SGZ_FIELD_SECTORS];    /* the sector's frames */
    uint32_t peak[SGZ_FIELD_SECTORS];     /* max r over the sector's frames, 0 when empty */
    uint32_t silent;                      /* frames with vL = vR = 0 */
    uint32_t skipped;                     /* frames with a NaN on either side */
    uint64_t reserved;                    /* written as 0 */
} sgz_field_record;         /* 528 bytes */
typedef struct sgz_field_reading {
    double share[SGZ_FIELD_SECTORS], mean[SGZ_FIELD_SECTORS], peak[SGZ_FIELD_SECTORS];
    double direction, spread, silent_share;
} sgz_field_reading;
sgz_status sgz_stage_field_columns(const float *d_planar, size_t channel_stride, uint32_t pairs, size_t nsamples, uint32_t m, uint32_t held,
                                   int flush, uint32_t slices, sgz_field_record *d_carry /*[pairs]*/, sgz_field_record *d_field /*[columns][pairs]*/,
                                   void *stream);
void       sgz_field_columns_limits(uint32_t *switch_over, uint32_t *tile_samples);
void       sgz_field_boundaries(int32_t cs[32][2]);
sgz_status sgz_pcm_stream_set_field(sgz_pcm_stream *s, uint32_t m /*0 = off*/, sgz_field_record *field_out /*HOST [capacity][pairs]*/,
                                    uint64_t capacity_columns);
uint64_t   sgz_pcm_stream_field_for(const sgz_pcm_stream *s, size_t nsamples, int flush);
sgz_status sgz_pcm_stream_field_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples);
sgz_status sgz_pcm_stream_flush_field(sgz_pcm_stream *s);
sgz_status sgz_field_fold(const sgz_field_record *in, size_t n, uint32_t pairs, size_t x0, size_t x1, uint32_t out_columns, sgz_field_record *out);
sgz_status sgz_field_readout(const sgz_field_record *rec, sgz_field_reading *out);

/* The band lane: three-band energy per screen column and channel of a file's samples -- the frequency colouring the Oscilloscope draws a
 * waveform with (StreamState::audioProcessing: a 3-band Linkwitz-Riley split, band energies, RGB), kept per column of a file beside the
 * waveform lane's envelope.  The live handle restates the network in fp32 sample by sample (scopeIngestKernel phase F); an fp32 or fp64
 * recurrence over a file has no cut-independent bits, so this lane takes the loudness lane's formulation with another filter: segments on
 * an absolute grid, every segment's start state an exact integer FIR, the fp64 recurrence only inside a segment in an order fixed here.
 * Definition (exact, no tolerance).
 *  Filter     sgz_band_filter: four section types as doubles, c[4][5] = {b0, b1, b2, a1, a2} (a0 = 1) of lp1, hp1, lp2, hp2; W, the memory
 *             in samples, and L, the segment length: powers of two, 16 <= L <= W <= 65536.  168 bytes.  The coefficients are inputs;
 *             nothing is derived from a sample rate inside the definition.
 *  Quantiser  and sample index: as the loudness lane, word for word -- v = (int32) clamp(rintf(x * 2^23), -2^26, +2^26), a NaN gives
 *             v = 0 and is not counted; v[k] = 0 for k < 0; i counts the samples since the lane was armed or reset.
 *  Section    transposed direct form II in fp64; every *, + and - is one IEEE operation rounded to nearest even, in this order, with no
 *             contraction, on a section's coefficients c and its state (z0, z1):
 *                 y = c0*x + z0;   z0 = (c1*x - c3*y) + z1;   z1 = c2*x - c4*y
 *  Tree       eight sections in the order lp1a, lp1b, hp1a, hp1b, lp2a, lp2b, hp2a, hp2b (the a and b of a type share its coefficients):
 *                 low = lp1b(lp1a(x));   rest = hp1b(hp1a(x));   mid = lp2b(lp2a(rest));   high = hp2b(hp2a(rest))
 *             The state has 16 components, section s owning components 2 s and 2 s + 1: the live scope's order.
 *  Tap table  S = 30 (the loudness lane's 32 would not hold the Oscilloscope's own filter: at 22050 Hz one state component of its
 *             impulse response reaches 0.5475).  The tree run from rest on x = 1, 0, 0, ..; h[c][k], c = 0 .. 15, k = 0 .. W - 1, is state
 *             component c after k + 1 steps; C[c][k] = (int32) rint(2^30 h[c][k]).  The filter is accepted only if every C fits int32
 *             and 2^26 max_c sum_k |C[c][k]| < 2^62 (sgz_band_taps; SGZ_EINVAL otherwise).
 *  Segment    segment j covers samples j L <= i < (j + 1) L.  Its start state is
 *                 state_c = (double)(int64) (sum over k = 0 .. W - 1 of C[c][k] v[j L - 1 - k]) * 2^-30
 *             -- an exact 64-bit integer in any order, one conversion rounded to nearest even, an exact scale.
 *  Output     z_b[i], b = low, mid, high, are the tree's outputs when the segment is run from that state over x = (double) v[j L], ..,
 *             (double) v[i]; q_b[i] = (int64) rint(z_b[i]), ties to even, clamped to +-(2^31 - 1).
 *  Record     one sgz_band_record per (column, channel), 64 bytes, layout [columns][channels], little-endian, arrays on the DEVICE
 *             aligned to 16: sumsq[b] = the sum of q_b^2 over the column as an unsigned 128-bit integer (low word first) for b = low,
 *             mid, high; count = the column's non-NaN samples; three reserved words written as 0.  Columns, a flush and a partial last
 *             column are the loudness lane's.  A flush does not move the segment grid.
 * Integer sums make a coarser column the field-wise sum of the finer ones (sgz_band_fold) and any cut of the stream or of a column gives
 * the same bytes.  Readout: mean square of a band = sumsq / count / 2^46 (1.0 = a full-scale square wave).  Measured against the
 * unsegmented fp64 recurrence with the helper's filter at 48000, 44100 and 8000 Hz, q differs by at most 1.55 units of 2^-23 and a
 * 1024-sample column's band energy by at most 8e-5 of the column's total (noise at 1e-4 rms, where rounding q to an integer dominates;
 * 2e-7 or less on louder signals): DESIGN.md section 4; tests/test_band_host.py.
 * What a cut of the stream carries, per channel: the open column's record, the last W + L - 1 quantised samples and a zero word --
 * 64 + 4 (W + L) bytes, [channels] of them, aligned to 16; opaque but for its size (sgz_band_columns_limits).
 *  sgz_stage_band_columns  DEVICE pointers; sgz_stage_loudness_columns' semantics and refusals in every point: filter HOST, its tap table
 *                      built and uploaded at the filter's first use on a device (the one blocking step) and kept; first_index, of which
 *                      only first_index % L matters; continued; d_carry read as a snapshot and written whole by a call with
 *                      nsamples > 0; nsamples == 0 with held > 0 and flush: one column from the carry alone, the carry untouched.  The
 *                      launches: one workgroup per (tile of max(4096, L) samples on the segment grid, channel) stages the tile behind
 *                      its W-sample halo in LDS, forms the 16 start-state dot products of every segment with 32 x 32 -> 64-bit integer
 *                      multiply-adds, runs the tree's three independent chains of every segment in fp64 and stores the three q as int32
 *                      planes to stream-ordered scratch; a second launch writes the history; the column sums follow in the loudness
 *                      lane's structure, one pass over a column reading all three planes (m up to the switch-over, 1024, in tiles;
 *                      longer columns in slices and a folding launch).  slices: 0 = the library's choice, 1 .. 64 forced, identical
 *                      bytes.  SGZ_EINVAL, nothing launched or written: what sgz_stage_loudness_columns refuses -- a null or refused
 *                      filter, W > 16384 (the host helpers take every W of the definition), nsamples above 2^40, first_index above
 *                      2^62 among it.
 *  sgz_band_columns_limits  the column sums' switch-over, the run tile's samples and the carry's bytes for `channels` channels (any result
 *                      may be NULL); SGZ_EINVAL where the stage call would refuse the filter or the channel count.
 * The lane inside the sgz_pcm_stream handle: as the loudness lane to the letter -- arm, drain, refuse, disarm, flush and reset -- launched,
 * refused, reserved and read back behind every other lane, with one exception: the stream refuses 0 < m < 64 with SGZ_EINVAL, as the
 * stereo-field lane does (a 64-byte record per channel for fewer samples would read back more than the samples it describes; the stage
 * call takes every m >= 1).  Everything an armed stream returns besides the records equals an unarmed stream's.
 * Host arithmetic, nothing launched, strict fp:
 *  sgz_band_filter_for_rate  the Oscilloscope's design (tuneCrossOver; 300 and 3000 Hz there): fn = (double)(float)(hz / rate), w0 = 2 pi
 *                      fn, alpha = sin w0 / sqrt 2, a0 = 1 + alpha; low-pass b = ((1 - cos w0) / 2, 1 - cos w0, (1 - cos w0) / 2) / a0,
 *                      high-pass b = ((1 + cos w0) / 2, -(1 + cos w0), (1 + cos w0) / 2) / a0, a1 = -2 cos w0 / a0, a2 = (1 - alpha) / a0;
 *                      each coefficient rounded to float and widened, so the sections are the live scope's.  W = the smallest power of
 *                      two >= 6 rate / low_hz (at least 256), L = W / 16: with 300 / 3000 at 8 .. 384 kHz, 20 / 200 and 2000 / 20000 every
 *                      impulse response is below 2^-33 at W and every table is accepted.  SGZ_EINVAL: a null f, a rate that is not
 *                      positive and finite, low_hz <= 0, high_hz <= low_hz, high_hz >= rate / 2, a W above 65536.  Not bit-normative
 *                      (libm decides the last bits): a caller may pass any coefficients.
 *  sgz_band_taps       the normative table, C[c][k] at taps[c * W + k] (16 W words), or SGZ_EINVAL with nothing written.
 *  sgz_band_fold       the zoom, with sgz_loudness_fold's rules and refusals.
 *  sgz_band_readout    reads ncols >= 1 consecutive columns [ncols][channels] of channel `channel` together: mean_square[b] = the sum
 *                      of the columns' sumsq[b] over the sum of their counts over 2^46 (0 without samples), db[b] = 10 log10 of it, -inf
 *                      when it is 0.  Either result may be NULL.  SGZ_EINVAL: a null recs, ncols == 0, channel >= channels.
 *  sgz_band_colours    one RGBA8 per column of channel `channel`, the live scope's colour rule applied to the column's mean band
 *                      energies: the column's three mean squares are rounded to float and take the place of the smoothed band states
 *                      in accumulateColour's fp32 arithmetic, in its order -- red, green, blue = sum_b state[b] band_colours[b][rgb];
 *                      255 / max(red, max(blue, green)) times each, truncated to a byte, alpha 255; then each byte a + (key - a) t with
 *                      t = 1 - (float) frequency_colouring_blend, truncated.  A silent column is 255 / 0 * 0, a NaN, which converts to 0
 *                      there: the column is (0, 0, 0, 255) before the lerp.  The scope's one-pole smoothing between columns is host arithmetic
 *                      on the readout and not part of this.  SGZ_EINVAL: a null argument, channel >= channels. */
typedef struct sgz_band_filter {
    double   c[4][5];   /* {b0, b1, b2, a1, a2} of lp1, hp1, lp2, hp2 (a0 = 1) */
    uint32_t W;         /* memory in samples, a power of two */
    uint32_t L;         /* segment length, a power of two, 16 <= L <= W <= 65536 */
} sgz_band_filter;         /* 168 bytes */
typedef struct sgz_band_record {
    uint64_t sumsq[3][2];  /* the sums of q^2 over the column of low, mid, high: unsigned 128-bit, low word first */
    uint32_t count;        /* the column's non-NaN samples */
    uint32_t reserved[3];  /* written as 0 */
} sgz_band_record;         /* 64 bytes */
sgz_status sgz_stage_band_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, const sgz_band_filter *filter,
                                  uint64_t first_index, uint32_t m, uint32_t held, int flush, uint32_t continued, uint32_t slices, void *d_carry,
                                  sgz_band_record *d_records /*[columns][channels]*/, void *stream);
sgz_status sgz_band_columns_limits(const sgz_band_filter *filter, uint32_t channels, uint32_t *switch_over, uint32_t *tile_samples,
                                   size_t *carry_bytes);
sgz_status sgz_band_filter_for_rate(double rate, double low_hz, double high_hz, sgz_band_filter *f);
sgz_status sgz_band_taps(const sgz_band_filter *f, int32_t *taps /*[16][W]*/);
sgz_status sgz_band_fold(const sgz_band_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns, sgz_band_record *out);
sgz_status sgz_band_readout(const sgz_band_record *recs, size_t ncols, uint32_t channels, uint32_t channel, double *mean_square /*[3]*/,
                            double *db /*[3]*/);
sgz_status sgz_band_colours(const sgz_band_record *recs, size_t ncols, uint32_t channels, uint32_t channel, const float band_colours[3][3],
                            const uint8_t key_rgba8[4], double frequency_colouring_blend, uint8_t *out_rgba8 /*[ncols][4]*/);
sgz_status sgz_pcm_stream_set_band(sgz_pcm_stream *s, const sgz_band_filter *filter, uint32_t m /*0 = off*/,
                                   sgz_band_record *out /*HOST [capacity][channels]*/, uint64_t capacity_columns);
uint64_t   sgz_pcm_stream_band_for(const sgz_pcm_stream *s, size_t nsamples, int flush);
sgz_status sgz_pcm_stream_band_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples);
sgz_status sgz_pcm_stream_flush_band(sgz_pcm_stream *s);

/* The histogram lane: how a column's samples are DISTRIBUTED over level, per screen column and channel of a file's samples -- the other
 * lanes keep extremes and sums.  It gives the percentiles of |x| (the median, the 10 % floor, the 95 % ceiling: the noise floor of a take,
 * the dynamic range of a passage) exactly at the resolution of fixed integer buckets, and a bit meter: which bits of the word a file uses
 * (a 16-bit file padded to 24, a stuck bit, a channel with only positive samples, true digital silence).  The reference has no
 * counterpart; nothing of it is reused or contradicted.
 * Definition (exact, no tolerance).  Samples, columns and counts are the level lane's: x[d][i] are the stream's converted fp32 samples of
 * channel d -- the lane is per channel --, column c covers samples c m <= i < min((c + 1) m, S), only a flushed last column may be
 * partial, and the counts are sgz_overview_step's with samples in the place of frames.  The quantiser is the level lane's, unchanged:
 *     v = (int32) clamp(rintf(x * 2^23), -2^26, +2^26)
 * (the identity on 8-, 16- and 24-bit PCM).  A NaN takes no part and is counted in `skipped`.
 * Bucket of a sample: a = |v|, 0 <= a <= 2^26; SGZ_HIST_BUCKETS = 106.  a = 0 is bucket 0.  Otherwise e = floor(log2 a) = 0 .. 26,
 * s = (a >> (e - 2)) & 3 for e >= 2 and (a << (2 - e)) & 3 for e < 2, and the bucket is 1 + 4 e + s: the integers with (4 + s) 2^(e-2) <=
 * a < (5 + s) 2^(e-2), an octave in four linear parts, 1.2 to 1.9 dB wide.  Full scale, 2^23, is the lower edge of bucket 93; 2^26, the
 * saturated value, alone is bucket 105; buckets 2, 3, 4, 6 and 8 hold no integer and stay 0; the reachable buckets tile 1 .. 2^26 without
 * gaps.  Integer arithmetic throughout: a conversion of a to float rounds above 2^24 and misfiles the upper edges there.
 * One sgz_hist_record per (column, channel), layout [columns][channels], 448 bytes = 112 little-endian 32-bit words; arrays of it on the
 * DEVICE are aligned to 16 bytes:
 *     bucket[b]  samples of bucket b                                      fold: add
 *     count      the samples that are no NaN (= the sum of bucket[])            add
 *     skipped    the NaNs                                                       add
 *     negative   samples with v < 0                                             add
 *     peak       max a, 0 when count = 0                                        max
 *     bits_or    OR of (uint32_t) v over the samples counted, 0 when none       or
 *     bits_and   AND of the same, 0xffffffff when none                          and
 * Every fold is associative and commutative, so any cut of the stream (feeds, pieces, calls with a carry) or of a column (lanes, waves,
 * slices) gives the same bytes, and a coarser column is the fold of the finer ones (sgz_hist_fold).  The identity is the record of zeros
 * with bits_and = 0xffffffff -- NOT all-zero: it is what a column of NaNs alone has beside `skipped`.
 *  sgz_stage_hist_columns  DEVICE pointers; sgz_stage_level_columns' arguments, semantics, carry rule and refusals to the letter, with
 *                      1 .. 64 channels in the place of pairs and sgz_hist_record in the place of sgz_level_record: d_planar
 *                      [channels][channel_stride] (any 4-byte-aligned address), held, the carry d_carry [channels] (the open column
 *                      alone; read iff held > 0, written iff samples stay open), d_hist [columns][channels], flush, nsamples == 0 with
 *                      held > 0 and flush: one column from the carry alone.  m up to the switch-over (1024; sgz_hist_columns_limits)
 *                      runs one workgroup per (channel, tile of min(4096 / m, 64) whole columns), a table per column in LDS; longer
 *                      columns are reduced in slices per column into scratch and folded by a second launch.  slices: 0 = the
 *                      library's choice, 1 .. 64 forced -- 2 and more take the sliced form whatever m is, 1 takes the form m implies --
 *                      identical bytes.  Only the documented bytes are written.  Asynchronous on `stream`, nothing is waited for;
 *                      scratch is allocated and freed in stream order.  SGZ_EINVAL, nothing launched or written: a null d_planar,
 *                      channels == 0 or > 64, m == 0, held >= m, channel_stride < nsamples, slices > 64, a needed d_carry or d_hist
 *                      that is NULL, d_planar not aligned to 4 bytes, d_carry or d_hist not aligned to 16.  nsamples == 0 with nothing
 *                      to flush: SGZ_OK, nothing launched.  m = 1 is legal: it writes a 448-byte record per sample.
 *  sgz_hist_columns_limits  the switch-over and the tile's samples (either result may be NULL).
 * The lane inside the sgz_pcm_stream handle -- above, "interleaved PCM in": the level lane's contract word for word, per channel, with
 * sgz_hist_record in the place of sgz_level_record and one exception.  While armed, every feed of either kind also reduces the new samples
 * of each piece on the compute stream behind the conversion (and behind the other lanes' launches) and reads the records that closed back
 * on the read-back stream into hist_out at a cursor.  The records of all feeds and the final flush, concatenated, are the lane of the
 * stream's converted floats byte for byte, however it is cut into feeds and pieces and whichever kind the feeds are; the image, lines,
 * overview, peaks and every other lane's records of an armed stream are those of an unarmed one byte for byte.  The lane's m is its own.
 * The exception: the stream refuses 0 < m < 128 with SGZ_EINVAL -- a 448-byte record per channel for fewer than 112 samples would read
 * back more than the samples it describes (the stage call takes every m >= 1).
 *  sgz_pcm_stream_set_hist    between feeds.  m >= 128 arms: hist_out HOST sgz_hist_record [capacity_columns][channels] (aligned to 4
 *                      bytes; pinned memory is written in place, pageable memory through a pinned twin per slot), the cursor restarts
 *                      at 0.  The same m with another buffer keeps the open column: how a caller with a small buffer drains.  m == 0
 *                      disarms and drops the open column.  SGZ_EINVAL: a null stream, 0 < m < 128, a null hist_out with
 *                      capacity_columns > 0, a hist_out that is not aligned, another m while samples are open.
 *  sgz_pcm_stream_hist_for    columns the next feed of nsamples closes (flush != 0: that feed followed by sgz_pcm_stream_flush_hist);
 *                      0 when disarmed.
 *  sgz_pcm_stream_hist_state  columns written since the lane was armed (the cursor) and the open column's samples; either may be NULL.
 *  sgz_pcm_stream_flush_hist  closes the open column: one launch on the carry, one column read back, waits.  Nothing open: SGZ_OK,
 *                      nothing done.  SGZ_EINVAL: disarmed, no column left in the buffer.
 * A feed that would close more columns than the buffer has left is refused with SGZ_EINVAL before anything is consumed.  reset drops the
 * open column and restarts the cursor.  Memory per slot as the level lane's, 448 bytes a record and channel.
 * Host arithmetic on HOST records, nothing launched:
 *  sgz_hist_edges      the integers of every bucket: lo[b] = ceil((4 + s) 2^(e-2)), hi[b] = ceil((5 + s) 2^(e-2)) - 1 for b = 1 + 4 e + s,
 *                      hi[105] = 2^26, bucket 0 is (0, 0); an empty bucket has lo > hi.  Either array may be NULL.
 *  sgz_hist_fold       the zoom, with sgz_level_fold's boundary rule: output column b is the fold of source columns x0 + ceil(b w /
 *                      cols) <= j < x0 + ceil((b + 1) w / cols), w = x1 - x0, cols = min(out_columns, w), every word by its rule, from
 *                      the identity.  out must not overlap in.  SGZ_EINVAL, nothing written: a null argument, channels == 0, what
 *                      sgz_overview_view_columns refuses, a folded count or skipped above 2^32 - 1.
 *  sgz_hist_percentile the bucket that holds the q-quantile of |v|: r = the least integer >= q count (the product is one fp64
 *                      multiply), clamped to [1, count]; *bucket = the least b with bucket[0] + .. + bucket[b] >= r; *lo, *hi = that
 *                      bucket's edges / 2^23 as doubles (1.0 is full scale; bucket 0 gives 0, 0).  SGZ_EINVAL: a null argument, q
 *                      outside [0, 1] or NaN, count == 0.
 *  sgz_hist_readout    what a host draws from one record, in fp64: zero_share = bucket[0] / count and negative_share = negative /
 *                      count (NaN for count 0); peak = peak / 2^23; peak_db = 20 log10(peak), -inf for a peak of 0, NaN for count 0;
 *                      median_db = the 0.5 percentile's hi in dB, -inf for bucket 0, NaN for count 0; toggling = bits_or & ~bits_and,
 *                      the bits that took both values; effective_bits = max(0, 24 - ctz(bits_or)) for bits_or != 0, else 0: 16-bit
 *                      PCM reads 16, 24-bit PCM up to 24.  SGZ_EINVAL: a null argument. */
#define SGZ_HIST_BUCKETS 106
typedef struct sgz_hist_record {
    uint32_t bucket[SGZ_HIST_BUCKETS];    /* samples per bucket */
    uint32_t count;                       /* the samples that are no NaN */
    uint32_t skipped;                     /* the NaNs */
    uint32_t negative;                    /* samples with v < 0 */
    uint32_t peak;                        /* max |v|, 0 when count = 0 */
    uint32_t bits_or;                     /* OR of (uint32_t) v, 0 when count = 0 */
    uint32_t bits_and;                    /* AND of (uint32_t) v, 0xffffffff when count = 0 */
} sgz_hist_record;          /* 448 bytes */
typedef struct sgz_hist_reading {
    double zero_share, negative_share, peak, peak_db, median_db;
    uint32_t toggling, effective_bits;
} sgz_hist_reading;
sgz_status sgz_stage_hist_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, uint32_t m, uint32_t held,
                                  int flush, uint32_t slices, sgz_hist_record *d_carry /*[channels]*/, sgz_hist_record *d_hist /*[columns][channels]*/,
                                  void *stream);
void       sgz_hist_columns_limits(uint32_t *switch_over, uint32_t *tile_samples);
void       sgz_hist_edges(uint32_t lo[SGZ_HIST_BUCKETS], uint32_t hi[SGZ_HIST_BUCKETS]);
sgz_status sgz_hist_fold(const sgz_hist_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns, sgz_hist_record *out);
sgz_status sgz_hist_percentile(const sgz_hist_record *rec, double q, uint32_t *bucket, double *lo, double *hi);
sgz_status sgz_hist_readout(const sgz_hist_record *rec, sgz_hist_reading *out);
sgz_status sgz_pcm_stream_set_hist(sgz_pcm_stream *s, uint32_t m /*0 = off*/, sgz_hist_record *hist_out /*HOST [capacity][channels]*/,
                                   uint64_t capacity_columns);
uint64_t   sgz_pcm_stream_hist_for(const sgz_pcm_stream *s, size_t nsamples, int flush);
sgz_status sgz_pcm_stream_hist_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples);
sgz_status sgz_pcm_stream_flush_hist(sgz_pcm_stream *s);

/* The run lane: clipped, flat and silent RUNS per screen column and channel of a file's samples -- what a file-QC view needs after level
 * and true peak.  Clipping is consecutive samples on a ceiling, not single samples over it (the level lane's `overs` counts single
 * samples); clipping that was attenuated afterwards sits under every threshold and shows only as flat tops; a dropout or a mute is a run
 * of identical or zero samples (the histogram lane says "23 % of this column is digital zero", not "one hole of 4410 samples starting
 * here").  Every other column lane is a commutative fold; this one is ordered: associative, not commutative.  The reference has no
 * counterpart; nothing of it is reused or contradicted.
 * Definition (exact, no tolerance).  Per channel, x[i] are the stream's converted fp32 samples, exactly what sgz_pcm_to_planar_device
 * writes, i counting the lane's samples since it was armed or reset, S the samples so far and m >= 1 the samples per column.  The
 * quantiser is the level lane's,
 *     v = (int32) clamp(rintf(x * 2^23), -2^26, +2^26)
 * and a NaN is INVALID: it has no v.  The thresholds are a sgz_run_params { hot, quiet }, valid when 1 <= hot <= 2^26 and quiet < hot;
 * sgz_run_params_default gives hot = 2^23 - 2^8 -- the positive full scale of 16-bit PCM, so a clipped 16-bit file trips it on both
 * rails -- and quiet = 0.  Three predicates, indices SGZ_RUN_HOT = 0, SGZ_RUN_QUIET = 1, SGZ_RUN_FLAT = 2:
 *     P_hot(i)   = valid(i) and |v[i]| >= hot
 *     P_quiet(i) = valid(i) and |v[i]| <= quiet
 *     P_flat(i)  = i >= 1 and valid(i) and valid(i - 1) and v[i] = v[i - 1]          (a flat run of length r is r + 1 equal samples)
 * and two derived terms:
 *     cross(i)   = i >= 1 and valid(i) and valid(i - 1) and (v[i] < 0) != (v[i - 1] < 0)       (zero counts as non-negative)
 *     start_k(i) = P_k(i) and not (i >= 1 and P_k(i - 1))
 * Column c covers samples c m <= i < min((c + 1) m, S), counted by sgz_overview_step with samples in the place of frames; only a flushed
 * last column may be partial.  A flush does not move i and does not drop the history: the first sample after a flush still relates to the
 * one before it.  One sgz_run_record per (column, channel), layout [columns][channels], 96 bytes = 24 little-endian 32-bit words; arrays
 * of it on the DEVICE are aligned to 16 bytes.  For the column [a, b):
 *     word 0          len          b - a, NaNs included
 *     word 1          skipped      the invalid samples
 *     word 2          crossings    the sum of cross(i)
 *     word 3          reserved0    0
 *     words 4 + 6 k.. of[k]        count, runs, longest, at, head, tail of predicate k:
 *         count       the sum of P_k(i)
 *         runs        the sum of start_k(i): the runs that BEGIN in the column
 *         longest     the greatest r such that r consecutive samples inside the column all have P_k (runs are clipped to the column)
 *         at          the least offset from a at which such a stretch of `longest` samples starts; 0 when longest = 0
 *         head, tail  the consecutive samples with P_k at the column's start / end; both equal len when every sample has P_k
 *     words 22, 23    reserved     0
 * A column of no samples is the all-zero record, the identity.  The fold of A followed by B: len, skipped, crossings, count and runs
 * add; head = (A.head == A.len) ? A.len + B.head : A.head; tail = (B.tail == B.len) ? B.len + A.tail : B.tail; longest is the greatest of
 * three candidates, (A.longest at A.at), (A.tail + B.head at A.len - A.tail) and (B.longest at A.len + B.at), and `at` the least position
 * among the candidates that attain it, 0 when longest is 0.  The fold is associative, so any cut of the stream (feeds, pieces, calls with
 * a carry) or of a column (lanes, waves, tiles, slices) gives the same bytes as long as the parts are folded IN ORDER, and a coarser
 * column is the fold of the finer ones in order (sgz_run_fold).  What a cut of the stream carries is one 112-byte sgz_run_carry per
 * channel, aligned to 16: the open column so far, prev[0] = v[i - 1] and prev[1] = v[i - 2] (SGZ_RUN_NAN = INT32_MIN stands for an invalid
 * sample or for none: "no sample before" and "a NaN before" are the same thing under the definition; v[i - 2] is needed because
 * start_flat(i) asks for P_flat(i - 1)), and two reserved words written as 0.
 *  sgz_stage_run_columns  DEVICE pointers; sgz_stage_truepeak_columns' arguments, semantics, carry rule, snapshot rule and refusals to the
 *                      letter, with 1 .. 64 channels, a two-sample history in the place of eleven, and `params` in the place the
 *                      loudness call has its filter: a NULL or invalid params is SGZ_EINVAL with nothing launched.  continued == 0: the
 *                      stream begins with this call, the history is two marks, held must be 0 -- exactly a carry whose prev are marks.
 *                      After a call with nsamples > 0 all 112 bytes of every channel's carry are written: prev is the last two of (the
 *                      old history followed by the new samples), open is the open column where samples stay open and all zero
 *                      otherwise, reserved is 0.  nsamples == 0 with held > 0 and flush: one column from the carry alone, the carry
 *                      untouched.  d_runs: DEVICE sgz_run_record [columns][channels] (NULL allowed when none closes).  m up to the
 *                      switch-over (1024; sgz_run_columns_limits) runs one workgroup per (channel, tile of 4096 / m whole columns)
 *                      behind a two-sample halo; longer columns are reduced in slices per column into scratch, each slice fetching its
 *                      own halo, and folded in order by a second launch.  slices: 0 = the library's choice, 1 .. 64 forced -- 2 and more
 *                      take the sliced form whatever m is, 1 takes the form m implies -- identical bytes.  Only the documented bytes are
 *                      written.  Asynchronous on `stream`, nothing is waited for; scratch is allocated and freed in stream order.
 *  sgz_run_columns_limits  the switch-over and the tile's samples (either result may be NULL).
 *  sgz_run_params_default  fills the defaults (NULL: nothing).
 * The lane inside the sgz_pcm_stream handle -- above, "interleaved PCM in": the true-peak lane's contract word for word, with
 * sgz_run_record in the place of sgz_truepeak_record, the thresholds handled as sgz_pcm_stream_set_loudness handles its filter, and one
 * exception: the stream refuses 0 < m < 32 with SGZ_EINVAL -- 96 bytes per 32 samples keeps the records under the samples' size (the
 * stage call takes every m >= 1).  The records of all feeds and the final flush, concatenated, are the definition applied to the stream's
 * converted floats, byte for byte, however the stream is cut into feeds and pieces and whichever kind the feeds are; everything else an
 * armed stream returns equals an unarmed stream's, byte for byte.  The lane's m is its own.
 *  sgz_pcm_stream_set_run   between feeds.  m >= 32 arms: out HOST sgz_run_record [capacity_columns][channels] (aligned to 4 bytes; pinned
 *                      memory is written in place, pageable memory through a pinned twin per slot), the cursor restarts at 0 and the
 *                      lane starts at the next sample, i = 0, with a history of marks.  The same m and params with another buffer keep
 *                      the open column and the history: how a caller with a small buffer drains.  m == 0 disarms and drops both (params
 *                      may be NULL then).  SGZ_EINVAL: a null stream, 0 < m < 32, NULL or invalid params, a null out with
 *                      capacity_columns > 0, an out that is not aligned, another m or other params while samples are open.
 *  sgz_pcm_stream_run_for   columns the next feed of nsamples closes (flush != 0: that feed followed by sgz_pcm_stream_flush_run); 0 when
 *                      disarmed.
 *  sgz_pcm_stream_run_state columns written since the lane was armed (the cursor) and the open column's samples; either may be NULL.
 *  sgz_pcm_stream_flush_run closes the open column: one launch on the carry, one column read back, waits; the history is kept.  Nothing
 *                      open: SGZ_OK, nothing done.  SGZ_EINVAL: disarmed, no column left in the buffer.
 * A feed that would close more columns than the buffer has left is refused with SGZ_EINVAL before anything is consumed.  reset drops the
 * open column, sets the history to marks and restarts the cursor.  The carry is kept twice and alternated: a piece reads one and writes
 * the other.  Memory per slot as the level lane's, 96 bytes a record and channel.
 * Host arithmetic on HOST records, nothing launched:
 *  sgz_run_fold        the zoom, with sgz_level_fold's boundary rule -- output column b is the fold of source columns x0 + ceil(b w /
 *                      cols) <= j < x0 + ceil((b + 1) w / cols), w = x1 - x0, cols = min(out_columns, w) --, so the lanes of a file zoom
 *                      together.  The fold above is applied in source order; `at` of an output column counts from the first sample of
 *                      its first source column.  out must not overlap in.  SGZ_EINVAL, nothing written: a null argument, channels == 0,
 *                      what sgz_overview_view_columns refuses, a folded len above 2^32 - 1.
 *  sgz_run_readout     what a host draws from one record at `rate` samples per second, in fp64: share[k] = count / len (NaN for len
 *                      == 0), longest_seconds[k] = longest / rate, at_seconds[k] = at / rate, crossing_hz = crossings rate / (2 len)
 *                      (NaN for len == 0).  SGZ_EINVAL: a null argument, a rate that is not a positive finite number. */
#define SGZ_RUN_HOT   0
#define SGZ_RUN_QUIET 1
#define SGZ_RUN_FLAT  2
#define SGZ_RUN_NAN   (-2147483647 - 1)       /* INT32_MIN: an invalid sample, or none */
typedef struct sgz_run_params {
    uint32_t hot;      /* |v| >= hot is hot; 1 .. 2^26 */
    uint32_t quiet;    /* |v| <= quiet is quiet; < hot */
} sgz_run_params;
typedef struct sgz_run_of {
    uint32_t count;    /* samples with the predicate */
    uint32_t runs;     /* runs that begin in the column */
    uint32_t longest;  /* the longest stretch inside the column */
    uint32_t at;       /* where the first such stretch starts, from the column's first sample; 0 when longest = 0 */
    uint32_t head;     /* the stretch at the column's start */
    uint32_t tail;     /* the stretch at the column's end */
} sgz_run_of;               /* 24 bytes */
typedef struct sgz_run_record {
    uint32_t   len;          /* the column's samples, NaNs included */
    uint32_t   skipped;      /* the invalid samples (NaNs) */
    uint32_t   crossings;    /* sign changes between neighbouring valid samples */
    uint32_t   reserved0;    /* 0 */
    sgz_run_of of[3];        /* SGZ_RUN_HOT, SGZ_RUN_QUIET, SGZ_RUN_FLAT */
    uint32_t   reserved[2];  /* 0 */
} sgz_run_record;           /* 96 bytes */
typedef struct sgz_run_carry {
    sgz_run_record open;         /* the open column so far */
    int32_t        prev[2];      /* v[i - 1], v[i - 2] of the next sample i; SGZ_RUN_NAN: invalid or none */
    uint32_t       reserved[2];  /* written as 0 */
} sgz_run_carry;            /* 112 bytes */
typedef struct sgz_run_reading {
    double share[3], longest_seconds[3], at_seconds[3], crossing_hz;
} sgz_run_reading;
sgz_status sgz_stage_run_columns(const float *d_planar, size_t channel_stride, uint32_t channels, size_t nsamples, const sgz_run_params *params,
                                 uint32_t m, uint32_t held, int flush, uint32_t continued, uint32_t slices, sgz_run_carry *d_carry /*[channels]*/,
                                 sgz_run_record *d_runs /*[columns][channels]*/, void *stream);
void       sgz_run_columns_limits(uint32_t *switch_over, uint32_t *tile_samples);
void       sgz_run_params_default(sgz_run_params *params);
sgz_status sgz_run_fold(const sgz_run_record *in, size_t n, uint32_t channels, size_t x0, size_t x1, uint32_t out_columns, sgz_run_record *out);
sgz_status sgz_run_readout(const sgz_run_record *rec, double rate, sgz_run_reading *out);
sgz_status sgz_pcm_stream_set_run(sgz_pcm_stream *s, const sgz_run_params *params, uint32_t m /*0 = off*/,
                                  sgz_run_record *out /*HOST [capacity][channels]*/, uint64_t capacity_columns);
uint64_t   sgz_pcm_stream_run_for(const sgz_pcm_stream *s, size_t nsamples, int flush);
sgz_status sgz_pcm_stream_run_state(const sgz_pcm_stream *s, uint64_t *columns_written, uint64_t *open_samples);
sgz_status sgz_pcm_stream_flush_run(sgz_pcm_stream *s);

/* The track lane: the tracker's curve over a file -- the reference's drawFrequencyTracking readout (SpectrumRendering.cpp:300-377, the
 * line-results branch) for every frame of a streamed file, in bounded memory.  sgz_spectrogram_track_device / _host want the whole file
 * resident and keep line results proportional to the frame count; this lane searches each piece's line results where the stream has
 * them anyway.
 * While armed, every feed of either kind (sgz_pcm_stream_feed and sgz_pcm_stream_feed_overview, any k, any flush, mixed where the rules
 * above allow) writes one sgz_line_peak per (frame, pair) for exactly the frames that became complete (sgz_stream_step), to track_out at a
 * cursor.  The records of all feeds, concatenated, equal sgz_spectrogram_track_host(plan, <the stream's converted planar floats>, graph,
 * mouse_fraction, ...) byte for byte, whatever the cuts into feeds and pieces, chunk_samples and SGZ_OPT_OVERVIEW_SLAB; the image, lines,
 * overview columns, peaks and waveform columns of an armed stream are those of an unarmed one byte for byte.  The tracker runs on the
 * compute stream behind the piece's render (in an overview feed: behind every slab's render, on the slab's line results) and the records
 * ride the piece's read-back: pinned track_out is written in place, pageable memory through a pinned twin per slot.
 *  sgz_pcm_stream_set_track    between feeds.  A non-NULL track_out arms: HOST sgz_line_peak [capacity_frames][pairs].  The lane has no open
 *                      state (records exist only for complete frames), so every call restarts the cursor at 0 and may change graph,
 *                      mouse_fraction or the buffer: how a caller with a small buffer drains.  NULL with capacity 0 disarms.
 *                      SGZ_EINVAL, the stream unchanged: a null stream, graph >= SGZ_NUM_GRAPHS, a non-finite mouse_fraction, a null
 *                      track_out with capacity_frames > 0, a track_out not aligned to 8 bytes.
 *  sgz_pcm_stream_track_for    frames whose records the next feed of nsamples writes (sgz_pcm_stream_frames_for while armed); 0 when disarmed
 *                      or for a null stream.
 *  sgz_pcm_stream_track_state  frames written since the lane was armed or the stream reset (the cursor); frames_written may be NULL.
 * A feed that would complete more frames than the buffer has left is refused with SGZ_EINVAL before anything is consumed.  reset restarts
 * the cursor and keeps the lane armed.
 * Memory: per slot maxFrames * pairs records of device (and, for a pageable buffer, pinned) memory, maxFrames = ceil(chunk_samples / hop),
 * made on first need.  An armed sgz_pcm_stream_feed renders with line results even when lines_out is NULL -- they stay on the device --
 * so each slot then holds maxFrames * pairs * graphs * P * 8 bytes of them, bounded by chunk_samples: the amount lines_out already costs.
 * An armed sgz_pcm_stream_feed_overview searches the plan's slab scratch and adds no line-result memory.  A track-only pass over a file is
 * therefore an overview feed with a large k and peaks_out only: one column of peaks per feed comes back beside the records. */
sgz_status sgz_pcm_stream_set_track(sgz_pcm_stream *s, uint32_t graph, double mouse_fraction,
                                    sgz_line_peak *track_out /*HOST [capacity_frames][pairs]; NULL with capacity 0 = off*/, uint64_t capacity_frames);
uint64_t   sgz_pcm_stream_track_for(const sgz_pcm_stream *s, size_t nsamples);
sgz_status sgz_pcm_stream_track_state(const sgz_pcm_stream *s, uint64_t *frames_written);

/* The view of kept peaks: any range of kept V at any width and in any colours, one small launch -- what a host calls per redraw of a file
 * lane (zoom, pan, resize, another gradient) instead of rendering the file again.
 * Definition (exact, no tolerance): given V [n][pairs][P] as any overview call writes its peaks, a source range x0 < x1 <= n, m = x1 - x0,
 * and out_columns >= 1: cols = min(out_columns, m); output column b covers source columns x0 + ceil(b m / cols) <= j < x0 +
 * ceil((b + 1) m / cols) (the rule of the dense scope columns; never empty -- zooming in past one source column per pixel is the texture
 * sampler's job); V'[b][p][i] = the greatest of V[j][p][i] over the column under the overview's total order (NaNs take no part, a group
 * of NaNs alone gives 0x7FC00000, -0 < +0); the pixel is the additive blend of the pairs' colours at V', then the 8-bit conversion, as
 * above.  The peak hold is a maximum under a total order, so a coarser column is exactly the maximum of the finer ones it covers: the
 * view of peaks kept at k has the bits of the direct overview at a multiple of k wherever the column boundaries coincide, and a view
 * of a view those of the direct view where the boundaries nest.  With cols == m the call is a pure recolour.  The colour tables and
 * scalars are the plan's; it only has to agree with the peaks in num_pairs and axis_points.
 *  sgz_overview_view_columns  host arithmetic, no GPU: *columns = cols and, when bounds != NULL, the cols + 1 boundaries x0 + ceil(b m /
 *                      cols), b = 0 .. cols.  SGZ_EINVAL: x0 >= x1, x1 > n, out_columns == 0, n >= 2^31, a null result.
 *  sgz_stage_overview_view    DEVICE pointers, asynchronous on `stream`, nothing waited for.  d_rgba [cols][P][4], d_peaks_out float
 *                      [cols][pairs][P] = V'; either may be NULL, not both.  slices as in sgz_stage_overview: 0 = the library's choice,
 *                      1 .. 64 forced, identical bits.  Only the documented bytes are written.  The outputs must not overlap d_peaks.
 *                      SGZ_EINVAL, nothing launched or written: a null plan or d_peaks, what sgz_overview_view_columns refuses,
 *                      slices > 64, both outputs NULL, an output that overlaps source columns [x0, x1).
 *  sgz_overview_view_host     HOST peaks, as the host overview and the stream return them: uploads only columns [x0, x1) into plan
 *                      scratch on the plan's own stream, runs the stage call, reads back the cols columns and waits.  timing->frames
 *                      counts the columns returned. */
sgz_status sgz_overview_view_columns(uint64_t n, uint64_t x0, uint64_t x1, uint32_t out_columns, uint64_t *columns, uint64_t *bounds /*[cols + 1] or NULL*/);
sgz_status sgz_stage_overview_view(sgz_plan *plan, const float *d_peaks, size_t n, size_t x0, size_t x1, uint32_t out_columns, uint32_t slices,
                                   uint8_t *d_rgba, float *d_peaks_out, void *stream);
sgz_status sgz_overview_view_host(sgz_plan *plan, const float *peaks, size_t n, size_t x0, size_t x1, uint32_t out_columns, uint8_t *rgba_out,
                                  float *peaks_out, sgz_timing *timing);

/* K_B in two steps, for the multi-GPU carry exchange (collective A2).  scan: the chunk scans of `frames` frames from a
 * ZERO carry-in; writes that zero-carry end state (what a rank publishes) to d_end_state [pairs][graphs][P][2] and keeps the chunk
 * aggregates inside the plan.  emit: folds the true carry-in d_carry (NULL = zero) into the kept aggregates -- one pass over the
 * aggregates, no second scan of the magnitudes -- and renders; d_state_out (optional) receives the state after the last frame.
 * Result == sgz_stage_decay_colour(..., d_state = carry) bit for bit.
 * SGZ_CH_PHASE: the magnitude half of the state -- a peak decay, and all the image is coloured from (SpectrumDSP.cpp:123) -- folds
 * the same way; the cancellation smoother (:1409-1412) is a linear fp32 recurrence without an exact fold, so emit renders the image
 * only (d_lines / d_state_out: SGZ_EUNSUPPORTED) and the phase halves of the scan's end state are not meaningful. */
sgz_status sgz_stage_decay_scan(sgz_plan *plan, const float *d_mapped, size_t frames, float *d_end_state, void *stream);
sgz_status sgz_stage_decay_emit(sgz_plan *plan, const float *d_mapped, size_t frames, const float *d_carry, uint8_t *d_rgba,
                                float *d_lines, float *d_state_out, void *stream);

/* std::log(float) as the dB map evaluates it (TransformDSP.inl:1345): glibc's logf algorithm, bit-identical to libm over every
 * positive finite float (tests/test_gpu_spectrum.py checks all 2^31 of them).  d_x > 0; DEVICE pointers. */
sgz_status sgz_stage_logf(const float *d_x, float *d_y, size_t n, void *stream);
/* the last step of every K_A pixel, magnitude = sqrt(re*re + im*im) with im == 0 (TransformDSP.inl:1331): evaluated as |x| where the
 * square is a normal float (the two are bit-identical there), as the correctly rounded root elsewhere */
sgz_status sgz_stage_finish_pixel(const float *d_x, float *d_y, size_t n, void *stream);

/* Multi-GPU time-chunk sharding (collective A2).  Rank q renders its frames with a zero
 * carry-in and publishes its end state A_q (the d_state output above).  Because fl(x*pole) is monotone,
 * the true state entering rank r is  fold_{q<r} carry = max(A_q, decay^{frames_q}(carry))  evaluated with
 * sequential fp32 multiplies -- bit-identical to the reference's sequential recurrence
 * (TransformDSP.inl:1336-1341) run over the whole stream on one device.
 * d_aggs: DEVICE float [world][pairs][graphs][P][2] (an all-gather of every rank's end state);
 * frames_per_rank: HOST int64 [world]; d_carry: DEVICE float [pairs][graphs][P][2] (out). */
sgz_status sgz_decay_fold_carry(sgz_plan *plan, const float *d_aggs, const int64_t *frames_per_rank,
                                uint32_t world, uint32_t rank, float *d_carry, void *stream);

/* The whole sharded render behind the ABI, on the host's own RCCL communicator (no torch, no Python): halo ncclSend / ncclRecv with
 * the neighbours (exactly the samples the last frames reach into the next rank's chunk), K_A, zero-carry K_B scan, ncclAllGather of
 * the end states, exact fold, K_B emit.  Rank r holds samples [r S, (r+1) S) of the stream in d_chunk (2*num_pairs channels, S =
 * chunk_samples, channel_stride >= S + halo_in: the halo is written behind the chunk); d_rgba receives this rank's columns
 * [local_frames][P][4].  Bit-identical to a single-device render of the concatenated stream.  (RSNT plans shard too: chunks of whole hops,
 * no halo; the resonators' linear recurrence is cut the same way -- every rank from rest, one all-gather of the resonators' end
 * states, the entering state folded in fp64 and added to every frame before the window kernel -- and the frames then equal a single
 * device's to within the bar its own chained frames are held to, not bit for bit: sharded.hip renderShardedResonator.)  nccl_comm: an ncclComm_t (RCCL is
 * bound with dlopen at first use; sgz_comm_* are conveniences for hosts that do not link RCCL themselves: sgz_comm_unique_id on
 * one rank, the 128 bytes handed to every rank by the host's own means, sgz_comm_create on all). */
sgz_status sgz_comm_unique_id(uint8_t out[128]);
sgz_status sgz_comm_create(const uint8_t id[128], uint32_t rank, uint32_t world, void **comm);
void       sgz_comm_destroy(void *comm);
sgz_status sgz_shard_layout(const sgz_plan *plan, uint32_t rank, uint32_t world, size_t chunk_samples, uint64_t *local_frames,
                            uint64_t *first_frame, uint64_t *halo_in, uint64_t *halo_out);
sgz_status sgz_spectrogram_render_sharded(sgz_plan *plan, void *nccl_comm, uint32_t rank, uint32_t world, float *d_chunk,
                                          size_t channel_stride, size_t chunk_samples, uint8_t *d_rgba, uint64_t *local_frames,
                                          void *stream);
/* The same render on the caller's own transport: the three collectives of the protocol as plain functions (counts in floats, device
 * pointers, 0 = success).  Each is ordered on `stream` the way ncclSend / ncclRecv / ncclAllGather are -- work queued on the stream
 * before the call is visible to it, work queued after it sees its result; an implementation may simply synchronise the stream and
 * move the data on the host.  Between group_begin and group_end (both optional) the send and the recv of one exchange are issued
 * back to back and must not deadlock on each other; abort (optional) is called when this rank fails while its peers may already be
 * waiting in a collective (ncclCommAbort on RCCL).  sgz_spectrogram_render_sharded is this call on RCCL. */
typedef struct sgz_transport {
    void *ctx;
    int (*send)(void *ctx, const float *d_buf, size_t count, uint32_t peer, void *stream);
    int (*recv)(void *ctx, float *d_buf, size_t count, uint32_t peer, void *stream);
    int (*allgather)(void *ctx, const float *d_send, float *d_recv /*[world][count]*/, size_t count, void *stream);
    int (*group_begin)(void *ctx);
    int (*group_end)(void *ctx);
    void (*abort)(void *ctx);
} sgz_transport;
sgz_status sgz_spectrogram_render_sharded_on(sgz_plan *plan, const sgz_transport *transport, uint32_t rank, uint32_t world, float *d_chunk,
                                             size_t channel_stride, size_t chunk_samples, uint8_t *d_rgba, uint64_t *local_frames,
                                             void *stream);
/* The same protocol for a host that drives several GPUs from ONE process (a thread per rank, no RCCL): an sgz_transport whose three
 * collectives are hipMemcpyPeerAsync copies over xGMI, each enqueued by the receiving rank on its own stream behind an event of the
 * sender's -- stream-ordered like their RCCL counterparts, and no host thread ever waits for a GPU (only for its peer to have enqueued).
 * devices[r] = HIP device of rank r (ranks may share a device: the copies are then plain device copies, which is how the tests run
 * it on one GPU).  One group per set of ranks; every rank takes its own transport from it and calls
 * sgz_spectrogram_render_sharded_on from its own thread with that device current.  *ctx_storage is released with
 * sgz_peer_transport_release when the rank is done. */
typedef struct sgz_peer_group sgz_peer_group;
sgz_status sgz_peer_group_create(uint32_t world, const int *devices /*[world]*/, sgz_peer_group **out);
void       sgz_peer_group_destroy(sgz_peer_group *group);
sgz_status sgz_peer_transport(sgz_peer_group *group, uint32_t rank, sgz_transport *out, void **ctx_storage);
void       sgz_peer_transport_release(void *ctx_storage);

/* ------------------------------------------------------------------------------------------------
 * Real-time per-block path: replaces Spectrum::ProcessorShell::onStreamAudio (SpectrumDSP.cpp:210-216)
 * -> AudioDispatcher::dispatch (:63-108) and the consumer side Spectrum::renderColourSpectrum's
 * frameQueue.popElement (SpectrumRendering.cpp:696-721) -- plus the two steps before the path: the additive
 * channel routing of MixGraphListener::deliver (Source/Common/MixGraphListener.cpp:247-334, sgz_spectrum_set_mix) and the audio
 * history ring, which lives in HBM (mirrored: the transform reads its window in place).  One producer thread (push) and one
 * consumer thread (pop_column, line_results, configure, set_view, resize, update, set_mix, clear_state) may run concurrently.  push never waits for the GPU
 * and allocates nothing: when the GPU is several blocks behind, or a configure is in progress, it returns SGZ_BUSY and the block
 * is not taken.  At most 131072 samples per push.
 */
typedef struct sgz_spectrum sgz_spectrum;
sgz_status sgz_spectrum_create(const sgz_spectrum_config *cfg, sgz_spectrum **out);
void       sgz_spectrum_destroy(sgz_spectrum *s);
sgz_status sgz_spectrum_configure(sgz_spectrum *s, const sgz_spectrum_config *cfg);   /* handleFlagUpdates */
/* onStreamAudio(ctx, float** buffer, numChannels, numSamples) */
sgz_status sgz_spectrum_push(sgz_spectrum *s, const float *const *planar, uint32_t num_channels, uint32_t nsamples);
/* frameQueue.popElement -> RGBA8 column of P pixels; SGZ_EMPTY when none is ready; SGZ_EINVAL on a LINE_GRAPH handle (display_mode 0 --
 * what a zero-initialised sgz_spectrum_config selects, as in the reference's enum -- produces no columns: sgz_spectrum_render_lines) */
sgz_status sgz_spectrum_pop_column(sgz_spectrum *s, uint8_t *rgba /*4*P*/, uint32_t *axis_points);
/* Display hand-off without the host: instead of popping columns and uploading each with
 * oglImage.updateSingleColumn (SpectrumRendering.cpp:696-721, :742-744), bind a device image of P rows x `columns` RGBA8 texels and
 * let sgz_spectrum_flush_columns (consumer thread, in place of the pop loop) scatter every ready column into it at
 * x = framePixelPosition, wrapping at `columns`; *first_column / *count name the texel columns written by this call (SGZ_EMPTY: none).
 *   sgz_spectrum_bind_image     caller-owned DEVICE memory (any mapped interop resource); d_image = NULL unbinds
 *   sgz_spectrum_create_image   the library allocates the image (whole 2 MiB blocks, see sgz_export_alloc) and exports it as a dma-buf
 *                               fd (the caller closes it): an MI355X has no graphics engine, the GL / Vulkan context of the display
 *                               GPU imports the fd (EXT_memory_object_fd, EGL_EXT_image_dma_buf_import; import size = pitch * P
 *                               rounded up to 2 MiB); dmabuf_fd may be NULL
 *   sgz_spectrum_bind_gl_buffer an OpenGL buffer object (e.g. a pixel-unpack buffer the texture is updated from) of a context that is
 *                               current on this thread and lives on the same device: hipGraphicsGLRegisterBuffer; flush_columns maps
 *                               and unmaps it around its writes.  tests/test_gpu_realtime.py test_gl_buffer_round_trip executes it where an
 *                               EGL surfaceless context can be made current; on the MI355X boxes this library is developed on it cannot (no
 *                               display engine; the image has libGL / GLX, which needs an X server, but neither libEGL nor libgbm) and the
 *                               test skips with the loader's error: there the call is only known to fail with a status
 * A configure drops the binding (the image height is the axis size); sgz_spectrum_set_view keeps it; sgz_spectrum_resize moves it. */
sgz_status sgz_spectrum_bind_image(sgz_spectrum *s, void *d_image, uint32_t columns, size_t pitch_bytes);
sgz_status sgz_spectrum_create_image(sgz_spectrum *s, uint32_t columns, void **d_image, size_t *pitch_bytes, int *dmabuf_fd);
sgz_status sgz_spectrum_bind_gl_buffer(sgz_spectrum *s, unsigned int gl_buffer, uint32_t columns, size_t pitch_bytes);
sgz_status sgz_spectrum_flush_columns(sgz_spectrum *s, uint32_t *first_column, uint32_t *count);
/* The render thread's colour-spectrum frame as the plugin runs it (consumer thread, once per video frame): Spectrum::renderColourSpectrum
 * (SpectrumRendering.cpp:672-749) = frame pacing + freeze around the pop loop, then the ring image drawn unrolled.  COLOUR_SPECTRUM handles
 * only (a LINE_GRAPH handle: SGZ_EINVAL).  The handle keeps three values for it: framesPerUpdate (0 from sgz_spectrum_create on: the
 * constructor zero-initialises it, Spectrum.cpp:59, and nothing but the loop assigns it), frame_update_smoothing (0) and frozen (0).  All
 * three survive sgz_spectrum_configure, _update, _resize, _set_view and every (re)binding of the image; sgz_spectrum_pop_column and
 * sgz_spectrum_flush_columns neither read nor write them.
 *   sgz_spectrum_set_pacing      content->frameUpdateSmoothing ("Upd. smoothing", SpectrumParameters.h:104, :122: the range is
 *                                [0, 0.996]; here finite in [0, 1), else SGZ_EINVAL)
 *   sgz_spectrum_set_frozen      Spectrum::freeze / unfreeze (Spectrum.cpp:161-169): state.isFrozen
 *   sgz_spectrum_render_columns  the pop loop of one video frame (:679-735) into the bound image (none bound: SGZ_EINVAL), a GL buffer
 *                                mapped and unmapped around the writes as in flush_columns.  With z = framesPerUpdate, s = the smoothing
 *                                and stored() = the columns in the queue now (getApproximateStoredFrames(), read live):
 *                                  z1 = stored() + s * (z - stored())            (:686-687; fp64, as written)
 *                                  s != 0: at most round(z) columns are popped  (:688, :693: round(framesPerUpdate), not round(z1))
 *                                  s == 0: every column is popped, and z1 = stored() + s * (z - stored()) again behind each pop
 *                                          (:727-731; processedFrames stays 0 there, its ++ sits behind `!shouldCap ||`)
 *                                  framesPerUpdate = z1                          (:735)
 *                                A pop ends the loop when the queue is empty or its first column's copy has not completed (popElement
 *                                fails), and -- this library's limits -- after 10 columns (the queue's depth: the slots go back to the
 *                                producer behind the write) or one lap of the image.  All columns taken are written by ONE kernel launch
 *                                at x = framePixelPosition, wrapping at `columns`, waited for; framePixelPosition advances by the count.
 *                                *first_column / *count name the texel columns written, *frames_per_update = framesPerUpdate after the
 *                                call (each may be NULL).  SGZ_EMPTY: none taken (framesPerUpdate is updated all the same).  Frozen
 *                                (:679): nothing is taken, framesPerUpdate and framePixelPosition stay, SGZ_EMPTY; the producer keeps
 *                                running and drops the columns a full queue cannot take (SpectrumDSP.cpp:185-186; dropped_columns of
 *                                sgz_spectrum_stats counts them)
 *   sgz_spectrum_present         OpenGLImageDrawer::drawCircular(framePixelPosition / (columns - 1)) (:742-744) of the bound image into
 *                                d_dst, DEVICE memory [P][dst_pitch_bytes] (pitch >= 4 * columns, 4-byte aligned), by
 *                                sgz_image_unroll_device's rule with x = framePixelPosition; waits for the texels.  Frozen or not.  A
 *                                d_dst whose bytes overlap the bound image's: SGZ_EINVAL.  A host that draws the ring itself (two quads
 *                                split at *first_column + *count) does not need it. */
sgz_status sgz_spectrum_set_pacing(sgz_spectrum *s, double frame_update_smoothing);
sgz_status sgz_spectrum_set_frozen(sgz_spectrum *s, int frozen);
sgz_status sgz_spectrum_render_columns(sgz_spectrum *s, uint32_t *first_column, uint32_t *count, double *frames_per_update);
sgz_status sgz_spectrum_present(sgz_spectrum *s, void *d_dst, size_t dst_pitch_bytes);
/* One pass of renderColourSpectrum's pop loop as written (:681-735) for a queue of `queued` columns that nobody adds to meanwhile and a
 * previous framesPerUpdate z (host only, no GPU; sgz_spectrum_render_columns runs the same arithmetic on the live queue).  Line by line,
 * with Q = queued, s = smoothing:
 *   :681      localFrameZ1 = framesPerUpdate = z
 *   :685-687  processedFrames = 0; approximateFrames = 0 + Q; localFrameZ1 = Q + s * (z - Q)
 *   :688      framesThisTime = round(framesPerUpdate) = round(z)     -- of the OLD value, not of localFrameZ1
 *   :691      shouldCap = s != 0
 *   :693      while (!shouldCap || processedFrames++ < framesThisTime): with shouldCap the body runs at most round(z) times and
 *             processedFrames counts them; without it the `||` short-circuits, processedFrames++ is never evaluated and stays 0
 *   :696-697  popElement fails -> break: after Q pops
 *   :727-732  only when !shouldCap: approximateFrames = processedFrames (0) + what is left; localFrameZ1 = left + s * (z - left)
 *   :735      framesPerUpdate = localFrameZ1
 * so
 *   smoothing != 0: *pop = min(queued, round(z));  *z_next = queued + smoothing * (z - queued)
 *   smoothing == 0: *pop = queued;                 *z_next = left + 0 * (z - left) with left = queued - *pop = 0, i.e. 0 (what :729-731
 *                                                  leave behind the last pop; with queued = 0 there is no pop and :687 gives the same)
 * round(v) = (size_t) floor(v + 0.5) (UNVERIFIED vs cpl: cpl::Math::round is not in the tree; this is the library's rule).  smoothing
 * finite in [0, 1), z finite >= 0: else SGZ_EINVAL. */
sgz_status sgz_frame_pacing_step(double z, double smoothing, uint32_t queued, uint32_t *pop, double *z_next);
/* The two kernels behind them as stateless stage calls: asynchronous on `stream`, DEVICE pointers, nothing waited for; a null pointer is
 * SGZ_EINVAL.  Both only move texels.
 * sgz_columns_to_image_device: n RGBA8 columns [n][P] into an image [P rows][pitch_bytes] of the bound image's layout (row y = axis point
 *   y): texel ((x0 + k) % columns, y) = d_columns[k][y] -- what oglImage.updateSingleColumn(framePixelPosition, ...) uploads for n popped
 *   frames in a row (SpectrumRendering.cpp:721-724), or a whole sgz_spectrogram_render_device result [frames][P] as a texture.  1 <= n <=
 *   columns < 2^31, x0 < columns, 1 <= P <= 2^20, pitch_bytes >= 4 * columns and a multiple of 4, both pointers 4-byte aligned.  Texels
 *   of other columns and beyond `columns` in a wider pitch are not touched.
 * sgz_image_unroll_device: drawCircular(x / (columns - 1)) (:742-744; UNVERIFIED vs cpl: cpl's OpenGLImageDrawer is not in the tree; this
 *   is the library's rule): dst[y][j] = src[y][(x + j) % columns] for j < columns -- column x (the oldest, the next to be overwritten) at
 *   the left, x - 1 (the newest) at the right.  x < columns < 2^31, 1 <= P <= 2^20, pitches as above.  d_src and d_dst must not overlap
 *   (SGZ_EINVAL); texels beyond `columns` in a wider destination pitch are not touched. */
sgz_status sgz_columns_to_image_device(const uint8_t *d_columns /*[n][P][4]*/, size_t n, uint32_t axis_points, void *d_image,
                                       uint32_t columns, size_t pitch_bytes, uint32_t x0, void *stream);
sgz_status sgz_image_unroll_device(const void *d_src, uint32_t columns, size_t src_pitch_bytes, uint32_t axis_points, uint32_t x, void *d_dst,
                                   size_t dst_pitch_bytes, void *stream);
/* Zoom / pan (consumer thread): Spectrum::handleFlagUpdates' viewChanged branch (Spectrum.cpp:532-575) for a change of viewLeft /
 * viewRight only -- what mouseWheelMove / mouseDrag (:172-290) cause.  The view is checked as sgz_spectrum_configure checks it (finite,
 * 0 <= left < right <= 1); SGZ_EINVAL leaves the handle exactly as it was.  Every other field stays as configured (a change of scaling or
 * min_log_freq is a sgz_spectrum_update, of size a sgz_spectrum_resize, of display mode a sgz_spectrum_configure).
 *   kept:     the audio history in HBM and the frame cadence (a frame fires where it would have; strict-quirks framing included), the mix
 *             matrix, the handle options, the column queue, the image binding and framePixelPosition
 *   replaced: remapFrequencies and what hangs on it (map tables, slope map, tracker tables, resonator tuning), built before push is held
 *             off: push returns SGZ_BUSY only while the new tables are swapped in and warmed up
 *   zeroed:   pair.clearLineGraphStates() (TransformPair.h:169-175): both graphs' decay states and results -- sgz_spectrum_line_results
 *             reads zeros until a frame computed after this call arrives.  RSNT: the resonators restart at rest under their new tuning
 *             (UNVERIFIED vs cpl: cpl's mapSystemHz is not in the tree)
 *   COLOUR_SPECTRUM with an image bound and a rect that changed: oglImage.freeLinearVerticalTranslation(oldViewRect, viewRect)
 *             (:560-561) on the bound image (sgz_view_translate_device's rule), waited for before the call returns.  Columns still in
 *             the queue keep the mapping they were computed with and land untranslated at the next flush_columns.
 * Waits for the GPU: not for the audio thread. */
sgz_status sgz_spectrum_set_view(sgz_spectrum *s, double view_left, double view_right);
/* freeLinearVerticalTranslation of a spectrogram image (UNVERIFIED vs cpl: cpl's resampling is not in the tree; this is the library's
 * rule).  Image row i is axis point i, at view fraction left + (right - left) * i / (P - 1) in every scaling and channel mode, so the
 * old image is resampled along rows.  In fp64, S0 = old_right - old_left, S1 = new_right - new_left, for every new row i:
 *     u = new_left + S1 * (i / (P - 1.0));  r = (u - old_left) / S0 * (P - 1.0)
 *     r outside [-0.5, P - 0.5]: src[i] = -1 (no source: texel 0x00000000, what sgz_spectrum_create_image holds)
 *     else r = clamp(r, 0, P - 1); j = floor(r); w = floor((r - j) * 256 + 0.5); w == 256 -> j += 1, w = 0;  src[i] = j, weight[i] = w
 *     every byte c of texel (x, i) = (a_c * (256 - w) + b_c * w + 128) >> 8 with a = old (x, j), b = old (x, min(j + 1, P - 1))
 * (w = 0 copies the row).  Every column of the image is translated; texels beyond `columns` in a wider pitch are not touched.
 * sgz_view_translation_rows: the table (host only, no GPU); SGZ_EINVAL for P < 2 or an invalid view.
 * sgz_view_translate_device: the stage call, stateless: d_image DEVICE [P][pitch_bytes], translated in place; allocates its scratch,
 * and waits for the result on `stream` before it returns.  P <= 2^20. */
sgz_status sgz_view_translation_rows(uint32_t axis_points, double old_left, double old_right, double new_left, double new_right,
                                     int32_t *src /*[P]*/, uint16_t *weight /*[P]*/);
sgz_status sgz_view_translate_device(void *d_image, uint32_t columns, size_t pitch_bytes, uint32_t axis_points, double old_left,
                                     double old_right, double new_left, double new_right, void *stream);
/* Resize (consumer thread): Spectrum::handleFlagUpdates' resized branch (Spectrum.cpp:503-515) -- what Spectrum::resized() (:156-159) and
 * the Spectrum stretch knob (:333-336) cause: axis_points is the editor's height in COLOUR_SPECTRUM and its width in LINE_GRAPH (:445-451);
 * the image is oglImage.resize(width / spectrumStretching, height, true), the columns it keeps.  axis_points is checked as
 * sgz_spectrum_configure checks it (2 ... 2^20); d_image is NULL or satisfies sgz_spectrum_bind_image's rules (columns > 0,
 * pitch >= 4 * columns, 4-byte aligned); a LINE_GRAPH handle takes NULL only.  SGZ_EINVAL leaves the handle exactly as it was; a handle
 * bound to a GL buffer returns SGZ_EUNSUPPORTED, unchanged (the host unbinds it first).  Every other config field stays as configured.
 *   kept:     the audio history in HBM and the frame cadence (strict-quirks framing included), the mix matrix, the handle options, the push
 *             backlog, the stats counters and the view
 *   replaced: both plans for the new size (map tables, slope map, tracker tables, resonator bank) and every buffer of the axis size, made
 *             before push is held off: push returns SGZ_BUSY only while they are swapped in and warmed up
 *   zeroed:   the viewChanged the resized branch sets (:532-575, :566) clears both graphs' decay states and results, also at an unchanged
 *             size -- sgz_spectrum_line_results reads zeros until a frame computed after this call arrives.  RSNT: the resonators restart
 *             at rest under the new bank (UNVERIFIED vs cpl: cpl's mapSystemHz is not in the tree)
 *   queue:    at an unchanged axis size the queued columns stay and land in the new image at the next flush_columns or pop_column; at a
 *             new size they are discarded, as queued frames of another size are skipped at render (SpectrumRendering.cpp:702), and not
 *             counted in dropped_columns
 *   image:    an image bound before and d_image given: the old content moves into d_image by sgz_image_resize_device's rule, and the
 *             binding moves to d_image, caller-owned -- it may be the old image's own memory.  An old image of sgz_spectrum_create_image
 *             is freed after the move (pass its own pointer to keep it: the new size must then fit its allocation; an exportable new
 *             image comes from sgz_export_alloc).  No image bound before: d_image is bound as sgz_spectrum_bind_image binds it (content
 *             untouched, x = 0).  d_image NULL: the binding is dropped, as sgz_spectrum_configure drops it.
 * Waits for the GPU: not for the audio thread. */
sgz_status sgz_spectrum_resize(sgz_spectrum *s, uint32_t axis_points, void *d_image, uint32_t columns, size_t pitch_bytes);
/* oglImage.resize(width, height, true) of a spectrogram image (UNVERIFIED vs cpl: cpl's COpenGLImage::resize is not in the tree; this is
 * the library's rule).  The old image has P0 rows, C0 columns and next-write column x0 (framePixelPosition); the new one P1 rows and C1
 * columns.
 *   rows (axis point i sits at the same view fraction i / (P - 1) at both sizes), for every new row i, in fp64:
 *     r = (i * (P0 - 1.0)) / (P1 - 1.0);  j = floor(r);  w = floor((r - j) * 256 + 0.5);  w == 256 -> j += 1, w = 0;  src[i] = j, weight[i] = w
 *     every byte c of a texel = (a_c * (256 - w) + b_c * w + 128) >> 8 with a from old row j, b from old row min(j + 1, P0 - 1)
 *     (sgz_view_translate_device's blend; P0 == P1 copies the rows)
 *   columns (time stays 1:1: a column is one frame): x1 = x0 mod C1; new column c has age a = (x1 - 1 - c) mod C1; a < min(C0, C1): its
 *     source is old column (x0 - 1 - a) mod C0, otherwise src[c] = -1 and the texel is 0x00000000 (what sgz_spectrum_create_image holds).
 *     The same size is the identity, x unchanged
 * Texels beyond `columns` in a wider pitch are never written.
 * sgz_image_resize_rows / sgz_image_resize_columns: the tables (host only, no GPU); SGZ_EINVAL for P outside 2 ... 2^20, no columns,
 * C >= 2^31 or old_x >= old_columns.
 * sgz_image_resize_device: the stage call, stateless: d_src [P0][src_pitch_bytes] into d_dst [P1][dst_pitch_bytes], both DEVICE; SGZ_EINVAL
 * when their byte ranges overlap; *new_x (may be NULL) = x1.  Allocates its scratch and waits for the result on `stream` before it
 * returns. */
sgz_status sgz_image_resize_rows(uint32_t old_axis_points, uint32_t new_axis_points, int32_t *src /*[P1]*/, uint16_t *weight /*[P1]*/);
sgz_status sgz_image_resize_columns(uint32_t old_columns, uint32_t old_x, uint32_t new_columns, int32_t *src /*[C1]*/, uint32_t *new_x);
sgz_status sgz_image_resize_device(const void *d_src, uint32_t old_columns, size_t src_pitch_bytes, uint32_t old_axis_points, uint32_t old_x,
                                   void *d_dst, uint32_t new_columns, size_t dst_pitch_bytes, uint32_t new_axis_points, uint32_t *new_x,
                                   void *stream);
/* Every other setting change (consumer thread): the rest of Spectrum::handleFlagUpdates (Spectrum.cpp:351-616), where each parameter
 * raises a flag that rebuilds only what depends on it (parameterChangedRT, :291-343).  cfg is a complete configuration; it is compared
 * field by field with the handle's current one and the union of what the changed fields' flags do is applied.
 *   refused, the handle left exactly as it was:
 *     SGZ_EINVAL        what sgz_spectrum_create refuses; a change of axis_points (that is sgz_spectrum_resize); a window_size above an
 *                       explicitly set SGZ_RT_OPT_AUDIO_HISTORY
 *     SGZ_EUNSUPPORTED  a change of sample_rate or num_pairs (a new stream) or of display_mode (a new display): sgz_spectrum_configure
 *   a configuration equal to the current one: SGZ_OK, nothing touched, no plan built, push never held off.
 *   kept, always:  the audio history in HBM and the frame cadence (processedSamplesSinceLastFrame), the mix matrix, the handle options, the
 *                  push backlog, the stats counters, the image binding and framePixelPosition, and the queued columns (the axis size is
 *                  unchanged: they land later as they were computed)
 *   replaced:      both plans, and the buffers whose size depends on a changed field (frames per piece = 16384 / hop + 1, the sides of the
 *                  channel mode, the tracker's [pairs][N + 1] bins, strict mode's [2 pairs][W] frame), made before push is held off: push
 *                  returns SGZ_BUSY only while they are swapped in and warmed up.  Blocks waiting in the push FIFO are transformed under
 *                  the new configuration.
 *   per field (sgz_spectrum_update_effects says which apply):
 *     low_db, high_db, clip_db, colours, ratios, pole, slope_a / slope_b, bin_interp (assigned every call, :365-413; slopeMapChanged,
 *         :578-581): nothing zeroed -- the decay states, the line results and the RSNT resonators continue
 *     window_type, window_symmetry, window_alpha, window_beta, free_q (windowKernelChange -> regenerateWindowKernel, remapResonator,
 *         :583-595): FFT: nothing zeroed; RSNT: the resonators restart at rest under the new bank (UNVERIFIED vs cpl, as in set_view)
 *     window_size (audioWindowWasResized -> setStorage, windowKernelChange, :481-494): as the row above; the ring keeps its newest samples
 *         at the new capacity by sgz_ring_resize_device's rule (UNVERIFIED vs cpl: cpl's AudioStream history resize is not in the tree)
 *     hop (sampleBufferSize, assigned every call, :365): nothing zeroed.  The cadence follows audioEntryPoint (TransformDSP.inl:1172-1201):
 *         when the samples since the last frame reach the new hop, the next push fires one frame at the position of the update (over the
 *         W newest samples as of then), then one every new hop; strict-quirks framing likewise
 *     view_scaling, min_log_freq, view_left / view_right, channel_mode (viewChanged, :422-431, :532-575): clearLineGraphStates -- both
 *         graphs' decay states and results are zeroed (sgz_spectrum_line_results reads zeros until a frame computed after this call); RSNT:
 *         the resonators restart at rest.  COLOUR_SPECTRUM with an image bound and a rect that changed: the image is translated as
 *         sgz_spectrum_set_view translates it (:560-561), waited for before the call returns
 *     algorithm (resetStateBuffers -> clearAudioState, :321-324, :608-612): what sgz_spectrum_clear_state zeroes -- decay states, line
 *         results, resonators
 * Waits for the GPU: not for the audio thread. */
sgz_status sgz_spectrum_update(sgz_spectrum *s, const sgz_spectrum_config *cfg);
/* What sgz_spectrum_update does for a change from `from` to `to` (host only, no GPU; the update decides by this call): SGZ_OK and
 * *effects = a mask of the flags below (0: the configurations are equal), or the update's refusal -- SGZ_EINVAL for an invalid `to` or an
 * axis_points change, SGZ_EUNSUPPORTED for a sample_rate, num_pairs or display_mode change (checked in that order: validity, then those
 * three, then axis_points).  Fields compare by value (_pad and _reserved are ignored).  The audio-history refusal depends on the handle and
 * is the update's alone.
 *   SGZ_UPDATE_PLANS                new plans are built and swapped in (every change)
 *   SGZ_UPDATE_CLEAR_LINES          both graphs' decay states and results are zeroed (a view-class or algorithm change)
 *   SGZ_UPDATE_CLEAR_STATE          clearAudioState: the above and the resonators (an algorithm change)
 *   SGZ_UPDATE_RESONATORS_AT_REST   `to` is RSNT and its resonators start at rest (window, window_size, view class or algorithm changed)
 *   SGZ_UPDATE_TRANSLATE_IMAGE      `to` is COLOUR_SPECTRUM and the rect (view_left / view_right) changed: a bound image is translated
 *   SGZ_UPDATE_RING_MOVED           the ring's capacity ((RSNT ? hop : window_size) + 32768, rounded up to 64) changes */
#define SGZ_UPDATE_PLANS 1u
#define SGZ_UPDATE_CLEAR_LINES 2u
#define SGZ_UPDATE_CLEAR_STATE 4u
#define SGZ_UPDATE_RESONATORS_AT_REST 8u
#define SGZ_UPDATE_TRANSLATE_IMAGE 16u
#define SGZ_UPDATE_RING_MOVED 32u
sgz_status sgz_spectrum_update_effects(const sgz_spectrum_config *from, const sgz_spectrum_config *to, uint32_t *effects);
/* The update's ring move, as a stateless stage call: d_old [channels][2 old_cap] and d_new [channels][2 new_cap] are mirrored rings (sample
 * t at t mod cap and t mod cap + cap) into which `written` samples have gone.  For every t in [written - new_cap, written), d_new receives
 * at both mirror positions (non-negative residues, so a t below 0 has its slot too) the old sample when t >= written - old_cap and t >= 0,
 * otherwise 0.0f (silence, as a ring starts).  DEVICE pointers; enqueued on `stream`, nothing waited for.  SGZ_EINVAL for a null ring, a
 * zero capacity or one of 2^31 or more, no channels or more than 65535, or byte ranges that overlap. */
sgz_status sgz_ring_resize_device(const float *d_old, uint32_t old_cap, float *d_new, uint32_t new_cap, uint32_t channels, uint64_t written,
                                  void *stream);
/* lineGraphs[graph].getResults(P) for pair `pair`: float2 [P] (TransformPair.h:72-76).  COLOUR_SPECTRUM: the results of the newest
 * frame whose copy has reached the host (a pinned triple buffer the producer's stream fills: this call waits for nothing and never
 * touches the producer's stream); LINE_GRAPH: the results of the last sgz_spectrum_render_lines. */
sgz_status sgz_spectrum_line_results(sgz_spectrum *s, uint32_t pair, uint32_t graph, float *out /*2*P*/);
/* DisplayMode::LineGraph, once per video frame on the render (consumer) thread: Spectrum::vectorGLRendering's
 *     pair.prepareTransform(constant, views) -> doTransform -> mapToLinearSpace -> postProcessStdTransform
 * for every pair (Source/Spectrum/SpectrumRendering.cpp:617-635; whole-ring prepareTransform TransformDSP.inl:39-231): the W newest
 * samples of the device ring are transformed and mapped, BOTH graphs' peak-decay filters advance once, and lineGraphs[k].results of every
 * pair come back: out = float2 [pairs][graphs][P] (what renderTransformAsGraph reads, SpectrumRendering.cpp:823-891).  RSNT: the windowed
 * state of the resonators as of the last pushed block (mapToLinearSpace's RSNT branch, :1103-1133).
 * poles: the graphs' decay for THIS video frame (the reference derives it from openGLDeltaTime(), Spectrum.cpp:388-394), or NULL =
 * the configured ones.  Waits for its own result (it is the render thread's call); never delays push.  SGZ_EINVAL on a
 * COLOUR_SPECTRUM handle. */
sgz_status sgz_spectrum_render_lines(sgz_spectrum *s, const float *poles /*[SGZ_NUM_GRAPHS] or NULL*/, float *out /*[pairs][graphs][P][2]*/);
/* Handle switches (consumer thread, between create / configure and the first push; a configure or an update keeps them):
 *   SGZ_RT_OPT_STRICT_REFERENCE_QUIRKS  0 (default): ideal STFT framing -- a frame fires every `hop` samples wherever that falls inside a
 *       host block.  1: audioEntryPoint as written (TransformDSP.inl:1165-1211): every frame of one callback is prepared
 *       from the history BEFORE the callback plus the first min(availableSamples, W) samples of the UN-offset block (Q1: a 512-sample
 *       block at hop 200 yields the same window twice), and with an audio history longer than the window the frame is
 *       `history - W` samples short and zero-padded (Q2, :245-257).  Identical to the default whenever blocks divide the hop.
 *   SGZ_RT_OPT_AUDIO_HISTORY            the reference stream's audioHistorySize in samples (>= W; default and 0 = W, what
 *       Spectrum.cpp:472-477 asks for).  Read in strict mode only. */
#define SGZ_RT_OPT_STRICT_REFERENCE_QUIRKS 1u
#define SGZ_RT_OPT_AUDIO_HISTORY 2u
sgz_status sgz_spectrum_set_option(sgz_spectrum *s, uint32_t option, uint64_t value);
sgz_status sgz_spectrum_clear_state(sgz_spectrum *s);                                   /* clearAudioState, TransformPair.h:177-184 */
/* MixGraphListener::deliver's routing: destination channel d (of the 2*num_pairs the transform sees) = the sum of the source channels
 * c with matrix[d * num_sources + c] != 0, added in ascending c onto a cleared row (copyFromHead<true> into matrix.clear()'ed
 * rows).  push then takes num_sources channels.  Default: identity over 2*num_pairs sources. */
sgz_status sgz_spectrum_set_mix(sgz_spectrum *s, uint32_t num_sources, const uint8_t *matrix /*[2*num_pairs][num_sources]*/);
/* columns dropped because the queue was full (SpectrumDSP.cpp:185-186) and pushes refused with SGZ_BUSY, since create */
sgz_status sgz_spectrum_stats(sgz_spectrum *s, uint64_t *dropped_columns, uint64_t *refused_pushes);
/* (sgz_spectrum_backlog and sgz_spectrum_stats read atomics: a UI thread may poll them while the audio thread pushes.)
 * push never waits and never leaves a hole in the stream: a block the GPU is not ready for (all 8 staging slots in flight) waits in a
 * host FIFO -- one second of audio deep, like the reference's cpl::AudioStream in front of its listeners (PluginProcessor.cpp:195-198,
 * MixGraphListener.cpp:336-387) -- and is enqueued, in order, by the next push that finds a slot free.  SGZ_BUSY is returned only when
 * that FIFO is full (or a reconfiguration holds the handle).  deferred_blocks: blocks that ever waited there; waiting_now: its depth.
 * The same FIFO sits in front of sgz_scope_push and sgz_vector_push. */
sgz_status sgz_spectrum_backlog(sgz_spectrum *s, uint64_t *deferred_blocks, uint32_t *waiting_now);
/* enqueue whatever still waits in that FIFO (a stream that ended, a test): may wait for the GPU, so NOT for the audio thread -- and
 * not while the audio thread pushes (a push that finds the handle held is refused) */
sgz_status sgz_spectrum_flush(sgz_spectrum *s);
/* the hipStream_t the handle enqueues its work on (so that a host can order its own device work behind the handle's) */
void      *sgz_spectrum_stream(sgz_spectrum *s);
/* the frequency tracker on the newest window of pair `pair` (consumer thread): transforms the device ring's current window and runs
 * sgz_stage_track_peak's search on it */
sgz_status sgz_spectrum_track_peak(sgz_spectrum *s, uint32_t pair, double mouse_fraction, sgz_peak *out);
/* sgz_track_peak_lines on the handle's newest line results of (pair, graph) -- what sgz_spectrum_line_results would return now
 * (Complex mode, RSNT and the LineMain / LineSecond graphs: SpectrumRendering.cpp:300-377) */
sgz_status sgz_spectrum_track_peak_lines(sgz_spectrum *s, uint32_t pair, uint32_t graph, double mouse_fraction, sgz_line_peak *out);
/* parity hook: the W newest samples of destination channel `channel`, exactly the range of the device ring a frame firing now
 * would transform (call it from the producer's thread, or with the producer idle) */
sgz_status sgz_spectrum_history(sgz_spectrum *s, uint32_t channel, float *out /*W*/);

/* ------------------------------------------------------------------------------------------------
 * The line graph's vertex stream: Spectrum::renderTransformAsGraph (SpectrumRendering.cpp:794-897), what its PrimitiveDrawers receive
 * for every pair, built on the device from the line results (float2 [pairs][SGZ_NUM_GRAPHS][P], .first = left / magnitude, .second =
 * right / phase, exactly what sgz_spectrum_render_lines returns).  S = 2 sides for SGZ_CH_SEPARATE, SGZ_CH_MIDSIDE and SGZ_CH_PHASE (the
 * fall-throughs at :831, :877), 1 for the other modes.  Per pair p in ascending order (one renderTransformAsGraph call each, :639-652):
 *   1. flood fill, when alphaFloodFill != 0 (:807): for k = 1, 0, then side = right (S == 2 only), then left: 2P vertices, GL_LINES,
 *      (i, y, z), (i, endPoint, z) for i = 0 .. P-1
 *   2. strips: for k = 1, 0, then right (S == 2 only), then left: P vertices, GL_LINE_STRIP, (i, y, z)
 * y = results[p][k][i].second on the right side (z = -0.5), .first on the left side (z = 0): the stored float as it is (NaN, inf, -0 bit
 * for bit; in Phase mode the right side is the phase, drawn anyway as the reference does).  x = (float) i.  endPoint = (dbs.high > dbs.low
 * ? 0 : 1) is always 0: the plan refuses high_db <= low_db and getDBs() only widens the range.  Vertices per pair:
 * SGZ_NUM_GRAPHS * S * P * (flood ? 3 : 1); float3 packed, 12 bytes a vertex, pair p's at p * that.
 * GL state is the host's, per draw: the model matrix translate(-1, -1, 0) then scale(1 / ((P - 1) * 0.5), 2, 1) (:801-802) -- it is not
 * applied to the vertices: x_clip = model[0] x + model[2], y_clip = model[1] y + model[3] --; fills blend SRC_ALPHA, ONE_MINUS_SRC_ALPHA
 * with multisampling off, strips blend ONE, ONE_MINUS_SRC_COLOR with multisampling as state.antialias.
 */
#define SGZ_PRIM_LINES      0x0001u   /* GL_LINES      (the flood fill) */
#define SGZ_PRIM_LINE_STRIP 0x0003u   /* GL_LINE_STRIP (the graph)      */
#define SGZ_SIDE_LEFT  0u             /* results .first,  z = 0    */
#define SGZ_SIDE_RIGHT 1u             /* results .second, z = -0.5 */
/* Colours are RGBA8, the bytes juce::Colour holds: colour_one[k] / colour_two[k] = content->lines[k].colourOne / colourTwo.  Pair p draws
 * ColourRotation(colour, pairs, false)[p] (Spectrum.cpp:384-385, :646) = withRotatedHue((float) p / (float) pairs), alpha kept (the RGB part
 * is sgz_rotate_hue_rgb8); a fill draws it withAlpha(flood_alpha): alpha byte = a <= 0 ? 0 : a >= 1 ? 255 : (uint8_t) (a * 255.996f)
 * (juce_Colour.cpp:27-30).  Line widths: fills rendering_scale (:797), strips max(0.001f, (float) (rendering_scale * primitive_size)) (:852). */
typedef struct sgz_line_graph_style {
    uint8_t colour_one[SGZ_NUM_GRAPHS][4];   /* left side (and the only side of a one-sided mode) */
    uint8_t colour_two[SGZ_NUM_GRAPHS][4];   /* right side                                        */
    float   flood_alpha;                     /* state.alphaFloodFill: 0 = no flood fill            */
    float   primitive_size;                  /* state.primitiveSize                               */
    double  rendering_scale;                 /* oglc->getRenderingScale()                         */
} sgz_line_graph_style;
typedef struct sgz_line_graph_draw {
    uint32_t first, count;      /* vertices [first, first + count) of the stream      */
    uint32_t primitive;         /* SGZ_PRIM_LINES (fill) / SGZ_PRIM_LINE_STRIP (graph) */
    uint32_t pair, graph, side; /* side: SGZ_SIDE_*                                    */
    uint8_t  rgba[4];
    float    line_width;
} sgz_line_graph_draw;
/* the stream's length for `pairs` pairs (0 for an unknown channel mode); host only */
size_t     sgz_line_graph_vertex_count(uint32_t channel_mode, uint32_t pairs, uint32_t axis_points, uint32_t flood);
/* The draw list in the order above (host only, no GPU): flood = style->flood_alpha != 0.  *count: capacity in records on entry, records
 * written on return; too small (or out NULL) -> SGZ_EINVAL with *count = the size needed.  model (or NULL): the four coefficients. */
sgz_status sgz_line_graph_draws(const sgz_line_graph_style *style, uint32_t channel_mode, uint32_t pairs, uint32_t axis_points,
                                sgz_line_graph_draw *out, uint32_t *count, float model[4]);
/* Stage call, stateless: d_lines DEVICE float2 [pairs][SGZ_NUM_GRAPHS][axis_points] -> d_xyz DEVICE float3 [sgz_line_graph_vertex_count].
 * One launch; asynchronous on `stream`.  axis_points <= 2^24. */
sgz_status sgz_line_graph_vertices_device(const float *d_lines, uint32_t pairs, uint32_t axis_points, uint32_t channel_mode,
                                          uint32_t flood, float *d_xyz, void *stream);
/* The handle's line graph straight into a vertex buffer: exactly sgz_spectrum_render_lines (the newest window -- RSNT: the resonator state --,
 * both filters advanced ONCE with this call's poles), then the vertex kernel on the same stream, then one wait.  xyz: pageable host,
 * pinned host or DEVICE memory (a mapped VBO) -- device memory and pinned, device-mapped host memory are written by the kernel itself,
 * anything else through a staging buffer the first such call allocates.  *count: capacity in vertices on entry, vertices written on return;
 * too small -> SGZ_EINVAL with *count = the size needed, nothing written and the filters untouched.  Afterwards sgz_spectrum_line_results and
 * sgz_spectrum_track_peak_lines see this call's results.  SGZ_EINVAL on a COLOUR_SPECTRUM handle; never delays push. */
sgz_status sgz_spectrum_render_line_vertices(sgz_spectrum *s, const float *poles /*[SGZ_NUM_GRAPHS] or NULL*/, uint32_t flood, float *xyz,
                                             uint32_t *count);

/* ------------------------------------------------------------------------------------------------
 * Oscilloscope: Lanczos-10 per-point resampler (drawWavePlot, OscilloscopeRendering.cpp:790-891),
 * zero-crossing trigger (ZeroCrossingProcessor::process, StreamPreprocessing.h:315-349) and the peak
 * envelope (runPeakFilter, OscilloscopeDSP.inl:713-886).
 */
typedef struct sgz_scope_view {
    double   window_size;       /* state.effectiveWindowSize, samples      */
    double   left, right;       /* state.viewOffsets[Left], [Right]        */
    double   rendering_scale;   /* oglc->getRenderingScale()               */
    uint32_t width;             /* getWidth(), pixels                      */
    uint32_t _pad;
} sgz_scope_view;
size_t     sgz_scope_num_points(const sgz_scope_view *view);
/* d_ring: DEVICE fp32 front buffer in time order (index 0 at the stream cursor), len samples, `channels`
 * buffers at d_ring + c*stride.  d_xy: DEVICE float2 [channels][points] = the (x, y) of addVertex(x, y, 0). */
sgz_status sgz_scope_lanczos_device(const sgz_scope_view *view, const float *d_ring, size_t len,
                                    size_t stride, uint32_t channels, float *d_xy, void *stream);
typedef struct sgz_zero_crossing_state {
    double   state;
    double   threshold;
    uint64_t steady_clock;
    uint64_t cross_origin;
    uint64_t count;
    int32_t  armed;
    int32_t  _pad;
} sgz_zero_crossing_state;
/* d_a/d_b: DEVICE trigger-pair channels for this block; d_triggers: DEVICE uint64 [max_triggers] absolute
 * sample indices (the values peaks.push receives); *num_triggers and *st are updated on the host
 * (this call synchronises the stream: the trigger list is consumed by host logic). */
sgz_status sgz_scope_zero_crossing_device(sgz_zero_crossing_state *st, uint32_t osc_mode, const float *d_a,
                                          const float *d_b, size_t n, uint64_t *d_triggers,
                                          size_t max_triggers, size_t *num_triggers, void *stream);
/* peak envelope over `channels` windows of n samples; env (host, in/out, [channels]); returns gain */
sgz_status sgz_peak_filter_device(const float *d_ch, size_t stride, uint32_t channels, size_t n,
                                  uint32_t lanes, double coeff_pow, double *env, double *gain, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Oscilloscope real-time handle: replaces Oscilloscope::ProcessorShell::onStreamAudio (Source/Oscilloscope/Oscilloscope.h:293) ->
 * StreamState::audioEntryPoint (OscilloscopeDSP.inl:401-424) on the audio thread, and on the render thread
 * Oscilloscope::runPeakFilter (OscilloscopeDSP.inl:713-886) and drawWavePlot (OscilloscopeRendering.cpp:551-891, the Linear and
 * Lanczos branches) -> the (x, y, z) + colour stream PrimitiveDrawer::addVertex / addColour receive.
 * The trigger detector, TriggeringProcessor::processMutating's window selection (StreamPreprocessing.h:79-206), the back / front
 * rings (ChannelData.h) and the envelope all live in HBM; push stages the block -- an idle GPU starts on it at once, a busy one takes
 * everything that arrived meanwhile in ONE staged copy + ONE launch (the blocks keep their boundaries) --, and push never waits for
 * the GPU (SGZ_BUSY instead).  One producer thread (push), one consumer thread (everything else).
 * trigger mode Spectral (sgz_scope_analyse = calculateFundamentalPeriod + calculateTriggeringOffset,
 * OscilloscopeDSP.inl:62-308, on the device ring) and the per-sample frequency colouring of audioProcessing (:445-647: 3-band
 * Linkwitz-Riley split -> smoothed band energies -> RGB, kept in colour rings beside the audio rings and swapped with them).
 * The remaining modes too: EnvelopeHold (PeakHoldProcessor, StreamPreprocessing.h:270-310, inside the ingest kernel), Window
 * (sgz_scope_set_transport), customTrigger, and the None / Rectangular interpolations of drawWavePlot. */
typedef struct sgz_scope_config {
    double   sample_rate;
    double   window_size;        /* the window value (windowSize's transformed value): samples in SGZ_TIME_TIME (= state.effectiveWindowSize,
                                    fractions allowed), periods of the fundamental in SGZ_TIME_CYCLES, beat division in SGZ_TIME_BEATS */
    uint32_t num_channels;       /* even, 2..64                                                                  */
    uint32_t trigger_mode;       /* SGZ_TRIG_* (Window: see sgz_scope_set_transport)                             */
    uint32_t channel_mode;       /* SGZ_OSC_* (OscChannels): trigger mix, envelope mix                           */
    uint32_t envelope_mode;      /* SGZ_ENV_*: RMS runs in push (audioProcessing), PEAK_DECAY in sgz_scope_peak_filter */
    uint32_t interpolation;      /* SGZ_SUBSAMPLE_*: None = the Linear vertex list, drawn as GL_POINTS (dotSamples,
                                    OscilloscopeRendering.cpp:652-700); Rectangular = two vertices per sample (:746-789) */
    uint32_t max_block;          /* longest block push will be given (0: 8192)                                   */
    double   trigger_threshold;  /* content->triggerThreshold                                                    */
    double   trigger_channel;    /* content->triggeringChannel, 1-based (calculateTriggerIndices)                */
    double   envelope_window;    /* content->envelopeWindow normalised value = seconds             */
    uint8_t  colours[64][4];     /* per channel: filterStates.channels[c].defaultKey as RGBA8                    */
    /* Spectral triggering (all ignored in the other modes) */
    double   trigger_hysteresis;   /* content->triggerHysteresis, 0..1                                           */
    double   trigger_phase_offset; /* content->triggerPhaseOffset in degrees                                     */
    /* frequency colouring */
    uint32_t colour_by_frequency;  /* state.colourChannelsByFrequency: colours computed in push, per-vertex colours from the rings */
    float    frequency_colouring_blend;   /* content->frequencyColouringBlend, 0..1                              */
    double   colour_smoothing_ms;  /* content->colourSmoothing (transformed value, milliseconds)                 */
    float    band_colours[3][3];   /* content->lowColour / midColour / highColour as float r, g, b               */
    /* Spectral triggering on a frequency the user names (state.customTrigger / customTriggerFrequency, OscilloscopeDSP.inl:71-81) */
    uint32_t custom_trigger;
    double   custom_trigger_frequency;    /* Hz, in (0, sample_rate / 2)                                          */
    /* state.timeMode (Oscilloscope.cpp:258): SGZ_TIME_*.  handleFlagUpdates' window step (Oscilloscope.cpp:291-307) runs at the top of
     * every sgz_scope_analyse, which then works with that frame's effectiveWindowSize (sgz_scope_effective_window):
     *   TIME    window_size samples.
     *   CYCLES  window_size * cycleSamples + 1, cycleSamples of the PREVIOUS analyse (0 before the first: a window of 1 sample) --
     *           computed on the device from the state the Spectral kernel keeps.  Spectral trigger only (checkAndInformInvalidCombinations,
     *           OscilloscopeRendering.cpp:244-259); any other: SGZ_EINVAL.
     *   BEATS   max(128, sample_rate * (60 / (max(10, bpm) * window_size))), bpm from sgz_scope_set_tempo (0 until the first call).
     * CYCLES / BEATS: window_size > 0 and finite; the largest window the mode can reach (window_size * sample_rate / 5 + 1 -- the
     * fundamental's 5 Hz floor, or the custom trigger frequency if lower --, resp. the 10 BPM floor's) must respect the 2^26 ring bound.
     * With the Spectral trigger the ring is allocated once for that largest window, and a new window only moves the frame's ring_size
     * (nothing is cleared).  BEATS with another trigger: a frame whose window differs from the last one's does what
     * sgz_scope_configure with window_size = the new window does (setSettings' windowChanged; a changed ceil resizes and clears the
     * rings), from inside sgz_scope_analyse.  (The reference's resize -- cpl's setStorageRequirements -- is not in its tree: UNVERIFIED
     * vs cpl that it clears like this.) */
    uint32_t time_mode;
} sgz_scope_config;
/* Oscilloscope::triggerState after analyseAndSetupState's first two steps (Oscilloscope.h:176-196) */
typedef struct sgz_trigger_state {
    uint64_t record_index;         /* triggerState.record: the winning bin, its magnitude and its fractional offset */
    double   record_value, record_offset;
    double   fundamental;          /* Hz, >= 5 */
    double   cycle_samples;        /* sampleRate / fundamental (0 outside Spectral mode)                          */
    double   sample_offset;        /* samples                                                                      */
    double   phase;                /* radians, [0, tau)                                                            */
    uint64_t ring_size;            /* ChannelData::resizeAudioStorage's size for this frame: the ring drawWavePlot wraps in */
} sgz_trigger_state;
typedef struct sgz_scope sgz_scope;
sgz_status sgz_scope_create(const sgz_scope_config *cfg, sgz_scope **out);
void       sgz_scope_destroy(sgz_scope *s);
/* handleFlagUpdates -> TriggeringProcessor::setSettings (Oscilloscope.cpp:310).  A changed ceil(window) resizes (and clears) the rings;
 * whenever the rings are reallocated, the trigger's buffered samples start over at the next block, even if another configure with the
 * same ceil comes first. */
sgz_status sgz_scope_configure(sgz_scope *s, const sgz_scope_config *cfg);
/* onStreamAudio(ctx, float** buffer, numChannels, numSamples); the steady clock is the running count of pushed samples */
sgz_status sgz_scope_push(sgz_scope *s, const float *const *planar, uint32_t num_channels, uint32_t nsamples);
sgz_status sgz_scope_flush(sgz_scope *s);      /* as sgz_spectrum_flush */
/* MixGraphListener::deliver's routing (Source/Common/MixGraphListener.cpp:247-334), as sgz_spectrum_set_mix: destination channel d (of
 * num_channels) = the sum of the source channels c with matrix[d * num_sources + c] != 0, added in ascending c onto a row of 0.0f
 * (copyFromHead<true> into a cleared row: -0.0 becomes +0.0, NaN propagates); a destination with no source is silence.  push then takes
 * num_sources channels (1..64; fewer, as many or more than num_channels) and refuses any other count with SGZ_EINVAL.  The ingest
 * launch routes the staged sources itself: no extra launch, push still allocates nothing.  Consumer thread, like configure: every
 * block pushed before the call (staged, batched, parked or deferred) goes through the old routing; a concurrent push is refused with
 * SGZ_BUSY while the switch holds the handle, it never waits.  A NULL matrix, 0 or more than 64 sources: SGZ_EINVAL, the handle
 * unchanged.  configure returns the routing to the identity over num_channels. */
sgz_status sgz_scope_set_mix(sgz_scope *s, uint32_t num_sources, const uint8_t *matrix /*[num_channels][num_sources]*/);
/* Handle switch (consumer thread, between create / configure and the first push; the library reads no environment variable):
 *   SGZ_RT_OPT_DEFER_SUBMIT  0 (default): a pushed block goes to the GPU at once when nothing of the handle is in flight, otherwise it
 *       joins the open batch, which the next submission takes in ONE launch.  1: every block waits for a full batch or a reader
 *       (flush on read) -- every launch a multi-callback one.  Results are identical; the tests pin the batched paths down with it.
 *   SGZ_RT_OPT_PARK_PUSHES   0 (default).  1: every pushed block is parked in the handle's host FIFO -- where a block goes whose push finds the
 *       render thread submitting at that moment, or no staging slot free -- until the next read (flush on read covers the FIFO), push or
 *       flush hands it on.  Results are identical; the tests reproduce a stopped transport with it. */
#define SGZ_RT_OPT_DEFER_SUBMIT 3u
#define SGZ_RT_OPT_PARK_PUSHES 4u
sgz_status sgz_scope_set_option(sgz_scope *s, uint32_t option, uint64_t value);
/* TriggeringMode::Window draws the window at the host transport's phase: position_in_samples = cs.transportPosition =
 * playhead.getPositionInSamples() + numSamples of the newest block (OscilloscopeDSP.inl:706; OscilloscopeRendering.cpp:588-592,
 * :798-801).  Any thread, any time (one atomic store); ignored by the other modes. */
sgz_status sgz_scope_set_transport(sgz_scope *s, int64_t position_in_samples);
/* cs.bpm = playhead.getBPM() of the newest block (OscilloscopeDSP.inl:707), read by SGZ_TIME_BEATS at the next sgz_scope_analyse.
 * Any thread, any time (one atomic store); 0 before the first call (the reference's `double bpm {}`), which the formula floors to 10. */
sgz_status sgz_scope_set_tempo(sgz_scope *s, double bpm);
/* state.effectiveWindowSize of the current frame (the window the vertex calls draw: time divisions and cursor readouts need it);
 * before the first sgz_scope_analyse the mode's window with cycleSamples 0 and the tempo of the moment */
double     sgz_scope_effective_window(const sgz_scope *s);
/* handleFlagUpdates' window step on the host (Oscilloscope.cpp:293-307), no GPU: time_mode SGZ_TIME_*, value = window_size,
 * cycle_samples read by CYCLES, bpm by BEATS.  (Time: value; an unknown mode: value.) */
double     sgz_scope_time_window(uint32_t time_mode, double value, double sample_rate, double bpm, double cycle_samples);
/* runPeakFilter once per rendered frame: delta_time = openGLDeltaTime(), lanes = the SIMD width whose tail the reference drops
 * (8 = AVX); *auto_gain = state.autoGain (optional; reading it waits for the kernel) */
sgz_status sgz_scope_peak_filter(sgz_scope *s, double delta_time, uint32_t lanes, double *auto_gain);
/* envelopeGain of the RMS mode and the per-channel envelope states (either may be NULL) */
sgz_status sgz_scope_gains(sgz_scope *s, double *envelope_gain, float *envelopes /*num_channels*/);
/* Once per rendered frame, before sgz_scope_vertices: calculateFundamentalPeriod + calculateTriggeringOffset
 * (OscilloscopeDSP.inl:62-308) for the trigger evaluator (evaluator / channel as in sgz_scope_vertices).  Spectral mode: one kernel
 * (8192-point fp64 transform of the newest samples in LDS, the harmonic peak pick with hysteresis, the median of 8, the Goertzel
 * phase) on the device ring; the state is read back (this call waits) and kept for the vertex calls.  Other modes: cycle_samples = 0
 * and the mode's fixed sample_offset, no GPU work.  The Spectral ring keeps the most the reference can ask for
 * ((size_t)(0.5 + sampleRate / 5 + ceil(window)) samples, the 5 Hz floor) and every read wraps in `ring_size`, the size
 * resizeAudioStorage gives the reference's ring for this frame (ChannelData.h:107-128), counted back from the newest sample.
 * SGZ_TIME_CYCLES / BEATS: the frame's window is set first (see sgz_scope_config::time_mode); vertex calls and
 * sgz_scope_vertex_count use it until the next analyse. */
sgz_status sgz_scope_analyse(sgz_scope *s, uint32_t evaluator, uint32_t channel, sgz_trigger_state *out);
size_t     sgz_scope_vertex_count(const sgz_scope *s, const sgz_scope_view *view);
/* One evaluator's line strip.  evaluator: SGZ_OSC_LEFT / RIGHT (channel `channel` / `channel` + 1) or SGZ_OSC_MID / SIDE (0.5 (l +- r)
 * of the pair at `channel`); view->window_size is ignored (the stream's is used).  xyz: float3 per vertex, rgba: RGBA8 per vertex
 * (may be NULL); *count: in = capacity of the buffers in vertices, out = vertices written.  Lanczos below one pixel per sample
 * falls back to Linear like the reference (OscilloscopeRendering.cpp:575-578): x is then the sample index (sample space).
 * Host buffers that are pinned (hipHostMalloc / hipHostRegister) are written by the DMA engine directly; pageable ones go through a
 * pinned bounce buffer and a host copy (the same holds for sgz_vector_vertices / _all). */
sgz_status sgz_scope_vertices(sgz_scope *s, const sgz_scope_view *view, uint32_t evaluator, uint32_t channel, float *xyz,
                              uint8_t *rgba, uint32_t *count);
/* Several evaluators' line strips of one rendered frame (the reference draws them one after the other inside one paint,
 * OscilloscopeRendering.cpp drawWavePlot per channel): item k is sgz_scope_vertices(s, view, evaluators[k], channels[k], xyz[k],
 * rgba ? rgba[k] : NULL, &counts[k]), but the kernels are enqueued back to back and the call waits ONCE.  Same results, same buffer
 * rules; any failing item fails the call (counts[k] holds the required size where a buffer was too small). */
sgz_status sgz_scope_vertices_all(sgz_scope *s, const sgz_scope_view *view, uint32_t items, const uint32_t *evaluators, const uint32_t *channels,
                                  float *const *xyz, uint8_t *const *rgba, uint32_t *counts);
/* (the buffers of sgz_scope_vertices_all may also be DEVICE memory -- all of them --: the kernels then write HBM, one wait, nothing crosses PCIe) */
/* the hipStream_t the handle enqueues its work on (so that a host can order or time its own device work against the handle's) */
void      *sgz_scope_stream(sgz_scope *s);
/* The same stream into DEVICE buffers -- a mapped vertex buffer object, or memory from sgz_export_alloc that the display GPU's GL /
 * Vulkan imported -- without the D2H copy.  In place when the call returns. */
sgz_status sgz_scope_vertices_device(sgz_scope *s, const sgz_scope_view *view, uint32_t evaluator, uint32_t channel, float *d_xyz,
                                     uint8_t *d_rgba, uint32_t *count);
/* The dense stream: the frame's sample-space Linear strip reduced on the device to a minimum and a maximum vertex per column -- what a
 * host draws when the window holds many samples per pixel (pixelsPerSample < 1, where drawWavePlot itself falls back to Linear and
 * sgz_scope_vertices returns one vertex per sample).  The reference has no counterpart.
 * V[0 .. n) is the Linear strip of the current frame, exactly what sgz_scope_vertices writes for a view below one pixel per sample
 * (or under SGZ_SUBSAMPLE_LINEAR): V[i] = (i, sample, 0) + RGBA8, n = max(2, ceil(window)) + quantizedCycleSamples; it depends on
 * neither sgz_scope_config::interpolation nor a view.  cols = min(columns, n); column b holds the indices
 * ceil(b n / cols) <= i < ceil((b + 1) n / cols).  lo(b): the lowest index whose y equals the minimum of the column's non-NaN y
 * (IEEE `<`: -0 and +0 tie, ties go to the lowest index); hi(b) likewise for the maximum; both the column's first index when every y is
 * NaN.  The stream is 2 cols vertices: column b gives V[min(lo, hi)] then V[max(lo, hi)] (twice the same vertex when they are equal),
 * xyz and RGBA8 copied bit for bit -- a subsequence of V, drawn with V's matrix and primitive (x is the sample index).
 * 0 for a NULL handle or columns == 0. */
size_t     sgz_scope_dense_vertex_count(const sgz_scope *s, uint32_t columns);
/* One evaluator's dense strip; evaluator / channel / xyz / rgba (may be NULL) / *count and the rules for pinned and pageable host
 * buffers as sgz_scope_vertices.  SGZ_EINVAL (nothing written, the handle untouched): columns == 0, an evaluator or channel out of
 * range, NULL xyz or count, *count < the need (*count then holds it). */
sgz_status sgz_scope_dense_vertices(sgz_scope *s, uint32_t columns, uint32_t evaluator, uint32_t channel, float *xyz, uint8_t *rgba,
                                    uint32_t *count);
/* Several evaluators' dense strips of one frame, enqueued back to back, ONE wait; host or (all of them) DEVICE buffers, as
 * sgz_scope_vertices_all. */
sgz_status sgz_scope_dense_vertices_all(sgz_scope *s, uint32_t columns, uint32_t items, const uint32_t *evaluators, const uint32_t *channels,
                                        float *const *xyz, uint8_t *const *rgba, uint32_t *counts);
/* ... into DEVICE buffers, as sgz_scope_vertices_device.  In place when the call returns. */
sgz_status sgz_scope_dense_vertices_device(sgz_scope *s, uint32_t columns, uint32_t evaluator, uint32_t channel, float *d_xyz,
                                           uint8_t *d_rgba, uint32_t *count);
/* The same reduction as a stage call on rings in time order (d_ring / len / stride / channels as sgz_scope_lanczos_device): V is the
 * newest n samples, V[i] = (i, ring[(len - n + i) mod len]); d_xy: DEVICE float2 [channels][2 min(columns, n)].  Enqueued on
 * `stream`, no wait; scratch is allocated and freed in stream order.  len, n < 2^31. */
sgz_status sgz_scope_dense_device(const float *d_ring, size_t len, size_t stride, uint32_t channels, size_t n, uint32_t columns,
                                  float *d_xy, void *stream);
/* parity hooks: front buffer memory of one channel (begin()) + its write cursor; TriggeringProcessor counters
 * {frontOrigin, bufferedSamples, oldPeak, currentPeak, steadyClock, peaks.size(), isWorkingOnPeak, swaps} */
sgz_status sgz_scope_front(sgz_scope *s, uint32_t channel, float *out /*size*/, uint32_t *size, uint32_t *cursor);
/* the colour ring beside it: aux = 0 colourData, 1 auxColourData (Mid at even, Side at odd channels); RGBA8 words */
sgz_status sgz_scope_front_colours(sgz_scope *s, uint32_t channel, uint32_t aux, uint8_t *out /*4*size*/);
sgz_status sgz_scope_debug_state(sgz_scope *s, uint64_t out[8]);

/* ------------------------------------------------------------------------------------------------
 * Vectorscope: polar transform (drawPolarPlot, VectorscopeRendering.cpp:500-746), Lissajous plot (drawRectPlot, :444-497) and
 * the audio-thread one-pole filters (Processor::audioProcessing, Vectorscope.cpp:268-377).
 */
/* d_xyz: DEVICE float3 [pairs][n]; pair p uses channels 2p, 2p+1 of d_planar */
sgz_status sgz_vector_polar_device(const float *d_planar, size_t stride, uint32_t pairs, size_t n,
                                   uint32_t lanes, float *d_xyz, void *stream);
/* The Lissajous plot (drawRectPlot, VectorscopeRendering.cpp:444-497) of `pairs` pairs of d_planar (DEVICE, oldest sample first;
 * pair p = channels 2p, 2p+1 at d_planar + c * stride, stride >= n, n <= 2^31): vertex v of pair p = (right, left, v * sampleFade - 1)
 * with sampleFade = 1 / max(1, n - 1); d_xyz: DEVICE float3 [pairs][n].  d_rgb (DEVICE float3 [pairs][n], or NULL): colours[p] * fade
 * (fade = v * sampleFade) when `fade` is set, colours[p] otherwise; colours: HOST float [pairs][3], needed only when d_rgb != NULL. */
sgz_status sgz_vector_lissajous_device(const float *d_planar, size_t stride, uint32_t pairs, size_t n, uint32_t fade,
                                       const float *colours, float *d_xyz, float *d_rgb, void *stream);
typedef struct sgz_vector_filters { float env[2]; float balance[2][2]; float phase[2]; } sgz_vector_filters;
sgz_status sgz_vector_audio_processing_device(sgz_vector_filters *f, const float *d_left, const float *d_right,
                                              size_t n, uint32_t lanes, float envelope_coeff, float stereo_coeff,
                                              float second_speed, int env_mode, float *gain_out, void *stream);

/* Vectorscope real-time handle: replaces VectorScope::Processor::onStreamAudio -> audioProcessing (Source/Vectorscope/Vectorscope.h:141,
 * Vectorscope.cpp:268-392) and the cpl::AudioStream history the renderer reads, and on the render thread VectorScope::runPeakFilter
 * (VectorscopeRendering.cpp:826-889), drawPolarPlot (:500-746) or drawRectPlot (:444-497) for every channel pair and drawStereoMeters
 * (:748-823) -> the (x, y, z) + (r, g, b) stream PrimitiveDrawer::addVertex / addColour receive.  History ring, filter states and gain live in HBM; push = (batched, as sgz_scope_push) one staged copy + one
 * launch and never waits for the GPU (SGZ_BUSY instead).  One producer thread (push), one consumer thread (everything else). */
typedef struct sgz_vector_config {
    double   sample_rate;
    uint32_t num_channels;       /* even, 2..64; pair p = channels 2p, 2p+1; the filters listen to channels 0, 1       */
    uint32_t window_size;        /* audio history in samples = vertices per pair                                       */
    uint32_t envelope_mode;      /* SGZ_ENV_*: RMS updates the gain in push, PEAK_DECAY in sgz_vector_peak_filter      */
    uint32_t lanes;              /* SIMD width of the reference build (8 = AVX): tails it drops / handles in scalar code */
    uint32_t fade_history;       /* state.fadeHistory: colours fade with age (VectorscopeRendering.cpp:637-746)         */
    uint32_t max_block;          /* longest block push will be given (0: 8192)                                          */
    double   envelope_window;    /* seconds (content->envelopeWindow normalised)                                        */
    double   stereo_window;      /* seconds (content->stereoWindow normalised)                                          */
    float    colours[32][3];     /* per pair: the waveform colour as getFloatRed / Green / Blue                         */
} sgz_vector_config;
typedef struct sgz_vector sgz_vector;
sgz_status sgz_vector_create(const sgz_vector_config *cfg, sgz_vector **out);
void       sgz_vector_destroy(sgz_vector *s);
sgz_status sgz_vector_configure(sgz_vector *s, const sgz_vector_config *cfg);
sgz_status sgz_vector_push(sgz_vector *s, const float *const *planar, uint32_t num_channels, uint32_t nsamples);
sgz_status sgz_vector_flush(sgz_vector *s);    /* as sgz_spectrum_flush */
/* the host graph's routing, exactly as sgz_scope_set_mix (Vectorscope.h:141's onStreamAudio receives the routed stream) */
sgz_status sgz_vector_set_mix(sgz_vector *s, uint32_t num_sources, const uint8_t *matrix /*[num_channels][num_sources]*/);
sgz_status sgz_vector_set_option(sgz_vector *s, uint32_t option, uint64_t value);   /* SGZ_RT_OPT_DEFER_SUBMIT / SGZ_RT_OPT_PARK_PUSHES, as sgz_scope_set_option */
sgz_status sgz_vector_peak_filter(sgz_vector *s, double delta_time, double *envelope_gain /*optional: reading it waits*/);
sgz_status sgz_vector_filters_get(sgz_vector *s, sgz_vector_filters *filters, double *envelope_gain);
/* xyz: float3 [window_size], rgb: float3 [window_size] or NULL; *count: in = capacity in vertices, out = window_size.  Vertex
 * order = the reference's: the older section of the ring ([cursor, size)) first, then [0, cursor). */
sgz_status sgz_vector_vertices(sgz_vector *s, uint32_t pair, float *xyz, float *rgb, uint32_t *count);
sgz_status sgz_vector_vertices_device(sgz_vector *s, uint32_t pair, float *d_xyz, float *d_rgb, uint32_t *count);   /* DEVICE buffers */
/* every pair's stream with ONE wait for the GPU (the render thread draws all pairs of a frame, VectorscopeRendering.cpp:253-276):
 * xyz / rgb: float3 [num_channels / 2][window_size]; *count: in = capacity PER PAIR, out = window_size */
sgz_status sgz_vector_vertices_all(sgz_vector *s, float *xyz, float *rgb, uint32_t *count);
/* (xyz / rgb of sgz_vector_vertices_all may also be DEVICE memory: the vertices stay in HBM) */
void      *sgz_vector_stream(sgz_vector *s);       /* as sgz_scope_stream */
/* parity hook: history ring memory of one channel + the write cursor */
sgz_status sgz_vector_history(sgz_vector *s, uint32_t channel, float *out /*window_size*/, uint32_t *size, uint32_t *cursor);
/* The Lissajous plot (state.isPolar off: drawRectPlot, VectorscopeRendering.cpp:444-497), the polar calls' twins: same buffers, same
 * count and wait rules, same vertex order (the older section of the ring first).  Vertex v of pair p = (right, left, fade - 1) with
 * fade = (float) v * sampleFade, sampleFade = 1 / max(1, window_size - 1) -- x, y are the samples as stored (NaN, inf, -0 included).
 * rgb = colours[p] * fade with fade_history, colours[p] without.  The strip's alpha is not in the stream (it is constant per strip):
 * with fade_history the reference draws it as getFloatGreen() -- colours[p][1] (quirk Q9) --, without it the colour's own alpha,
 * which the host's adapter supplies.  Gain, rotation and the primitive type (fillPath) are GL state, as for the polar stream.
 * These reads leave the polar stream's fade-ramp work alone. */
sgz_status sgz_vector_lissajous_vertices(sgz_vector *s, uint32_t pair, float *xyz, float *rgb, uint32_t *count);
sgz_status sgz_vector_lissajous_vertices_all(sgz_vector *s, float *xyz, float *rgb, uint32_t *count);   /* one launch, one wait; host or DEVICE */
sgz_status sgz_vector_lissajous_vertices_device(sgz_vector *s, uint32_t pair, float *d_xyz, float *d_rgb, uint32_t *count);   /* DEVICE buffers */
/* drawStereoMeters (VectorscopeRendering.cpp:748-823): the four indicator positions along their meters (0 .. 1 for the non-negative balance states push produces), by filter index k:
 * balance[k] = atanf(balance[k][1] / balance[k][0]) / (pi_f * 0.5f), 0.5f where that is not normal; stereo[k] = phase[k] * 0.5f + 0.5f.
 * Reference quirk: drawStereoMeters draws index 0 as the thin full-brightness "quick" indicator, while FilterStates (Vectorscope.h:99-105)
 * names index 0 Slow -- the fields keep the index, the host draws [0] as the quick and [1] as the slow indicator to match the plugin.
 * (A struct tag without a typedef, as struct stat beside stat(): the reading function has the same name.) */
struct sgz_vector_meters { float balance[2]; float stereo[2]; };
sgz_status sgz_vector_meters_from_filters(const sgz_vector_filters *f, struct sgz_vector_meters *out);   /* host arithmetic only, no GPU */
sgz_status sgz_vector_meters(sgz_vector *s, struct sgz_vector_meters *out);      /* = sgz_vector_filters_get + the above (flushes, waits) */

#ifdef __cplusplus
}
#endif
#endif /* SGZ_H */
