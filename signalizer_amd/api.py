"""Host-side binding of libsgz.so (include/sgz.h) for Python callers, tests and bench.py.

A thin ctypes layer over the C ABI: `Plan` (the TransformConstant mirror and the batch / stage entry points),
`render_spectrogram` (host buffers), and the argtypes of the real-time handles (sgz_spectrum_* / sgz_scope_* / sgz_vector_*:
onStreamAudio in, columns / vertices out), which the tests drive directly.
PyTorch is used only as the device allocator / stream provider.  No CPU fallback: if libsgz.so is
missing or no GPU is visible, compute calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np

from . import build as _build

NUM_SPEC_COLOURS = 5
NUM_GRAPHS = 2

SGZ_OK, SGZ_EMPTY, SGZ_SKIPPED_FRAME, SGZ_BUSY = 0, 1, 2, 3
SGZ_EINVAL, SGZ_EHIP, SGZ_ENOMEM, SGZ_EUNSUPPORTED = -1, -2, -3, -4


class SgzError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"sgz status {status}: {msg}")
        self.status = status


class SpectrumConfig(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_float), ("window_size", C.c_uint32), ("hop", C.c_uint32), ("axis_points", C.c_uint32),
        ("channel_mode", C.c_uint32), ("bin_interp", C.c_uint32), ("view_scaling", C.c_uint32),
        ("window_type", C.c_uint32), ("window_symmetry", C.c_uint32), ("num_pairs", C.c_uint32),
        ("window_alpha", C.c_double), ("window_beta", C.c_double), ("view_left", C.c_double),
        ("view_right", C.c_double), ("min_log_freq", C.c_double), ("low_db", C.c_double), ("high_db", C.c_double),
        ("clip_db", C.c_double), ("slope_a", C.c_double), ("slope_b", C.c_double),
        ("pole", C.c_float * NUM_GRAPHS), ("colours", (C.c_uint8 * 3) * (NUM_SPEC_COLOURS + 1)),
        ("_pad", C.c_uint8 * 2), ("ratios", C.c_double * NUM_SPEC_COLOURS),
        ("algorithm", C.c_uint32), ("free_q", C.c_uint32), ("display_mode", C.c_uint32), ("_reserved", C.c_uint32),
    ]


class Peak(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("peak_offset", "peak_fraction", "peak_frequency", "peak_dbs", "alpha", "beta", "gamma", "phi")]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LinePeak(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("peak_offset", "peak_frequency", "peak_deviance", "peak_fraction_y", "peak_dbs", "peak_slope")]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Timing(C.Structure):
    _fields_ = [("h2d_ms", C.c_double), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("frames", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PcmTiming(C.Structure):
    _fields_ = [("wall_ms", C.c_double), ("h2d_ms", C.c_double), ("convert_ms", C.c_double), ("render_ms", C.c_double), ("d2h_ms", C.c_double),
                ("frames", C.c_uint64), ("chunks", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# sgz_pcm_to_planar_device / sgz_pcm_stream: the interleaved sample formats (SGZ_PCM_*) and their bytes per sample
PCM_F32, PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F64, PCM_END = range(7)
PCM_SAMPLE_BYTES = {PCM_F32: 4, PCM_U8: 1, PCM_S16: 2, PCM_S24: 3, PCM_S32: 4, PCM_F64: 8}


class ScopeView(C.Structure):
    _fields_ = [("window_size", C.c_double), ("left", C.c_double), ("right", C.c_double),
                ("rendering_scale", C.c_double), ("width", C.c_uint32), ("_pad", C.c_uint32)]


class ZeroCrossingState(C.Structure):
    _fields_ = [("state", C.c_double), ("threshold", C.c_double), ("steady_clock", C.c_uint64),
                ("cross_origin", C.c_uint64), ("count", C.c_uint64), ("armed", C.c_int32), ("_pad", C.c_int32)]


class ScopeConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("window_size", C.c_double), ("num_channels", C.c_uint32), ("trigger_mode", C.c_uint32),
                ("channel_mode", C.c_uint32), ("envelope_mode", C.c_uint32), ("interpolation", C.c_uint32), ("max_block", C.c_uint32),
                ("trigger_threshold", C.c_double), ("trigger_channel", C.c_double), ("envelope_window", C.c_double),
                ("colours", (C.c_uint8 * 4) * 64),
                ("trigger_hysteresis", C.c_double), ("trigger_phase_offset", C.c_double), ("colour_by_frequency", C.c_uint32),
                ("frequency_colouring_blend", C.c_float), ("colour_smoothing_ms", C.c_double), ("band_colours", (C.c_float * 3) * 3),
                ("custom_trigger", C.c_uint32), ("custom_trigger_frequency", C.c_double), ("time_mode", C.c_uint32)]


# OscilloscopeContent::TimeMode (sgz_scope_config::time_mode): what window_size counts -- samples, periods, beat division
TIME_TIME, TIME_CYCLES, TIME_BEATS = 0, 1, 2


class TriggerState(C.Structure):
    _fields_ = [("record_index", C.c_uint64), ("record_value", C.c_double), ("record_offset", C.c_double), ("fundamental", C.c_double),
                ("cycle_samples", C.c_double), ("sample_offset", C.c_double), ("phase", C.c_double), ("ring_size", C.c_uint64)]


class VectorFilters(C.Structure):
    _fields_ = [("env", C.c_float * 2), ("balance", (C.c_float * 2) * 2), ("phase", C.c_float * 2)]


class VectorMeters(C.Structure):
    _fields_ = [("balance", C.c_float * 2), ("stereo", C.c_float * 2)]


class LevelReading(C.Structure):
    _fields_ = [("rms", C.c_double * 2), ("rms_db", C.c_double * 2), ("dc", C.c_double * 2), ("correlation", C.c_double)]


# sgz_level_record: one per (column, pair) of the level lane; 80 bytes, little-endian
LEVEL_DTYPE = np.dtype([("sumsq", "<u8", (2, 2)), ("cross", "<u8", (2,)), ("sum", "<i8", (2,)), ("count", "<u4", (2,)), ("overs", "<u4", (2,))])
assert LEVEL_DTYPE.itemsize == 80

# sgz_truepeak_record: one per (column, channel) of the true-peak lane, 16 bytes; sgz_truepeak_carry: one per channel, 64 bytes
TRUEPEAK_DTYPE = np.dtype([("peak", "<u8"), ("count", "<u4"), ("overs", "<u4")])
TRUEPEAK_CARRY_DTYPE = np.dtype([("open", TRUEPEAK_DTYPE), ("hist", "<i4", (11,)), ("reserved", "<u4")])
assert TRUEPEAK_DTYPE.itemsize == 16 and TRUEPEAK_CARRY_DTYPE.itemsize == 64

# sgz_loudness_record: one per (column, channel) of the loudness lane, 32 bytes (sumsq: unsigned 128-bit, low word first)
LOUDNESS_DTYPE = np.dtype([("sumsq", "<u8", (2,)), ("count", "<u4"), ("reserved", "<u4", (3,))])
assert LOUDNESS_DTYPE.itemsize == 32


# sgz_field_record: one per (column, pair) of the stereo-field lane, 528 bytes: 32 sectors of stereo direction
FIELD_SECTORS = 32
FIELD_DTYPE = np.dtype([("radius", "<u8", (FIELD_SECTORS,)), ("count", "<u4", (FIELD_SECTORS,)), ("peak", "<u4", (FIELD_SECTORS,)),
                        ("silent", "<u4"), ("skipped", "<u4"), ("reserved", "<u8")])
assert FIELD_DTYPE.itemsize == 528


class FieldReading(C.Structure):
    _fields_ = [("share", C.c_double * FIELD_SECTORS), ("mean", C.c_double * FIELD_SECTORS), ("peak", C.c_double * FIELD_SECTORS),
                ("direction", C.c_double), ("spread", C.c_double), ("silent_share", C.c_double)]


# sgz_hist_record: one per (column, channel) of the histogram lane, 448 bytes = 112 words: 106 buckets of |v| and six fields
HIST_BUCKETS = 106
HIST_DTYPE = np.dtype([("bucket", "<u4", (HIST_BUCKETS,)), ("count", "<u4"), ("skipped", "<u4"), ("negative", "<u4"), ("peak", "<u4"),
                       ("bits_or", "<u4"), ("bits_and", "<u4")])
assert HIST_DTYPE.itemsize == 448


class HistReading(C.Structure):
    _fields_ = [("zero_share", C.c_double), ("negative_share", C.c_double), ("peak", C.c_double), ("peak_db", C.c_double),
                ("median_db", C.c_double), ("toggling", C.c_uint32), ("effective_bits", C.c_uint32)]


# sgz_run_record: one per (column, channel) of the run lane, 96 bytes = 24 words: of[k] for the predicates hot, quiet, flat;
# sgz_run_carry: one per channel, 112 bytes (RUN_NAN in prev: an invalid sample, or none)
RUN_HOT, RUN_QUIET, RUN_FLAT = 0, 1, 2
RUN_NAN = -2**31
RUN_OF_DTYPE = np.dtype([("count", "<u4"), ("runs", "<u4"), ("longest", "<u4"), ("at", "<u4"), ("head", "<u4"), ("tail", "<u4")])
RUN_DTYPE = np.dtype([("len", "<u4"), ("skipped", "<u4"), ("crossings", "<u4"), ("reserved0", "<u4"), ("of", RUN_OF_DTYPE, (3,)),
                      ("reserved", "<u4", (2,))])
RUN_CARRY_DTYPE = np.dtype([("open", RUN_DTYPE), ("prev", "<i4", (2,)), ("reserved", "<u4", (2,))])
assert RUN_DTYPE.itemsize == 96 and RUN_CARRY_DTYPE.itemsize == 112


class RunParams(C.Structure):
    _fields_ = [("hot", C.c_uint32), ("quiet", C.c_uint32)]


class RunReading(C.Structure):
    _fields_ = [("share", C.c_double * 3), ("longest_seconds", C.c_double * 3), ("at_seconds", C.c_double * 3), ("crossing_hz", C.c_double)]


class LoudnessFilter(C.Structure):
    _fields_ = [("b", (C.c_double * 3) * 2), ("a", (C.c_double * 2) * 2), ("W", C.c_uint32), ("L", C.c_uint32)]


assert C.sizeof(LoudnessFilter) == 88

# sgz_band_record: one per (column, channel) of the band lane, 64 bytes (sumsq[band]: unsigned 128-bit, low word first; low, mid, high)
BAND_DTYPE = np.dtype([("sumsq", "<u8", (3, 2)), ("count", "<u4"), ("reserved", "<u4", (3,))])
assert BAND_DTYPE.itemsize == 64


class BandFilter(C.Structure):
    _fields_ = [("c", (C.c_double * 5) * 4), ("W", C.c_uint32), ("L", C.c_uint32)]


assert C.sizeof(BandFilter) == 168


class LineGraphStyle(C.Structure):
    _fields_ = [("colour_one", (C.c_uint8 * 4) * NUM_GRAPHS), ("colour_two", (C.c_uint8 * 4) * NUM_GRAPHS), ("flood_alpha", C.c_float),
                ("primitive_size", C.c_float), ("rendering_scale", C.c_double)]


class LineGraphDraw(C.Structure):
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("primitive", C.c_uint32), ("pair", C.c_uint32), ("graph", C.c_uint32),
                ("side", C.c_uint32), ("rgba", C.c_uint8 * 4), ("line_width", C.c_float)]


# sgz_line_graph_draw as a numpy record (line_graph_draws' result)
LINE_GRAPH_DRAW_DTYPE = np.dtype([("first", np.uint32), ("count", np.uint32), ("primitive", np.uint32), ("pair", np.uint32),
                                  ("graph", np.uint32), ("side", np.uint32), ("rgba", np.uint8, (4,)), ("line_width", np.float32)])
PRIM_LINES, PRIM_LINE_STRIP = 0x0001, 0x0003
SIDE_LEFT, SIDE_RIGHT = 0, 1


class VectorConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("num_channels", C.c_uint32), ("window_size", C.c_uint32), ("envelope_mode", C.c_uint32),
                ("lanes", C.c_uint32), ("fade_history", C.c_uint32), ("max_block", C.c_uint32), ("envelope_window", C.c_double),
                ("stereo_window", C.c_double), ("colours", (C.c_float * 3) * 32)]


def config_from_dict(d: dict) -> SpectrumConfig:
    c = SpectrumConfig()
    for k, v in d.items():
        if k == "pole":
            for i in range(NUM_GRAPHS):
                c.pole[i] = v[i]
        elif k == "colours":
            for i in range(NUM_SPEC_COLOURS + 1):
                for j in range(3):
                    c.colours[i][j] = int(v[i][j])
        elif k == "ratios":
            for i in range(NUM_SPEC_COLOURS):
                c.ratios[i] = float(v[i])
        else:
            setattr(c, k, v)
    return c


_lib = None
LIB_PATH = _build.LIB

# every symbol include/sgz.h declares (tests check that the library exports all of them)
EXPORTS = [
    "sgz_last_error", "sgz_abi_version", "sgz_device_count", "sgz_set_device",
    "sgz_plan_create", "sgz_plan_destroy", "sgz_plan_upload", "sgz_plan_transform_size",
    "sgz_plan_window_scale", "sgz_plan_break_pixel", "sgz_plan_path", "sgz_plan_dc_pixels", "sgz_plan_get_window",
    "sgz_plan_get_mapped_frequencies", "sgz_plan_get_slope_map", "sgz_plan_get_colour_ratios",
    "sgz_plan_get_colour_table", "sgz_rotate_hue_rgb8", "sgz_num_frames", "sgz_plan_num_frames", "sgz_plan_get_resonator", "sgz_plan_reset_resonator",
    "sgz_render_queue_create", "sgz_render_queue_destroy", "sgz_render_queue_submit", "sgz_render_queue_wait", "sgz_render_queue_join", "sgz_render_queue_set_option", "sgz_render_queue_distinct_lanes",
    "sgz_spectrogram_render_device", "sgz_spectrogram_render", "sgz_stage_bins", "sgz_stage_mapped", "sgz_stage_mapped_dominant", "sgz_stage_nyquist", "sgz_plan_set_option",
    "sgz_stage_map_from_bins", "sgz_stage_track_peak", "sgz_spectrum_track_peak", "sgz_track_peak_lines", "sgz_spectrum_track_peak_lines", "sgz_stage_decay_colour", "sgz_stage_decay_scan", "sgz_stage_decay_emit", "sgz_stage_logf", "sgz_stage_finish_pixel", "sgz_decay_fold_carry", "sgz_comm_unique_id", "sgz_comm_create", "sgz_comm_destroy", "sgz_shard_layout", "sgz_spectrogram_render_sharded_on",
    "sgz_spectrogram_render_sharded", "sgz_peer_group_create", "sgz_peer_group_destroy", "sgz_peer_transport", "sgz_peer_transport_release",
    "sgz_spectrum_create", "sgz_spectrum_destroy", "sgz_spectrum_configure", "sgz_spectrum_push",
    "sgz_spectrum_pop_column", "sgz_spectrum_line_results", "sgz_spectrum_clear_state", "sgz_spectrum_set_mix",
    "sgz_spectrogram_render_host", "sgz_spectrum_stats", "sgz_spectrum_history", "sgz_spectrum_bind_image", "sgz_spectrum_create_image", "sgz_spectrum_bind_gl_buffer",
    "sgz_spectrum_flush_columns", "sgz_spectrum_render_lines", "sgz_spectrum_set_option",
    "sgz_scope_create", "sgz_scope_destroy", "sgz_scope_configure", "sgz_scope_set_option", "sgz_vector_set_option", "sgz_scope_stream", "sgz_vector_stream", "sgz_scope_push", "sgz_scope_peak_filter", "sgz_scope_gains",
    "sgz_scope_vertex_count", "sgz_scope_vertices", "sgz_scope_vertices_all", "sgz_scope_front", "sgz_scope_debug_state", "sgz_scope_analyse",
    "sgz_scope_front_colours", "sgz_scope_vertices_device", "sgz_vector_vertices_device", "sgz_export_alloc", "sgz_export_free",
    "sgz_vector_create", "sgz_vector_destroy", "sgz_vector_configure", "sgz_vector_push", "sgz_vector_peak_filter",
    "sgz_vector_filters_get", "sgz_vector_vertices", "sgz_vector_vertices_all", "sgz_spectrum_backlog", "sgz_spectrum_stream", "sgz_spectrum_flush", "sgz_scope_flush", "sgz_scope_set_transport", "sgz_vector_flush", "sgz_vector_history",
    "sgz_scope_num_points", "sgz_scope_lanczos_device", "sgz_scope_zero_crossing_device",
    "sgz_peak_filter_device", "sgz_vector_polar_device", "sgz_vector_audio_processing_device",
    "sgz_vector_lissajous_vertices", "sgz_vector_lissajous_vertices_all", "sgz_vector_lissajous_vertices_device", "sgz_vector_lissajous_device",
    "sgz_vector_meters_from_filters", "sgz_vector_meters",
    "sgz_line_graph_vertex_count", "sgz_line_graph_draws", "sgz_line_graph_vertices_device", "sgz_spectrum_render_line_vertices",
    "sgz_spectrum_set_view", "sgz_view_translation_rows", "sgz_view_translate_device",
    "sgz_spectrum_resize", "sgz_image_resize_rows", "sgz_image_resize_columns", "sgz_image_resize_device",
    "sgz_spectrum_update", "sgz_spectrum_update_effects", "sgz_ring_resize_device",
    "sgz_scope_set_mix", "sgz_vector_set_mix",
    "sgz_scope_set_tempo", "sgz_scope_effective_window", "sgz_scope_time_window",
    "sgz_spectrum_set_pacing", "sgz_spectrum_set_frozen", "sgz_spectrum_render_columns", "sgz_spectrum_present", "sgz_frame_pacing_step",
    "sgz_columns_to_image_device", "sgz_image_unroll_device",
    "sgz_scope_dense_vertex_count", "sgz_scope_dense_vertices", "sgz_scope_dense_vertices_all", "sgz_scope_dense_vertices_device",
    "sgz_scope_dense_device",
    "sgz_pcm_sample_bytes", "sgz_pcm_to_planar_device", "sgz_stream_step", "sgz_pcm_stream_create", "sgz_pcm_stream_destroy",
    "sgz_pcm_stream_frames_for", "sgz_pcm_stream_feed", "sgz_pcm_stream_reset", "sgz_spectrogram_render_pcm",
    "sgz_stage_track_peaks", "sgz_stage_track_peaks_lines", "sgz_spectrogram_track_device", "sgz_spectrogram_track_host",
    "sgz_overview_step", "sgz_stage_overview", "sgz_spectrogram_overview_device", "sgz_spectrogram_overview_host",
    "sgz_overview_view_columns", "sgz_stage_overview_view", "sgz_overview_view_host",
    "sgz_pcm_stream_feed_overview", "sgz_pcm_stream_columns_for", "sgz_pcm_stream_open_frames", "sgz_spectrogram_overview_pcm",
    "sgz_pcm_stream_set_option",
    "sgz_stage_overview_stats", "sgz_spectrogram_overview_stats_device", "sgz_spectrogram_overview_stats_host", "sgz_stage_overview_stats_view",
    "sgz_overview_stats_view_host", "sgz_overview_stats_fold", "sgz_overview_stats_readout", "sgz_pcm_stream_feed_overview_stats",
    "sgz_spectrogram_overview_stats_pcm",
    "sgz_stage_overview_power", "sgz_spectrogram_overview_power_device", "sgz_spectrogram_overview_power_host", "sgz_stage_overview_power_view",
    "sgz_overview_power_view_host", "sgz_overview_power_quantise", "sgz_overview_power_fold", "sgz_overview_power_readout",
    "sgz_overview_power_levels", "sgz_pcm_stream_feed_overview_power", "sgz_spectrogram_overview_power_pcm",
    "sgz_plan_set_cross_edges", "sgz_stage_overview_cross", "sgz_spectrogram_overview_cross_device", "sgz_spectrogram_overview_cross_host",
    "sgz_overview_cross_quantise", "sgz_overview_cross_fold", "sgz_overview_cross_readout", "sgz_overview_cross_unit", "sgz_cross_edges_octave",
    "sgz_pcm_stream_set_cross_edges", "sgz_pcm_stream_feed_overview_cross", "sgz_spectrogram_overview_cross_pcm",
    "sgz_stage_overview_flux", "sgz_spectrogram_overview_flux_device", "sgz_spectrogram_overview_flux_host", "sgz_overview_flux_quantise",
    "sgz_overview_flux_fold", "sgz_overview_flux_readout", "sgz_overview_flux_hz", "sgz_pcm_stream_feed_overview_flux",
    "sgz_spectrogram_overview_flux_pcm",
    "sgz_stage_overview_pct", "sgz_spectrogram_overview_pct_device", "sgz_spectrogram_overview_pct_host", "sgz_overview_pct_bucket",
    "sgz_overview_pct_fold", "sgz_overview_pct_readout", "sgz_pcm_stream_feed_overview_pct", "sgz_spectrogram_overview_pct_pcm",
    "sgz_stage_wave_columns", "sgz_wave_columns_limits", "sgz_pcm_stream_set_waveform", "sgz_pcm_stream_waveform_for",
    "sgz_pcm_stream_waveform_state", "sgz_pcm_stream_flush_waveform",
    "sgz_track_peak_values", "sgz_stage_track_peaks_values", "sgz_pcm_stream_set_track", "sgz_pcm_stream_track_for", "sgz_pcm_stream_track_state",
    "sgz_stage_level_columns", "sgz_level_columns_limits", "sgz_pcm_stream_set_level", "sgz_pcm_stream_level_for", "sgz_pcm_stream_level_state",
    "sgz_pcm_stream_flush_level", "sgz_level_fold", "sgz_level_readout",
    "sgz_stage_truepeak_columns", "sgz_truepeak_columns_limits", "sgz_truepeak_taps", "sgz_truepeak_fold", "sgz_truepeak_readout",
    "sgz_pcm_stream_set_truepeak", "sgz_pcm_stream_truepeak_for", "sgz_pcm_stream_truepeak_state", "sgz_pcm_stream_flush_truepeak",
    "sgz_stage_loudness_columns", "sgz_loudness_columns_limits", "sgz_loudness_filter_for_rate", "sgz_loudness_taps", "sgz_loudness_fold",
    "sgz_loudness_readout", "sgz_loudness_integrated",
    "sgz_pcm_stream_set_loudness", "sgz_pcm_stream_loudness_for", "sgz_pcm_stream_loudness_state", "sgz_pcm_stream_flush_loudness",
    "sgz_stage_field_columns", "sgz_field_columns_limits", "sgz_field_boundaries", "sgz_field_fold", "sgz_field_readout",
    "sgz_pcm_stream_set_field", "sgz_pcm_stream_field_for", "sgz_pcm_stream_field_state", "sgz_pcm_stream_flush_field",
    "sgz_stage_band_columns", "sgz_band_columns_limits", "sgz_band_filter_for_rate", "sgz_band_taps", "sgz_band_fold", "sgz_band_readout",
    "sgz_band_colours", "sgz_pcm_stream_set_band", "sgz_pcm_stream_band_for", "sgz_pcm_stream_band_state", "sgz_pcm_stream_flush_band",
    "sgz_stage_hist_columns", "sgz_hist_columns_limits", "sgz_hist_edges", "sgz_hist_fold", "sgz_hist_percentile", "sgz_hist_readout",
    "sgz_pcm_stream_set_hist", "sgz_pcm_stream_hist_for", "sgz_pcm_stream_hist_state", "sgz_pcm_stream_flush_hist",
    "sgz_stage_run_columns", "sgz_run_columns_limits", "sgz_run_params_default", "sgz_run_fold", "sgz_run_readout",
    "sgz_pcm_stream_set_run", "sgz_pcm_stream_run_for", "sgz_pcm_stream_run_state", "sgz_pcm_stream_flush_run",
]


def lib() -> C.CDLL:
    """Load libsgz.so (building it with hipcc if the in-tree .so is missing or stale)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SGZ_LIB", LIB_PATH)          # (SGZ_LIB: another build of the library, for A/B timing on one box: tools/ab.sh)
    if not os.path.exists(path):
        _build.build()
    # PyTorch-ROCm bundles its own HIP/HSA runtime: if torch is going to share this process it must be
    # loaded first so that libsgz.so binds to the same runtime instance (two runtimes cannot both own the GPU).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    fp, bp, rp = C.POINTER(LoudnessFilter), C.POINTER(BandFilter), C.POINTER(RunParams)
    L.sgz_last_error.restype = C.c_char_p
    L.sgz_plan_create.argtypes = [C.POINTER(SpectrumConfig), C.POINTER(vp)]
    L.sgz_plan_destroy.argtypes = [vp]
    L.sgz_plan_destroy.restype = None
    L.sgz_plan_upload.argtypes = [vp]
    L.sgz_render_queue_create.argtypes = [C.POINTER(SpectrumConfig), u32, C.POINTER(vp)]
    L.sgz_render_queue_destroy.argtypes = [vp]
    L.sgz_render_queue_destroy.restype = None
    L.sgz_render_queue_submit.argtypes = [vp, vp, sz, sz, vp, vp, C.POINTER(C.c_uint64)]
    L.sgz_render_queue_wait.argtypes = [vp, C.c_uint64]
    L.sgz_render_queue_join.argtypes = [vp, vp]
    L.sgz_render_queue_set_option.argtypes = [vp, u32, u32]
    L.sgz_render_queue_distinct_lanes.argtypes = [vp]
    L.sgz_render_queue_distinct_lanes.restype = u32
    L.sgz_plan_transform_size.argtypes = [vp]
    L.sgz_plan_transform_size.restype = u32
    L.sgz_plan_window_scale.argtypes = [vp]
    L.sgz_plan_window_scale.restype = C.c_double
    L.sgz_plan_break_pixel.argtypes = [vp]
    L.sgz_plan_break_pixel.restype = u32
    L.sgz_plan_path.argtypes = [vp]
    L.sgz_plan_path.restype = u32
    L.sgz_plan_dc_pixels.argtypes = [vp, vp, u32]
    L.sgz_plan_dc_pixels.restype = u32
    for f in ("sgz_plan_get_window", "sgz_plan_get_mapped_frequencies", "sgz_plan_get_slope_map",
              "sgz_plan_get_colour_ratios"):
        getattr(L, f).argtypes = [vp, vp]
    L.sgz_plan_get_colour_table.argtypes = [vp, u32, vp]
    L.sgz_rotate_hue_rgb8.argtypes = [vp, C.c_float, vp]
    L.sgz_rotate_hue_rgb8.restype = None
    L.sgz_num_frames.argtypes = [sz, u32, u32]
    L.sgz_num_frames.restype = C.c_long
    L.sgz_plan_num_frames.argtypes = [vp, sz]
    L.sgz_plan_num_frames.restype = C.c_uint64
    L.sgz_plan_get_resonator.argtypes = [vp, vp, vp, vp, vp]
    L.sgz_plan_reset_resonator.argtypes = [vp, vp]
    L.sgz_scope_set_transport.argtypes = [vp, C.c_int64]
    L.sgz_scope_set_tempo.argtypes = [vp, C.c_double]
    L.sgz_scope_effective_window.argtypes = [vp]
    L.sgz_scope_effective_window.restype = C.c_double
    L.sgz_scope_time_window.argtypes = [u32, C.c_double, C.c_double, C.c_double, C.c_double]
    L.sgz_scope_time_window.restype = C.c_double
    L.sgz_spectrogram_render_device.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp]
    L.sgz_spectrogram_render.argtypes = [C.POINTER(SpectrumConfig), vp, u32, sz, vp, vp, C.POINTER(Timing)]
    L.sgz_spectrogram_render_host.argtypes = [vp, vp, u32, sz, vp, vp, C.POINTER(Timing)]
    L.sgz_stage_bins.argtypes = [vp, vp, sz, sz, vp, vp]
    L.sgz_stage_mapped.argtypes = [vp, vp, sz, sz, vp, vp]
    L.sgz_stage_mapped_dominant.argtypes = [vp, vp, sz, sz, vp, vp]
    L.sgz_stage_nyquist.argtypes = [vp, vp, sz, sz, C.c_int, vp, C.POINTER(u32), C.POINTER(u32), vp]
    L.sgz_stage_map_from_bins.argtypes = [vp, vp, sz, vp, vp]
    L.sgz_stage_decay_colour.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    L.sgz_decay_fold_carry.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    L.sgz_stage_logf.argtypes = [vp, vp, sz, vp]
    L.sgz_plan_set_option.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.sgz_stage_finish_pixel.argtypes = [vp, vp, sz, vp]
    L.sgz_stage_track_peak.argtypes = [vp, vp, C.c_double, C.POINTER(Peak), vp]
    L.sgz_spectrum_track_peak.argtypes = [vp, u32, C.c_double, C.POINTER(Peak)]
    L.sgz_track_peak_lines.argtypes = [vp, vp, C.c_double, C.POINTER(LinePeak)]
    L.sgz_spectrum_track_peak_lines.argtypes = [vp, u32, u32, C.c_double, C.POINTER(LinePeak)]
    L.sgz_stage_track_peaks.argtypes = [vp, vp, sz, C.c_double, vp, vp]
    L.sgz_stage_track_peaks_lines.argtypes = [vp, vp, sz, u32, C.c_double, vp, vp]
    L.sgz_spectrogram_track_device.argtypes = [vp, vp, sz, sz, u32, C.c_double, vp, vp, vp, vp]
    L.sgz_spectrogram_track_host.argtypes = [vp, vp, u32, sz, u32, C.c_double, vp, vp, C.POINTER(Timing)]
    L.sgz_overview_step.argtypes = [u32, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sgz_stage_overview.argtypes = [vp, vp, sz, u32, u32, C.c_int, u32, vp, vp, vp, vp]
    L.sgz_spectrogram_overview_device.argtypes = [vp, vp, sz, sz, u32, vp, vp, vp, vp]
    L.sgz_spectrogram_overview_host.argtypes = [vp, vp, u32, sz, u32, vp, vp, C.POINTER(Timing)]
    L.sgz_overview_view_columns.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u32, C.POINTER(C.c_uint64), vp]
    L.sgz_stage_overview_view.argtypes = [vp, vp, sz, sz, sz, u32, u32, vp, vp, vp]
    L.sgz_overview_view_host.argtypes = [vp, vp, sz, sz, sz, u32, vp, vp, C.POINTER(Timing)]
    L.sgz_stage_overview_stats.argtypes = [vp, vp, sz, u32, u32, C.c_int, u32, vp, vp, vp, vp, vp]
    L.sgz_spectrogram_overview_stats_device.argtypes = [vp, vp, sz, sz, u32, vp, vp, vp, vp, vp]
    L.sgz_spectrogram_overview_stats_host.argtypes = [vp, vp, u32, sz, u32, vp, vp, vp, C.POINTER(Timing)]
    L.sgz_stage_overview_stats_view.argtypes = [vp, vp, sz, sz, sz, u32, u32, vp, vp, vp, vp]
    L.sgz_overview_stats_view_host.argtypes = [vp, vp, sz, sz, sz, u32, vp, vp, vp, C.POINTER(Timing)]
    L.sgz_overview_stats_fold.argtypes = [vp, sz, sz, sz, sz, u32, vp]
    L.sgz_overview_stats_readout.argtypes = [vp, sz, vp, vp, vp]
    L.sgz_stage_overview_pct.argtypes = [vp, vp, sz, u32, u32, C.c_int, u32, vp, u32, vp, vp, vp, vp, vp]
    L.sgz_spectrogram_overview_pct_device.argtypes = [vp, vp, sz, sz, u32, vp, u32, vp, vp, vp, vp, vp]
    L.sgz_spectrogram_overview_pct_host.argtypes = [vp, vp, u32, sz, u32, vp, u32, vp, vp, vp, C.POINTER(Timing)]
    L.sgz_overview_pct_bucket.argtypes = [C.c_float, C.POINTER(u32)]
    L.sgz_overview_pct_fold.argtypes = [vp, sz, sz, sz, sz, u32, vp]
    L.sgz_overview_pct_readout.argtypes = [vp, sz, vp, u32, vp]
    L.sgz_stage_overview_power.argtypes = [vp, vp, sz, u32, u32, C.c_int, u32, vp, vp, vp, vp, vp]
    L.sgz_spectrogram_overview_power_device.argtypes = [vp, vp, sz, sz, u32, vp, vp, vp, vp]
    L.sgz_spectrogram_overview_power_host.argtypes = [vp, vp, u32, sz, u32, vp, vp, vp, C.POINTER(Timing)]
    L.sgz_stage_overview_power_view.argtypes = [vp, vp, sz, sz, sz, u32, u32, vp, vp, vp, vp]
    L.sgz_overview_power_view_host.argtypes = [vp, vp, sz, sz, sz, u32, vp, vp, vp, C.POINTER(Timing)]
    L.sgz_overview_power_quantise.argtypes = [vp, sz, vp]
    L.sgz_overview_power_fold.argtypes = [vp, sz, sz, sz, sz, u32, vp]
    L.sgz_overview_power_readout.argtypes = [vp, sz, vp, vp, vp, vp]
    L.sgz_overview_power_levels.argtypes = [vp, vp, sz, vp]
    L.sgz_plan_set_cross_edges.argtypes = [vp, vp, u32]
    L.sgz_stage_overview_cross.argtypes = [vp, vp, sz, u32, u32, C.c_int, u32, vp, vp, vp]
    L.sgz_spectrogram_overview_cross_device.argtypes = [vp, vp, sz, sz, u32, vp, vp]
    L.sgz_spectrogram_overview_cross_host.argtypes = [vp, vp, u32, sz, u32, vp, C.POINTER(Timing)]
    L.sgz_overview_cross_quantise.argtypes = [u32, vp, vp, vp, vp, sz, vp, vp]
    L.sgz_overview_cross_fold.argtypes = [vp, sz, sz, vp, u32, sz, sz, u32, vp, u32, vp]
    L.sgz_overview_cross_readout.argtypes = [vp, sz, vp]
    L.sgz_overview_cross_unit.argtypes = [vp, C.POINTER(C.c_double)]
    L.sgz_cross_edges_octave.argtypes = [C.c_double, u32, u32, C.c_double, C.c_double, vp, u32, C.POINTER(u32), vp]
    L.sgz_stage_overview_flux.argtypes = [vp, vp, sz, u32, u32, C.c_int, C.c_uint64, u32, vp, vp, vp, vp]
    L.sgz_spectrogram_overview_flux_device.argtypes = [vp, vp, sz, sz, u32, vp, vp]
    L.sgz_spectrogram_overview_flux_host.argtypes = [vp, vp, u32, sz, u32, vp, C.POINTER(Timing)]
    L.sgz_overview_flux_quantise.argtypes = [vp, sz, vp]
    L.sgz_overview_flux_fold.argtypes = [vp, sz, sz, sz, sz, u32, vp]
    L.sgz_overview_flux_readout.argtypes = [vp, sz, u32, vp, vp, vp, vp, vp]
    L.sgz_overview_flux_hz.argtypes = [vp, vp, sz, vp]
    L.sgz_comm_unique_id.argtypes = [vp]
    L.sgz_comm_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
    L.sgz_comm_destroy.argtypes = [vp]
    L.sgz_comm_destroy.restype = None
    L.sgz_shard_layout.argtypes = [vp, u32, u32, sz] + [C.POINTER(C.c_uint64)] * 4
    L.sgz_spectrogram_render_sharded.argtypes = [vp, vp, u32, u32, vp, sz, sz, vp, C.POINTER(C.c_uint64), vp]
    L.sgz_stage_decay_scan.argtypes = [vp, vp, sz, vp, vp]
    L.sgz_stage_decay_emit.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    L.sgz_spectrum_create.argtypes = [C.POINTER(SpectrumConfig), C.POINTER(vp)]
    L.sgz_spectrum_destroy.argtypes = [vp]
    L.sgz_spectrum_destroy.restype = None
    L.sgz_spectrum_configure.argtypes = [vp, C.POINTER(SpectrumConfig)]
    L.sgz_spectrum_push.argtypes = [vp, vp, u32, u32]
    L.sgz_spectrum_pop_column.argtypes = [vp, vp, C.POINTER(u32)]
    L.sgz_spectrum_line_results.argtypes = [vp, u32, u32, vp]
    L.sgz_spectrum_render_lines.argtypes = [vp, vp, vp]
    L.sgz_spectrum_set_option.argtypes = [vp, u32, C.c_uint64]
    L.sgz_spectrum_clear_state.argtypes = [vp]
    L.sgz_spectrum_set_mix.argtypes = [vp, u32, vp]
    L.sgz_spectrum_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sgz_spectrum_history.argtypes = [vp, u32, vp]
    L.sgz_spectrum_bind_image.argtypes = [vp, vp, u32, sz]
    L.sgz_spectrum_create_image.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]
    L.sgz_spectrum_bind_gl_buffer.argtypes = [vp, C.c_uint, u32, sz]
    L.sgz_spectrum_flush_columns.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.sgz_scope_create.argtypes = [C.POINTER(ScopeConfig), C.POINTER(vp)]
    L.sgz_scope_set_option.argtypes = [vp, u32, C.c_uint64]
    L.sgz_scope_stream.argtypes = [vp]
    L.sgz_scope_stream.restype = vp
    L.sgz_vector_stream.argtypes = [vp]
    L.sgz_vector_stream.restype = vp
    L.sgz_vector_set_option.argtypes = [vp, u32, C.c_uint64]
    L.sgz_scope_destroy.argtypes = [vp]
    L.sgz_scope_destroy.restype = None
    L.sgz_scope_configure.argtypes = [vp, C.POINTER(ScopeConfig)]
    L.sgz_scope_push.argtypes = [vp, vp, u32, u32]
    L.sgz_scope_set_mix.argtypes = [vp, u32, vp]
    L.sgz_scope_peak_filter.argtypes = [vp, C.c_double, u32, C.POINTER(C.c_double)]
    L.sgz_scope_gains.argtypes = [vp, C.POINTER(C.c_double), vp]
    L.sgz_scope_vertex_count.argtypes = [vp, C.POINTER(ScopeView)]
    L.sgz_scope_vertex_count.restype = sz
    L.sgz_scope_vertices.argtypes = [vp, C.POINTER(ScopeView), u32, u32, vp, vp, C.POINTER(u32)]
    L.sgz_scope_front.argtypes = [vp, u32, vp, C.POINTER(u32), C.POINTER(u32)]
    L.sgz_scope_debug_state.argtypes = [vp, vp]
    L.sgz_scope_analyse.argtypes = [vp, u32, u32, C.POINTER(TriggerState)]
    L.sgz_scope_front_colours.argtypes = [vp, u32, u32, vp]
    L.sgz_scope_vertices_device.argtypes = [vp, C.POINTER(ScopeView), u32, u32, vp, vp, C.POINTER(u32)]
    L.sgz_scope_vertices_all.argtypes = [vp, C.POINTER(ScopeView), u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(vp), C.POINTER(vp), C.POINTER(u32)]
    L.sgz_vector_vertices_device.argtypes = [vp, u32, vp, vp, C.POINTER(u32)]
    L.sgz_scope_dense_vertex_count.argtypes = [vp, u32]
    L.sgz_scope_dense_vertex_count.restype = sz
    L.sgz_scope_dense_vertices.argtypes = [vp, u32, u32, u32, vp, vp, C.POINTER(u32)]
    L.sgz_scope_dense_vertices_device.argtypes = [vp, u32, u32, u32, vp, vp, C.POINTER(u32)]
    L.sgz_scope_dense_vertices_all.argtypes = [vp, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(vp), C.POINTER(vp), C.POINTER(u32)]
    L.sgz_scope_dense_device.argtypes = [vp, sz, sz, u32, sz, u32, vp, vp]
    L.sgz_export_alloc.argtypes = [sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_int)]
    L.sgz_export_free.argtypes = [vp]
    L.sgz_export_free.restype = None
    L.sgz_vector_create.argtypes = [C.POINTER(VectorConfig), C.POINTER(vp)]
    L.sgz_vector_destroy.argtypes = [vp]
    L.sgz_vector_destroy.restype = None
    L.sgz_vector_configure.argtypes = [vp, C.POINTER(VectorConfig)]
    L.sgz_vector_push.argtypes = [vp, vp, u32, u32]
    L.sgz_vector_set_mix.argtypes = [vp, u32, vp]
    L.sgz_vector_peak_filter.argtypes = [vp, C.c_double, C.POINTER(C.c_double)]
    L.sgz_vector_filters_get.argtypes = [vp, C.POINTER(VectorFilters), C.POINTER(C.c_double)]
    L.sgz_vector_vertices.argtypes = [vp, u32, vp, vp, C.POINTER(u32)]
    L.sgz_vector_vertices_all.argtypes = [vp, vp, vp, C.POINTER(u32)]
    L.sgz_vector_history.argtypes = [vp, u32, vp, C.POINTER(u32), C.POINTER(u32)]
    L.sgz_vector_lissajous_vertices.argtypes = [vp, u32, vp, vp, C.POINTER(u32)]
    L.sgz_vector_lissajous_vertices_all.argtypes = [vp, vp, vp, C.POINTER(u32)]
    L.sgz_vector_lissajous_vertices_device.argtypes = [vp, u32, vp, vp, C.POINTER(u32)]
    L.sgz_vector_lissajous_device.argtypes = [vp, sz, u32, sz, u32, vp, vp, vp, vp]
    L.sgz_vector_meters_from_filters.argtypes = [C.POINTER(VectorFilters), C.POINTER(VectorMeters)]
    L.sgz_vector_meters.argtypes = [vp, C.POINTER(VectorMeters)]
    L.sgz_line_graph_vertex_count.argtypes = [u32, u32, u32, u32]
    L.sgz_line_graph_vertex_count.restype = sz
    L.sgz_line_graph_draws.argtypes = [C.POINTER(LineGraphStyle), u32, u32, u32, vp, C.POINTER(u32), vp]
    L.sgz_line_graph_vertices_device.argtypes = [vp, u32, u32, u32, u32, vp, vp]
    L.sgz_spectrum_render_line_vertices.argtypes = [vp, vp, u32, vp, C.POINTER(u32)]
    dbl = C.c_double
    L.sgz_spectrum_set_view.argtypes = [vp, dbl, dbl]
    L.sgz_view_translation_rows.argtypes = [u32, dbl, dbl, dbl, dbl, vp, vp]
    L.sgz_view_translate_device.argtypes = [vp, u32, sz, u32, dbl, dbl, dbl, dbl, vp]
    L.sgz_spectrum_resize.argtypes = [vp, u32, vp, u32, sz]
    L.sgz_image_resize_rows.argtypes = [u32, u32, vp, vp]
    L.sgz_image_resize_columns.argtypes = [u32, u32, u32, vp, C.POINTER(u32)]
    L.sgz_image_resize_device.argtypes = [vp, u32, sz, u32, u32, vp, u32, sz, u32, C.POINTER(u32), vp]
    L.sgz_spectrum_update.argtypes = [vp, C.POINTER(SpectrumConfig)]
    L.sgz_spectrum_update_effects.argtypes = [C.POINTER(SpectrumConfig), C.POINTER(SpectrumConfig), C.POINTER(u32)]
    L.sgz_ring_resize_device.argtypes = [vp, u32, vp, u32, u32, C.c_uint64, vp]
    L.sgz_spectrum_set_pacing.argtypes = [vp, dbl]
    L.sgz_spectrum_set_frozen.argtypes = [vp, C.c_int]
    L.sgz_spectrum_render_columns.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(dbl)]
    L.sgz_spectrum_present.argtypes = [vp, vp, sz]
    L.sgz_frame_pacing_step.argtypes = [dbl, dbl, u32, C.POINTER(u32), C.POINTER(dbl)]
    L.sgz_columns_to_image_device.argtypes = [vp, sz, u32, vp, u32, sz, u32, vp]
    L.sgz_image_unroll_device.argtypes = [vp, u32, sz, u32, u32, vp, sz, vp]
    L.sgz_scope_num_points.argtypes = [C.POINTER(ScopeView)]
    L.sgz_scope_num_points.restype = sz
    L.sgz_scope_lanczos_device.argtypes = [C.POINTER(ScopeView), vp, sz, sz, u32, vp, vp]
    L.sgz_scope_zero_crossing_device.argtypes = [C.POINTER(ZeroCrossingState), u32, vp, vp, sz, vp, sz,
                                                 C.POINTER(sz), vp]
    L.sgz_peak_filter_device.argtypes = [vp, sz, u32, sz, u32, C.c_double, vp, C.POINTER(C.c_double), vp]
    L.sgz_vector_polar_device.argtypes = [vp, sz, u32, sz, u32, vp, vp]
    L.sgz_vector_audio_processing_device.argtypes = [C.POINTER(VectorFilters), vp, vp, sz, u32, C.c_float,
                                                     C.c_float, C.c_float, C.c_int, C.POINTER(C.c_float), vp]
    u64 = C.c_uint64
    L.sgz_pcm_sample_bytes.argtypes = [u32]
    L.sgz_pcm_sample_bytes.restype = u32
    L.sgz_pcm_to_planar_device.argtypes = [vp, u32, u32, sz, vp, u32, vp, sz, vp]
    L.sgz_stream_step.argtypes = [u32, u32, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    L.sgz_pcm_stream_create.argtypes = [C.POINTER(SpectrumConfig), u32, u32, vp, sz, C.POINTER(vp)]
    L.sgz_pcm_stream_destroy.argtypes = [vp]
    L.sgz_pcm_stream_destroy.restype = None
    L.sgz_pcm_stream_frames_for.argtypes = [vp, sz]
    L.sgz_pcm_stream_frames_for.restype = u64
    L.sgz_pcm_stream_feed.argtypes = [vp, vp, sz, vp, vp, u64, C.POINTER(u64), C.POINTER(PcmTiming)]
    L.sgz_pcm_stream_reset.argtypes = [vp]
    L.sgz_spectrogram_render_pcm.argtypes = [C.POINTER(SpectrumConfig), vp, u32, u32, vp, sz, vp, vp, C.POINTER(PcmTiming)]
    L.sgz_pcm_stream_feed_overview.argtypes = [vp, vp, sz, u32, C.c_int, vp, vp, u64, C.POINTER(u64), C.POINTER(PcmTiming)]
    L.sgz_pcm_stream_columns_for.argtypes = [vp, sz, u32, C.c_int]
    L.sgz_pcm_stream_columns_for.restype = u64
    L.sgz_pcm_stream_open_frames.argtypes = [vp]
    L.sgz_pcm_stream_open_frames.restype = u64
    L.sgz_pcm_stream_set_option.argtypes = [vp, u32, u32]
    L.sgz_track_peak_values.argtypes = [vp, vp, C.c_double, C.POINTER(LinePeak)]
    L.sgz_stage_track_peaks_values.argtypes = [vp, vp, sz, C.c_double, vp, vp]
    L.sgz_pcm_stream_set_track.argtypes = [vp, u32, C.c_double, vp, u64]
    L.sgz_pcm_stream_track_for.argtypes = [vp, sz]
    L.sgz_pcm_stream_track_for.restype = u64
    L.sgz_pcm_stream_track_state.argtypes = [vp, C.POINTER(u64)]
    L.sgz_spectrogram_overview_pcm.argtypes = [C.POINTER(SpectrumConfig), vp, u32, u32, vp, sz, u32, vp, vp, C.POINTER(PcmTiming)]
    L.sgz_pcm_stream_feed_overview_stats.argtypes = [vp, vp, sz, u32, C.c_int, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(PcmTiming)]
    L.sgz_spectrogram_overview_stats_pcm.argtypes = [C.POINTER(SpectrumConfig), vp, u32, u32, vp, sz, u32, vp, vp, vp, C.POINTER(PcmTiming)]
    L.sgz_pcm_stream_feed_overview_pct.argtypes = [vp, vp, sz, u32, C.c_int, vp, u32, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(PcmTiming)]
    L.sgz_spectrogram_overview_pct_pcm.argtypes = [C.POINTER(SpectrumConfig), vp, u32, u32, vp, sz, u32, vp, u32, vp, vp, vp, C.POINTER(PcmTiming)]
    L.sgz_pcm_stream_feed_overview_power.argtypes = [vp, vp, sz, u32, C.c_int, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(PcmTiming)]
    L.sgz_spectrogram_overview_power_pcm.argtypes = [C.POINTER(SpectrumConfig), vp, u32, u32, vp, sz, u32, vp, vp, vp, C.POINTER(PcmTiming)]
    L.sgz_pcm_stream_set_cross_edges.argtypes = [vp, vp, u32]
    L.sgz_pcm_stream_feed_overview_cross.argtypes = [vp, vp, sz, u32, C.c_int, vp, u64, C.POINTER(u64), C.POINTER(PcmTiming)]
    L.sgz_spectrogram_overview_cross_pcm.argtypes = [C.POINTER(SpectrumConfig), vp, u32, u32, vp, sz, vp, u32, u32, vp, C.POINTER(PcmTiming)]
    L.sgz_pcm_stream_feed_overview_flux.argtypes = [vp, vp, sz, u32, C.c_int, vp, u64, C.POINTER(u64), C.POINTER(PcmTiming)]
    L.sgz_spectrogram_overview_flux_pcm.argtypes = [C.POINTER(SpectrumConfig), vp, u32, u32, vp, sz, u32, vp, C.POINTER(PcmTiming)]
    L.sgz_level_readout.argtypes = [vp, C.POINTER(LevelReading)]
    L.sgz_truepeak_taps.argtypes = [vp]
    L.sgz_truepeak_taps.restype = None
    L.sgz_truepeak_readout.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sgz_loudness_filter_for_rate.argtypes = [C.c_double, fp]
    L.sgz_loudness_taps.argtypes = [fp, vp]
    L.sgz_loudness_readout.argtypes = [vp, sz, u32, vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sgz_loudness_integrated.argtypes = [vp, sz, u32, vp, C.POINTER(C.c_double)]
    L.sgz_field_boundaries.argtypes = [vp]
    L.sgz_field_boundaries.restype = None
    L.sgz_field_readout.argtypes = [vp, C.POINTER(FieldReading)]
    L.sgz_band_filter_for_rate.argtypes = [C.c_double, C.c_double, C.c_double, bp]
    L.sgz_band_taps.argtypes = [bp, vp]
    L.sgz_band_readout.argtypes = [vp, sz, u32, u32, vp, vp]
    L.sgz_band_colours.argtypes = [vp, sz, u32, u32, vp, vp, C.c_double, vp]
    L.sgz_hist_edges.argtypes = [vp, vp]
    L.sgz_hist_edges.restype = None
    L.sgz_hist_percentile.argtypes = [vp, C.c_double, C.POINTER(u32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sgz_hist_readout.argtypes = [vp, C.POINTER(HistReading)]
    L.sgz_run_params_default.argtypes = [rp]
    L.sgz_run_params_default.restype = None
    L.sgz_run_readout.argtypes = [vp, C.c_double, C.POINTER(RunReading)]
    # the eight column lanes: what a lane's stage call takes between nsamples and m and its set call in front of m -- the filter or the
    # thresholds by reference, and behind a filter the first index --, and whether the stage call takes `continued`
    lanes = {"wave": ([], False), "level": ([], False), "truepeak": ([], True), "loudness": ([fp, u64], True), "field": ([], False),
             "band": ([bp, u64], True), "hist": ([], False), "run": ([rp], True)}
    for lane, (front, history) in lanes.items():
        getattr(L, f"sgz_stage_{lane}_columns").argtypes = [vp, sz, u32, sz, *front, u32, u32, C.c_int, *([u32] if history else []), u32, vp, vp, vp]
        limits = getattr(L, f"sgz_{lane}_columns_limits")
        if len(front) == 2:                                             # (by the filter: a status, and the carry's bytes too)
            limits.argtypes = [front[0], u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(sz)]
        else:
            limits.argtypes, limits.restype = [C.POINTER(u32), C.POINTER(u32)], None
        if lane != "wave":
            getattr(L, f"sgz_{lane}_fold").argtypes = [vp, sz, u32, sz, sz, u32, vp]
        lane = "waveform" if lane == "wave" else lane                   # the PCM stream's calls: one set each
        getattr(L, f"sgz_pcm_stream_set_{lane}").argtypes = [vp, *front[:1], u32, vp, u64]
        getattr(L, f"sgz_pcm_stream_{lane}_for").argtypes = [vp, sz, C.c_int]
        getattr(L, f"sgz_pcm_stream_{lane}_for").restype = u64
        getattr(L, f"sgz_pcm_stream_{lane}_state").argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        getattr(L, f"sgz_pcm_stream_flush_{lane}").argtypes = [vp]
    _lib = L
    return L


def check(status: int) -> int:
    if status < 0:
        raise SgzError(status, (lib().sgz_last_error() or b"").decode(errors="replace"))
    return status


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _buf_ptr(a):
    """a numpy array's or a torch tensor's (host or device) data pointer"""
    return C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else _np_ptr(a)


def vector_meters_from_filters(filters: VectorFilters) -> VectorMeters:
    """drawStereoMeters' indicator positions from the filter states (sgz_vector_meters_from_filters; host arithmetic, no GPU)"""
    m = VectorMeters()
    check(lib().sgz_vector_meters_from_filters(C.byref(filters), C.byref(m)))
    return m


def line_graph_style(colour_one, colour_two, flood_alpha: float, primitive_size: float = 1.0, rendering_scale: float = 1.0) -> LineGraphStyle:
    """sgz_line_graph_style from RGBA8 colours per graph (colour_one / colour_two: [SGZ_NUM_GRAPHS][4])"""
    st = LineGraphStyle()
    for k in range(NUM_GRAPHS):
        for j in range(4):
            st.colour_one[k][j] = int(colour_one[k][j])
            st.colour_two[k][j] = int(colour_two[k][j])
    st.flood_alpha, st.primitive_size, st.rendering_scale = flood_alpha, primitive_size, rendering_scale
    return st


def line_graph_vertex_count(channel_mode: int, pairs: int, axis_points: int, flood: bool) -> int:
    """renderTransformAsGraph's vertex count for `pairs` pairs (sgz_line_graph_vertex_count; host only)"""
    return int(lib().sgz_line_graph_vertex_count(channel_mode, pairs, axis_points, int(bool(flood))))


def line_graph_draws(style: LineGraphStyle, channel_mode: int, pairs: int, axis_points: int):
    """renderTransformAsGraph's draw list (sgz_line_graph_draws; host only): (records as a LINE_GRAPH_DRAW_DTYPE array, model float32 [4])"""
    cnt = C.c_uint32(0)
    st = lib().sgz_line_graph_draws(C.byref(style), channel_mode, pairs, axis_points, None, C.byref(cnt), None)
    if st != SGZ_EINVAL or cnt.value == 0:                     # (the size query: a refusal that reports the count)
        check(st)
    out = np.zeros(cnt.value, LINE_GRAPH_DRAW_DTYPE)
    model = np.zeros(4, np.float32)
    check(lib().sgz_line_graph_draws(C.byref(style), channel_mode, pairs, axis_points, _np_ptr(out), C.byref(cnt), _np_ptr(model)))
    return out[:cnt.value], model


def spectrum_render_line_vertices(handle, poles, flood: bool, out):
    """sgz_spectrum_render_line_vertices on a LINE_GRAPH spectrum handle: render_lines' work, then the vertex stream into `out` -- float32
    [vertices][3] (or any shape of that size), a numpy array or a torch tensor, host (pinned or not) or device.  poles: [SGZ_NUM_GRAPHS]
    or None.  Returns the vertex count."""
    if hasattr(out, "numel"):
        assert str(out.dtype) == "torch.float32" and out.is_contiguous()
        n = out.numel() // 3
    else:
        assert out.dtype == np.float32 and out.flags.c_contiguous
        n = out.size // 3
    cnt = C.c_uint32(n)
    pl = (C.c_float * NUM_GRAPHS)(*poles) if poles is not None else None
    check(lib().sgz_spectrum_render_line_vertices(handle, pl, int(bool(flood)), _buf_ptr(out), C.byref(cnt)))
    return cnt.value


def spectrum_set_view(handle, left: float, right: float) -> None:
    """sgz_spectrum_set_view: zoom / pan a spectrum handle (viewLeft / viewRight) keeping its audio history, queue and image binding;
    the bound image of a colour-spectrum handle follows the view (freeLinearVerticalTranslation)"""
    check(lib().sgz_spectrum_set_view(handle, float(left), float(right)))


def view_translation_rows(axis_points: int, old_left: float, old_right: float, new_left: float, new_right: float):
    """the translation's row table (sgz_view_translation_rows; host only): (src int32 [P], -1 = no source; weight uint16 [P])"""
    src = np.zeros(axis_points, np.int32)
    weight = np.zeros(axis_points, np.uint16)
    check(lib().sgz_view_translation_rows(axis_points, old_left, old_right, new_left, new_right, _np_ptr(src), _np_ptr(weight)))
    return src, weight


def view_translate_device(image, columns: int, pitch_bytes: int, axis_points: int, old_left: float, old_right: float, new_left: float,
                          new_right: float, stream=None) -> None:
    """sgz_view_translate_device: translate a DEVICE image [P][pitch_bytes] of RGBA8 texels in place (a torch tensor or a device
    pointer); waits for the result"""
    ptr = C.c_void_p(image.data_ptr()) if hasattr(image, "data_ptr") else C.c_void_p(int(image))
    check(lib().sgz_view_translate_device(ptr, columns, pitch_bytes, axis_points, old_left, old_right, new_left, new_right,
                                          C.c_void_p(stream) if stream else None))


def _dev_ptr(image):
    return C.c_void_p(image.data_ptr()) if hasattr(image, "data_ptr") else C.c_void_p(int(image)) if image else None


def spectrum_resize(handle, axis_points: int, image=None, columns: int = 0, pitch_bytes: int = 0) -> None:
    """sgz_spectrum_resize: a new axis size (the editor resized, or Spectrum stretch changed) keeping the audio history and cadence; the
    bound image's content moves into `image` (a torch tensor or a device pointer, caller-owned), or the binding is dropped (None)"""
    check(lib().sgz_spectrum_resize(handle, axis_points, _dev_ptr(image), columns, pitch_bytes))


def image_resize_rows(old_axis_points: int, new_axis_points: int):
    """the resize's row table (sgz_image_resize_rows; host only): (src int32 [P1], weight uint16 [P1])"""
    src = np.zeros(new_axis_points, np.int32)
    weight = np.zeros(new_axis_points, np.uint16)
    check(lib().sgz_image_resize_rows(old_axis_points, new_axis_points, _np_ptr(src), _np_ptr(weight)))
    return src, weight


def image_resize_columns(old_columns: int, old_x: int, new_columns: int):
    """the resize's column table (sgz_image_resize_columns; host only): (src int32 [C1], -1 = no source; the new write column x1)"""
    src = np.zeros(new_columns, np.int32)
    x1 = C.c_uint32(0)
    check(lib().sgz_image_resize_columns(old_columns, old_x, new_columns, _np_ptr(src), C.byref(x1)))
    return src, x1.value


def image_resize_device(src, old_columns: int, src_pitch_bytes: int, old_axis_points: int, old_x: int, dst, new_columns: int,
                        dst_pitch_bytes: int, new_axis_points: int, stream=None) -> int:
    """sgz_image_resize_device: resample a DEVICE image [P0][src_pitch_bytes] of RGBA8 texels into another, [P1][dst_pitch_bytes] (torch
    tensors or device pointers; their memory must not overlap); waits for the result.  Returns the new write column x1."""
    x1 = C.c_uint32(0)
    check(lib().sgz_image_resize_device(_dev_ptr(src), old_columns, src_pitch_bytes, old_axis_points, old_x, _dev_ptr(dst), new_columns,
                                        dst_pitch_bytes, new_axis_points, C.byref(x1), C.c_void_p(stream) if stream else None))
    return x1.value


# sgz_spectrum_update_effects' flags
UPDATE_PLANS, UPDATE_CLEAR_LINES, UPDATE_CLEAR_STATE, UPDATE_RESONATORS_AT_REST, UPDATE_TRANSLATE_IMAGE, UPDATE_RING_MOVED = 1, 2, 4, 8, 16, 32


def _sides(cfg) -> int:
    """value planes per pair: 2 for Phase (4; magnitude and cancellation planes), Separate and MidSide"""
    return 2 if cfg.channel_mode in (4, 5, 6) else 1


def _as_config(cfg) -> SpectrumConfig:
    return cfg if isinstance(cfg, SpectrumConfig) else config_from_dict(cfg)


def spectrum_update(handle, cfg) -> None:
    """sgz_spectrum_update: any setting change short of a new stream, display mode or axis size (a config dict or SpectrumConfig), keeping
    the audio history, the cadence, the mix, the queued columns and the image binding; what it zeroes is spectrum_update_effects'"""
    c = _as_config(cfg)
    check(lib().sgz_spectrum_update(handle, C.byref(c)))


def spectrum_update_effects(old, new) -> int:
    """what sgz_spectrum_update does for a change from `old` to `new` (config dicts or SpectrumConfig; host only): the UPDATE_* mask, 0 for
    equal configurations; raises SgzError with the update's refusal"""
    a, b, fx = _as_config(old), _as_config(new), C.c_uint32(0)
    check(lib().sgz_spectrum_update_effects(C.byref(a), C.byref(b), C.byref(fx)))
    return fx.value


def ring_resize_device(old_ring, old_cap: int, new_ring, new_cap: int, channels: int, written: int, stream=None) -> None:
    """sgz_ring_resize_device: the mirrored ring [channels][2 old_cap] into [channels][2 new_cap] keeping its newest samples (DEVICE float32:
    torch tensors or device pointers); enqueued on `stream`, not waited for"""
    check(lib().sgz_ring_resize_device(_dev_ptr(old_ring), old_cap, _dev_ptr(new_ring), new_cap, channels, written,
                                       C.c_void_p(stream) if stream else None))


def frame_pacing_step(z: float, smoothing: float, queued: int):
    """one pass of renderColourSpectrum's pop loop (sgz_frame_pacing_step; host only): (columns popped, framesPerUpdate afterwards)"""
    pop, z_next = C.c_uint32(0), C.c_double(0.0)
    check(lib().sgz_frame_pacing_step(z, smoothing, queued, C.byref(pop), C.byref(z_next)))
    return pop.value, z_next.value


def spectrum_set_pacing(handle, frame_update_smoothing: float) -> None:
    """sgz_spectrum_set_pacing: content->frameUpdateSmoothing of a colour-spectrum handle, in [0, 1)"""
    check(lib().sgz_spectrum_set_pacing(handle, float(frame_update_smoothing)))


def spectrum_set_frozen(handle, frozen: bool) -> None:
    """sgz_spectrum_set_frozen: Spectrum::freeze / unfreeze"""
    check(lib().sgz_spectrum_set_frozen(handle, int(bool(frozen))))


def spectrum_render_columns(handle):
    """sgz_spectrum_render_columns: one video frame's pop loop into the bound image: (status SGZ_OK / SGZ_EMPTY, first column, count,
    framesPerUpdate afterwards)"""
    first, cnt, fpu = C.c_uint32(0), C.c_uint32(0), C.c_double(0.0)
    st = check(lib().sgz_spectrum_render_columns(handle, C.byref(first), C.byref(cnt), C.byref(fpu)))
    return st, first.value, cnt.value, fpu.value


def spectrum_present(handle, dst, dst_pitch_bytes: int) -> None:
    """sgz_spectrum_present: the bound ring image unrolled (oldest column at the left) into `dst`, DEVICE [P][dst_pitch_bytes] (a torch
    tensor or a device pointer); waits for the texels"""
    check(lib().sgz_spectrum_present(handle, _dev_ptr(dst), dst_pitch_bytes))


def columns_to_image_device(columns_rgba, n: int, axis_points: int, image, columns: int, pitch_bytes: int, x0: int = 0, stream=None) -> None:
    """sgz_columns_to_image_device: DEVICE columns [n][P] RGBA8 into a DEVICE image [P][pitch_bytes] at texel columns (x0 + k) % columns
    (torch tensors or device pointers); enqueued on `stream`, not waited for"""
    check(lib().sgz_columns_to_image_device(_dev_ptr(columns_rgba), n, axis_points, _dev_ptr(image), columns, pitch_bytes, x0,
                                            C.c_void_p(stream) if stream else None))


def image_unroll_device(src, columns: int, src_pitch_bytes: int, axis_points: int, x: int, dst, dst_pitch_bytes: int, stream=None) -> None:
    """sgz_image_unroll_device: dst[y][j] = src[y][(x + j) % columns] (DEVICE images: torch tensors or device pointers, not overlapping);
    enqueued on `stream`, not waited for"""
    check(lib().sgz_image_unroll_device(_dev_ptr(src), columns, src_pitch_bytes, axis_points, x, _dev_ptr(dst), dst_pitch_bytes,
                                        C.c_void_p(stream) if stream else None))


RT_OPT_STRICT_REFERENCE_QUIRKS, RT_OPT_AUDIO_HISTORY, RT_OPT_DEFER_SUBMIT, RT_OPT_PARK_PUSHES = 1, 2, 3, 4
OPT_CHANNEL_SPLIT, OPT_FUSED_COLOUR, OPT_FETCH_WINDOW, OPT_MATRIX_RESONATOR, OPT_RESONATOR_SLAB, OPT_WIDE_GROUPS = 1, 2, 3, 4, 5, 6   # OPT_WIDE_GROUPS: retired, accepted and ignored (sgz.h)
OPT_RESONATOR_SHARD_BOUND = 7
OPT_PIPELINED = 8
OPT_IMAGE_ONLY_SPLIT = 9
OPT_OVERVIEW_SLAB = 10


def overview_step(k: int, held: int, frames: int, flush: bool):
    """sgz_overview_step (host arithmetic, no GPU): (columns that become complete, frames of the column left open)"""
    c, h = C.c_uint64(0), C.c_uint64(0)
    check(lib().sgz_overview_step(k, held, frames, int(bool(flush)), C.byref(c), C.byref(h)))
    return c.value, h.value


def overview_view_columns(n: int, x0: int, x1: int, out_columns: int, want_bounds: bool = False):
    """sgz_overview_view_columns (host arithmetic, no GPU): the view's column count min(out_columns, x1 - x0), or with want_bounds (count,
    uint64 [count + 1] boundaries x0 + ceil(b m / count))"""
    c = C.c_uint64(0)
    check(lib().sgz_overview_view_columns(n, x0, x1, out_columns, C.byref(c), None))
    if not want_bounds:
        return int(c.value)
    bounds = np.zeros(c.value + 1, np.uint64)
    check(lib().sgz_overview_view_columns(n, x0, x1, out_columns, C.byref(c), _np_ptr(bounds)))
    return int(c.value), bounds


def _records_from_device(t, dtype) -> np.ndarray:
    """cuda int64 [..., words] (records as the overview calls write them) -> numpy `dtype` [...]"""
    h = np.ascontiguousarray(t.cpu().numpy())
    return h.view(dtype).reshape(h.shape[:-1])


def _records_to_device(records: np.ndarray, dtype, words: int, device):
    """numpy `dtype` [...] -> cuda int64 [..., words]"""
    import torch
    r = np.ascontiguousarray(records, dtype)
    return torch.from_numpy(r.view(np.int64).reshape(*r.shape, words).copy()).to(device)


def _overview_fold(symbol: str, dtype, records: np.ndarray, out_columns: int, x0: int, x1: int | None) -> np.ndarray:
    """the kinds' sgz_overview_<kind>_fold: `dtype` records [n, ...], source columns [x0, x1) -> [min(out_columns, x1 - x0), ...]"""
    records = np.ascontiguousarray(records, dtype)
    n = int(records.shape[0])
    x1 = n if x1 is None else x1
    width = int(np.prod(records.shape[1:], dtype=np.int64))
    out = np.zeros((overview_view_columns(n, x0, x1, out_columns), *records.shape[1:]), dtype)
    check(getattr(lib(), symbol)(_np_ptr(records), n, width, x0, x1, out_columns, _np_ptr(out)))
    return out


# sgz_overview_stat_record (sgz.h, "The mean overview"): 24 bytes, 8-aligned.  On the device a record is three int64 words of a torch tensor
# [..., 3]; stats_from_device turns such a tensor into a numpy array of this dtype
OVERVIEW_STAT_DTYPE = np.dtype({"names": ["sum", "count", "nans", "lo", "hi"], "formats": ["<i8", "<u4", "<u4", "<f4", "<f4"],
                                "offsets": [0, 8, 12, 16, 20], "itemsize": 24})


def stats_from_device(t) -> np.ndarray:
    """cuda int64 [..., 3] (records as the stats calls write them) -> numpy OVERVIEW_STAT_DTYPE [...]"""
    return _records_from_device(t, OVERVIEW_STAT_DTYPE)


def stats_to_device(records: np.ndarray, device):
    """numpy OVERVIEW_STAT_DTYPE [...] -> cuda int64 [..., 3]"""
    return _records_to_device(records, OVERVIEW_STAT_DTYPE, 3, device)


def overview_stats_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_overview_stats_fold (host, no GPU): OVERVIEW_STAT_DTYPE records [n, ...], source columns [x0, x1) -> [min(out_columns, x1 - x0), ...]"""
    return _overview_fold("sgz_overview_stats_fold", OVERVIEW_STAT_DTYPE, records, out_columns, x0, x1)


def overview_stats_readout(records: np.ndarray):
    """sgz_overview_stats_readout (host, no GPU): OVERVIEW_STAT_DTYPE records [...] -> (mean, lo, hi), float32 planes of the same shape"""
    records = np.ascontiguousarray(records, OVERVIEW_STAT_DTYPE)
    mean, lo, hi = (np.zeros(records.shape, np.float32) for _ in range(3))
    check(lib().sgz_overview_stats_readout(_np_ptr(records), records.size, _np_ptr(mean), _np_ptr(lo), _np_ptr(hi)))
    return mean, lo, hi


# sgz_overview_pct_record (sgz.h, "The percentile overview"): 272 bytes.  On the device a record is 34 int64 words of a torch tensor [..., 34]
# (whose storage torch aligns well beyond the 16 bytes the calls ask for); pct_from_device turns such a tensor into a numpy array of this dtype
OVERVIEW_PCT_BUCKETS, OVERVIEW_PCT_MAX_QUANTILES = 66, 8
OVERVIEW_PCT_DTYPE = np.dtype({"names": ["bucket", "nans", "reserved"], "formats": [("<u4", (OVERVIEW_PCT_BUCKETS,)), "<u4", "<u4"],
                               "offsets": [0, 264, 268], "itemsize": 272})


def pct_from_device(t) -> np.ndarray:
    """cuda int64 [..., 34] (records as the percentile calls write them) -> numpy OVERVIEW_PCT_DTYPE [...]"""
    return _records_from_device(t, OVERVIEW_PCT_DTYPE)


def pct_to_device(records: np.ndarray, device):
    """numpy OVERVIEW_PCT_DTYPE [...] -> cuda int64 [..., 34]"""
    return _records_to_device(records, OVERVIEW_PCT_DTYPE, 34, device)


def _quantiles(q):
    """the calls' (const double *q, uint32_t nq): a scalar or a sequence -> (float64 array kept alive by the caller, its pointer, nq)"""
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(q, np.float64)))
    return a, _np_ptr(a), int(a.size)


def overview_pct_bucket(x: float) -> int:
    """sgz_overview_pct_bucket (host, no GPU): the bucket of a non-NaN value"""
    b = C.c_uint32(0)
    check(lib().sgz_overview_pct_bucket(C.c_float(x), C.byref(b)))
    return int(b.value)


def overview_pct_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_overview_pct_fold (host, no GPU): OVERVIEW_PCT_DTYPE records [n, ...], source columns [x0, x1) -> [min(out_columns, x1 - x0), ...]"""
    return _overview_fold("sgz_overview_pct_fold", OVERVIEW_PCT_DTYPE, records, out_columns, x0, x1)


def overview_pct_readout(records: np.ndarray, q) -> np.ndarray:
    """sgz_overview_pct_readout (host, no GPU): OVERVIEW_PCT_DTYPE records [...] and nq quantiles -> float32 values [nq, ...]"""
    records = np.ascontiguousarray(records, OVERVIEW_PCT_DTYPE)
    qa, qp, nq = _quantiles(q)
    values = np.zeros((nq, *records.shape), np.float32)
    check(lib().sgz_overview_pct_readout(_np_ptr(records), records.size, qp, nq, _np_ptr(values)))
    return values


# sgz_overview_power_record (sgz.h, "The power overview"): 32 bytes, 8-aligned; sum = (low word, high word) of the 128-bit sum.  On the device
# a record is four int64 words of a torch tensor [..., 4]; power_from_device turns such a tensor into a numpy array of this dtype
OVERVIEW_POWER_DTYPE = np.dtype({"names": ["sum", "count", "nans", "lo", "hi"], "formats": [("<u8", (2,)), "<u4", "<u4", "<f4", "<f4"],
                                 "offsets": [0, 16, 20, 24, 28], "itemsize": 32})


def power_from_device(t) -> np.ndarray:
    """cuda int64 [..., 4] (records as the power calls write them) -> numpy OVERVIEW_POWER_DTYPE [...]"""
    return _records_from_device(t, OVERVIEW_POWER_DTYPE)


def power_to_device(records: np.ndarray, device):
    """numpy OVERVIEW_POWER_DTYPE [...] -> cuda int64 [..., 4]"""
    return _records_to_device(records, OVERVIEW_POWER_DTYPE, 4, device)


def overview_power_quantise(x: np.ndarray) -> np.ndarray:
    """sgz_overview_power_quantise (host, no GPU): float32 [...] -> uint64 [...], q of the power overview's definition (0 for a NaN)"""
    x = np.ascontiguousarray(x, np.float32)
    q = np.zeros(x.shape, np.uint64)
    check(lib().sgz_overview_power_quantise(_np_ptr(x), x.size, _np_ptr(q)))
    return q


def overview_power_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_overview_power_fold (host, no GPU): OVERVIEW_POWER_DTYPE records [n, ...], source columns [x0, x1) -> [min(out_columns, x1 - x0), ...]"""
    return _overview_fold("sgz_overview_power_fold", OVERVIEW_POWER_DTYPE, records, out_columns, x0, x1)


def overview_power_readout(records: np.ndarray):
    """sgz_overview_power_readout (host, no GPU): OVERVIEW_POWER_DTYPE records [...] -> (mean_square float64, rms, lo, hi float32), planes of
    the same shape"""
    records = np.ascontiguousarray(records, OVERVIEW_POWER_DTYPE)
    ms = np.zeros(records.shape, np.float64)
    rms, lo, hi = (np.zeros(records.shape, np.float32) for _ in range(3))
    check(lib().sgz_overview_power_readout(_np_ptr(records), records.size, _np_ptr(ms), _np_ptr(rms), _np_ptr(lo), _np_ptr(hi)))
    return ms, rms, lo, hi


# sgz_overview_cross_record (sgz.h, "The cross overview"): 80 bytes, 8-aligned; every sum = (low word, high word) of a 128-bit integer, re and
# im in two's complement.  On the device a record is ten int64 words of a torch tensor [..., 10]; cross_from_device turns such a tensor into a
# numpy array of this dtype.  OVERVIEW_CROSS_READING_DTYPE: sgz_overview_cross_reading, nine doubles
OVERVIEW_CROSS_DTYPE = np.dtype({"names": ["ll", "rr", "re", "im", "count", "skipped"],
                                 "formats": [("<u8", (2,)), ("<u8", (2,)), ("<u8", (2,)), ("<u8", (2,)), "<u8", "<u8"],
                                 "offsets": [0, 16, 32, 48, 64, 72], "itemsize": 80})
OVERVIEW_CROSS_READING_DTYPE = np.dtype([(name, "<f8") for name in ("ll", "rr", "mid", "side", "re", "im", "coherence", "phase", "correlation")])


def cross_from_device(t) -> np.ndarray:
    """cuda int64 [..., 10] (records as the cross calls write them) -> numpy OVERVIEW_CROSS_DTYPE [...]"""
    return _records_from_device(t, OVERVIEW_CROSS_DTYPE)


def cross_to_device(records: np.ndarray, device):
    """numpy OVERVIEW_CROSS_DTYPE [...] -> cuda int64 [..., 10]"""
    return _records_to_device(records, OVERVIEW_CROSS_DTYPE, 10, device)


# sgz_overview_flux_record (sgz.h, "The flux overview"): 88 bytes, 8-aligned; every sum = (low word, high word) of a 128-bit integer.  On the
# device a record is eleven int64 words of a torch tensor [..., 11]; flux_from_device turns such a tensor into a numpy array of this dtype
OVERVIEW_FLUX_DTYPE = np.dtype({"names": ["amp", "mom1", "mom2", "flux", "flux_max", "flux_at", "count", "nans"],
                                "formats": [("<u8", (2,)), ("<u8", (2,)), ("<u8", (2,)), ("<u8", (2,)), "<u8", "<u8", "<u4", "<u4"],
                                "offsets": [0, 16, 32, 48, 64, 72, 80, 84], "itemsize": 88})


def flux_from_device(t) -> np.ndarray:
    """cuda int64 [..., 11] (records as the flux calls write them) -> numpy OVERVIEW_FLUX_DTYPE [...]"""
    return _records_from_device(t, OVERVIEW_FLUX_DTYPE)


def flux_to_device(records: np.ndarray, device):
    """numpy OVERVIEW_FLUX_DTYPE [...] -> cuda int64 [..., 11]"""
    return _records_to_device(records, OVERVIEW_FLUX_DTYPE, 11, device)


def overview_flux_quantise(x: np.ndarray) -> np.ndarray:
    """sgz_overview_flux_quantise (host, no GPU): float32 [...] -> uint64 [...], a of the flux overview's definition (0 for a NaN)"""
    x = np.ascontiguousarray(x, np.float32)
    a = np.zeros(x.shape, np.uint64)
    check(lib().sgz_overview_flux_quantise(_np_ptr(x), x.size, _np_ptr(a)))
    return a


def overview_flux_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_overview_flux_fold (host, no GPU): OVERVIEW_FLUX_DTYPE records [n, ...], source columns [x0, x1) -> [min(out_columns, x1 - x0), ...]"""
    return _overview_fold("sgz_overview_flux_fold", OVERVIEW_FLUX_DTYPE, records, out_columns, x0, x1)


def overview_flux_readout(records: np.ndarray, pixels: int):
    """sgz_overview_flux_readout (host, no GPU): OVERVIEW_FLUX_DTYPE records [...] of rows of `pixels` pixels -> (mean amplitude, centroid in
    pixels, spread in pixels, mean flux, relative flux), float64 planes of the same shape"""
    records = np.ascontiguousarray(records, OVERVIEW_FLUX_DTYPE)
    planes = [np.zeros(records.shape, np.float64) for _ in range(5)]
    check(lib().sgz_overview_flux_readout(_np_ptr(records), records.size, pixels, *[_np_ptr(a) for a in planes]))
    return tuple(planes)


def overview_flux_hz(plan, pixel) -> np.ndarray:
    """sgz_overview_flux_hz (host, no GPU): fractional pixels, float64 [...] -> Hz by linear interpolation of the plan's mapped frequencies"""
    return plan.overview_flux_hz(pixel)


def _edges(edges) -> np.ndarray:
    e = np.ascontiguousarray(edges, np.uint32)
    assert e.ndim == 1 and e.size >= 2, e.shape
    return e


def overview_cross_quantise(n: int, lr, li, rr, ri):
    """sgz_overview_cross_quantise (host, no GPU): the bins (lr + i li, rr + i ri), float32 [...], of a transform of size 2^n -> (q int64
    [..., 4]: a, b, c, d of the cross overview's definition, skipped bool [...])"""
    lr, li, rr, ri = (np.ascontiguousarray(a, np.float32) for a in (lr, li, rr, ri))
    assert lr.shape == li.shape == rr.shape == ri.shape
    q = np.zeros((*lr.shape, 4), np.int64)
    skipped = np.zeros(lr.shape, np.uint8)
    check(lib().sgz_overview_cross_quantise(n, _np_ptr(lr), _np_ptr(li), _np_ptr(rr), _np_ptr(ri), lr.size, _np_ptr(q), _np_ptr(skipped)))
    return q, skipped.astype(bool)


def overview_cross_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None, edges=None, coarse_edges=None) -> np.ndarray:
    """sgz_overview_cross_fold (host, no GPU): OVERVIEW_CROSS_DTYPE records [n, pairs, bands], source columns [x0, x1) -> [min(out_columns,
    x1 - x0), pairs, bands]; with coarse_edges (every one of them among the fine `edges`) also over bands -> [..., pairs, len(coarse_edges) - 1]"""
    records = np.ascontiguousarray(records, OVERVIEW_CROSS_DTYPE)
    assert records.ndim == 3, records.shape
    n, pairs, bands = (int(v) for v in records.shape)
    x1 = n if x1 is None else x1
    e = _edges(edges) if edges is not None else None
    assert e is None or e.size == bands + 1
    ce = _edges(coarse_edges) if coarse_edges is not None else None
    out = np.zeros((overview_view_columns(n, x0, x1, out_columns), pairs, bands if ce is None else ce.size - 1), OVERVIEW_CROSS_DTYPE)
    check(lib().sgz_overview_cross_fold(_np_ptr(records), n, pairs, _np_ptr(e) if e is not None else None, bands, x0, x1, out_columns,
                                        _np_ptr(ce) if ce is not None else None, ce.size - 1 if ce is not None else 0, _np_ptr(out)))
    return out


def overview_cross_readout(records: np.ndarray) -> np.ndarray:
    """sgz_overview_cross_readout (host, no GPU): OVERVIEW_CROSS_DTYPE records [...] -> OVERVIEW_CROSS_READING_DTYPE [...]: the planes ll, rr,
    mid, side, re, im (means per bin-frame in unit power), coherence, phase, correlation"""
    records = np.ascontiguousarray(records, OVERVIEW_CROSS_DTYPE)
    out = np.zeros(records.shape, OVERVIEW_CROSS_READING_DTYPE)
    check(lib().sgz_overview_cross_readout(_np_ptr(records), records.size, _np_ptr(out)))
    return out


def cross_edges_octave(sample_rate: float, N: int, bands_per_octave: int, f_lo: float, f_hi: float, capacity: int = 4097):
    """sgz_cross_edges_octave (host, no GPU): (edges uint32 [bands + 1], centres float64 [bands]) of the fractional-octave bands whose centres
    1000 * 2^(j / bands_per_octave) lie in [f_lo, f_hi]"""
    edges = np.zeros(capacity, np.uint32)
    centres = np.zeros(max(capacity - 1, 1), np.float64)
    bands = C.c_uint32(0)
    check(lib().sgz_cross_edges_octave(sample_rate, N, bands_per_octave, f_lo, f_hi, _np_ptr(edges), capacity, C.byref(bands), _np_ptr(centres)))
    return edges[:bands.value + 1].copy(), centres[:bands.value].copy()


# The overview kinds: what each has of its own in sgz.h.  Plan's stage / render / view helpers, PcmStream.feed_overview* and the overview*_pcm
# one-shots read it from here.  A shape names its extents -- "C" pairs, "sides", "P" axis points, "bands" of the cross table, "bins" N + 1 --
# and _overview_shape puts a plan's or a config's numbers in.
#   suffix        behind sgz_stage_overview, sgz_spectrogram_overview and sgz_pcm_stream_feed_overview
#   source        what the stage call reduces: the shape of one frame of it
#   cell          the shape of the carry and of one column of records
#   dtype, words  the record on the host, and its int64 words [..., words] on the device (0: plain float32 there as well)
#   outputs       in C order: (the want_* keyword that selects it, None where it is compulsory; column shape; dtype[; True: nq leading planes])
#   state, view   the render's device form takes a decay state; the kind has the _view forms
OverviewKind = namedtuple("OverviewKind", "suffix source cell dtype words outputs state view")
_LINES, _MAPPED, _BINS = ("C", NUM_GRAPHS, "P", 2), ("C", "sides", "P"), ("C", "bins", 2)
_RGBA = ("want_rgba", ("P", 4), np.uint8)
OVERVIEW_KINDS = {
    "peaks": OverviewKind("", _LINES, ("C", "P"), np.dtype(np.float32), 0,
                          (_RGBA, ("want_peaks", ("C", "P"), np.float32)), True, True),
    "stats": OverviewKind("_stats", _LINES, ("C", "P"), OVERVIEW_STAT_DTYPE, 3,
                          (_RGBA, ("want_stats", ("C", "P"), OVERVIEW_STAT_DTYPE), ("want_means", ("C", "P"), np.float32)), True, True),
    "pct": OverviewKind("_pct", _LINES, ("C", "P"), OVERVIEW_PCT_DTYPE, 34,
                        (_RGBA, ("want_records", ("C", "P"), OVERVIEW_PCT_DTYPE), ("want_values", ("C", "P"), np.float32, True)), True, False),
    "power": OverviewKind("_power", _MAPPED, ("C", "sides", "P"), OVERVIEW_POWER_DTYPE, 4,
                          (_RGBA, ("want_power", ("C", "sides", "P"), OVERVIEW_POWER_DTYPE), ("want_levels", ("C", "sides", "P"), np.float32)),
                          False, True),
    "cross": OverviewKind("_cross", _BINS, ("C", "bands"), OVERVIEW_CROSS_DTYPE, 10, ((None, ("C", "bands"), OVERVIEW_CROSS_DTYPE),), False, False),
    "flux": OverviewKind("_flux", _MAPPED, ("C", "sides"), OVERVIEW_FLUX_DTYPE, 11, ((None, ("C", "sides"), OVERVIEW_FLUX_DTYPE),), False, False),
}


def _overview_shape(shape, dims) -> tuple:
    """a shape of the kind table at dims = (C, sides, P, bands[, bins])"""
    at = dict(zip(("C", "sides", "P", "bands", "bins"), dims))
    return tuple(at.get(d, d) for d in shape)


def _overview_outputs(kind: OverviewKind, dims, wants=(), planes=None) -> list:
    """the kind's outputs at dims, as (wanted, the shape of one column, dtype[, planes]) each.  wants: the flags of the outputs that have one,
    in C order; planes: how many the output with leading planes has"""
    wants = iter(wants)
    return [(next(wants) if o[0] else True, _overview_shape(o[1], dims), o[2], *((planes,) if o[3:] else ())) for o in kind.outputs]


def _overview_out(cols: int, want, shape, dtype, planes=None, device=None):
    """an overview output's buffer: [columns, *shape], or [planes, columns, *shape]; never an empty array (its pointer may be null).  On the host
    np.zeros; on `device` torch.empty, a record dtype as int64 with its words as the last axis"""
    if not want:
        return None
    full = (max(cols, 1), *shape) if planes is None else (planes, max(cols, 1), *shape)
    if device is None:
        return np.zeros(full, dtype)
    import torch
    dtype = np.dtype(dtype)
    if dtype.fields:
        return torch.empty((*full, dtype.itemsize // 8), dtype=torch.int64, device=device)
    return torch.empty(full, dtype=getattr(torch, dtype.name), device=device)


def _overview_cut(a, cols: int, want, shape, dtype, planes=None):
    return None if a is None else a[:cols] if planes is None else a[:, :cols]


def _buf_ptrs(arrays) -> list:
    return [_buf_ptr(a) if a is not None else None for a in arrays]


def _channel_ptrs(planar: np.ndarray):
    """the calls' `const float *const *channels`: the rows of a contiguous float32 [channels, S] array"""
    return (C.c_void_p * planar.shape[0])(*[planar[i].ctypes.data for i in range(planar.shape[0])])


def _stream(stream):
    import torch
    return stream if stream is not None else torch.cuda.current_stream().cuda_stream


class Plan:
    """The Spectrum constant block (TransformConstant mirror). Host tables need no GPU."""

    def __init__(self, cfg: dict | SpectrumConfig):
        self.cfg = cfg if isinstance(cfg, SpectrumConfig) else config_from_dict(cfg)
        h = C.c_void_p()
        check(lib().sgz_plan_create(C.byref(self.cfg), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().sgz_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self):
        check(lib().sgz_plan_upload(self.h))
        return self

    def set_option(self, option: int, value: int):
        """sgz_plan_set_option: OPT_CHANNEL_SPLIT / OPT_FUSED_COLOUR / OPT_FETCH_WINDOW"""
        check(lib().sgz_plan_set_option(self.h, option, value))
        return self

    @property
    def N(self) -> int:
        return lib().sgz_plan_transform_size(self.h)

    @property
    def P(self) -> int:
        return self.cfg.axis_points

    @property
    def C(self) -> int:
        return self.cfg.num_pairs

    @property
    def sides(self) -> int:
        return _sides(self.cfg)

    @property
    def window_scale(self) -> float:
        return lib().sgz_plan_window_scale(self.h)

    @property
    def break_pixel(self) -> int:
        return lib().sgz_plan_break_pixel(self.h)

    @property
    def path(self) -> int:
        """SGZ_PATH_*: 0 generic, 1 fused, 2 halves (+4: per-side LDS map usable)"""
        return lib().sgz_plan_path(self.h)

    def dc_pixels(self) -> np.ndarray:
        n = lib().sgz_plan_dc_pixels(self.h, None, 0)
        out = np.zeros(max(n, 1), np.uint32)
        lib().sgz_plan_dc_pixels(self.h, _np_ptr(out), n)
        return out[:n]

    def window(self) -> np.ndarray:
        out = np.zeros(self.N, np.float32)
        check(lib().sgz_plan_get_window(self.h, _np_ptr(out)))
        return out

    def mapped_frequencies(self) -> np.ndarray:
        out = np.zeros(self.P, np.float32)
        check(lib().sgz_plan_get_mapped_frequencies(self.h, _np_ptr(out)))
        return out

    def slope_map(self) -> np.ndarray:
        out = np.zeros(self.P, np.float32)
        check(lib().sgz_plan_get_slope_map(self.h, _np_ptr(out)))
        return out

    def colour_ratios(self) -> np.ndarray:
        out = np.zeros(NUM_SPEC_COLOURS + 1, np.float32)
        check(lib().sgz_plan_get_colour_ratios(self.h, _np_ptr(out)))
        return out

    def track_peak_lines(self, results: np.ndarray, mouse_fraction: float) -> dict:
        """sgz_track_peak_lines: the tracker's line-results branch on host results float2 [P] (no upload needed: host arithmetic)"""
        r = np.ascontiguousarray(results, np.float32)
        assert r.size == 2 * self.P
        out = LinePeak()
        check(lib().sgz_track_peak_lines(self.h, _np_ptr(r), float(mouse_fraction), C.byref(out)))
        return out.asdict()

    def track_peak_values(self, values: np.ndarray, mouse_fraction: float) -> dict:
        """sgz_track_peak_values: the same search on a host value plane float [P] -- one (column, pair) of the peaks any overview or view
        call writes (no upload needed: host arithmetic)"""
        v = np.ascontiguousarray(values, np.float32)
        assert v.size == self.P
        out = LinePeak()
        check(lib().sgz_track_peak_values(self.h, _np_ptr(v), float(mouse_fraction), C.byref(out)))
        return out.asdict()

    # the batched tracker: records come back as float64 rows in the field order of Peak (8) / LinePeak (6)
    def track_peaks(self, bins, mouse_fraction: float, out=None, stream=None):
        """sgz_stage_track_peaks: bins -- cuda float32 [..., N + 1] (sgz_stage_bins' records); returns cuda float64 [records, 8]"""
        import torch
        assert bins.is_cuda and bins.dtype == torch.float32 and bins.is_contiguous() and bins.shape[-1] == self.N + 1
        records = bins.numel() // (self.N + 1)
        if out is None:
            out = torch.empty((records, len(Peak._fields_)), dtype=torch.float64, device=bins.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(lib().sgz_stage_track_peaks(self.h, bins.data_ptr(), records, float(mouse_fraction), out.data_ptr(), s))
        return out

    def track_peaks_lines(self, lines, graph: int, mouse_fraction: float, out=None, stream=None):
        """sgz_stage_track_peaks_lines: lines -- cuda float32 [frames, pairs, graphs, P, 2]; returns cuda float64 [frames, pairs, 6]"""
        import torch
        assert lines.is_cuda and lines.dtype == torch.float32 and lines.is_contiguous()
        assert tuple(lines.shape[1:]) == (self.C, NUM_GRAPHS, self.P, 2)
        frames = lines.shape[0]
        if out is None:
            out = torch.empty((frames, self.C, len(LinePeak._fields_)), dtype=torch.float64, device=lines.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(lib().sgz_stage_track_peaks_lines(self.h, lines.data_ptr(), frames, graph, float(mouse_fraction), out.data_ptr(), s))
        return out

    def track_peaks_values(self, values, mouse_fraction: float, out=None, stream=None):
        """sgz_stage_track_peaks_values: values -- cuda float32 [..., P], the peaks of any overview or view call ([columns, pairs, P]);
        returns cuda float64 [*values.shape[:-1], 6]"""
        import torch
        assert values.is_cuda and values.dtype == torch.float32 and values.is_contiguous() and values.shape[-1] == self.P
        records = values.numel() // self.P
        if out is None:
            out = torch.empty(tuple(values.shape[:-1]) + (len(LinePeak._fields_),), dtype=torch.float64, device=values.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(lib().sgz_stage_track_peaks_values(self.h, values.data_ptr(), records, float(mouse_fraction), out.data_ptr(), s))
        return out

    def track_render(self, planar, graph: int, mouse_fraction: float, want_rgba: bool = True, state=None, stream=None):
        """The render that returns a track.  planar a numpy array [2 C, S]: sgz_spectrogram_track_host -> (track float64 [F, C, 6], rgba uint8
        [F, P, 4] or None, timing dict).  planar a cuda tensor: sgz_spectrogram_track_device, asynchronous -> (cuda track, cuda rgba or None).
        Fewer samples than a window: None."""
        if isinstance(planar, np.ndarray):
            planar = np.ascontiguousarray(planar, np.float32)
            nch, S = planar.shape
            F = self.num_frames(S)
            track = np.zeros((max(F, 1), self.C, len(LinePeak._fields_)), np.float64)            # (never a NULL pointer: F == 0 is the call's to refuse)
            rgba = np.zeros((max(F, 1), self.P, 4), np.uint8) if want_rgba else None
            t = Timing()
            st = check(lib().sgz_spectrogram_track_host(self.h, _channel_ptrs(planar), nch, S, graph, float(mouse_fraction),
                                                        _np_ptr(rgba) if want_rgba else None, _np_ptr(track), C.byref(t)))
            if st == SGZ_SKIPPED_FRAME:
                return None
            return track[:F], (rgba[:F] if want_rgba else None), t.asdict()
        import torch
        assert planar.is_cuda and planar.dtype == torch.float32 and planar.stride(1) == 1
        S = planar.shape[1]
        F = self.num_frames(S)
        track = torch.empty((max(F, 1), self.C, len(LinePeak._fields_)), dtype=torch.float64, device=planar.device)      # (never a NULL
        rgba = torch.empty((max(F, 1), self.P, 4), dtype=torch.uint8, device=planar.device) if want_rgba else None        # pointer)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        st = check(lib().sgz_spectrogram_track_device(self.h, planar.data_ptr(), planar.stride(0), S, graph, float(mouse_fraction),
                                                      rgba.data_ptr() if want_rgba else None,
                                                      state.data_ptr() if state is not None else None, track.data_ptr(), s))
        if st == SGZ_SKIPPED_FRAME:
            return None
        return track[:F], (rgba[:F] if want_rgba else None)

    # The overview: k frames per image column, reduced and coloured on the device.  What a kind has of its own is its entry of OVERVIEW_KINDS;
    # the three helpers are every kind's stage call, render and view.  wants: the flags of the kind's optional outputs in C order; front / mid:
    # what the C call takes between flush and slices / in front of the carry (stage) or the outputs (render); bands: of the cross table; planes:
    # of pct's values
    def _overview_stage(self, kind: str, x, k: int, held: int, flush: bool, slices: int, carry, wants=(), front=(), mid=(), bands: int = 0,
                        planes=None, stream=None):
        """sgz_stage_overview<suffix> -> (every output's columns, None where not wanted, frames of the column left open)"""
        import torch
        kind = OVERVIEW_KINDS[kind]
        dims = (self.C, self.sides, self.P, bands, self.N + 1)
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        assert tuple(x.shape[1:]) == _overview_shape(kind.source, dims), tuple(x.shape)
        assert carry is None or (carry.is_cuda and carry.dtype == (torch.int64 if kind.words else torch.float32) and carry.is_contiguous()
                                 and carry.numel() == int(np.prod(_overview_shape(kind.cell, dims))) * max(kind.words, 1))
        frames = x.shape[0]
        columns, held_out = overview_step(k, held, frames, flush)
        outputs = _overview_outputs(kind, dims, wants, planes)
        arrays = [_overview_out(columns, *o, device=x.device) for o in outputs]
        check(getattr(lib(), "sgz_stage_overview" + kind.suffix)(self.h, x.data_ptr(), frames, k, held, int(bool(flush)), *front, slices, *mid,
                                                                 carry.data_ptr() if carry is not None else None, *_buf_ptrs(arrays),
                                                                 _stream(stream)))
        return (*[_overview_cut(a, columns, *o) for a, o in zip(arrays, outputs)], held_out)

    def _overview_render(self, kind: str, planar, k: int, wants=(), mid=(), state=None, bands: int = 0, planes=None, stream=None):
        """sgz_spectrogram_overview<suffix>_host for a numpy array -> (every output's columns, None where not wanted, timing dict);
        sgz_spectrogram_overview<suffix>_device for a cuda tensor -> the outputs alone, a kind's single output bare.  A skipped frame: None"""
        kind = OVERVIEW_KINDS[kind]
        call = "sgz_spectrogram_overview" + kind.suffix
        outputs = _overview_outputs(kind, (self.C, self.sides, self.P, bands), wants, planes)
        host = isinstance(planar, np.ndarray)
        if host:
            planar = np.ascontiguousarray(planar, np.float32)
            nch, S = planar.shape
            columns = -(-self.num_frames(S) // k)
            arrays = [_overview_out(columns, *o) for o in outputs]
            t = Timing()
            st = check(getattr(lib(), call + "_host")(self.h, _channel_ptrs(planar), nch, S, k, *mid, *_buf_ptrs(arrays), C.byref(t)))
        else:
            import torch
            assert planar.is_cuda and planar.dtype == torch.float32 and planar.stride(1) == 1
            S = planar.shape[1]
            columns = -(-self.num_frames(S) // k)
            arrays = [_overview_out(columns, *o, device=planar.device) for o in outputs]
            tail = (state.data_ptr() if state is not None else None,) if kind.state else ()
            st = check(getattr(lib(), call + "_device")(self.h, planar.data_ptr(), planar.stride(0), S, k, *mid, *_buf_ptrs(arrays), *tail,
                                                        _stream(stream)))
        if st == SGZ_SKIPPED_FRAME:
            return None
        cut = [_overview_cut(a, columns, *o) for a, o in zip(arrays, outputs)]
        if host:
            return (*cut, t.asdict())
        return cut[0] if len(cut) == 1 else tuple(cut)

    def _overview_view(self, kind: str, kept, out_columns: int, x0: int, x1, slices: int, wants, stream=None):
        """sgz_overview<suffix>_view_host for kept numpy records [n, *cell] -> (every output, None where not wanted, timing dict);
        sgz_stage_overview<suffix>_view for a cuda tensor of them -> the outputs alone"""
        kind = OVERVIEW_KINDS[kind]
        n = int(kept.shape[0])
        x1 = n if x1 is None else x1
        dims = (self.C, self.sides, self.P)
        cell = _overview_shape(kind.cell, dims)
        outputs = _overview_outputs(kind, dims, wants)
        if isinstance(kept, np.ndarray):
            kept = np.ascontiguousarray(kept, kind.dtype)
            assert tuple(kept.shape[1:]) == cell, tuple(kept.shape)
            cols = overview_view_columns(n, x0, x1, out_columns)
            arrays = [_overview_out(cols, *o) for o in outputs]
            t = Timing()
            check(getattr(lib(), f"sgz_overview{kind.suffix}_view_host")(self.h, _np_ptr(kept), n, x0, x1, out_columns, *_buf_ptrs(arrays), C.byref(t)))
            return (*[_overview_cut(a, cols, *o) for a, o in zip(arrays, outputs)], t.asdict())
        import torch
        assert kept.is_cuda and kept.dtype == (torch.int64 if kind.words else torch.float32) and kept.is_contiguous()
        assert tuple(kept.shape[1:]) == ((*cell, kind.words) if kind.words else cell), tuple(kept.shape)
        cols = overview_view_columns(n, x0, x1, out_columns)
        arrays = [_overview_out(cols, *o, device=kept.device) for o in outputs]
        check(getattr(lib(), f"sgz_stage_overview{kind.suffix}_view")(self.h, kept.data_ptr(), n, x0, x1, out_columns, slices, *_buf_ptrs(arrays),
                                                                      _stream(stream)))
        return tuple(_overview_cut(a, cols, *o) for a, o in zip(arrays, outputs))

    # the peak hold of the main graph
    def overview_columns(self, lines, k: int, held: int = 0, flush: bool = True, slices: int = 0, carry=None, want_rgba: bool = True,
                         want_peaks: bool = False, stream=None):
        """sgz_stage_overview: lines -- cuda float32 [frames, pairs, graphs, P, 2]; carry -- cuda float32 [pairs, P], the open column (read
        when held > 0, written when frames stay open).  Returns (cuda rgba uint8 [columns, P, 4] or None, cuda peaks float32 [columns,
        pairs, P] or None, frames of the column left open)."""
        return self._overview_stage("peaks", lines, k, held, flush, slices, carry, (want_rgba, want_peaks), stream=stream)

    def overview(self, planar, k: int, want_rgba: bool = True, want_peaks: bool = False, state=None, stream=None):
        """The overview render.  planar a numpy array [2 C, S]: sgz_spectrogram_overview_host -> (rgba uint8 [columns, P, 4] or None, peaks
        float32 [columns, C, P] or None, timing dict).  planar a cuda tensor: sgz_spectrogram_overview_device, asynchronous -> (cuda rgba
        or None, cuda peaks or None).  columns = ceil(frames / k).  Fewer samples than a window: None."""
        return self._overview_render("peaks", planar, k, (want_rgba, want_peaks), state=state, stream=stream)

    def overview_view(self, peaks, out_columns: int, x0: int = 0, x1: int | None = None, slices: int = 0, want_rgba: bool = True,
                      want_peaks: bool = False, stream=None):
        """The view of kept peaks [n, C, P] over source columns [x0, x1) (default: to the end) at min(out_columns, x1 - x0) columns.  peaks a
        cuda float32 tensor: sgz_stage_overview_view, asynchronous -> (cuda rgba uint8 [cols, P, 4] or None, cuda peaks float32 [cols, C, P]
        or None).  peaks a numpy array: sgz_overview_view_host -> (rgba or None, peaks or None, timing dict)."""
        return self._overview_view("peaks", peaks, out_columns, x0, x1, slices, (want_rgba, want_peaks), stream)

    # the mean overview: the same columns, reduced to sum / count / nans / lo / hi records and coloured from the mean
    def overview_stats_columns(self, lines, k: int, held: int = 0, flush: bool = True, slices: int = 0, carry=None, want_rgba: bool = True,
                               want_stats: bool = False, want_means: bool = False, stream=None):
        """sgz_stage_overview_stats: lines -- cuda float32 [frames, pairs, graphs, P, 2]; carry -- cuda int64 [pairs, P, 3], the open column's
        records (read when held > 0, written when frames stay open).  Returns (cuda rgba uint8 [columns, P, 4] or None, cuda records int64
        [columns, pairs, P, 3] or None -- see stats_from_device --, cuda means float32 [columns, pairs, P] or None, frames left open)."""
        return self._overview_stage("stats", lines, k, held, flush, slices, carry, (want_rgba, want_stats, want_means), stream=stream)

    def overview_stats(self, planar, k: int, want_rgba: bool = True, want_stats: bool = False, want_means: bool = False, state=None, stream=None):
        """The mean overview's render.  planar a numpy array [2 C, S]: sgz_spectrogram_overview_stats_host -> (rgba or None, records
        OVERVIEW_STAT_DTYPE [columns, C, P] or None, means float32 [columns, C, P] or None, timing dict).  planar a cuda tensor:
        sgz_spectrogram_overview_stats_device, asynchronous -> (cuda rgba, cuda records int64 [columns, C, P, 3], cuda means), None where not
        wanted.  Fewer samples than a window: None."""
        return self._overview_render("stats", planar, k, (want_rgba, want_stats, want_means), state=state, stream=stream)

    def overview_stats_view(self, stats, out_columns: int, x0: int = 0, x1: int | None = None, slices: int = 0, want_rgba: bool = True,
                            want_stats: bool = False, want_means: bool = False, stream=None):
        """The view of kept records over source columns [x0, x1) (default: to the end) at min(out_columns, x1 - x0) columns.  stats a cuda
        int64 tensor [n, C, P, 3]: sgz_stage_overview_stats_view, asynchronous -> (cuda rgba, cuda records, cuda means), None where not
        wanted.  stats a numpy OVERVIEW_STAT_DTYPE array [n, C, P]: sgz_overview_stats_view_host -> (rgba, records, means, timing dict)."""
        return self._overview_view("stats", stats, out_columns, x0, x1, slices, (want_rgba, want_stats, want_means), stream)

    # the percentile overview: the same columns, reduced to 66-bucket records; nq quantile planes, the image coloured from quantile 0
    def overview_pct_columns(self, lines, k: int, q=0.5, held: int = 0, flush: bool = True, slices: int = 0, carry=None, want_rgba: bool = True,
                             want_records: bool = False, want_values: bool = False, stream=None):
        """sgz_stage_overview_pct: lines -- cuda float32 [frames, pairs, graphs, P, 2]; q -- a quantile or up to 8 of them; carry -- cuda
        int64 [pairs, P, 34], the open column's records (read when held > 0, written when frames stay open).  Returns (cuda rgba uint8
        [columns, P, 4] or None, cuda records int64 [columns, pairs, P, 34] or None -- see pct_from_device --, cuda values float32
        [nq, columns, pairs, P] or None, frames left open)."""
        qa, qp, nq = _quantiles(q)
        return self._overview_stage("pct", lines, k, held, flush, slices, carry, (want_rgba, want_records, want_values), mid=(qp, nq),
                                    planes=max(nq, 1), stream=stream)

    def overview_pct(self, planar, k: int, q=0.5, want_rgba: bool = True, want_records: bool = False, want_values: bool = False, state=None, stream=None):
        """The percentile overview's render.  planar a numpy array [2 C, S]: sgz_spectrogram_overview_pct_host -> (rgba or None, records
        OVERVIEW_PCT_DTYPE [columns, C, P] or None, values float32 [nq, columns, C, P] or None, timing dict).  planar a cuda tensor:
        sgz_spectrogram_overview_pct_device, asynchronous -> (cuda rgba, cuda records int64 [columns, C, P, 34], cuda values), None where
        not wanted.  Fewer samples than a window: None."""
        qa, qp, nq = _quantiles(q)
        return self._overview_render("pct", planar, k, (want_rgba, want_records, want_values), mid=(qp, nq), state=state, planes=max(nq, 1),
                                     stream=stream)

    # the power overview: the same columns over the mapped magnitudes, reduced to 128-bit sums of squares and coloured from the rms' level
    def overview_power_columns(self, mapped, k: int, held: int = 0, flush: bool = True, slices: int = 0, carry=None, want_rgba: bool = True,
                               want_power: bool = False, want_levels: bool = False, stream=None):
        """sgz_stage_overview_power: mapped -- cuda float32 [frames, pairs, sides, P]; carry -- cuda int64 [pairs, sides, P, 4], the open column's
        records (read when held > 0, written when frames stay open).  Returns (cuda rgba uint8 [columns, P, 4] or None, cuda records int64
        [columns, pairs, sides, P, 4] or None -- see power_from_device --, cuda levels float32 [columns, pairs, sides, P] or None, frames left
        open)."""
        return self._overview_stage("power", mapped, k, held, flush, slices, carry, (want_rgba, want_power, want_levels), stream=stream)

    def overview_power(self, planar, k: int, want_rgba: bool = True, want_power: bool = False, want_levels: bool = False, stream=None):
        """The power overview's render.  planar a numpy array [2 C, S]: sgz_spectrogram_overview_power_host -> (rgba or None, records
        OVERVIEW_POWER_DTYPE [columns, C, sides, P] or None, levels float32 [columns, C, sides, P] or None, timing dict).  planar a cuda tensor:
        sgz_spectrogram_overview_power_device, asynchronous -> (cuda rgba, cuda records int64 [columns, C, sides, P, 4], cuda levels), None
        where not wanted.  Fewer samples than a window: None."""
        return self._overview_render("power", planar, k, (want_rgba, want_power, want_levels), stream=stream)

    def overview_power_view(self, power, out_columns: int, x0: int = 0, x1: int | None = None, slices: int = 0, want_rgba: bool = True,
                            want_power: bool = False, want_levels: bool = False, stream=None):
        """The view of kept power records over source columns [x0, x1) (default: to the end) at min(out_columns, x1 - x0) columns.  power a
        cuda int64 tensor [n, C, sides, P, 4]: sgz_stage_overview_power_view, asynchronous -> (cuda rgba, cuda records, cuda levels), None where
        not wanted.  power a numpy OVERVIEW_POWER_DTYPE array [n, C, sides, P]: sgz_overview_power_view_host -> (rgba, records, levels, timing
        dict)."""
        return self._overview_view("power", power, out_columns, x0, x1, slices, (want_rgba, want_power, want_levels), stream)

    def overview_power_levels(self, records: np.ndarray) -> np.ndarray:
        """sgz_overview_power_levels (host, no GPU): OVERVIEW_POWER_DTYPE records [columns, C, sides, P] (or [C, sides, P]: one column) -> float32
        levels of the same shape, by the plan's host tables -- the spectrum of a selection is overview_power_fold, then this"""
        records = np.ascontiguousarray(records, OVERVIEW_POWER_DTYPE)
        assert tuple(records.shape[-3:]) == (self.C, self.sides, self.P), tuple(records.shape)
        levels = np.zeros(records.shape, np.float32)
        check(lib().sgz_overview_power_levels(self.h, _np_ptr(records), records.size // (self.C * self.sides * self.P), _np_ptr(levels)))
        return levels

    # the cross overview: the complex bins of an SGZ_CH_PHASE plan reduced to band sums of |L|^2, |R|^2 and L conj R per column
    def set_cross_edges(self, edges) -> None:
        """sgz_plan_set_cross_edges: the band table, uint32 [bands + 1]; band b holds the bins edges[b] <= k < edges[b + 1]"""
        e = _edges(edges)
        check(lib().sgz_plan_set_cross_edges(self.h, _np_ptr(e), e.size - 1))
        self.cross_bands = int(e.size - 1)

    def overview_cross_unit(self) -> float:
        unit = C.c_double(0.0)
        check(lib().sgz_overview_cross_unit(self.h, C.byref(unit)))
        return unit.value

    def overview_cross_columns(self, bins, k: int, held: int = 0, flush: bool = True, slices: int = 0, carry=None, stream=None):
        """sgz_stage_overview_cross: bins -- cuda float32 [frames, pairs, N + 1, 2] (stage_bins of a Phase plan); carry -- cuda int64 [pairs,
        bands, 10], the open column's records (read when held > 0, written when frames stay open).  Returns (cuda records int64 [columns,
        pairs, bands, 10] -- see cross_from_device --, frames left open)."""
        return self._overview_stage("cross", bins, k, held, flush, slices, carry, bands=self.cross_bands, stream=stream)

    def overview_cross(self, planar, k: int, stream=None):
        """The cross overview's render.  planar a numpy array [2 C, S]: sgz_spectrogram_overview_cross_host -> (records OVERVIEW_CROSS_DTYPE
        [columns, C, bands], timing dict).  planar a cuda tensor: sgz_spectrogram_overview_cross_device, asynchronous -> cuda records int64
        [columns, C, bands, 10].  Fewer samples than a window: None."""
        return self._overview_render("cross", planar, k, bands=self.cross_bands, stream=stream)

    # the flux overview: the mapped magnitudes reduced along the axis to amplitude, two moments and the rectified difference against the frame before
    def overview_flux_columns(self, mapped, k: int, held: int = 0, flush: bool = True, first_frame: int = 0, slices: int = 0, prev=None, carry=None,
                              stream=None):
        """sgz_stage_overview_flux: mapped -- cuda float32 [frames, pairs, sides, P]; prev -- cuda float32 [pairs, sides, P], the frame before
        mapped[0] (None: the first frame has no predecessor), overwritten with mapped[-1]; carry -- cuda int64 [pairs, sides, 11], the open
        column's records (read when held > 0, written when frames stay open).  Returns (cuda records int64 [columns, pairs, sides, 11] -- see
        flux_from_device --, frames left open)."""
        import torch
        assert prev is None or (prev.is_cuda and prev.dtype == torch.float32 and prev.is_contiguous() and prev.numel() == self.C * self.sides * self.P)
        return self._overview_stage("flux", mapped, k, held, flush, slices, carry, front=(first_frame,),
                                    mid=(prev.data_ptr() if prev is not None else None,), stream=stream)

    def overview_flux(self, planar, k: int, stream=None):
        """The flux overview's render.  planar a numpy array [2 C, S]: sgz_spectrogram_overview_flux_host -> (records OVERVIEW_FLUX_DTYPE
        [columns, C, sides], timing dict).  planar a cuda tensor: sgz_spectrogram_overview_flux_device, asynchronous -> cuda records int64
        [columns, C, sides, 11].  Fewer samples than a window: None."""
        return self._overview_render("flux", planar, k, stream=stream)

    def overview_flux_hz(self, pixel) -> np.ndarray:
        """sgz_overview_flux_hz (host, no GPU): fractional pixels (a centroid), float64 [...] -> Hz, float64 [...], by linear interpolation of
        the plan's mapped frequencies"""
        x = np.ascontiguousarray(pixel, np.float64)
        hz = np.zeros(x.shape, np.float64)
        check(lib().sgz_overview_flux_hz(self.h, _np_ptr(x), x.size, _np_ptr(hz)))
        return hz

    def colour_table(self, pair: int) -> np.ndarray:
        out = np.zeros((NUM_SPEC_COLOURS + 1, 3), np.float32)
        check(lib().sgz_plan_get_colour_table(self.h, pair, _np_ptr(out)))
        return out

    def num_frames(self, nsamples: int) -> int:
        return int(lib().sgz_plan_num_frames(self.h, nsamples))

    def resonator(self):
        """RSNT plans: (coeff [V][P] complex64, gain [P], weights [V]) of the resonator bank."""
        V = C.c_uint32(0)
        check(lib().sgz_plan_get_resonator(self.h, C.byref(V), None, None, None))
        coeff = np.zeros((V.value, self.P), np.complex64)
        gain = np.zeros(self.P, np.float32)
        weights = np.zeros(V.value, np.float32)
        check(lib().sgz_plan_get_resonator(self.h, None, _np_ptr(coeff), _np_ptr(gain), _np_ptr(weights)))
        return coeff, gain, weights

    def reset_resonator(self, stream=None):
        import torch
        check(lib().sgz_plan_reset_resonator(self.h, stream if stream is not None else torch.cuda.current_stream().cuda_stream))

    # ---- device entry points (torch tensors on the GPU) -------------------------------------------
    def render(self, planar, rgba=None, lines=None, state=None, stream=None):
        """planar: torch.float32 [2*C, S] (cuda, contiguous rows). Returns rgba uint8 [F, P, 4]."""
        import torch
        assert planar.is_cuda and planar.dtype == torch.float32 and planar.stride(1) == 1
        S = planar.shape[1]
        F = self.num_frames(S)
        if rgba is None:
            rgba = torch.empty((F, self.P, 4), dtype=torch.uint8, device=planar.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(lib().sgz_spectrogram_render_device(
            self.h, planar.data_ptr(), planar.stride(0), S, rgba.data_ptr(),
            lines.data_ptr() if lines is not None else None,
            state.data_ptr() if state is not None else None, s))
        return rgba

    def stage_bins(self, planar):
        import torch
        S = planar.shape[1]
        F = self.num_frames(S)
        # Phase mode keeps the bins complex: (re, im) pairs instead of magnitudes
        shape = (F, self.C, self.N + 1, 2) if self.cfg.channel_mode == 4 else (F, self.C, self.N + 1)
        out = torch.empty(shape, dtype=torch.float32, device=planar.device)
        check(lib().sgz_stage_bins(self.h, planar.data_ptr(), planar.stride(0), S, out.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream))
        return out

    def stage_mapped(self, planar):
        import torch
        S = planar.shape[1]
        F = self.num_frames(S)
        out = torch.empty((F, self.C, self.sides, self.P), dtype=torch.float32, device=planar.device)
        check(lib().sgz_stage_mapped(self.h, planar.data_ptr(), planar.stride(0), S, out.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream))
        return out

    def stage_nyquist(self, planar, image_only: bool):
        """sgz_stage_nyquist: (ny [F][C][2] float32 on the device, frames per Nyquist workgroup (0: two-channel launch), low pixels)"""
        import torch
        S = planar.shape[1]
        F = self.num_frames(S)
        out = torch.empty((F, self.C, 2), dtype=torch.float32, device=planar.device)
        nyf, low = C.c_uint32(0), C.c_uint32(0)
        check(lib().sgz_stage_nyquist(self.h, planar.data_ptr(), planar.stride(0), S, 1 if image_only else 0, out.data_ptr(),
                                      C.byref(nyf), C.byref(low), torch.cuda.current_stream().cuda_stream))
        return out, nyf.value, low.value

    def stage_map_from_bins(self, bins):
        import torch
        F = bins.shape[0]
        out = torch.empty((F, self.C, self.sides, self.P), dtype=torch.float32, device=bins.device)
        check(lib().sgz_stage_map_from_bins(self.h, bins.data_ptr(), F, out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
        return out

    def stage_decay_colour(self, mapped, want_lines=False, state=None, want_rgba=True):
        import torch
        F = mapped.shape[0]
        rgba = torch.empty((F, self.P, 4), dtype=torch.uint8, device=mapped.device) if want_rgba else None
        lines = torch.empty((F, self.C, NUM_GRAPHS, self.P, 2), dtype=torch.float32, device=mapped.device) if want_lines else None
        check(lib().sgz_stage_decay_colour(self.h, mapped.data_ptr(), F, rgba.data_ptr() if want_rgba else None,
                                           lines.data_ptr() if want_lines else None,
                                           state.data_ptr() if state is not None else None,
                                           torch.cuda.current_stream().cuda_stream))
        return rgba, lines


    def fold_carry(self, aggs, frames_per_rank, rank: int, carry):
        """aggs: cuda float32 [world, C, G, P, 2]; carry: cuda float32 [C, G, P, 2] (out)."""
        import torch
        world = aggs.shape[0]
        fr = (C.c_int64 * world)(*[int(f) for f in frames_per_rank])
        check(lib().sgz_decay_fold_carry(self.h, aggs.data_ptr(), fr, world, rank, carry.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream))
        return carry


class RenderQueue:
    """sgz_render_queue: `depth` lanes of (plan, stream); renders of independent device buffers submitted round-robin (sgz.h)."""

    def __init__(self, cfg: dict, depth: int = 3):
        self.cfg = config_from_dict(cfg)
        self.h = C.c_void_p()
        check(lib().sgz_render_queue_create(C.byref(self.cfg), depth, C.byref(self.h)))
        self.depth = depth
        self.distinct_lanes = int(lib().sgz_render_queue_distinct_lanes(self.h))

    def submit(self, planar, rgba, after_stream=None) -> int:
        """planar: torch.float32 [2*C, S] (cuda), rgba: torch.uint8 [F, P, 4] (cuda); returns the ticket"""
        t = C.c_uint64(0)
        check(lib().sgz_render_queue_submit(self.h, C.c_void_p(planar.data_ptr()), C.c_size_t(planar.stride(0)), C.c_size_t(planar.shape[1]),
                                            C.c_void_p(rgba.data_ptr()), C.c_void_p(after_stream) if after_stream else None, C.byref(t)))
        return int(t.value)

    def wait(self, ticket: int = 0):
        check(lib().sgz_render_queue_wait(self.h, C.c_uint64(ticket)))

    def join(self, stream: int):
        check(lib().sgz_render_queue_join(self.h, C.c_void_p(stream)))

    def set_option(self, option: int, value: int):
        check(lib().sgz_render_queue_set_option(self.h, option, value))
        return self

    def close(self):
        if self.h:
            lib().sgz_render_queue_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:                                           # noqa: BLE001
            pass


def render_spectrogram(cfg: dict, planar: np.ndarray, want_lines: bool = False):
    """Host-buffer batch render (sgz_spectrogram_render). planar: float32 [2*C, S]."""
    c = config_from_dict(cfg)
    planar = np.ascontiguousarray(planar, np.float32)
    nch, S = planar.shape
    F = S // c.hop if c.algorithm == 1 else lib().sgz_num_frames(S, c.window_size, c.hop)
    rgba = np.zeros((F, c.axis_points, 4), np.uint8)
    lines = np.zeros((F, c.num_pairs, NUM_GRAPHS, c.axis_points, 2), np.float32) if want_lines else None
    t = Timing()
    check(lib().sgz_spectrogram_render(C.byref(c), _channel_ptrs(planar), nch, S, _np_ptr(rgba),
                                       _np_ptr(lines) if want_lines else None, C.byref(t)))
    return rgba, lines, t.asdict()


def render_spectrogram_host(plan, planar: np.ndarray, want_lines: bool = False):
    """Host-buffer render on a plan the caller keeps (sgz_spectrogram_render_host): no table rebuild, no allocation after the first call."""
    planar = np.ascontiguousarray(planar, np.float32)
    nch, S = planar.shape
    F = plan.num_frames(S)
    rgba = np.zeros((F, plan.P, 4), np.uint8)
    lines = np.zeros((F, plan.cfg.num_pairs, NUM_GRAPHS, plan.P, 2), np.float32) if want_lines else None
    t = Timing()
    check(lib().sgz_spectrogram_render_host(plan.h, _channel_ptrs(planar), nch, S, _np_ptr(rgba), _np_ptr(lines) if want_lines else None, C.byref(t)))
    return rgba, lines, t.asdict()


def stream_step(window_size: int, hop: int, held: int, incoming: int):
    """sgz_stream_step (host arithmetic, no GPU): (frames that become complete, samples kept for the next step)"""
    f, k = C.c_uint64(0), C.c_uint64(0)
    check(lib().sgz_stream_step(window_size, hop, held, incoming, C.byref(f), C.byref(k)))
    return int(f.value), int(k.value)


def _channel_map(channel_map):
    if channel_map is None:
        return None, None
    m = np.ascontiguousarray(channel_map, np.uint32)
    return m, _np_ptr(m)


def pcm_to_planar_device(pcm, fmt: int, src_channels: int, nsamples: int, planar, channel_map=None, num_channels: int | None = None,
                         channel_stride: int | None = None, stream=None) -> None:
    """sgz_pcm_to_planar_device: pcm -- a cuda tensor of interleaved bytes (any dtype; its data pointer is the first sample), planar -- a cuda
    float32 tensor [num_channels, >= nsamples] with contiguous rows.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    m, mp = _channel_map(channel_map)
    nch = num_channels if num_channels is not None else (len(m) if m is not None else planar.shape[0])
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    check(lib().sgz_pcm_to_planar_device(_buf_ptr(pcm), fmt, src_channels, nsamples, mp, nch, _buf_ptr(planar),
                                         channel_stride if channel_stride is not None else planar.stride(0), s))


class PcmStream:
    """sgz_pcm_stream: interleaved PCM in pieces -> spectrogram columns as they become complete (sgz.h "interleaved PCM in").
    pcm: a numpy array or a host torch tensor (pinned memory is uploaded from in place) holding nsamples * src_channels samples of the
    format; the bytes are taken as they lie."""

    def __init__(self, cfg, fmt: int, src_channels: int, channel_map=None, chunk_samples: int = 0):
        self.cfg = _as_config(cfg)
        self.format, self.src_channels = fmt, src_channels
        self.frame_bytes = src_channels * PCM_SAMPLE_BYTES.get(fmt, 0)
        m, mp = _channel_map(channel_map)
        self.h = C.c_void_p()
        check(lib().sgz_pcm_stream_create(C.byref(self.cfg), fmt, src_channels, mp, chunk_samples, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().sgz_pcm_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                                           # noqa: BLE001
            pass

    def frames_for(self, nsamples: int) -> int:
        return int(lib().sgz_pcm_stream_frames_for(self.h, nsamples))

    def reset(self):
        check(lib().sgz_pcm_stream_reset(self.h))

    def feed_into(self, pcm, nsamples: int, rgba, lines, capacity_frames: int, timing: bool = True):
        """the C call as it is: (status, frames_out, PcmTiming or None); rgba / lines: numpy arrays or host torch tensors (lines may be None)"""
        t, f = PcmTiming() if timing else None, C.c_uint64(0)
        st = lib().sgz_pcm_stream_feed(self.h, _buf_ptr(pcm) if pcm is not None else None, nsamples, _buf_ptr(rgba) if rgba is not None else None,
                                       _buf_ptr(lines) if lines is not None else None, capacity_frames, C.byref(f), C.byref(t) if timing else None)
        return st, int(f.value), t

    def feed(self, pcm, nsamples: int | None = None, want_lines: bool = False):
        """Feeds nsamples (default: all of pcm) and returns (rgba uint8 [frames, P, 4], lines float32 [frames, pairs, graphs, P, 2] or None,
        timing dict)."""
        nbytes = pcm.numel() * pcm.element_size() if hasattr(pcm, "data_ptr") else pcm.nbytes
        n = nbytes // self.frame_bytes if nsamples is None else nsamples
        F, P = self.frames_for(n), self.cfg.axis_points
        rgba = np.zeros((max(F, 1), P, 4), np.uint8)
        lines = np.zeros((max(F, 1), self.cfg.num_pairs, NUM_GRAPHS, P, 2), np.float32) if want_lines else None
        st, f, t = self.feed_into(pcm if n else None, n, rgba, lines, F)
        check(st)
        assert f == F, (f, F)
        return rgba[:F], lines[:F] if want_lines else None, t.asdict()

    def set_option(self, option: int, value: int) -> None:
        """sgz_pcm_stream_set_option: a plan option (OPT_*) on the stream's own plan"""
        check(lib().sgz_pcm_stream_set_option(self.h, option, value))

    def columns_for(self, nsamples: int, k: int, flush: bool = False) -> int:
        """sgz_pcm_stream_columns_for: overview columns the next feed of nsamples yields at k"""
        return int(lib().sgz_pcm_stream_columns_for(self.h, nsamples, k, int(bool(flush))))

    def open_frames(self) -> int:
        """sgz_pcm_stream_open_frames: frames of the overview column that is open"""
        return int(lib().sgz_pcm_stream_open_frames(self.h))

    # the six overview feeds: `call` is the C call's suffix behind sgz_pcm_stream_feed_overview; mid: what the C call takes between flush and
    # its outputs.  What the outputs are comes from the kind's entry of OVERVIEW_KINDS
    def _feed_overview_into(self, call: str, pcm, nsamples: int, k: int, flush: bool, outputs, capacity_columns: int, timing: bool, mid=()):
        t, c = PcmTiming() if timing else None, C.c_uint64(0)
        st = getattr(lib(), "sgz_pcm_stream_feed_overview" + call)(self.h, _buf_ptr(pcm) if pcm is not None else None, nsamples, k, int(bool(flush)),
                                                                   *mid, *_buf_ptrs(outputs), capacity_columns, C.byref(c),
                                                                   C.byref(t) if timing else None)
        return st, int(c.value), t

    def _feed_overview(self, kind: str, pcm, k: int, flush: bool, nsamples, wants=(), mid=(), planes=None):
        """kind: of OVERVIEW_KINDS; wants: the flags of its optional outputs in C order; planes: of pct's values -> the columns that closed of
        every output, None where not wanted, and the timing dict"""
        kind, cfg = OVERVIEW_KINDS[kind], self.cfg
        outputs = _overview_outputs(kind, (cfg.num_pairs, _sides(cfg), cfg.axis_points, getattr(self, "cross_bands", 1)), wants, planes)
        if pcm is None:
            n = 0
        else:
            nbytes = pcm.numel() * pcm.element_size() if hasattr(pcm, "data_ptr") else pcm.nbytes
            n = nbytes // self.frame_bytes if nsamples is None else nsamples
        cols = self.columns_for(n, k, flush)                        # (0 as well for a k the call refuses)
        arrays = [_overview_out(cols, *o) for o in outputs]
        st, c, t = self._feed_overview_into(kind.suffix, pcm if n else None, n, k, flush, arrays, cols, True, mid)
        check(st)
        assert c == cols, (c, cols)
        return (*[_overview_cut(a, cols, *o) for a, o in zip(arrays, outputs)], t.asdict())

    def feed_overview_into(self, pcm, nsamples: int, k: int, flush: bool, rgba, peaks, capacity_columns: int, timing: bool = True):
        """the C call as it is: (status, columns_out, PcmTiming or None); rgba / peaks: numpy arrays, host torch tensors or None"""
        return self._feed_overview_into("", pcm, nsamples, k, flush, (rgba, peaks), capacity_columns, timing)

    def feed_overview(self, pcm, k: int, flush: bool = False, nsamples: int | None = None, want_rgba: bool = True, want_peaks: bool = False):
        """Feeds nsamples (default: all of pcm; pcm None: none) into the overview at k frames per column and returns the columns that closed:
        (rgba uint8 [columns, P, 4] or None, peaks float32 [columns, pairs, P] or None, timing dict)."""
        return self._feed_overview("peaks", pcm, k, flush, nsamples, (want_rgba, want_peaks))

    def feed_overview_stats_into(self, pcm, nsamples: int, k: int, flush: bool, rgba, stats, means, capacity_columns: int, timing: bool = True):
        """the C call as it is: (status, columns_out, PcmTiming or None); rgba / stats / means: numpy arrays, host torch tensors or None"""
        return self._feed_overview_into("_stats", pcm, nsamples, k, flush, (rgba, stats, means), capacity_columns, timing)

    def feed_overview_stats(self, pcm, k: int, flush: bool = False, nsamples: int | None = None, want_rgba: bool = True, want_stats: bool = True,
                            want_means: bool = False):
        """Feeds nsamples (default: all of pcm; pcm None: none) into the mean overview at k frames per column and returns the columns that
        closed: (rgba uint8 [columns, P, 4] or None, records OVERVIEW_STAT_DTYPE [columns, pairs, P] or None, means float32 [columns,
        pairs, P] or None, timing dict)."""
        return self._feed_overview("stats", pcm, k, flush, nsamples, (want_rgba, want_stats, want_means))

    def feed_overview_pct_into(self, pcm, nsamples: int, k: int, flush: bool, q, rgba, records, values, capacity_columns: int, timing: bool = True):
        """the C call as it is: (status, columns_out, PcmTiming or None); rgba / records / values: numpy arrays, host torch tensors or None;
        values is [nq, capacity_columns, pairs, P]"""
        qa, qp, nq = _quantiles(q)
        return self._feed_overview_into("_pct", pcm, nsamples, k, flush, (rgba, records, values), capacity_columns, timing, (qp, nq))

    def feed_overview_pct(self, pcm, k: int, q=0.5, flush: bool = False, nsamples: int | None = None, want_rgba: bool = True, want_records: bool = True,
                          want_values: bool = False):
        """Feeds nsamples (default: all of pcm; pcm None: none) into the percentile overview at k frames per column and returns the columns
        that closed: (rgba uint8 [columns, P, 4] or None, records OVERVIEW_PCT_DTYPE [columns, pairs, P] or None, values float32 [nq,
        columns, pairs, P] or None, timing dict)."""
        qa, qp, nq = _quantiles(q)
        return self._feed_overview("pct", pcm, k, flush, nsamples, (want_rgba, want_records, want_values), (qp, nq), max(nq, 1))

    def feed_overview_power_into(self, pcm, nsamples: int, k: int, flush: bool, rgba, power, levels, capacity_columns: int, timing: bool = True):
        """the C call as it is: (status, columns_out, PcmTiming or None); rgba / power / levels: numpy arrays, host torch tensors or None"""
        return self._feed_overview_into("_power", pcm, nsamples, k, flush, (rgba, power, levels), capacity_columns, timing)

    def feed_overview_power(self, pcm, k: int, flush: bool = False, nsamples: int | None = None, want_rgba: bool = True, want_power: bool = True,
                            want_levels: bool = False):
        """Feeds nsamples (default: all of pcm; pcm None: none) into the power overview at k frames per column and returns the columns that
        closed: (rgba uint8 [columns, P, 4] or None, records OVERVIEW_POWER_DTYPE [columns, pairs, sides, P] or None, levels float32 [columns,
        pairs, sides, P] or None, timing dict).  The stream's decay state is neither read nor advanced."""
        return self._feed_overview("power", pcm, k, flush, nsamples, (want_rgba, want_power, want_levels))

    def set_cross_edges(self, edges) -> None:
        """sgz_pcm_stream_set_cross_edges: the band table of the stream's cross feeds, uint32 [bands + 1]"""
        e = _edges(edges)
        check(lib().sgz_pcm_stream_set_cross_edges(self.h, _np_ptr(e), e.size - 1))
        self.cross_bands = int(e.size - 1)

    def feed_overview_cross_into(self, pcm, nsamples: int, k: int, flush: bool, cross, capacity_columns: int, timing: bool = True):
        """the C call as it is: (status, columns_out, PcmTiming or None); cross: a numpy array, a host torch tensor or None"""
        return self._feed_overview_into("_cross", pcm, nsamples, k, flush, (cross,), capacity_columns, timing)

    def feed_overview_cross(self, pcm, k: int, flush: bool = False, nsamples: int | None = None):
        """Feeds nsamples (default: all of pcm; pcm None: none) into the cross overview at k frames per column and returns the columns that
        closed: (records OVERVIEW_CROSS_DTYPE [columns, pairs, bands], timing dict).  The stream's decay state is neither read nor advanced."""
        return self._feed_overview("cross", pcm, k, flush, nsamples)

    def feed_overview_flux_into(self, pcm, nsamples: int, k: int, flush: bool, flux, capacity_columns: int, timing: bool = True):
        """the C call as it is: (status, columns_out, PcmTiming or None); flux: a numpy array, a host torch tensor or None"""
        return self._feed_overview_into("_flux", pcm, nsamples, k, flush, (flux,), capacity_columns, timing)

    def feed_overview_flux(self, pcm, k: int, flush: bool = False, nsamples: int | None = None):
        """Feeds nsamples (default: all of pcm; pcm None: none) into the flux overview at k frames per column and returns the columns that
        closed: (records OVERVIEW_FLUX_DTYPE [columns, pairs, sides], timing dict).  The stream's decay state is neither read nor advanced."""
        return self._feed_overview("flux", pcm, k, flush, nsamples)

    # the eight column lanes (waveform, level, truepeak, loudness, field, band, hist, run): one helper per kind of call, the lane's name picks the C call
    def _lane_set(self, lane: str, m: int, out, capacity_columns, *front) -> None:
        if capacity_columns is None:
            capacity_columns = 0 if out is None else int(out.shape[0])
        check(getattr(lib(), f"sgz_pcm_stream_set_{lane}")(self.h, *front, m, _buf_ptr(out) if out is not None and m else None,
                                                           capacity_columns if m else 0))
        setattr(self, f"_{lane}_out", out if m else None)                # (kept alive here: the stream writes to it)

    def _lane_for(self, lane: str, nsamples: int, flush: bool) -> int:
        return int(getattr(lib(), f"sgz_pcm_stream_{lane}_for")(self.h, nsamples, int(bool(flush))))

    def _lane_state(self, lane: str):
        c, o = C.c_uint64(0), C.c_uint64(0)
        check(getattr(lib(), f"sgz_pcm_stream_{lane}_state")(self.h, C.byref(c), C.byref(o)))
        return int(c.value), int(o.value)

    def _lane_flush(self, lane: str) -> None:
        check(getattr(lib(), f"sgz_pcm_stream_flush_{lane}")(self.h))

    # the waveform lane: (lo, hi) per column of m samples and channel, beside whatever the feeds render
    def set_waveform(self, m: int, out=None, capacity_columns: int | None = None) -> None:
        """sgz_pcm_stream_set_waveform: out -- a float32 numpy array or host torch tensor [capacity, channels, 2] (kept alive here; pinned
        memory is written in place); m == 0 disarms"""
        self._lane_set("waveform", m, out, capacity_columns)

    def waveform_for(self, nsamples: int, flush: bool = False) -> int:
        """sgz_pcm_stream_waveform_for: waveform columns the next feed of nsamples closes"""
        return self._lane_for("waveform", nsamples, flush)

    def waveform_state(self):
        """sgz_pcm_stream_waveform_state: (columns written since the lane was armed, samples of the open column)"""
        return self._lane_state("waveform")

    def flush_waveform(self) -> None:
        """sgz_pcm_stream_flush_waveform: closes the open column (one more column at the cursor); waits"""
        self._lane_flush("waveform")

    # the level lane: one sgz_level_record per column of m samples and pair, beside whatever the feeds render
    def set_level(self, m: int, out=None, capacity_columns: int | None = None) -> None:
        """sgz_pcm_stream_set_level: out -- a LEVEL_DTYPE numpy array [capacity, pairs] or a host torch uint8 tensor [capacity, pairs, 80] (kept
        alive here; pinned memory is written in place); m == 0 disarms"""
        self._lane_set("level", m, out, capacity_columns)

    def level_for(self, nsamples: int, flush: bool = False) -> int:
        """sgz_pcm_stream_level_for: level columns the next feed of nsamples closes"""
        return self._lane_for("level", nsamples, flush)

    def level_state(self):
        """sgz_pcm_stream_level_state: (columns written since the lane was armed, samples of the open column)"""
        return self._lane_state("level")

    def flush_level(self) -> None:
        """sgz_pcm_stream_flush_level: closes the open column (one more record per pair at the cursor); waits"""
        self._lane_flush("level")

    # the true-peak lane: one sgz_truepeak_record per column of m samples and channel, beside whatever the feeds render
    def set_truepeak(self, m: int, out=None, capacity_columns: int | None = None) -> None:
        """sgz_pcm_stream_set_truepeak: out -- a TRUEPEAK_DTYPE numpy array [capacity, channels] or a host torch uint8 tensor [capacity, channels,
        16] (kept alive here; pinned memory is written in place); m == 0 disarms"""
        self._lane_set("truepeak", m, out, capacity_columns)

    def truepeak_for(self, nsamples: int, flush: bool = False) -> int:
        """sgz_pcm_stream_truepeak_for: true-peak columns the next feed of nsamples closes"""
        return self._lane_for("truepeak", nsamples, flush)

    def truepeak_state(self):
        """sgz_pcm_stream_truepeak_state: (columns written since the lane was armed, samples of the open column)"""
        return self._lane_state("truepeak")

    def flush_truepeak(self) -> None:
        """sgz_pcm_stream_flush_truepeak: closes the open column (one more record per channel at the cursor); waits"""
        self._lane_flush("truepeak")

    # the loudness lane: one sgz_loudness_record per column of m samples and channel, beside whatever the feeds render
    def set_loudness(self, filter, m: int, out=None, capacity_columns: int | None = None) -> None:
        """sgz_pcm_stream_set_loudness: filter -- a LoudnessFilter (None allowed with m == 0); out -- a LOUDNESS_DTYPE numpy array [capacity,
        channels] or a host torch uint8 tensor [capacity, channels, 32] (kept alive here; pinned memory is written in place); m == 0 disarms"""
        self._lane_set("loudness", m, out, capacity_columns, C.byref(filter) if filter is not None else None)

    def loudness_for(self, nsamples: int, flush: bool = False) -> int:
        """sgz_pcm_stream_loudness_for: loudness columns the next feed of nsamples closes"""
        return self._lane_for("loudness", nsamples, flush)

    def loudness_state(self):
        """sgz_pcm_stream_loudness_state: (columns written since the lane was armed, samples of the open column)"""
        return self._lane_state("loudness")

    def flush_loudness(self) -> None:
        """sgz_pcm_stream_flush_loudness: closes the open column (one more record per channel at the cursor); waits"""
        self._lane_flush("loudness")

    # the stereo-field lane: one sgz_field_record per column of m >= 64 samples and pair, beside whatever the feeds render
    def set_field(self, m: int, out=None, capacity_columns: int | None = None) -> None:
        """sgz_pcm_stream_set_field: out -- a FIELD_DTYPE numpy array [capacity, pairs] or a host torch uint8 tensor [capacity, pairs, 528] (kept
        alive here; pinned memory is written in place); m == 0 disarms, 0 < m < 64 is refused"""
        self._lane_set("field", m, out, capacity_columns)

    def field_for(self, nsamples: int, flush: bool = False) -> int:
        """sgz_pcm_stream_field_for: stereo-field columns the next feed of nsamples closes"""
        return self._lane_for("field", nsamples, flush)

    def field_state(self):
        """sgz_pcm_stream_field_state: (columns written since the lane was armed, samples of the open column)"""
        return self._lane_state("field")

    def flush_field(self) -> None:
        """sgz_pcm_stream_flush_field: closes the open column (one more record per pair at the cursor); waits"""
        self._lane_flush("field")

    # the band lane: one sgz_band_record per column of m >= 64 samples and channel, beside whatever the feeds render
    def set_band(self, filter, m: int, out=None, capacity_columns: int | None = None) -> None:
        """sgz_pcm_stream_set_band: filter -- a BandFilter (None allowed with m == 0); out -- a BAND_DTYPE numpy array [capacity, channels] or a
        host torch uint8 tensor [capacity, channels, 64] (kept alive here; pinned memory is written in place); m == 0 disarms, 0 < m < 64 is
        refused"""
        self._lane_set("band", m, out, capacity_columns, C.byref(filter) if filter is not None else None)

    def band_for(self, nsamples: int, flush: bool = False) -> int:
        """sgz_pcm_stream_band_for: band columns the next feed of nsamples closes"""
        return self._lane_for("band", nsamples, flush)

    def band_state(self):
        """sgz_pcm_stream_band_state: (columns written since the lane was armed, samples of the open column)"""
        return self._lane_state("band")

    def flush_band(self) -> None:
        """sgz_pcm_stream_flush_band: closes the open column (one more record per channel at the cursor); waits"""
        self._lane_flush("band")

    # the histogram lane: one sgz_hist_record per column of m >= 128 samples and channel, beside whatever the feeds render
    def set_hist(self, m: int, out=None, capacity_columns: int | None = None) -> None:
        """sgz_pcm_stream_set_hist: out -- a HIST_DTYPE numpy array [capacity, channels] or a host torch uint8 tensor [capacity, channels, 448]
        (kept alive here; pinned memory is written in place); m == 0 disarms, 0 < m < 128 is refused"""
        self._lane_set("hist", m, out, capacity_columns)

    def hist_for(self, nsamples: int, flush: bool = False) -> int:
        """sgz_pcm_stream_hist_for: histogram columns the next feed of nsamples closes"""
        return self._lane_for("hist", nsamples, flush)

    def hist_state(self):
        """sgz_pcm_stream_hist_state: (columns written since the lane was armed, samples of the open column)"""
        return self._lane_state("hist")

    def flush_hist(self) -> None:
        """sgz_pcm_stream_flush_hist: closes the open column (one more record per channel at the cursor); waits"""
        self._lane_flush("hist")

    # the run lane: one sgz_run_record per column of m >= 32 samples and channel, beside whatever the feeds render
    def set_run(self, params, m: int, out=None, capacity_columns: int | None = None) -> None:
        """sgz_pcm_stream_set_run: params -- a RunParams (None allowed with m == 0); out -- a RUN_DTYPE numpy array [capacity, channels] or a
        host torch uint8 tensor [capacity, channels, 96] (kept alive here; pinned memory is written in place); m == 0 disarms, 0 < m < 32 is
        refused"""
        self._lane_set("run", m, out, capacity_columns, C.byref(params) if params is not None else None)

    def run_for(self, nsamples: int, flush: bool = False) -> int:
        """sgz_pcm_stream_run_for: run columns the next feed of nsamples closes"""
        return self._lane_for("run", nsamples, flush)

    def run_state(self):
        """sgz_pcm_stream_run_state: (columns written since the lane was armed, samples of the open column)"""
        return self._lane_state("run")

    def flush_run(self) -> None:
        """sgz_pcm_stream_flush_run: closes the open column (one more record per channel at the cursor); waits; the history is kept"""
        self._lane_flush("run")

    # the track lane: one tracked peak per (frame, pair) that becomes complete, beside whatever the feeds render
    def set_track(self, graph: int = 0, mouse_fraction: float = 0.5, out=None, capacity_frames: int | None = None) -> None:
        """sgz_pcm_stream_set_track: out -- a float64 numpy array or host torch tensor [capacity, pairs, 6] (kept alive here; pinned memory is
        written in place); the cursor restarts at 0.  out None disarms"""
        if capacity_frames is None:
            capacity_frames = 0 if out is None else int(out.shape[0])
        check(lib().sgz_pcm_stream_set_track(self.h, graph, float(mouse_fraction), _buf_ptr(out) if out is not None else None, capacity_frames))
        self._track_out = out

    def track_for(self, nsamples: int) -> int:
        """sgz_pcm_stream_track_for: frames whose records the next feed of nsamples writes; 0 when disarmed"""
        return int(lib().sgz_pcm_stream_track_for(self.h, nsamples))

    def track_state(self) -> int:
        """sgz_pcm_stream_track_state: frames written since the lane was armed or the stream reset (the cursor)"""
        f = C.c_uint64(0)
        check(lib().sgz_pcm_stream_track_state(self.h, C.byref(f)))
        return int(f.value)


def _columns_limits(symbol: str):
    s, t = C.c_uint32(0), C.c_uint32(0)
    getattr(lib(), symbol)(C.byref(s), C.byref(t))
    return int(s.value), int(t.value)


def _by_ref(x):
    return C.byref(x) if x is not None else None


def _stage_columns(symbol: str, planar, channel_stride: int, cells: int, nsamples: int, front, m: int, held: int, flush, continued, slices: int, carry,
                   out, stream) -> int:
    """sgz_stage_<lane>_columns.  front: what the C call takes between nsamples and m; continued: None where the call has none"""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    ptr = lambda t: _buf_ptr(t) if t is not None else None                      # noqa: E731
    history = () if continued is None else (int(bool(continued)),)
    return getattr(lib(), symbol)(ptr(planar), channel_stride, cells, nsamples, *front, m, held, int(bool(flush)), *history, slices, ptr(carry), ptr(out),
                                  C.c_void_p(s) if s else None)


def _lane_fold(symbol: str, dtype, records: np.ndarray, out_columns: int, x0: int, x1: int | None) -> np.ndarray:
    records = np.ascontiguousarray(records, dtype)
    n, cells = records.shape
    x1 = n if x1 is None else x1
    out = np.zeros((max(min(out_columns, x1 - x0), 1), cells), dtype)
    check(getattr(lib(), symbol)(_np_ptr(records), n, cells, x0, x1, out_columns, _np_ptr(out)))
    return out[:min(out_columns, x1 - x0)]


def wave_columns_limits():
    """sgz_wave_columns_limits: (the switch-over between the tile form and the sliced form, the tile's samples)"""
    return _columns_limits("sgz_wave_columns_limits")


def stage_wave_columns(planar, channel_stride: int, channels: int, nsamples: int, m: int, held: int = 0, flush: bool = True, slices: int = 0,
                       carry=None, wave=None, stream=None) -> int:
    """sgz_stage_wave_columns as it is: planar / carry / wave -- cuda float32 tensors (their data pointers; any may be None where the call
    allows NULL); returns the status.  Asynchronous on `stream` (default: torch's current stream)."""
    return _stage_columns("sgz_stage_wave_columns", planar, channel_stride, channels, nsamples, (), m, held, flush, None, slices, carry, wave, stream)


def level_columns_limits():
    """sgz_level_columns_limits: (the switch-over between the tile form and the sliced form, the tile's samples per row)"""
    return _columns_limits("sgz_level_columns_limits")


def stage_level_columns(planar, channel_stride: int, pairs: int, nsamples: int, m: int, held: int = 0, flush: bool = True, slices: int = 0,
                        carry=None, level=None, stream=None) -> int:
    """sgz_stage_level_columns as it is: planar / carry / level -- cuda tensors (their data pointers; any may be None where the call allows
    NULL); returns the status.  Asynchronous on `stream` (default: torch's current stream)."""
    return _stage_columns("sgz_stage_level_columns", planar, channel_stride, pairs, nsamples, (), m, held, flush, None, slices, carry, level, stream)


def level_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_level_fold: LEVEL_DTYPE records [n, pairs], source columns [x0, x1) -> [min(out_columns, x1 - x0), pairs]"""
    return _lane_fold("sgz_level_fold", LEVEL_DTYPE, records, out_columns, x0, x1)


def level_readout(record) -> dict:
    """sgz_level_readout of one LEVEL_DTYPE record: {rms, rms_db, dc: (L, R), correlation}"""
    rec = np.ascontiguousarray(record, LEVEL_DTYPE).reshape(1)
    r = LevelReading()
    check(lib().sgz_level_readout(_np_ptr(rec), C.byref(r)))
    return dict(rms=tuple(r.rms), rms_db=tuple(r.rms_db), dc=tuple(r.dc), correlation=r.correlation)


def field_columns_limits():
    """sgz_field_columns_limits: (the switch-over between the tile form and the sliced form, the tile's sample frames)"""
    return _columns_limits("sgz_field_columns_limits")


def field_boundaries() -> np.ndarray:
    """sgz_field_boundaries: the normative table, int32 [32, 2]: (C_k, S_k)"""
    cs = np.zeros((FIELD_SECTORS, 2), np.int32)
    lib().sgz_field_boundaries(_np_ptr(cs))
    return cs


def stage_field_columns(planar, channel_stride: int, pairs: int, nsamples: int, m: int, held: int = 0, flush: bool = True, slices: int = 0,
                        carry=None, field=None, stream=None) -> int:
    """sgz_stage_field_columns as it is: planar / carry / field -- cuda tensors (their data pointers; any may be None where the call allows
    NULL); returns the status.  Asynchronous on `stream` (default: torch's current stream)."""
    return _stage_columns("sgz_stage_field_columns", planar, channel_stride, pairs, nsamples, (), m, held, flush, None, slices, carry, field, stream)


def field_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_field_fold: FIELD_DTYPE records [n, pairs], source columns [x0, x1) -> [min(out_columns, x1 - x0), pairs]"""
    return _lane_fold("sgz_field_fold", FIELD_DTYPE, records, out_columns, x0, x1)


def field_readout(record) -> dict:
    """sgz_field_readout of one FIELD_DTYPE record: {share, mean, peak: float64 [32], direction, spread, silent_share}"""
    rec = np.ascontiguousarray(record, FIELD_DTYPE).reshape(1)
    r = FieldReading()
    check(lib().sgz_field_readout(_np_ptr(rec), C.byref(r)))
    return dict(share=np.array(r.share), mean=np.array(r.mean), peak=np.array(r.peak), direction=r.direction, spread=r.spread,
                silent_share=r.silent_share)


def hist_columns_limits():
    """sgz_hist_columns_limits: (the switch-over between the tile form and the sliced form, the tile's samples)"""
    return _columns_limits("sgz_hist_columns_limits")


def hist_edges():
    """sgz_hist_edges: (lo, hi), uint32 [106] each: the integers |v| of every bucket; lo > hi where a bucket holds none"""
    lo, hi = np.zeros(HIST_BUCKETS, np.uint32), np.zeros(HIST_BUCKETS, np.uint32)
    lib().sgz_hist_edges(_np_ptr(lo), _np_ptr(hi))
    return lo, hi


def stage_hist_columns(planar, channel_stride: int, channels: int, nsamples: int, m: int, held: int = 0, flush: bool = True, slices: int = 0,
                       carry=None, hist=None, stream=None) -> int:
    """sgz_stage_hist_columns as it is: planar / carry / hist -- cuda tensors (their data pointers; any may be None where the call allows
    NULL); returns the status.  Asynchronous on `stream` (default: torch's current stream)."""
    return _stage_columns("sgz_stage_hist_columns", planar, channel_stride, channels, nsamples, (), m, held, flush, None, slices, carry, hist, stream)


def hist_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_hist_fold: HIST_DTYPE records [n, channels], source columns [x0, x1) -> [min(out_columns, x1 - x0), channels]"""
    return _lane_fold("sgz_hist_fold", HIST_DTYPE, records, out_columns, x0, x1)


def hist_percentile(record, q: float):
    """sgz_hist_percentile of one HIST_DTYPE record: (bucket, lo, hi) -- the bucket of the q-quantile of |v| and its edges, 1.0 = full scale"""
    rec = np.ascontiguousarray(record, HIST_DTYPE).reshape(1)
    b, lo, hi = C.c_uint32(0), C.c_double(0), C.c_double(0)
    check(lib().sgz_hist_percentile(_np_ptr(rec), q, C.byref(b), C.byref(lo), C.byref(hi)))
    return int(b.value), lo.value, hi.value


def hist_readout(record) -> dict:
    """sgz_hist_readout of one HIST_DTYPE record: {zero_share, negative_share, peak, peak_db, median_db, toggling, effective_bits}"""
    rec = np.ascontiguousarray(record, HIST_DTYPE).reshape(1)
    r = HistReading()
    check(lib().sgz_hist_readout(_np_ptr(rec), C.byref(r)))
    return {k: getattr(r, k) for k, _ in r._fields_}


def run_params_default() -> RunParams:
    """sgz_run_params_default: hot = 2^23 - 2^8 (the positive full scale of 16-bit PCM), quiet = 0"""
    p = RunParams()
    lib().sgz_run_params_default(C.byref(p))
    return p


def run_columns_limits():
    """sgz_run_columns_limits: (the switch-over between the tile form and the sliced form, the tile's samples)"""
    return _columns_limits("sgz_run_columns_limits")


def stage_run_columns(planar, channel_stride: int, channels: int, nsamples: int, params, m: int, held: int = 0, flush: bool = True,
                      continued: bool = False, slices: int = 0, carry=None, runs=None, stream=None) -> int:
    """sgz_stage_run_columns as it is: params -- a RunParams or None; planar / carry / runs -- cuda tensors (their data pointers; any may be
    None where the call allows NULL); returns the status.  Asynchronous on `stream` (default: torch's current stream)."""
    return _stage_columns("sgz_stage_run_columns", planar, channel_stride, channels, nsamples, (_by_ref(params),), m, held, flush, continued, slices, carry, runs, stream)


def run_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_run_fold: RUN_DTYPE records [n, channels], source columns [x0, x1) -> [min(out_columns, x1 - x0), channels], folded in order"""
    return _lane_fold("sgz_run_fold", RUN_DTYPE, records, out_columns, x0, x1)


def run_readout(record, rate: float) -> dict:
    """sgz_run_readout of one RUN_DTYPE record at `rate` samples per second: {share, longest_seconds, at_seconds} -- three each, for hot,
    quiet and flat -- and crossing_hz"""
    rec = np.ascontiguousarray(record, RUN_DTYPE).reshape(1)
    r = RunReading()
    check(lib().sgz_run_readout(_np_ptr(rec), rate, C.byref(r)))
    return dict(share=tuple(r.share), longest_seconds=tuple(r.longest_seconds), at_seconds=tuple(r.at_seconds), crossing_hz=r.crossing_hz)


def truepeak_columns_limits():
    """sgz_truepeak_columns_limits: (the switch-over between the tile form and the sliced form, the tile's samples)"""
    return _columns_limits("sgz_truepeak_columns_limits")


def truepeak_taps() -> np.ndarray:
    """sgz_truepeak_taps: the filter's table, int32 [4 phases, 12 taps]"""
    taps = np.zeros((4, 12), np.int32)
    lib().sgz_truepeak_taps(_np_ptr(taps))
    return taps


def stage_truepeak_columns(planar, channel_stride: int, channels: int, nsamples: int, m: int, held: int = 0, flush: bool = True,
                           continued: bool = False, slices: int = 0, carry=None, peaks=None, stream=None) -> int:
    """sgz_stage_truepeak_columns as it is: planar / carry / peaks -- cuda tensors (their data pointers; any may be None where the call allows
    NULL); returns the status.  Asynchronous on `stream` (default: torch's current stream)."""
    return _stage_columns("sgz_stage_truepeak_columns", planar, channel_stride, channels, nsamples, (), m, held, flush, continued, slices, carry, peaks, stream)


def truepeak_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_truepeak_fold: TRUEPEAK_DTYPE records [n, channels], source columns [x0, x1) -> [min(out_columns, x1 - x0), channels]"""
    return _lane_fold("sgz_truepeak_fold", TRUEPEAK_DTYPE, records, out_columns, x0, x1)


def truepeak_readout(record):
    """sgz_truepeak_readout of one TRUEPEAK_DTYPE record: (peak with 1.0 = full scale, dBTP)"""
    rec = np.ascontiguousarray(record, TRUEPEAK_DTYPE).reshape(1)
    p, d = C.c_double(0), C.c_double(0)
    check(lib().sgz_truepeak_readout(_np_ptr(rec), C.byref(p), C.byref(d)))
    return p.value, d.value


def loudness_filter_for_rate(rate: float) -> LoudnessFilter:
    """sgz_loudness_filter_for_rate: BS.1770's K-weighting at `rate`, W = the smallest power of two >= 0.08 rate, L = W / 16"""
    f = LoudnessFilter()
    check(lib().sgz_loudness_filter_for_rate(float(rate), C.byref(f)))
    return f


def loudness_filter(b, a, W: int, L: int) -> LoudnessFilter:
    """a LoudnessFilter of any coefficients: b [2][3], a [2][2] (a1, a2 of each stage)"""
    f = LoudnessFilter()
    for s in range(2):
        for i in range(3):
            f.b[s][i] = float(b[s][i])
        for i in range(2):
            f.a[s][i] = float(a[s][i])
    f.W, f.L = W, L
    return f


def loudness_taps(f: LoudnessFilter):
    """sgz_loudness_taps: (status, the normative table int32 [4, W] or None)"""
    taps = np.full((4, max(int(f.W), 1)), 0x5A5A5A5A, np.int32)
    st = lib().sgz_loudness_taps(C.byref(f), _np_ptr(taps))
    return st, (taps if st == SGZ_OK else None)


def loudness_columns_limits(f: LoudnessFilter, channels: int = 1):
    """sgz_loudness_columns_limits: (the column sums' switch-over, the run tile's samples, the carry's bytes for `channels` channels)"""
    s, t, b = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
    check(lib().sgz_loudness_columns_limits(C.byref(f), channels, C.byref(s), C.byref(t), C.byref(b)))
    return int(s.value), int(t.value), int(b.value)


def stage_loudness_columns(planar, channel_stride: int, channels: int, nsamples: int, filter, first_index: int, m: int, held: int = 0,
                           flush: bool = True, continued: bool = False, slices: int = 0, carry=None, records=None, stream=None) -> int:
    """sgz_stage_loudness_columns as it is: planar / carry / records -- cuda tensors (their data pointers; any may be None where the call allows
    NULL); returns the status.  Asynchronous on `stream` (default: torch's current stream)."""
    return _stage_columns("sgz_stage_loudness_columns", planar, channel_stride, channels, nsamples, (_by_ref(filter), first_index), m, held, flush, continued, slices,
                          carry, records, stream)


def loudness_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_loudness_fold: LOUDNESS_DTYPE records [n, channels], source columns [x0, x1) -> [min(out_columns, x1 - x0), channels]"""
    return _lane_fold("sgz_loudness_fold", LOUDNESS_DTYPE, records, out_columns, x0, x1)


def loudness_readout(records: np.ndarray, weights=None):
    """sgz_loudness_readout of LOUDNESS_DTYPE records [ncols, channels] read together: (LUFS, the weighted mean square)"""
    records = np.ascontiguousarray(records, LOUDNESS_DTYPE)
    ncols, channels = records.shape
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    l, z = C.c_double(0), C.c_double(0)
    check(lib().sgz_loudness_readout(_np_ptr(records), ncols, channels, _np_ptr(w) if w is not None else None, C.byref(l), C.byref(z)))
    return l.value, z.value


def loudness_integrated(records: np.ndarray, weights=None) -> float:
    """sgz_loudness_integrated of LOUDNESS_DTYPE records [n, channels] of 100 ms columns: the gated loudness in LUFS"""
    records = np.ascontiguousarray(records, LOUDNESS_DTYPE)
    n, channels = records.shape
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    l = C.c_double(0)
    check(lib().sgz_loudness_integrated(_np_ptr(records), n, channels, _np_ptr(w) if w is not None else None, C.byref(l)))
    return l.value


def band_filter_for_rate(rate: float, low_hz: float = 300.0, high_hz: float = 3000.0) -> BandFilter:
    """sgz_band_filter_for_rate: the Oscilloscope's crossover at `rate`, W = the smallest power of two >= 6 rate / low_hz, L = W / 16"""
    f = BandFilter()
    check(lib().sgz_band_filter_for_rate(float(rate), float(low_hz), float(high_hz), C.byref(f)))
    return f


def band_filter(c, W: int, L: int) -> BandFilter:
    """a BandFilter of any coefficients: c [4][5] = {b0, b1, b2, a1, a2} of lp1, hp1, lp2, hp2"""
    f = BandFilter()
    for s in range(4):
        for i in range(5):
            f.c[s][i] = float(c[s][i])
    f.W, f.L = W, L
    return f


def band_taps(f: BandFilter):
    """sgz_band_taps: (status, the normative table int32 [16, W] or None)"""
    taps = np.full((16, max(int(f.W), 1)), 0x5A5A5A5A, np.int32)
    st = lib().sgz_band_taps(C.byref(f), _np_ptr(taps))
    return st, (taps if st == SGZ_OK else None)


def band_columns_limits(f: BandFilter, channels: int = 1):
    """sgz_band_columns_limits: (the column sums' switch-over, the run tile's samples, the carry's bytes for `channels` channels)"""
    s, t, b = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
    check(lib().sgz_band_columns_limits(C.byref(f), channels, C.byref(s), C.byref(t), C.byref(b)))
    return int(s.value), int(t.value), int(b.value)


def stage_band_columns(planar, channel_stride: int, channels: int, nsamples: int, filter, first_index: int, m: int, held: int = 0,
                       flush: bool = True, continued: bool = False, slices: int = 0, carry=None, records=None, stream=None) -> int:
    """sgz_stage_band_columns as it is: planar / carry / records -- cuda tensors (their data pointers; any may be None where the call allows
    NULL); returns the status.  Asynchronous on `stream` (default: torch's current stream)."""
    return _stage_columns("sgz_stage_band_columns", planar, channel_stride, channels, nsamples, (_by_ref(filter), first_index), m, held, flush, continued, slices,
                          carry, records, stream)


def band_fold(records: np.ndarray, out_columns: int, x0: int = 0, x1: int | None = None) -> np.ndarray:
    """sgz_band_fold: BAND_DTYPE records [n, channels], source columns [x0, x1) -> [min(out_columns, x1 - x0), channels]"""
    return _lane_fold("sgz_band_fold", BAND_DTYPE, records, out_columns, x0, x1)


def band_readout(records: np.ndarray, channel: int = 0):
    """sgz_band_readout of BAND_DTYPE records [ncols, channels] of one channel read together: (mean squares float64 [3], dB float64 [3])"""
    records = np.ascontiguousarray(records, BAND_DTYPE)
    ncols, channels = records.shape
    ms, db = np.zeros(3, np.float64), np.zeros(3, np.float64)
    check(lib().sgz_band_readout(_np_ptr(records), ncols, channels, channel, _np_ptr(ms), _np_ptr(db)))
    return ms, db


def band_colours(records: np.ndarray, channel: int, band_colours, key_rgba8, frequency_colouring_blend: float) -> np.ndarray:
    """sgz_band_colours of BAND_DTYPE records [ncols, channels]: uint8 [ncols, 4], the Oscilloscope's colour of every column of `channel`;
    band_colours float32 [3][3] (band, rgb), key_rgba8 the channel's key colour"""
    records = np.ascontiguousarray(records, BAND_DTYPE)
    ncols, channels = records.shape
    bc = np.ascontiguousarray(band_colours, np.float32).reshape(3, 3)
    key = np.ascontiguousarray(key_rgba8, np.uint8).reshape(4)
    out = np.zeros((ncols, 4), np.uint8)
    check(lib().sgz_band_colours(_np_ptr(records), ncols, channels, channel, _np_ptr(bc), _np_ptr(key), float(frequency_colouring_blend), _np_ptr(out)))
    return out


def _overview_pcm(kind: str, cfg, pcm, fmt: int, src_channels: int, k: int, channel_map, nsamples, wants=(), front=(), mid=(), bands: int = 0,
                  planes=None):
    """sgz_spectrogram_overview<suffix>_pcm of a kind of OVERVIEW_KINDS.  wants: the flags of its optional outputs in C order; front: what the C
    call takes between nsamples and k, mid: between k and its outputs; bands: of the cross table; planes: of pct's values -> (status, every
    output's columns or None where not wanted, timing dict)"""
    kind, c = OVERVIEW_KINDS[kind], _as_config(cfg)
    nbytes = pcm.numel() * pcm.element_size() if hasattr(pcm, "data_ptr") else pcm.nbytes
    n = nbytes // (src_channels * PCM_SAMPLE_BYTES[fmt]) if nsamples is None else nsamples
    F = max(0, int(lib().sgz_num_frames(n, c.window_size, c.hop)))
    cols = -(-F // k) if k else 0
    outs = _overview_outputs(kind, (c.num_pairs, _sides(c), c.axis_points, bands), wants, planes)
    arrays = [_overview_out(cols, *o) for o in outs]
    m, mp = _channel_map(channel_map)
    t = PcmTiming()
    st = check(getattr(lib(), f"sgz_spectrogram_overview{kind.suffix}_pcm")(C.byref(c), _buf_ptr(pcm), fmt, src_channels, mp, n, *front, k, *mid,
                                                                            *_buf_ptrs(arrays), C.byref(t)))
    if st == SGZ_SKIPPED_FRAME:
        cols = 0
    return (st, *[_overview_cut(a, cols, *o) for a, o in zip(arrays, outs)], t.asdict())


def overview_pcm(cfg, pcm, fmt: int, src_channels: int, k: int, channel_map=None, nsamples: int | None = None, want_rgba: bool = True,
                 want_peaks: bool = False):
    """One-shot overview of an interleaved PCM buffer (sgz_spectrogram_overview_pcm): (status, rgba or None, peaks or None, timing dict);
    status is SGZ_SKIPPED_FRAME for fewer samples than one window."""
    return _overview_pcm("peaks", cfg, pcm, fmt, src_channels, k, channel_map, nsamples, (want_rgba, want_peaks))


def overview_stats_pcm(cfg, pcm, fmt: int, src_channels: int, k: int, channel_map=None, nsamples: int | None = None, want_rgba: bool = True,
                       want_stats: bool = True, want_means: bool = False):
    """One-shot mean overview of an interleaved PCM buffer (sgz_spectrogram_overview_stats_pcm): (status, rgba or None, records
    OVERVIEW_STAT_DTYPE or None, means or None, timing dict); SGZ_SKIPPED_FRAME and empty outputs for fewer samples than a window"""
    return _overview_pcm("stats", cfg, pcm, fmt, src_channels, k, channel_map, nsamples, (want_rgba, want_stats, want_means))


def overview_pct_pcm(cfg, pcm, fmt: int, src_channels: int, k: int, q=0.5, channel_map=None, nsamples: int | None = None, want_rgba: bool = True,
                     want_records: bool = True, want_values: bool = False):
    """One-shot percentile overview of an interleaved PCM buffer (sgz_spectrogram_overview_pct_pcm): (status, rgba or None, records
    OVERVIEW_PCT_DTYPE or None, values float32 [nq, columns, pairs, P] or None, timing dict); SGZ_SKIPPED_FRAME and empty outputs for fewer
    samples than a window"""
    qa, qp, nq = _quantiles(q)
    return _overview_pcm("pct", cfg, pcm, fmt, src_channels, k, channel_map, nsamples, (want_rgba, want_records, want_values), mid=(qp, nq),
                         planes=max(nq, 1))


def overview_power_pcm(cfg, pcm, fmt: int, src_channels: int, k: int, channel_map=None, nsamples: int | None = None, want_rgba: bool = True,
                       want_power: bool = True, want_levels: bool = False):
    """One-shot power overview of an interleaved PCM buffer (sgz_spectrogram_overview_power_pcm): (status, rgba or None, records
    OVERVIEW_POWER_DTYPE or None, levels or None, timing dict); SGZ_SKIPPED_FRAME and empty outputs for fewer samples than a window"""
    return _overview_pcm("power", cfg, pcm, fmt, src_channels, k, channel_map, nsamples, (want_rgba, want_power, want_levels))


def overview_cross_pcm(cfg, pcm, fmt: int, src_channels: int, edges, k: int, channel_map=None, nsamples: int | None = None):
    """One-shot cross overview of an interleaved PCM buffer (sgz_spectrogram_overview_cross_pcm): (status, records OVERVIEW_CROSS_DTYPE
    [columns, pairs, bands], timing dict); SGZ_SKIPPED_FRAME and no records for fewer samples than a window"""
    e = _edges(edges)
    return _overview_pcm("cross", cfg, pcm, fmt, src_channels, k, channel_map, nsamples, front=(_np_ptr(e), e.size - 1), bands=e.size - 1)


def overview_flux_pcm(cfg, pcm, fmt: int, src_channels: int, k: int, channel_map=None, nsamples: int | None = None):
    """One-shot flux overview of an interleaved PCM buffer (sgz_spectrogram_overview_flux_pcm): (status, records OVERVIEW_FLUX_DTYPE [columns,
    pairs, sides], timing dict); SGZ_SKIPPED_FRAME and no records for fewer samples than a window"""
    return _overview_pcm("flux", cfg, pcm, fmt, src_channels, k, channel_map, nsamples)


def render_spectrogram_pcm(cfg, pcm, fmt: int, src_channels: int, channel_map=None, nsamples: int | None = None, want_lines: bool = False):
    """One-shot render of an interleaved PCM buffer (sgz_spectrogram_render_pcm): (status, rgba, lines, timing dict); status is
    SGZ_SKIPPED_FRAME for fewer samples than one window."""
    c = _as_config(cfg)
    nbytes = pcm.numel() * pcm.element_size() if hasattr(pcm, "data_ptr") else pcm.nbytes
    n = nbytes // (src_channels * PCM_SAMPLE_BYTES[fmt]) if nsamples is None else nsamples
    F = max(0, int(lib().sgz_num_frames(n, c.window_size, c.hop)))
    rgba = np.zeros((max(F, 1), c.axis_points, 4), np.uint8)               # (never an empty array: its pointer may be null)
    lines = np.zeros((max(F, 1), c.num_pairs, NUM_GRAPHS, c.axis_points, 2), np.float32) if want_lines else None
    m, mp = _channel_map(channel_map)
    t = PcmTiming()
    st = check(lib().sgz_spectrogram_render_pcm(C.byref(c), _buf_ptr(pcm), fmt, src_channels, mp, n, _np_ptr(rgba),
                                                _np_ptr(lines) if want_lines else None, C.byref(t)))
    return st, rgba[:F], lines[:F] if want_lines else None, t.asdict()


def rotate_hue(rgb, amount: float) -> np.ndarray:
    a = np.asarray(rgb, np.uint8)
    out = np.zeros(3, np.uint8)
    lib().sgz_rotate_hue_rgb8(_np_ptr(a), C.c_float(amount), _np_ptr(out))
    return out


def time_window(time_mode: int, value: float, sample_rate: float, bpm: float = 0.0, cycle_samples: float = 0.0) -> float:
    """sgz_scope_time_window: handleFlagUpdates' effectiveWindowSize for a time mode, on the host"""
    return lib().sgz_scope_time_window(int(time_mode), float(value), float(sample_rate), float(bpm), float(cycle_samples))


def scope_dense_device(ring, n: int, columns: int, xy, length: int | None = None, stride: int | None = None, stream=None) -> None:
    """sgz_scope_dense_device: ring DEVICE float32 [channels][stride] in time order (the first `length` of each row), xy DEVICE float32
    [channels][2 min(columns, n)][2]; the per-column min / max vertices of the newest n samples.  Enqueued on `stream`, no wait."""
    channels = int(ring.shape[0])
    stride = int(ring.shape[1]) if stride is None else int(stride)
    length = stride if length is None else int(length)
    check(lib().sgz_scope_dense_device(_buf_ptr(ring), length, stride, channels, int(n), int(columns), _buf_ptr(xy),
                                       C.c_void_p(stream) if stream else None))


class _BatchedIngest:
    """What api.Scope and api.Vector take audio with: sgz_scope_* / sgz_vector_* push, set_mix, set_option, flush (_c: the C prefix)."""

    def _call(self, name: str, *args) -> int:
        return check(getattr(lib(), f"{self._c}_{name}")(self.h, *args))

    def set_option(self, option: int, value: int):
        """sgz_scope_set_option / sgz_vector_set_option (RT_OPT_DEFER_SUBMIT, RT_OPT_PARK_PUSHES)"""
        self._call("set_option", option, value)
        return self

    def push(self, block: np.ndarray) -> int:
        """sgz_scope_push / sgz_vector_push: block float32 [channels, samples]; returns SGZ_OK or SGZ_BUSY"""
        b = np.ascontiguousarray(block, np.float32)
        ptrs = (C.c_void_p * b.shape[0])(*[b[c].ctypes.data for c in range(b.shape[0])])
        return self._call("push", ptrs, b.shape[0], b.shape[1])

    def set_mix(self, matrix: np.ndarray):
        """sgz_scope_set_mix / sgz_vector_set_mix: matrix uint8 [num_channels, num_sources]; push then takes num_sources channels"""
        m = np.ascontiguousarray(matrix, np.uint8)
        if m.ndim != 2 or m.shape[0] != self.cfg.num_channels:
            raise ValueError(f"mix matrix must be [num_channels = {self.cfg.num_channels}, num_sources], got {m.shape}")
        self._call("set_mix", m.shape[1], _np_ptr(m))
        return self

    def flush(self):
        """blocks that waited for a staging slot are enqueued now (sgz_scope_flush / sgz_vector_flush): readers of results call it first"""
        self._call("flush")


class Scope(_BatchedIngest):
    """sgz_scope_* handle: the Oscilloscope's audio-thread state machine in HBM + drawWavePlot vertices."""
    _c = "sgz_scope"

    def __init__(self, **kw):
        self.cfg = ScopeConfig()
        colours = kw.pop("colours", None)
        bands = kw.pop("band_colours", None)
        for k, v in kw.items():
            setattr(self.cfg, k, v)
        for c in range(64):
            col = colours[c] if colours is not None and c < len(colours) else (255, 255, 255, 255)
            for j in range(4):
                self.cfg.colours[c][j] = int(col[j])
        if bands is not None:
            for i in range(3):
                for j in range(3):
                    self.cfg.band_colours[i][j] = float(bands[i][j])
        self.h = C.c_void_p()
        check(lib().sgz_scope_create(C.byref(self.cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().sgz_scope_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def configure(self, **kw):
        for k, v in kw.items():
            setattr(self.cfg, k, v)
        check(lib().sgz_scope_configure(self.h, C.byref(self.cfg)))

    def set_transport(self, position_in_samples: int):
        """cs.transportPosition (TriggeringMode::Window)"""
        check(lib().sgz_scope_set_transport(self.h, C.c_int64(int(position_in_samples))))

    def set_tempo(self, bpm: float):
        """cs.bpm, the host playhead's tempo (TIME_BEATS reads it at the next analyse); any thread"""
        check(lib().sgz_scope_set_tempo(self.h, float(bpm)))

    def effective_window(self) -> float:
        """state.effectiveWindowSize of the current frame (set by analyse in TIME_CYCLES / TIME_BEATS)"""
        return lib().sgz_scope_effective_window(self.h)

    def front(self, channel: int):
        self.flush()
        size, cur = C.c_uint32(0), C.c_uint32(0)
        check(lib().sgz_scope_front(self.h, channel, None, C.byref(size), C.byref(cur)))
        out = np.zeros(size.value, np.float32)
        check(lib().sgz_scope_front(self.h, channel, _np_ptr(out), C.byref(size), C.byref(cur)))
        return out, int(cur.value)

    def front_colours(self, channel: int, aux: bool = False) -> np.ndarray:
        self.flush()
        """colour ring memory beside front(channel): uint32 RGBA8 words [size]"""
        size = C.c_uint32(0)
        check(lib().sgz_scope_front(self.h, channel, None, C.byref(size), None))
        out = np.zeros(size.value, np.uint32)
        check(lib().sgz_scope_front_colours(self.h, channel, int(aux), _np_ptr(out)))
        return out

    def analyse(self, evaluator: int = 0, channel: int = 0) -> TriggerState:
        self.flush()
        ts = TriggerState()
        check(lib().sgz_scope_analyse(self.h, evaluator, channel, C.byref(ts)))
        return ts

    def state(self) -> dict:
        self.flush()
        out = np.zeros(8, np.uint64)
        check(lib().sgz_scope_debug_state(self.h, _np_ptr(out)))
        keys = ("frontOrigin", "bufferedSamples", "oldPeak", "currentPeak", "steadyClock", "peaks", "isWorkingOnPeak", "swaps")
        return {k: int(v) for k, v in zip(keys, out)}

    def gains(self):
        self.flush()
        g = C.c_double(0)
        env = np.zeros(self.cfg.num_channels, np.float32)
        check(lib().sgz_scope_gains(self.h, C.byref(g), _np_ptr(env)))
        return g.value, env

    def peak_filter(self, delta_time: float, lanes: int = 8) -> float:
        self.flush()
        g = C.c_double(0)
        check(lib().sgz_scope_peak_filter(self.h, delta_time, lanes, C.byref(g)))
        return g.value

    def vertices(self, view: ScopeView, evaluator: int, channel: int = 0, want_colours: bool = True, out=None):
        """out: (xyz float32 [>= n][3], rgba uint8 [>= n][4] or None) buffers the caller keeps (pinned ones make the read-back a DMA);
        default: fresh arrays"""
        self.flush()
        n = lib().sgz_scope_vertex_count(self.h, C.byref(view))
        if out is not None:
            xyz, rgba = out
            assert xyz.shape[0] >= n and (rgba is None or rgba.shape[0] >= n)
            want_colours = rgba is not None
        else:
            xyz = np.empty((n, 3), np.float32)
            rgba = np.empty((n, 4), np.uint8) if want_colours else None
        cnt = C.c_uint32(n)
        check(lib().sgz_scope_vertices(self.h, C.byref(view), evaluator, channel, _np_ptr(xyz),
                                       _np_ptr(rgba) if want_colours else None, C.byref(cnt)))
        return xyz[:cnt.value], (rgba[:cnt.value] if want_colours else None)


    def vertices_all(self, view: ScopeView, evaluators, channels, out):
        """sgz_scope_vertices_all: out = [(xyz, rgba or None), ...] one per item, buffers the caller keeps; one wait for all of them"""
        self.flush()
        k = len(evaluators)
        n = lib().sgz_scope_vertex_count(self.h, C.byref(view))
        ev = (C.c_uint32 * k)(*evaluators); ch = (C.c_uint32 * k)(*channels)
        xs = (C.c_void_p * k)(*[o[0].ctypes.data for o in out])
        want = all(o[1] is not None for o in out)
        cs = (C.c_void_p * k)(*[o[1].ctypes.data if o[1] is not None else None for o in out])
        cnt = (C.c_uint32 * k)(*[o[0].shape[0] for o in out])
        check(lib().sgz_scope_vertices_all(self.h, C.byref(view), k, ev, ch, xs, cs if want else None, cnt))
        return [(o[0][:cnt[i]], o[1][:cnt[i]] if o[1] is not None else None) for i, o in enumerate(out)]

    def dense_vertex_count(self, columns: int) -> int:
        """sgz_scope_dense_vertex_count: 2 min(columns, n) for the current frame"""
        return lib().sgz_scope_dense_vertex_count(self.h, int(columns))

    def dense_vertices(self, columns: int, evaluator: int, channel: int = 0, want_colours: bool = True, out=None):
        """sgz_scope_dense_vertices: the Linear strip's minimum and maximum vertex per column.  out: (xyz [>= 2 cols][3], rgba
        [>= 2 cols][4] or None), numpy arrays or torch tensors (host, pinned or device) the caller keeps; default: fresh arrays"""
        n = self.dense_vertex_count(columns)
        if out is not None:
            xyz, rgba = out
            want_colours = rgba is not None
            cap = int(xyz.shape[0])
        else:
            xyz = np.empty((n, 3), np.float32)
            rgba = np.empty((n, 4), np.uint8) if want_colours else None
            cap = n
        cnt = C.c_uint32(cap)
        check(lib().sgz_scope_dense_vertices(self.h, int(columns), evaluator, channel, _buf_ptr(xyz),
                                             _buf_ptr(rgba) if want_colours else None, C.byref(cnt)))
        return xyz[:cnt.value], (rgba[:cnt.value] if want_colours else None)

    def dense_vertices_all(self, columns: int, evaluators, channels, out):
        """sgz_scope_dense_vertices_all: out = [(xyz, rgba or None), ...] one per item (numpy arrays or torch tensors, host or all of
        them device); the strips are enqueued back to back, one wait"""
        k = len(evaluators)
        ev = (C.c_uint32 * k)(*evaluators); ch = (C.c_uint32 * k)(*channels)
        xs = (C.c_void_p * k)(*[_buf_ptr(o[0]).value for o in out])
        want = any(o[1] is not None for o in out)
        cs = (C.c_void_p * k)(*[_buf_ptr(o[1]).value if o[1] is not None else None for o in out])
        cnt = (C.c_uint32 * k)(*[int(o[0].shape[0]) for o in out])
        check(lib().sgz_scope_dense_vertices_all(self.h, int(columns), k, ev, ch, xs, cs if want else None, cnt))
        return [(o[0][:cnt[i]], o[1][:cnt[i]] if o[1] is not None else None) for i, o in enumerate(out)]


class Vector(_BatchedIngest):
    """sgz_vector_* handle: history ring + audio-thread filters + polar vertices in HBM."""
    _c = "sgz_vector"

    def __init__(self, **kw):
        self.cfg = VectorConfig()
        colours = kw.pop("colours", None)
        for k, v in kw.items():
            setattr(self.cfg, k, v)
        for p in range(32):
            col = colours[p] if colours is not None and p < len(colours) else (1.0, 1.0, 1.0)
            for j in range(3):
                self.cfg.colours[p][j] = float(col[j])
        self.h = C.c_void_p()
        check(lib().sgz_vector_create(C.byref(self.cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().sgz_vector_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def history(self, channel: int):
        self.flush()
        size, cur = C.c_uint32(0), C.c_uint32(0)
        out = np.zeros(self.cfg.window_size, np.float32)
        check(lib().sgz_vector_history(self.h, channel, _np_ptr(out), C.byref(size), C.byref(cur)))
        return out, int(cur.value)

    def filters(self):
        self.flush()
        f, g = VectorFilters(), C.c_double(0)
        check(lib().sgz_vector_filters_get(self.h, C.byref(f), C.byref(g)))
        return f, g.value

    def peak_filter(self, delta_time: float) -> float:
        self.flush()
        g = C.c_double(0)
        check(lib().sgz_vector_peak_filter(self.h, delta_time, C.byref(g)))
        return g.value

    def vertices_all(self, want_colours: bool = True, out=None):
        """out: (xyz float32 [pairs][n][3], rgb float32 [pairs][n][3] or None) buffers the caller keeps; default: fresh arrays"""
        self.flush()
        n, pairs = self.cfg.window_size, self.cfg.num_channels // 2
        if out is not None:
            xyz, rgb = out
            assert xyz.shape == (pairs, n, 3) and (rgb is None or rgb.shape == (pairs, n, 3))
            want_colours = rgb is not None
        else:
            xyz = np.empty((pairs, n, 3), np.float32)
            rgb = np.empty((pairs, n, 3), np.float32) if want_colours else None
        cnt = C.c_uint32(n)
        check(lib().sgz_vector_vertices_all(self.h, _np_ptr(xyz), _np_ptr(rgb) if want_colours else None, C.byref(cnt)))
        return xyz, rgb

    def vertices(self, pair: int = 0, want_colours: bool = True):
        self.flush()
        n = self.cfg.window_size
        xyz = np.zeros((n, 3), np.float32)
        rgb = np.zeros((n, 3), np.float32) if want_colours else None
        cnt = C.c_uint32(n)
        check(lib().sgz_vector_vertices(self.h, pair, _np_ptr(xyz), _np_ptr(rgb) if want_colours else None, C.byref(cnt)))
        return xyz, rgb

    def lissajous(self, pair: int = 0, want_colours: bool = True):
        """drawRectPlot's stream of one pair (sgz_vector_lissajous_vertices): xyz float32 [n][3], rgb float32 [n][3] or None"""
        self.flush()
        n = self.cfg.window_size
        xyz = np.zeros((n, 3), np.float32)
        rgb = np.zeros((n, 3), np.float32) if want_colours else None
        cnt = C.c_uint32(n)
        check(lib().sgz_vector_lissajous_vertices(self.h, pair, _np_ptr(xyz), _np_ptr(rgb) if want_colours else None, C.byref(cnt)))
        return xyz, rgb

    def lissajous_all(self, xyz=None, rgb=None):
        """every pair's Lissajous stream with one wait (sgz_vector_lissajous_vertices_all).  xyz / rgb: [pairs][n][3] float32 buffers
        the caller keeps -- numpy arrays or torch tensors, host (pinned or not) or device --; xyz None: fresh numpy arrays for both"""
        self.flush()
        n, pairs = self.cfg.window_size, self.cfg.num_channels // 2
        if xyz is None:
            xyz, rgb = np.empty((pairs, n, 3), np.float32), np.empty((pairs, n, 3), np.float32)
        assert tuple(xyz.shape) == (pairs, n, 3) and (rgb is None or tuple(rgb.shape) == (pairs, n, 3))
        cnt = C.c_uint32(n)
        check(lib().sgz_vector_lissajous_vertices_all(self.h, _buf_ptr(xyz), _buf_ptr(rgb) if rgb is not None else None, C.byref(cnt)))
        return xyz, rgb

    def meters(self) -> VectorMeters:
        """drawStereoMeters' indicator positions from the handle's filter states (sgz_vector_meters; waits)"""
        self.flush()
        m = VectorMeters()
        check(lib().sgz_vector_meters(self.h, C.byref(m)))
        return m
